// Layout of the training step (train_api.hip): what a T5 layer is, and every offset, stride and order that follows from it.
// A layer is two residual sub-blocks in the encoder and three in the decoder, each y = x + mid(norm(x, ln) W_in^T) W_out^T
// with mid = self-attention, cross-attention or the feed-forward's activation (ReLU in place, or the gated GELU of T5 v1.1:
// W_in stacks wi_0 over wi_1, n_in = 2 d_ff, and mid = gelu_new(gate half) * linear half is a slot of its own). That is written ONCE here, as the table of a stack (StackLayout); the
// saved activations, the saved X^T slots, the dY^T room of a layer's weight-gradient group, the flat parameter order and a
// layer's gradient bucket are derived from the table, so the encoder's and the decoder's answers are the same code. The
// same order names a model's weights for the loader and the forward passes (api.hip, passes.hip): which field of the ABI's
// desc a slot comes from, the shape of a sub-block's GEMM weights and the norm weight folded into their f16 planes. Plain
// host arithmetic — no HIP types: tests/test_train_layout.py compiles it with the host compiler and checks it without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/ripor_hip.h"

namespace rpr {

inline int pad32(int n) { return (n + 31) & ~31; }
inline int pad64(int n) { return (n + 63) & ~63; }
// row stride (elements) of the transposed bf16 operands [cols][pad64(rows)] of the weight-gradient products. (Padding it off
// the power of two — 8192 rows = 16 KB looked like a memory-channel hazard for K-tiles that are 128-byte pieces of 256 rows —
// measured no different: 27.4 ms per step unpadded, 27.6 with 64 elements, 28.3 with 32; HISTORY.md.)
inline int ldT(int rows) { return pad64(rows); }

struct TrainDims {
  int bz, Lq, L, docs, S, R, T, dm, inner, dff, H, ne, nd, V, xld, buckets;   // docs: decoder sequences per query (S = bz docs)
  float eps, post;
  bool gated;       // feed-forward kind: gated GELU (W_in of 2 d_ff rows) instead of ReLU
  int ff_in() const { return gated ? 2 * dff : dff; }   // output width of the FF block's inner projection
};
// a batch of bz queries of Lq padded tokens, docs decoder sequences of L positions per query
inline TrainDims train_dims(const rpr_model_desc& d, int bz, int Lq, int L, int docs, bool gated = false) {
  TrainDims D{};
  D.bz = bz; D.Lq = Lq; D.L = L; D.docs = docs; D.S = bz * docs; D.R = D.S * L; D.T = bz * Lq; D.dm = d.d_model; D.inner = d.num_heads * d.d_kv;
  D.dff = d.d_ff; D.H = d.num_heads; D.ne = d.num_layers; D.nd = d.num_decoder_layers; D.V = d.V; D.xld = D.nd * 2 * D.inner;
  D.buckets = d.rel_buckets; D.gated = gated;
  D.eps = d.layer_norm_eps; D.post = d.scaleup_output_hidden ? (float)pow((double)D.dm, -0.5) : 1.0f;
  return D;
}

// ---- a sub-block and a stack ------------------------------------------------------------------------------------------------
enum SubKind { SUB_SELF, SUB_CROSS, SUB_FF };
// n_in: output width of the inner projection W_in [n_in][d_model]; k_out: reduction width of the outer one W_out [d_model][k_out]
struct SubBlock { SubKind kind; int n_in, k_out; };
// gated (SUB_FF only): W_in is wi_0 (the gate, through gelu_new) stacked over wi_1, [2 d_ff][d_model]
inline SubBlock sub_block(SubKind kind, int inner, int dff, bool gated = false) {
  return kind == SUB_SELF ? SubBlock{kind, 3 * inner, inner} : kind == SUB_CROSS ? SubBlock{kind, inner, inner}
                                                                                  : SubBlock{kind, gated ? 2 * dff : dff, dff};
}

// Trainable tensors in the order of the flat gradient / optimizer-state buffers: the kinds in front of the layers, then per
// encoder layer and per decoder layer (ln, W_in, W_out) of every sub-block: K_ENC_LAYER + 3 j + role, K_DEC_LAYER + 3 j + role.
enum ParamKind { K_SHARED, K_ENC_REL, K_DEC_REL, K_ENC_FLN, K_DEC_FLN, K_START, K_IN_EMB, K_OUT_EMB, K_XKV, K_ENC_LAYER, K_DEC_LAYER = K_ENC_LAYER + 6,
                 K_END = K_DEC_LAYER + 9 };
enum ParamRole { P_LN, P_WIN, P_WOUT };

// Where sub-block j keeps its tensors inside ONE layer of its stack. Saved activations (floats): the input stream x
// [rows][d_model], the inner projection's output in [rows][n_in] and the middle op's output mid [rows][k_out] (a ReLU FF has
// none: its ReLU is applied in place, mid = in; a gated FF keeps both halves of in and the gate's product in mid). Saved X^T slots (bf16 elements): the inner projection's input [d_model][ld] and
// the outer one's [k_out][ld].
struct SubSlots { size_t x, in, mid, xt_in, xt_out; };

struct StackLayout {
  bool dec;
  int rows, ld, layers, nsub, dm, kind0;   // ld = ldT(rows); kind0: the ParamKind of sub-block 0's ln
  SubBlock sub[3] = {};
  SubSlots at[3] = {};
  size_t act_stride, xt_stride, dyT_elems;   // floats / X^T elements of one layer; dY^T elements of one layer's group
  size_t xt_base = 0;                        // the stack's first X^T slot (TrainLayout places the stacks)

  StackLayout(bool dec_, int rows_, int layers_, int dm_, int inner, int dff, bool gated = false)
      : dec(dec_), rows(rows_), ld(ldT(rows_)), layers(layers_), nsub(dec_ ? 3 : 2), dm(dm_), kind0(dec_ ? K_DEC_LAYER : K_ENC_LAYER) {
    const SubKind kinds[2][3] = {{SUB_SELF, SUB_FF}, {SUB_SELF, SUB_CROSS, SUB_FF}};
    size_t act = 0, xt = 0, dy = 0;
    for (int j = 0; j < nsub; ++j) {
      const SubBlock b = sub[j] = sub_block(kinds[dec][j], inner, dff, gated);
      at[j].x = act; act += (size_t)rows * dm;
      at[j].in = at[j].mid = act; act += (size_t)rows * b.n_in;
      if (b.kind != SUB_FF || gated) { at[j].mid = act; act += (size_t)rows * b.k_out; }
      at[j].xt_in = xt; xt += (size_t)ld * dm;
      at[j].xt_out = xt; xt += (size_t)ld * b.k_out;
      dy += (size_t)ld * (b.n_in + dm);   // dY^T of the W_out product [d_model][ld] and of the W_in product [n_in][ld]
    }
    act_stride = act; xt_stride = xt; dyT_elems = dy;
  }
  size_t act(int layer, size_t slot) const { return (size_t)layer * act_stride + slot; }          // at[j].x / .in / .mid
  size_t xt(int layer, size_t slot) const { return xt_base + (size_t)layer * xt_stride + slot; }   // at[j].xt_in / .xt_out
  int kind(int j, int role) const { return kind0 + 3 * j + role; }
  size_t numel(int j, int role) const {
    return role == P_LN ? (size_t)dm : role == P_WIN ? (size_t)sub[j].n_in * dm : (size_t)dm * sub[j].k_out;
  }
};

// Both stacks and what sits between them: the X^T buffer holds the encoder's layers, the cross-K/V projection's input
// [d_model][ldT(T)], then the decoder's layers.
struct TrainLayout {
  StackLayout enc, dec;
  size_t xt_xkv, xt_total;
  size_t dyT_xkv;   // dY^T elements of the cross-K/V product [xld][ldT(T)]: a group of its own
  explicit TrainLayout(const TrainDims& D) : enc(false, D.T, D.ne, D.dm, D.inner, D.dff, D.gated), dec(true, D.R, D.nd, D.dm, D.inner, D.dff, D.gated) {
    xt_xkv = enc.xt_stride * D.ne;
    dec.xt_base = xt_xkv + (size_t)enc.ld * D.dm;
    xt_total = dec.xt_base + dec.xt_stride * D.nd;
    dyT_xkv = (size_t)D.xld * enc.ld;
  }
  size_t dyT_max() const { return std::max(std::max(dec.dyT_elems, enc.dyT_elems), dyT_xkv); }
};

// ---- the ABI's names of the layer tensors -----------------------------------------------------------------------------------
// rpr_model_desc names a layer's tensors field by field, one host array of device pointers per kind. The ONE table that maps
// a layer ParamKind to its field: (ln, W_in, W_out) of the encoder's self-attention and FF sub-blocks, then of the decoder's
// self-attention, cross-attention and FF.
typedef const float* const* rpr_model_desc::*LayerField;
inline LayerField layer_field(int kind) {
  static const LayerField fields[K_END - K_ENC_LAYER] = {
      &rpr_model_desc::enc_ln0, &rpr_model_desc::enc_qkv, &rpr_model_desc::enc_o, &rpr_model_desc::enc_ln1, &rpr_model_desc::enc_wi,
      &rpr_model_desc::enc_wo, &rpr_model_desc::dec_ln0, &rpr_model_desc::dec_qkv, &rpr_model_desc::dec_o, &rpr_model_desc::dec_ln1,
      &rpr_model_desc::dec_xq, &rpr_model_desc::dec_xo, &rpr_model_desc::dec_ln2, &rpr_model_desc::dec_wi, &rpr_model_desc::dec_wo};
  return fields[kind - K_ENC_LAYER];
}

// ---- the flat parameter order -----------------------------------------------------------------------------------------------
// (observable: rpr_param_info and the checkpoints follow it). ptr: the tensor on the device (fill)
struct ParamSlot { int kind, layer; float* ptr; size_t numel, offset; };
// One GEMM weight of a sub-block as the loader and the forward passes see it: its slot, its shape [N][K] (the product is
// x W^T: N output columns, K the reduction) and the slot of the norm weight folded into its f16 planes (-1: none)
struct WeightRef { int slot, N, K, fold; };
struct ParamOrder {
  std::vector<ParamSlot> slots;
  size_t total = 0;
  bool own_out;   // the output codebooks are tensors of their own (K_OUT_EMB present)
  int ne;
  StackLayout stack[2];   // encoder, decoder: the tables of sub-blocks only (no rows)

  explicit ParamOrder(const rpr_model_desc& d, bool gated = false)
      : own_out(d.out_embeds != d.in_embeds), ne(d.num_layers),
        stack{StackLayout(false, 0, d.num_layers, d.d_model, d.num_heads * d.d_kv, d.d_ff, gated),
              StackLayout(true, 0, d.num_decoder_layers, d.d_model, d.num_heads * d.d_kv, d.d_ff, gated)} {
    const size_t dm = d.d_model, inner = (size_t)d.num_heads * d.d_kv, nd = d.num_decoder_layers;
    auto add = [&](int kind, int layer, size_t n) { slots.push_back({kind, layer, nullptr, n, total}); total += n; };
    add(K_SHARED, -1, (size_t)d.vocab_size * dm);
    add(K_ENC_REL, -1, (size_t)d.rel_buckets * d.num_heads);
    add(K_DEC_REL, -1, (size_t)d.rel_buckets * d.num_heads);
    add(K_ENC_FLN, -1, dm);
    add(K_DEC_FLN, -1, dm);
    add(K_START, -1, dm);
    add(K_IN_EMB, -1, (size_t)d.L * d.V * dm);
    if (own_out) add(K_OUT_EMB, -1, (size_t)d.L * d.V * dm);
    add(K_XKV, -1, nd * 2 * inner * dm);
    for (const StackLayout& st : stack)
      for (int i = 0; i < st.layers; ++i)
        for (int j = 0; j < st.nsub; ++j)
          for (int role = P_LN; role <= P_WOUT; ++role) add(st.kind(j, role), i, st.numel(j, role));
  }
  // Every slot gets its tensor from the desc. False if a tensor, a per-layer array or one of its entries is null.
  bool fill(const rpr_model_desc& d) {
    const float* global[K_ENC_LAYER] = {d.shared, d.enc_rel_bias, d.dec_rel_bias, d.enc_final_ln, d.dec_final_ln, d.start_embed,
                                        d.in_embeds, d.out_embeds, d.dec_xkv};
    bool ok = true;
    for (ParamSlot& p : slots) {
      const float* const* per_layer = p.kind < K_ENC_LAYER ? nullptr : d.*layer_field(p.kind);
      const float* t = p.kind < K_ENC_LAYER ? global[p.kind] : per_layer ? per_layer[p.layer] : nullptr;
      p.ptr = const_cast<float*>(t);
      ok = ok && t;
    }
    return ok;
  }
  // position of a tensor in the order (K_OUT_EMB only where own_out); a layer holds 3 nsub tensors: 6 in the encoder, 9 in the decoder
  int index(int kind, int layer = -1) const {
    const int globals = K_ENC_LAYER - !own_out;
    if (kind < K_ENC_LAYER) return kind > K_OUT_EMB ? globals - 1 : kind;
    return kind < K_DEC_LAYER ? globals + layer * 6 + (kind - K_ENC_LAYER) : globals + ne * 6 + layer * 9 + (kind - K_DEC_LAYER);
  }
  const ParamSlot& at(int kind, int layer = -1) const { return slots[(size_t)index(kind, layer)]; }
  // (ln, W_in, W_out) of sub-block j of a layer
  const ParamSlot* sub(const StackLayout& st, int layer, int j) const { return &at(st.kind(j, P_LN), layer); }
  // W_in [n_in][d_model], folded with the ln of its own sub-block, or W_out [d_model][k_out], folded with nothing
  WeightRef weight(bool dec, int layer, int j, int role) const {
    const StackLayout& st = stack[dec];
    const int ln = index(st.kind(j, P_LN), layer);
    return role == P_WIN ? WeightRef{ln + P_WIN, st.sub[j].n_in, st.dm, ln} : WeightRef{ln + P_WOUT, st.dm, st.sub[j].k_out, -1};
  }
  // the gradient bucket of a layer as (offset, numel): its tensors are contiguous, ln of sub-block 0 up to the end of the last W_out
  void bucket(const StackLayout& st, int layer, size_t* offset, size_t* numel) const {
    const ParamSlot &lo = at(st.kind0, layer), &hi = at(st.kind(st.nsub - 1, P_WOUT), layer);
    *offset = lo.offset; *numel = hi.offset + hi.numel - lo.offset;
  }
};

}  // namespace rpr
