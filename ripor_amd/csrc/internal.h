// Internal declarations shared by the translation units behind the C ABI (api.hip: the ABI and the search driver,
// passes.hip: the forward passes it enqueues, train_api.hip: the training step, rq_api.hip: docid creation). What the driver
// decides about one search is search_plan.h (host arithmetic only); here are the objects it decides about. Not part of the
// ABI: include/ripor_hip.h is.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "common.h"
#include "gemm_route.h"
#include "search_plan.h"
#include "train_layout.h"
#include "trie.h"

namespace rpr {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};
// The operands of one linear layer C = act(A @ W^T) (+ residual) (linear(), below), each in both representations: the ctx
// precision picks the exact fp32 MFMA kernel or the f16x2 split kernel. (Up here: a model hands out its weights as LinW.)
struct LinIn {                                                               // activation [M, K]
  const float* f; const __half* h; size_t ps; int ld; float scale = A_PLANE_SCALE;   //   fp32 / planes (+ their scale)
  const unsigned long long* ssq = nullptr; float inv_d_fix = 0.f, eps = 0.f;         //   fused RMSNorm: h = planes of x, W folded
};
struct LinW {                                                                // weight [N, K] (+ planes)
  const float* f; const __half* h; int N, K;                                 //   N: fp32 rows = columns the profile accounts
  size_t ps = 0;                                                             //   plane stride (0 = N * K)
  int Nh = 0;                                                                //   rows of a plane padded beyond N (0 = N): what the split kernel computes
  bool no_scratch = false;                                                   //   the ctx's split-K scratch is not lent to this product: the mid-size
                                                                             //   split-K route (gemm_route.h: part, mid_split) stays closed to it
  bool row_split_ok = false;                                                 //   the launcher's no_row_split does not reach this product
  bool force_pp = false;                                                     //   the 256x256 ping-pong kernel whatever the shape (GemmH2Args::force_pp)
};

}  // namespace rpr

using rpr::DevBuf;

struct rpr_model {
  rpr_ctx* ctx;
  rpr_model_desc d;   // (its per-layer host arrays are null: the tensors of a layer are reached through params)
  // Every trainable tensor, in the order of the flat gradient / optimizer-state buffers, filled at load (train_layout.h), and,
  // indexed like params.slots, the f16 hi/lo planes of every per-layer GEMM weight (split once at load; [2][N][K], plane
  // stride N*K; null for a norm weight and for the tensors in front of the layers)
  rpr::ParamOrder params;
  std::vector<__half*> planes;
  // The weights of sub-block j of layer i of a stack as the passes use them: the norm weight, W_in [n_in, d_model] and
  // W_out [d_model, k_out] with their planes; the cross-K/V weight of all decoder layers; the output codebook of position t
  const float* ln(bool dec, int i, int j) const { return params.sub(params.stack[dec], i, j)->ptr; }
  rpr::LinW weight(bool dec, int i, int j, int role) const {   // role: rpr::P_WIN, P_WOUT
    const rpr::WeightRef r = params.weight(dec, i, j, role);
    return {params.slots[r.slot].ptr, planes[r.slot], r.N, r.K};
  }
  rpr::LinW w_xkv() const { return {d.dec_xkv, h_dec_xkv, d.num_decoder_layers * 2 * inner(), d.d_model}; }
  // codebook t: V fp32 rows; its planes (times the final layer-norm weight and the scaleup factor) are Vp rows inside the
  // stacked [2][L*Vp][d] buffer
  rpr::LinW w_codebook(int t) const {
    rpr::LinW w{d.out_embeds + (size_t)t * d.V * d.d_model, h_out_embeds + (size_t)t * Vp() * d.d_model, d.V, d.d_model};
    w.ps = (size_t)d.L * Vp() * d.d_model; w.Nh = Vp();
    return w;
  }
  int32_t* enc_bucket = nullptr;  // [2*MAX_LQ-1]
  int32_t* dec_bucket = nullptr;  // [MAX_DEC_LEN]
  __half* h_dec_xkv = nullptr;
  __half* h_out_embeds = nullptr;  // [2][L*Vp][d]: every codebook padded to Vp = V rounded up to 64 rows (zero rows)
  int Vp() const { return (d.V + 63) & ~63; }   // width of the selection kernel's token axis and of a logits row
  // Fused RMSNorm: the planes of every projection that consumes a normalised input hold W * diag(ln_weight)
  // (W_in of a sub-block: the sub-block's ln, ParamOrder::weight; out_embeds: final ln * scaleup factor);
  // the fp32 weights of the caller stay untouched and serve the exact-fp32 mode.
  bool f32_only = false;           // a weight does not fit the f16 planes: every search of this model runs exact fp32
  bool planes_dirty = false;       // the fp32 weights changed (rpr_adamw_step) since the planes were split
  // Layer-0 Q/K/V table of the decoder (passes.hip: ensure_l0_table): q | k | v of every (position, token)
  // input row and of the start token's, [L * V + 1][3 * inner] fp32, as the layer-0 projection writes them in split
  // precision. Made on first use by a search, in place again after anything replaced the weights it is made from
  // (l0_valid: rpr_adamw_step, refresh_weight_planes) or switched the ctx's precision (l0_epoch against rpr_ctx::l0_epoch);
  // the allocation stays (captured graphs hold its address). l0_state -1: not for this model (over L0_TABLE_CAP, or no memory).
  float* l0_table = nullptr;
  bool l0_valid = false;
  unsigned l0_epoch = 0;
  int l0_state = 0;
  size_t l0_rows() const { return rpr::l0_table_rows(d.L, d.V); }
  size_t l0_bytes() const { return rpr::l0_table_bytes(d.L, d.V, inner()); }
  bool l0_ready(const rpr_ctx* c) const;   // made, and current for this ctx state (defined below rpr_ctx)
  std::vector<void*> owned;
  // how every plane buffer was produced (replayed by refresh_weight_planes after an optimizer step changed the weights)
  struct PlaneJob { const float* w; size_t n; __half* dst; const float* ln; float pre; size_t plane_stride; };   // plane_stride 0 = n
  std::vector<PlaneJob> plane_jobs;
  // bound of |logit| for any decoder state: sqrt(d_model) * max row norm of the output codebooks times the final
  // layer-norm weight (Cauchy-Schwarz on the RMS-normalised hidden state), times the scaleup factor; computed at load.
  // The forced-tail fork uses it to prove that no masked (-1e9) candidate can overtake a valid one (passes.hip: enqueue_fork).
  float logit_bound = INFINITY;
  int inner() const { return d.num_heads * d.d_kv; }
  // feed-forward kind (rpr_model_ext::ff_kind): RPR_FF_GATED_GELU = wo(gelu_new(wi_0 x) * wi_1 x), W_in of the FF sub-blocks
  // holds wi_0 over wi_1 ([2 d_ff][d_model], the table in params says so) and the passes run the gate kernel behind it
  const int ff_kind;
  bool gated() const { return ff_kind == RPR_FF_GATED_GELU; }
  rpr_model(rpr_ctx* c, const rpr_model_desc& desc, int ff_kind_ = RPR_FF_RELU)
      : ctx(c), d(desc), params(desc, ff_kind_ == RPR_FF_GATED_GELU), planes(params.slots.size(), nullptr), ff_kind(ff_kind_) {}
  ~rpr_model() {   // device memory goes with the object, also on the error paths of rpr_load_model
    if (enc_bucket) (void)hipFree(enc_bucket);
    if (dec_bucket) (void)hipFree(dec_bucket);
    for (void* p : owned) (void)hipFree(p);
  }
};

struct rpr_trie {
  rpr_ctx* ctx;
  int64_t N;
  int L, V;
  uint16_t* codes = nullptr;  // [dev] sorted [N, L]
  // [dev] child arrays of the first two trie levels (round 5): lvl0[c] = first sorted row whose code 0 is >= c (V + 1 entries,
  // lvl0[V] = N), lvl1[c0 * V + c1] = first row >= (c0, c1) (V * V + 1 entries; only for V <= 1024, L >= 2). The selection
  // kernel reads a child's row range from them at steps 0 and 1 instead of walking 23 / 16 dependent probes of a binary
  // search over the code matrix. Built for the trie's V at upload; dropped by rpr_trie_set_vocab.
  int32_t* lvl0 = nullptr;
  int32_t* lvl1 = nullptr;
  int lvl_V = 0;
  // [dev] round 6: CSR child arrays of the deeper levels (trie.h ChildLevels::deep: children of every node of more than
  // TRIE_NARROW rows) and the level-2 entry of every (c0, c1) node; read by the radix selection (select_radix.hip)
  int32_t* idx2 = nullptr;
  int32_t* d_start[rpr::TRIE_MAX_DEEP] = {};
  uint16_t* d_tok[rpr::TRIE_MAX_DEEP] = {};
  int d_n[rpr::TRIE_MAX_DEEP] = {};
  int n_deep = 0;
  void free_levels() {
    if (lvl0) (void)hipFree(lvl0);
    if (lvl1) (void)hipFree(lvl1);
    if (idx2) (void)hipFree(idx2);
    for (int i = 0; i < rpr::TRIE_MAX_DEEP; ++i) {
      if (d_start[i]) (void)hipFree(d_start[i]);
      if (d_tok[i]) (void)hipFree(d_tok[i]);
      d_start[i] = nullptr; d_tok[i] = nullptr; d_n[i] = 0;
    }
    lvl0 = lvl1 = idx2 = nullptr; n_deep = 0; lvl_V = 0;
  }
  std::vector<int64_t> perm;
  std::vector<uint16_t> host_sorted;
  std::string keys;           // docid strings in original row order, '\n'-joined (only when loaded from a file that has them)
  std::map<int, std::vector<double>> single_frac;   // per search length L: trie_single_frac (lazily, first search of that length)
  std::map<int, std::vector<double>> extra_mean;    //   and its extra_mean, from the same pass
  ~rpr_trie() { if (codes) (void)hipFree(codes); free_levels(); }
};

struct rpr_d2s {
  std::vector<uint16_t> codes;
  std::string keys;
  int64_t N = 0;
  int L = 0;
};

struct GraphKey {
  const rpr_model* m; const rpr_trie* t; rpr::SearchPlan plan;
  bool operator<(const GraphKey& o) const { return std::tie(m, t, plan) < std::tie(o.m, o.t, o.plan); }
};

// Forced-tail search (passes.hip::enqueue_search): a compacted batch of queries that goes on step by step after a fork
struct StageBufs {
  DevBuf qmap;              // int32 [cap]: stage query -> query of the call
  DevBuf cnt;               // int32 [4]: live queries, live rows (queries x beams)
  DevBuf src;               // int32 [cap]: source query (in the previous stage) of every query
  DevBuf offs, last, mask;  // first encoder row / attended length / mask row of every stage query
  DevBuf kcache, vcache;    // [nd][cap][H][depth][B][64]
  DevBuf score[2], lo[2], hi[2], tokens[2], anc[2];
};
// ... and the queries that leave at that fork: their remaining positions are scored in one teacher-forced pass
// cap = the stage's queries + the spare entries of the queries forced with extras (SearchPlan::pool)
struct TailBufs {
  DevBuf flag, flist;       // int32 [cap]: forced? (1 + extras), tail entry -> stage query (a spare entry: the virtual query cap_q + k)
  DevBuf cnt;               // int32 [4]: entries, sequences (x B), rows (x B x (L - T)), forced queries (= entries - spare entries in use)
  DevBuf kvq;               // int32 [cap]: tail entry -> the stage query whose caches, mask and encoder rows it reads (a spare entry: its owner)
  DevBuf spare;             // int32 [cap_q + 1 + pool + pool * B]: own entry -> spare entry index or -1 | spare entries in use |
                            //   owner of spare k | parent beam of slot s of spare k (-1 = filler)
  DevBuf qmap, offs, last, mask;
  DevBuf tokens;            // uint16 [cap * B][L]
  DevBuf gold;              // float [cap * B][L - T]
};
using rpr::MAX_FORKS;

struct Workspace {
  // encoder
  DevBuf ids, mask, last, offs, row_src, ex, eh, eqkv, eattn, eff, enc_out, xkv;
  // decoder
  DevBuf x, h, q, attn, ff, logits, kcache, vcache, lb;
  DevBuf sel_rs;          // radix selection (many beams): RadixWs scratch (select_radix_carve)
  // beam state (2 ping-pong buffers)
  DevBuf score[2], lo[2], hi[2], tokens[2], anc[2];
  // staged outputs
  DevBuf o_tokens, o_scores, o_lo, o_hi;
  // rpr_search_prefixes only: the same four per prefix length of the plan (SearchPlan::depths), tokens [Q, B, p]
  DevBuf d_tokens[rpr::MAX_DEPTHS], d_scores[rpr::MAX_DEPTHS], d_lo[rpr::MAX_DEPTHS], d_hi[rpr::MAX_DEPTHS];
  // rpr_search_margins only: the child bitmap of the current step [Q, B * Vp / 64] (the selection's tap_valid export) and
  // the per-query pruning margins [Q] float64 (prune_margin.hip)
  DevBuf mg_valid, o_margin;
  // f16 hi/lo planes of the GEMM inputs (split-precision mode): attention outputs, FF intermediates, the final
  // encoder states, and the UN-normalised residual streams (fused RMSNorm) with their row sums of squares
  DevBuf eattn_h, eff_h, enc_out_h, attn_h, ff_h, ex_h, x_h, ssq_e, ssq_d;
  // gated feed-forward only (rpr_model::gated): the W_in product's fp32 result [rows, 2 d_ff] (gate | linear half) of the
  // encoder, the decoder steps / teacher-forced forward and the tail pass; the gate kernel reads it into ff / ff_h
  DevBuf egu, gu, t_gu;
  DevBuf tr_x, tr_misc;   // rpr_train_forward scratch (teacher-forced decoder)
  DevBuf part;            // split-K partial sums of the mid-size GEMM route (gemm_h2.hip): 9 M floats
  // forced-tail search: stages 1.. (stage 0 = the buffers above), one tail job per fork, and the activations of a tail
  // pass (rows = queries x beams x remaining positions), shared by the forks
  StageBufs stage[MAX_FORKS];
  TailBufs tail[MAX_FORKS];
  DevBuf t_x, t_h, t_qkv, t_q, t_attn, t_ff, t_x_h, t_attn_h, t_ff_h, t_ssq;
  DevBuf t_logits;        // log-softmax mode: the V logits of every tail row (fp32)
  // residual quantization (rpr_rq_train / rpr_rq_encode, rq_api.hip): residuals [n, d], codes, counting-sort
  // histogram / row order, codeword norms, per-block fp64 sums of |r|^2, initial centroid rows
  DevBuf rq_r, rq_code, rq_hist, rq_order, rq_cnorm, rq_part, rq_idx;
  // rpr_rq_search: the LUT of a query chunk [Qc, M * K] and the selection scratch (state, histograms, candidate lists)
  DevBuf rq_lut, rq_sel;
  // rpr_flat_search: the scores of one (query chunk, row sub-block) [Qc, ld]; its selection scratch is rq_sel
  DevBuf flat_sc;
  // rpr_rq_encode_beam: the second residual plane (the first is rq_r), |r|^2 of the beam entries (two planes), the
  // candidates of a level (scores, then codes) and the parent slot / code history of every level (slots, then codes)
  DevBuf rq_r2, rq_bnorm, rq_cand, rq_bhist;
  // rpr_xenc_score (xenc_api.hip): hidden states [T, H] fp32, q | k | v [T, 3 H], attention output [T, H], a product's raw
  // result [T, H] fp32, the feed-forward intermediate [T, d_ff], the tile list + sequence offsets, and the f16 mode's f16
  // copy of the hidden states. xe_qkv, xe_ctx and xe_ff hold the elements of the call's mode (fp32 or f16)
  DevBuf xe_x, xe_qkv, xe_ctx, xe_tmp, xe_ff, xe_meta, xe_xh;
};

static_assert(sizeof(Workspace) % sizeof(DevBuf) == 0 && std::is_standard_layout<Workspace>::value,
              "Workspace must consist of DevBuf members only (rpr_free_ctx walks it as an array)");

// Half of a large search batch: its own workspace (KV cache, graphs are keyed by the lane) and a HIP stream confined to
// half of the CUs (hipExtStreamCreateWithCUMask). The two halves of a batch run side by side: the HBM-bound attention of
// one under the power-bound GEMMs of the other — on one stream every kernel has all CUs in the same phase.
struct Lane {
  Workspace ws;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
};

struct rpr_ctx : rpr::SearchSettings {   // (what a search is planned from: precision, forced tail, fork depths, extras, layer-0 table mode, lane CUs)
  int device;
  unsigned int* status = nullptr;       // [dev, 64 words] [8] weight-range probe; sticky words: [0] a value left the f16 plane range, [1] a query attends to nothing, [2] a query was left unforced by the last fork of an optimistic forced-tail search
  unsigned int* status_host = nullptr;  // pinned mirror filled by rpr_get_status
  struct TrainWs* tws = nullptr;        // activations / scratch of the training step (train_api.hip), freed by free_train_ws
  struct { float rate = 0.f; uint64_t seed = 0, step = 0; } train_drop;   // rpr_set_train_dropout: what the backward entry points apply (rate 0 = off)
  Workspace ws;
  Lane lanes[2];
  int lanes_state = 0;          // 0 not tried yet, 1 ready, -1 masked streams unavailable on this device
  int lane_min_rows = 10240;    // batches of at least this many decoder rows (queries x beams) are split over the two lanes (0 = never)
  hipEvent_t fork_ev = nullptr;
  std::vector<int> last_forks;  // fork depths of the last rpr_search and the workspaces it ran in (bit 0: ctx, 1 / 2: lanes)
  int last_ws_mask = 0;         //   -> rpr_last_fork_stats
  size_t ws_bytes = 0;
  int enc_rows_accounted = 0;   // live encoder rows of the last enqueue (profile accounting)
  unsigned l0_epoch = 0;        // bumped by rpr_set_precision: a model's layer-0 Q/K/V table of another epoch is made again
  hipStream_t cap_stream = nullptr;
  std::map<GraphKey, hipGraphExec_t> graphs;
  // profiling
  bool profiling = false;
  // one timed launch of the eager profile pass. live_dev (nullable): device word holding the live rows of a compacted /
  // packed launch whose flops and bytes were accounted for live_static rows at enqueue time; read back when the
  // records are flushed — no synchronisation while a step is being enqueued, so both lanes run side by side exactly as
  // in the timed region
  struct Rec { int cls; hipEvent_t a, b; double flops, bytes; const int* live_dev; int live_static; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  rpr_kernel_stats done[RPR_K_COUNT];
};

inline bool rpr_model::l0_ready(const rpr_ctx* c) const { return c->l0_mode > 0 && l0_table && l0_valid && l0_epoch == c->l0_epoch; }

namespace rpr {

// re-split every GEMM weight into its f16 planes (api.hip); sets model->f32_only if a weight no longer fits
int refresh_weight_planes(rpr_ctx* c, rpr_model* m, hipStream_t s);
inline int ensure_weight_planes(rpr_ctx* c, rpr_model* m, hipStream_t s) {
  if (!m->planes_dirty) return 0;
  const int e = refresh_weight_planes(c, m, s);
  if (!e) m->planes_dirty = false;
  return e;
}
// the table is there and current for the search about to be enqueued on stream s (split precision only); passes.hip
int ensure_l0_table(rpr_ctx* c, rpr_model* m, hipStream_t s);
void free_train_ws(rpr_ctx* c);   // train_api.hip
void train_forget_model(rpr_ctx* c, const rpr_model* m);   // train_api.hip: drop the per-model weight cache table

// destroy the captured graphs whose key `stale` names: whatever they reference is about to go or to change
template <class Pred> void drop_graphs(rpr_ctx* c, Pred&& stale) {
  for (auto it = c->graphs.begin(); it != c->graphs.end();) {
    if (stale(it->first)) { (void)hipGraphExecDestroy(it->second); it = c->graphs.erase(it); } else ++it;
  }
}

inline int ensure(rpr_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return 0;
  if (b.p) {
    RPR_HIP(hipFree(b.p));
    c->ws_bytes -= b.cap;
    b.p = nullptr; b.cap = 0;
    drop_graphs(c, [](const GraphKey&) { return true; });   // graphs captured against the old pointers are stale
  }
  const size_t want = (bytes + 255) & ~(size_t)255;
  RPR_HIP(hipMalloc(&b.p, want));
  b.cap = want;
  c->ws_bytes += want;
  return 0;
}

template <class T> T* P(const DevBuf& b) { return reinterpret_cast<T*>(b.p); }

// scoped temporary device buffer (test hooks): freed on every return path
struct DevTmp {
  void* p = nullptr;
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  ~DevTmp() { if (p) (void)hipFree(p); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Launch wrapper: optional hipEvent timing per kernel class (bench.py roofline leg).
struct Launcher {
  rpr_ctx* c;
  hipStream_t s;
  int err = 0;
  const int* live_dev = nullptr;   // profile accounting of the launches that follow (see rpr_ctx::Rec)
  int live_static = 0;
  // what the split-precision GEMM launches that follow are told (passes.hip: h2_args)
  int cus = 0;                     // CUs of the stream (0 = the whole chip): GemmH2Args.cus
  int no_row_split = 0;            // 1 while the packed encoder (and the cross-K/V product on its rows) is enqueued: GemmH2Args.no_row_split
  int small_live = 0;              // > 0 while a leftover stage is enqueued: its GEMMs are paired (GemmH2Args.small_live)
  int mfma16 = 0;                  // 1 while a tail pass is enqueued on a plan with SearchPlan::mfma16 (passes.hip: enqueue_tail): GemmH2Args.mfma16
  struct Mfma16Scope {             // the MFMA shape of the launches enqueued while the scope lives; the previous one comes back with it
    Launcher& L; const int old;
    Mfma16Scope(Launcher& L_, int v) : L(L_), old(L_.mfma16) { L.mfma16 = v; }
    ~Mfma16Scope() { L.mfma16 = old; }
  };
  void account_live(const int* dev, int rows_static) { live_dev = dev; live_static = rows_static; }
  hipEvent_t get_event() {
    if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  template <class F> void run(int cls, double flops, double bytes, F&& f, const int* cls_after = nullptr) {
    if (err) return;
    hipEvent_t ea = nullptr, eb = nullptr;
    if (c->profiling) {
      ea = get_event(); eb = get_event();
      if (ea) (void)hipEventRecord(ea, s);
    }
    hipError_t e = f();
    if (e != hipSuccess) { err = hip_fail(e, "kernel launch", __FILE__, __LINE__); return; }
    if (c->profiling && ea && eb) {
      (void)hipEventRecord(eb, s);
      c->recs.push_back({cls_after ? *cls_after : cls, ea, eb, flops, bytes, live_dev, live_static});
    }
  }
};

// ---- the forward passes (passes.hip) and the linear layer they are made of --------------------------------------------
// (LinIn and LinW: at the top)
struct LinOut {                                                              // destination
  float* f[3]; int ldo[3]; int split_n;                                      //   fp32 (up to 3 column blocks)
  __half* h; size_t ps; int ldh;                                             //   or f16 planes (next GEMM's input)
  const float* resid; int relu;
  int rm_B; size_t rm_stride, rm_slot, rm_head;                              //   KV-cache element map (common.h)
  int rm_dshift;                                                             //   log2(d_kv) of the map (0 = 6)
  float plane_scale;                                                         //   scale of the planes written to h (0 = 1)
  const __half* resid_h; unsigned long long* ssq_out;                        //   fused RMSNorm producer: residual read from the
};                                                                           //   planes h (in place), row sums accumulated
LinOut out_f32(float* p, int ld, int N, const float* resid = nullptr, int relu = 0);
// m_dev (nullable): device-side live row count (packed encoder); m_acc = rows to account flops/bytes for
void linear(Launcher& L, const LinIn& A, const LinW& W, int M, const LinOut& O, const int* m_dev = nullptr, int m_acc = -1);
// sizes c->ws for the plan (a lane's workspace: swapped in by the caller)
int alloc_workspace(rpr_ctx* c, const rpr_model* m, const SearchPlan& plan);
int alloc_train_workspace(rpr_ctx* c, const rpr_model* m, int bz, int Lq, int ndoc, int L);
void enqueue_encoder(Launcher& Ln, rpr_ctx* c, const rpr_model* m, int Q, int Lq, bool packed);
void enqueue_search(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const rpr_trie* tr, const SearchPlan& plan, const rpr_debug_taps* taps);
// hidden (nullable): decoder_last_hidden_state of every row [bz * ndoc * L, d_model] instead of the gold-code scores (rpr_embed)
void enqueue_train_forward(Launcher& Ln, rpr_ctx* c, const rpr_model* m, int bz, int Lq, int ndoc, int L,
                           const int32_t* codes /*[bz, ndoc, L]*/, float* pos_scores /*[bz, ndoc, L]*/, float* hidden = nullptr);

}  // namespace rpr
