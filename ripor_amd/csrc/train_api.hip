// Training step of the prefix-oriented ranking fine-tune (BASELINE config 5) behind the C ABI:
//   rpr_lngknp_backward  = forward (activations kept) + backward of T5SeqAQEncoderForLngKnpMarginMSE
//                          (reference modeling/t5_generative_retriever.py:902-966; loss.backward() in
//                          tasks/trainer.py:203-275) into one flat fp32 gradient buffer,
//   rpr_adamw_step       = clip_grad_norm_ + torch.optim.AdamW as HF Trainer configures them for main.py:131-155,
//   rpr_param_*          = the layout of the flat buffers (so the host can all-reduce them over RCCL and map them back
//                          to the checkpoint's tensor names).
// Arithmetic: fp32 activations and gradients. Matrix products: the search path's split-precision GEMM (f16 hi/lo planes,
// 3 f16 MFMAs per product, fp32 accumulation) with PER-TENSOR dynamic plane scales — gradients span ten orders of
// magnitude, so every operand's absolute maximum is found on the device and a power of two brings it to [2^13, 2^14)
// before the split; in RPR_PREC_F32 mode the exact-fp32 MFMA kernel (gemm_f32.hip). The reference trains under bf16
// autocast: both are the more precise side. The backward products reuse the forward kernels on transposed operands
// (train_kernels.hip); the reductions are deterministic (fixed-order partials, fixed-point integer atomics).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "internal.h"

using namespace rpr;

struct TrainWs;
namespace { int tensure(rpr_ctx* c, DevBuf& b, size_t bytes); }   // allocate or grow a buffer of the training workspace

// The weight-gradient products dW[N, K] = dY^T X run on ONE side stream beside the input-gradient chain. This struct owns that
// stream and all that lives by its clock; nothing outside it touches them. dW reduces over all rows of the batch into
// 9 .. 36 tiles of 256 x 256: split-K over the rows and a reduce pass.
// Measured, t5-base bz 128, against a whole-K route (one K-loop per 256 x 256 tile, products round-robin on 2-4 side
// streams; removed): bf16 32.4 ms whole-K vs 32.7 split-K; f16x2 56.3 vs 52.3 (a lone 256 x 256 block walks 256 K-tiles
// of the two-plane operands in 670 us and the side streams fall behind the main chain). And once the search path's two
// CU-masked lane streams exist in the process, a second side stream lands on the main stream's hardware queue and the
// step serialises (bf16 50 ms). The split-K route on ONE side stream does not depend on how the runtime maps streams to
// queues.
// Per-product route: the transposed-operand scratch rotates over NSIDE sets; a set is reused NSIDE products later, after
// its product has finished. Grouped route (bf16 mode, where the shapes allow it; measured: DESIGN.md section 9): the dY^T
// operands of one layer's products live side by side in one of two sets (a set is rewritten two layers later, after its
// group launch has finished), the products are collected in `grp` while the layer's input-gradient chain is enqueued and
// go out as ONE launch (gemm_h2_pp_group_kernel; gtab = the device table it reads its argument structs from).
struct WGradSide {
  static constexpr int NSIDE = 4, NGRP = 2;
  // fork: recorded on the main stream, the side stream waits for it; done: recorded behind the side stream's work;
  // pending: done has been recorded and the main stream has not been made to wait for it yet
  struct Sync { hipEvent_t fork = nullptr, done = nullptr; bool pending = false; };
  struct Set { DevBuf tX, tY; Sync sync; };   // X^T and dY^T of one product (fp32, two f16 planes or bf16)
  enum Fit { FIT_OPEN, FIT_EMPTY, FIT_NONE };
  // a dY the producing dX product's epilogue left converted: bf16 rows, and the transposed copy in a reserved slot of `gset`
  struct Pre { const float* dY = nullptr; const void* py = nullptr; __half* pyt = nullptr; int gset = -1; };

  // set_bytes: one transposed operand; dyT_bytes: one layer's dY^T operands (0 = no grouped route: every mode but bf16)
  int create(rpr_ctx* c, size_t set_bytes, size_t dyT_bytes) {
    int e = 0;
    for (Set& t : set) { if (!e) e = tensure(c, t.tX, set_bytes); if (!e) e = tensure(c, t.tY, set_bytes); }
    static_assert(GemmGroupArgs::MAXP * sizeof(GemmH2Args) <= GemmGroupArgs::TABLE_BYTES, "argument table");
    for (DevBuf& b : dyT) if (!e && dyT_bytes) e = tensure(c, b, dyT_bytes);
    if (!e && dyT_bytes) e = tensure(c, gtab, GemmGroupArgs::SCRATCH_BYTES);
    if (e || side) return e;
    hipError_t he = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
    each_sync([&](Sync& y) {
      for (hipEvent_t* ev : {&y.fork, &y.done}) if (he == hipSuccess) he = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    });
    RPR_HIP(he);
    return 0;
  }
  void destroy() {   // the buffers go with the workspace's registry (free_train_ws)
    each_sync([](Sync& y) { for (hipEvent_t ev : {y.fork, y.done}) if (ev) (void)hipEventDestroy(ev); });
    if (side) (void)hipStreamDestroy(side);
  }
  // the next rotating scratch set: the product that last read it (NSIDE products ago) must be over before Ln's stream rewrites it
  Set& next_set(Launcher& Ln) {
    Set& t = set[flip++ % NSIDE];
    wait(Ln, Ln.s, t.sync, true);
    return t;
  }
  // f32 mode runs both products on the main stream and borrows the X^T buffer of set 0 (no product is pending between passes)
  float* main_stream_scratch() const { return P<float>(set[0].tX); }
  // body(L2) runs on the side stream after everything Ln's stream holds so far; Ln's stream goes on at once
  template <class F> void run(Launcher& Ln, Sync& y, F&& body) {
    if (Ln.err) return;
    if (hipEventRecord(y.fork, Ln.s) != hipSuccess || hipStreamWaitEvent(side, y.fork, 0) != hipSuccess) { Ln.err = RPR_ERR_HIP; return; }
    Launcher L2{Ln.c, side};
    body(L2);
    if (L2.err) { Ln.err = L2.err; return; }
    if (hipEventRecord(y.done, side) != hipSuccess) { Ln.err = RPR_ERR_HIP; return; }
    y.pending = true;
  }
  // stream x waits for every per-product launch (the last product of every set: stream order covers the earlier ones) /
  // every group launch still in flight. clear: x is the main stream, the marks go; a communication stream leaves them
  void wait_products(Launcher& Ln, hipStream_t x, bool clear) { for (Set& t : set) wait(Ln, x, t.sync, clear); }
  void wait_groups(Launcher& Ln, hipStream_t x, bool clear) { for (Sync& y : gsync) wait(Ln, x, y, clear); }

  // ---- the group collector. A product is dW[N, K] reduced over `rows` (padded), its dY^T slot [N][ld] bf16 (256-byte aligned)
  static size_t slot_bytes(int N, int ld) { return (((size_t)N * ld * sizeof(__half)) + 255) & ~(size_t)255; }
  static int tiles(int N, int K) { return ((N + 255) / 256) * ((K + 255) / 256); }
  // does the product join the group being collected, only an empty group (flush first), or no group at all?
  Fit fit(int N, int K, int rows, size_t slot) const {
    if (tiles(N, K) > GemmGroupArgs::MAX_TILES || slot > dyT[gset].cap) return FIT_NONE;   // (the two sets have one size)
    const bool open = grp.n > 0 && grp.K == rows && grp.n < GemmGroupArgs::MAXP && grp_tiles + tiles(N, K) <= GemmGroupArgs::MAX_TILES &&
                      dyT_used + slot <= dyT[gset].cap;
    return open ? FIT_OPEN : FIT_EMPTY;
  }
  __half* reserve(size_t slot) {   // after fit() said FIT_OPEN, or flush() and FIT_EMPTY
    dyT_used += slot;
    return reinterpret_cast<__half*>(static_cast<char*>(dyT[gset].p) + dyT_used - slot);
  }
  void add(const __half* dyT_slot, const void* xT, float* dW, int N, int K, int rows, int ld) {
    const int i = grp.n++;
    grp.A[i] = dyT_slot; grp.W[i] = reinterpret_cast<const __half*>(xT); grp.out[i] = dW;
    grp.M[i] = N; grp.N[i] = K; grp.ldo[i] = K; grp.K = rows; grp.lda = ld; grp.ldw = ld;
    grp_tiles += tiles(N, K);
    grp_flops += 2.0 * N * (double)K * rows;
    grp_bytes += 2.0 * ((double)N * rows + (double)K * rows) + 4.0 * (double)N * K;
  }
  // enqueue the products collected since the last flush on the side stream; the main stream goes on
  void flush(Launcher& Ln) {
    if (grp.n == 0 || Ln.err) return;
    run(Ln, gsync[gset], [&](Launcher& L2) {
      const GemmGroupArgs g = grp;
      L2.run(RPR_K_GEMM, grp_flops, grp_bytes, [&] { return launch_gemm_h2_group(g, gtab.p, side); });
    });
    if (Ln.err) return;
    clear_group();
    gset ^= 1;
    wait(Ln, Ln.s, gsync[gset], true);   // the next layer writes into the other set: its last group launch must be over
  }
  // a backward that aborted on Ln.err leaves collected-but-unflushed products behind: never carry them into the next pass
  void reset() { clear_group(); pre = Pre{}; }
  bool pre_is(const float* dY) const { return pre.dY == dY && pre.gset == gset; }
  void leave_pre(const float* dY, const void* py, __half* pyt) { pre.dY = dY; pre.py = py; pre.pyt = pyt; pre.gset = gset; }
  Pre take_pre() { const Pre p = pre; pre = Pre{}; return p; }
  bool pre_left() const { return pre.dY != nullptr; }

 private:
  hipStream_t side = nullptr;
  Set set[NSIDE];
  unsigned flip = 0;
  DevBuf dyT[NGRP], gtab;
  Sync gsync[NGRP];
  GemmGroupArgs grp = {};
  int gset = 0, grp_tiles = 0;
  size_t dyT_used = 0;
  double grp_flops = 0, grp_bytes = 0;
  Pre pre;
  template <class F> void each_sync(F&& f) { for (Set& t : set) f(t.sync); for (Sync& y : gsync) f(y); }
  void clear_group() { grp.n = 0; grp_tiles = 0; grp_flops = grp_bytes = 0; dyT_used = 0; }
  static void wait(Launcher& Ln, hipStream_t x, Sync& y, bool clear) {
    if (!y.pending) return;
    if (hipStreamWaitEvent(x, y.done, 0) != hipSuccess) Ln.err = RPR_ERR_HIP;
    if (clear) y.pending = false;
  }
};

struct TrainWs {
  std::vector<DevBuf*> bufs;   // every buffer tensure() has allocated, wherever it lives: what free_train_ws frees
  // saved forward activations
  DevBuf enc_act, dec_act, enc_out, xkv, x_last, scores, margins, dscores, in_idx, out_idx;
  // seq2seq head: the decoder's last hidden state (after the final norm), dlogits of every row, the row losses
  DevBuf hF, dlog, row_loss;
  DevBuf dense_codes;   // dense head: the zero codes the one-position decoder pass is indexed by (it reads none of them)
  // scratch
  DevBuf dmid_ff;   // gated feed-forward only: the W_out product's input gradient [rows, d_ff] (the backward gate kernel's dmid)
  DevBuf h, dxa, dxb, dbig, dattn, dxkv, denc, tA, wT, w_part, bias_part, fix, gn_part, gn_out, amax, part, part2;
  WGradSide side;
  std::vector<hipEvent_t> bucket_ev;   // gradient buckets handed to the caller's communication stream (one event each)
  // bf16 mode: the GEMM weights are converted once per step (plain + transposed copies at the tensors' offsets of the flat
  // parameter layout) instead of once per GEMM call, and the forward pass leaves the transposed bf16 copy of every
  // linear layer's input behind — the X^T operand of its weight-gradient product — so the backward pass neither converts
  // X again nor recomputes the normalised inputs it would only need for that
  DevBuf wc, wcT, wseg, wpref, xT;
  // bf16 mode, round 6: the feed-forward block's wide intermediate leaves its producing GEMM's epilogue in bf16 (rows here, the
  // transposed copy in the consumer's X^T / dY^T slot) instead of through a conversion launch: relu(h Wi^T) in the forward
  // pass, the masked gradient w.r.t. it in the backward pass (GemmH2Args::out_b / out_bt / mask_src)
  DevBuf bfb;
  DevBuf drop_dy;                      // dropout: the masked gradient w.r.t. a sub-block's output, the dY of its W_out products
  DevBuf aseg, apref;                 // rpr_adamw_step: one launch over all tensors (table built once per model)
  const rpr_model* aw_model = nullptr;
  int aw_nseg = 0, aw_chunks = 0;
  const rpr_model* wc_model = nullptr;
  int wc_nseg = 0, wc_tiles = 0;
  std::unordered_map<const float*, size_t> wc_off;
  int amax_next = 0;
  // forward GEMM site (keyed by its weight tensor) -> {amax of its input activations, amax of the weight}: the backward
  // multiplies the same two tensors again (dW = dY^T X, dX = dY W) and reuses both maxima
  std::unordered_map<const float*, float*> site_amax;
  size_t bytes = 0;
};

namespace {

int tensure(rpr_ctx* c, DevBuf& b, size_t bytes) {   // like ensure(), without touching the search graphs
  if (bytes <= b.cap) return 0;
  auto& bufs = c->tws->bufs;
  if (std::find(bufs.begin(), bufs.end(), &b) == bufs.end()) bufs.push_back(&b);
  if (b.p) { RPR_HIP(hipFree(b.p)); c->tws->bytes -= b.cap; b.p = nullptr; b.cap = 0; }
  const size_t want = (bytes + 255) & ~(size_t)255;
  RPR_HIP(hipMalloc(&b.p, want));
  b.cap = want;
  c->tws->bytes += want;
  return 0;
}

// Split-precision training GEMM: both operands are fp32 tensors of unknown magnitude (activations, gradients, weights
// that change every step), so each gets a per-tensor power-of-two scale from its absolute maximum, found on the device
// (no host round trip; slots of a ring that is zeroed once per pass) and undone in the GEMM epilogue.
struct Planes { __half* p; size_t ps; int ld; const float* amax; };
constexpr int AMAX_SLOTS = 8192;
float* amax_slots(rpr_ctx* c, int n) {          // n fresh (zero) slots
  TrainWs& w = *c->tws;
  if (w.amax_next + n > AMAX_SLOTS) return nullptr;
  float* p = P<float>(w.amax) + w.amax_next;
  w.amax_next += n;
  return p;
}
void amax_reset(Launcher& Ln) {
  TrainWs& w = *Ln.c->tws;
  w.amax_next = 0;
  w.site_amax.clear();
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_zero_u64(P<unsigned long long>(w.amax), AMAX_SLOTS / 2, Ln.s); });
}
void gemm_planes(Launcher& Ln, const Planes& A, const Planes& B, float* C, int ldc, int M, int N, int K, const float* resid, int relu,
                 DevBuf* part = nullptr) {
  GemmH2Args g{};
  g.A = A.p; g.a_ps = A.ps; g.lda = A.ld; g.W = B.p; g.w_ps = B.ps; g.ldw = B.ld;
  g.resid = resid; g.ldr = ldc;
  g.out[0] = g.out[1] = g.out[2] = C; g.ldo[0] = g.ldo[1] = g.ldo[2] = ldc; g.split_n = N;
  g.M = M; g.N = N; g.K = K; g.relu = relu; g.acc_scale = 1.0f; g.sat = Ln.c->status;
  g.dyn_a = A.amax; g.dyn_b = B.amax;
  if (!part) part = &Ln.c->tws->part;
  g.part = P<float>(*part); g.part_cap = part->cap / sizeof(float);
  Ln.run(RPR_K_GEMM, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N), [&] { return launch_gemm_h2(g, Ln.s); },
         &g.kernel_cls);
}

// bf16 outputs of the epilogue (256 x 256 kernel only; see GemmH2Args::out_b): rows [M][N], transposed [N][ldt], optional mask
struct BOut { void* rows = nullptr; void* tr = nullptr; int ldt = 0; const float* mask = nullptr; };
// a product whose result may leave its epilogue as bf16 operands: whole 256 x 256 tiles, and as many of them as send a bf16
// product to the ping-pong kernel anyway (launch_gemm_h2: 200) — the fusion never changes which kernel computes the product,
// so the gradients are the conversion launches' bit for bit (RPR_TRAIN_FUSE_FF=0, development builds, selects those).
// Measured, t5-base bz 128 (profiles/r06f_train_fuse_ab.txt): 23.2 -> 22.6 ms per step; the conversion launches of the
// feed-forward blocks were 1.8 ms, the two extra output formats cost the 48 producing launches 0.85 ms of epilogue
// (32 instead of 16 store instructions per lane and strip).
bool fused_ok(const rpr_ctx* c, int M, int N) {
  static const bool on = [] { const char* e = dev_getenv("RPR_TRAIN_FUSE_FF"); return !(e && atoi(e) == 0); }();
  return on && c->precision == RPR_PREC_BF16 && M % 256 == 0 && N % 256 == 0 && (long)(M / 256) * (N / 256) >= 200;
}
void gemm_bf16(Launcher& Ln, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, const float* resid,
               int relu, DevBuf* part = nullptr, const BOut* bo = nullptr) {
  GemmH2Args g{};
  g.A = reinterpret_cast<const __half*>(A); g.lda = lda; g.W = reinterpret_cast<const __half*>(B); g.ldw = ldb;
  g.resid = resid; g.ldr = ldc;
  g.out[0] = g.out[1] = g.out[2] = C; g.ldo[0] = g.ldo[1] = g.ldo[2] = ldc; g.split_n = N;
  g.M = M; g.N = N; g.K = K; g.relu = relu; g.acc_scale = 1.0f; g.bf16 = 1;
  if (bo) { g.out_b = bo->rows; g.ldob = N; g.out_bt = bo->tr; g.ldobt = bo->ldt; g.mask_src = bo->mask; g.ldmask = N; }
  if (!part) part = &Ln.c->tws->part;
  g.part = P<float>(*part); g.part_cap = part->cap / sizeof(float);
  Ln.run(RPR_K_GEMM, 2.0 * M * (double)N * K, 2.0 * ((double)M * K + (double)N * K) + 4.0 * (double)M * N, [&] { return launch_gemm_h2(g, Ln.s); },
         &g.kernel_cls);
}

// C[M, N] = act(A[M, K] B[N, K]^T) (+ resid): exact fp32 MFMA, or (split-precision mode) f16x2 planes with dynamic scales,
// or one bf16 plane per operand, one MFMA per product (RPR_PREC_BF16)
// save_xt (bf16 mode): where to leave the transposed copy [K][pad64(M)] (row stride ldT(M)) of A for the weight-gradient product
// a_ready (bf16 mode): A's bf16 rows — and its transposed copy in save_xt — were written by the epilogue that produced A
void gemm(Launcher& Ln, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
          const float* resid = nullptr, int relu = 0, void* save_xt = nullptr, const void* a_ready = nullptr) {
  if (Ln.c->precision == RPR_PREC_BF16) {
    // the reference's bf16 autocast (main.py:152 bf16=args.use_fp16; tasks/trainer.py:229): operands rounded to bf16, fp32
    // accumulation. One conversion pass per operand, no maxima, no second plane.
    TrainWs& w = *Ln.c->tws;
    if (lda != K || ldb != K) { Ln.err = RPR_ERR_INVALID; return; }
    hipStream_t s = Ln.s;
    const void* ab = a_ready ? a_ready : w.tA.p;
    if (!a_ready && save_xt) Ln.run(RPR_K_OTHER, 0, 8.0 * M * K, [&] { return launch_to_bf16_T(A, M, K, lda, pad64(M), save_xt, w.tA.p, s, nullptr, ldT(M)); });
    else if (!a_ready) Ln.run(RPR_K_OTHER, 0, 6.0 * M * K, [&] { return launch_to_bf16(A, M, K, lda, w.tA.p, s); });
    const void* wb = w.wT.p;
    auto it = w.wc_off.find(B);
    if (it != w.wc_off.end() && w.wc.p) wb = reinterpret_cast<const __half*>(w.wc.p) + it->second;   // converted once per step
    else Ln.run(RPR_K_OTHER, 0, 6.0 * N * K, [&] { return launch_to_bf16(B, N, K, ldb, w.wT.p, s); });
    gemm_bf16(Ln, ab, K, wb, K, C, ldc, M, N, K, resid, relu);
    return;
  }
  if (Ln.c->precision == RPR_PREC_F16X2) {
    TrainWs& w = *Ln.c->tws;
    float* am = amax_slots(Ln.c, 2);
    if (!am || lda != K || ldb != K) { Ln.err = RPR_ERR_INVALID; return; }
    __half *pa = P<__half>(w.tA), *pb = P<__half>(w.wT);
    hipStream_t s = Ln.s;
    Ln.run(RPR_K_OTHER, 0, 4.0 * (M + N) * K, [&] { return launch_absmax2(A, (size_t)M * K, B, (size_t)N * K, am, s); });
    w.site_amax[B] = am;
    Ln.run(RPR_K_OTHER, 0, 8.0 * M * K, [&] { return launch_split_dyn(A, M, K, lda, pa, am, s); });
    Ln.run(RPR_K_OTHER, 0, 8.0 * N * K, [&] { return launch_split_dyn(B, N, K, ldb, pb, am + 1, s); });
    gemm_planes(Ln, {pa, (size_t)M * K, K, am}, {pb, (size_t)N * K, K, am + 1}, C, ldc, M, N, K, resid, relu);
    return;
  }
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = B; g.ldw = ldb; g.resid = resid; g.ldr = ldc;
  g.out[0] = g.out[1] = g.out[2] = C; g.ldo[0] = g.ldo[1] = g.ldo[2] = ldc; g.split_n = N;
  g.M = M; g.N = N; g.K = K; g.relu = relu;
  Ln.run(RPR_K_GEMM, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N), [&] { return launch_gemm(g, Ln.s); });
}

// One stack on the device: its table (train_layout.h) with the buffers the table's offsets index, and what its self-attention
// takes. Sub-block j of layer i reads the stream x(i, j) and writes x(i, j + 1); the last one writes the next layer's input,
// the last layer's x_end.
struct Stack {
  const StackLayout& lay;
  const ParamOrder& po;
  float *act, *x_end;           // saved activations; the stream behind the last layer
  __half* xT;                   // saved X^T operands (bf16 mode); null: nothing is saved (every other mode)
  const int32_t* mask;          // self-attention: key mask (encoder) or none, bias table and buckets, sequences x length, causal?
  const float* rel_bias; const int32_t* bucket;
  int nseq, len, causal;
  float* x(int i, int j) const {
    if (j == lay.nsub) { ++i; j = 0; }
    return i == lay.layers ? x_end : act + lay.act(i, lay.at[j].x);
  }
  float* in(int i, int j) const { return act + lay.act(i, lay.at[j].in); }
  float* mid(int i, int j) const { return act + lay.act(i, lay.at[j].mid); }
  void* xt_in(int i, int j) const { return xT ? xT + lay.xt(i, lay.at[j].xt_in) : nullptr; }
  void* xt_out(int i, int j) const { return xT ? xT + lay.xt(i, lay.at[j].xt_out) : nullptr; }
  const ParamSlot* params(int i, int j) const { return po.sub(lay, i, j); }   // ln, W_in, W_out
};
Stack enc_stack(const rpr_ctx* c, const rpr_model* m, const TrainDims& D, const TrainLayout& Y, const int32_t* mask) {
  TrainWs& w = *c->tws;
  float* act = P<float>(w.enc_act);
  return {Y.enc, m->params, act, act + Y.enc.act(D.ne, 0), c->precision == RPR_PREC_BF16 ? P<__half>(w.xT) : nullptr,
          mask, m->d.enc_rel_bias, m->enc_bucket, D.bz, D.Lq, 0};
}
Stack dec_stack(const rpr_ctx* c, const rpr_model* m, const TrainDims& D, const TrainLayout& Y) {
  TrainWs& w = *c->tws;
  return {Y.dec, m->params, P<float>(w.dec_act), P<float>(w.x_last), c->precision == RPR_PREC_BF16 ? P<__half>(w.xT) : nullptr,
          nullptr, m->d.dec_rel_bias, m->dec_bucket, D.S, D.L, 1};
}

// The dropout of one pass (rpr_set_train_dropout; the mask function and its sites: dropout.h). Off — rate 0, or an entry point
// that stays in evaluation mode — nothing here launches anything and the pass enqueues what it always did. On, every site is
// a small pass of its own over the activation (rows) or a training-only attention kernel (attn); the backward walks the same
// sites and draws the same masks again. The feed-forward block then takes the unfused route (fused_ok hands bf16 operands
// from the inner product's epilogue to the outer product: the mask would have to go into the hot GEMM's epilogue).
struct Drop {
  DropKey key{};
  bool on = false;
  Drop() = default;
  Drop(float rate, uint64_t seed, uint64_t step) : key(drop_key(rate, seed, step)), on(rate > 0.f) {}   // dropout.h
  explicit Drop(const rpr_ctx* c) : Drop(c->train_drop.rate, c->train_drop.seed, c->train_drop.step) {}
  // out = (resid +) mask(x) over the rows [nseq * len][nfeat] of nseq sequences of len positions
  void rows(Launcher& Ln, int nseq, int len, const float* x, const float* resid, float* out, int nfeat, int site) const {
    Ln.run(RPR_K_OTHER, 0, (resid ? 12.0 : 8.0) * nseq * len * nfeat,
           [&] { return launch_dropout_rows(x, resid, out, (size_t)nseq, len, nfeat, key, site, Ln.s); });
  }
  void rows(Launcher& Ln, const Stack& k, const float* x, const float* resid, float* out, int nfeat, int site) const {
    rows(Ln, k.nseq, k.len, x, resid, out, nfeat, site);
  }
  DropAttn attn(int site, int L) const { return drop_attn(key, site, L); }
};

// bf16 copies of every GEMM weight, refreshed at the start of each pass (the weights change between passes: AdamW, or the
// caller writing through rpr_param_info's pointers). The table of tensors is built once per model.
int refresh_weight_cache(Launcher& Ln, rpr_ctx* c, rpr_model* m) {
  TrainWs& w = *c->tws;
  if (w.wc_model != m) {
    std::vector<WSeg> segs;
    std::vector<int> pref;
    w.wc_off.clear();
    int tiles = 0;
    auto add = [&](const ParamSlot& p, int R, int C) {
      if ((R & 1) || (C & 3)) return;
      segs.push_back(WSeg{p.ptr, R, C, (unsigned long long)p.offset});
      pref.push_back(tiles);
      tiles += ((R + 63) / 64) * ((C + 63) / 64);
      w.wc_off[p.ptr] = p.offset;
    };
    const auto& d = m->d;
    auto add_stack = [&](const StackLayout& st) {   // W_in [n_in][d_model] and W_out [d_model][k_out] of every sub-block
      for (int i = 0; i < st.layers; ++i)
        for (int j = 0; j < st.nsub; ++j) {
          const ParamSlot* p = m->params.sub(st, i, j);
          add(p[P_WIN], st.sub[j].n_in, st.dm); add(p[P_WOUT], st.dm, st.sub[j].k_out);
        }
    };
    add_stack(m->params.stack[0]);
    add(m->params.at(K_XKV), d.num_decoder_layers * 2 * m->inner(), d.d_model);
    add_stack(m->params.stack[1]);
    int e = tensure(c, w.wseg, segs.size() * sizeof(WSeg));
    if (!e) e = tensure(c, w.wpref, pref.size() * sizeof(int));
    if (!e) e = tensure(c, w.wc, m->params.total * sizeof(__half));
    if (!e) e = tensure(c, w.wcT, m->params.total * sizeof(__half));
    if (e) { w.wc_off.clear(); return e; }
    RPR_HIP(hipMemcpyAsync(w.wseg.p, segs.data(), segs.size() * sizeof(WSeg), hipMemcpyHostToDevice, Ln.s));
    RPR_HIP(hipMemcpyAsync(w.wpref.p, pref.data(), pref.size() * sizeof(int), hipMemcpyHostToDevice, Ln.s));
    RPR_HIP(hipStreamSynchronize(Ln.s));              // the host vectors go out of scope
    w.wc_model = m; w.wc_nseg = (int)segs.size(); w.wc_tiles = tiles;
  }
  Ln.run(RPR_K_OTHER, 0, 8.0 * (double)m->params.total, [&] {
    return launch_weights_bf16(P<WSeg>(w.wseg), P<int>(w.wpref), w.wc_nseg, w.wc_tiles, w.wc.p, w.wcT.p, Ln.s);
  });
  return Ln.err;
}

struct Bwd {
  Launcher& Ln; rpr_ctx* c; TrainWs& w; const TrainDims& D;
  // dX[M, K] = dY[M, N] W[N, K]  and  dW[N, K] = dY[M, N]^T X[M, K]  (dX may alias X: X is consumed first); dX on the main
  // stream, dW on the side stream (w.side) except in f32 mode
  // relu_act (bf16 mode only): dY is the gradient w.r.t. relu(.) and relu_act the stored activation; the mask is applied
  // while dY is converted (the caller skips launch_relu_bwd)
  // fuse_mask (bf16 mode, grouped route): dX is only read by the NEXT dxdw call, as its dY with relu_act = fuse_mask (the
  // feed-forward block: dX = gradient w.r.t. relu(.), [M, K]); when the shapes allow it the dX product's epilogue writes that
  // dY's bf16 rows and transposed copy itself (masked), no fp32 dX is written, and the next call finds them left with w.side
  void dxdw(const float* dY, const float* W, const float* X, float* dX, float* dW, int M, int N, int K, const void* saved_xt = nullptr,
            const float* relu_act = nullptr, const float* fuse_mask = nullptr) {
    if (Ln.err) return;
    if (c->precision == RPR_PREC_BF16) dxdw_bf16(dY, W, X, dX, dW, M, N, K, saved_xt, relu_act, fuse_mask);
    else if (c->precision == RPR_PREC_F16X2) dxdw_f16x2(dY, W, X, dX, dW, M, N, K);
    else dxdw_f32(dY, W, X, dX, dW, M, N, K);
  }
  // bf16 operands (see gemm()): one read of dY gives its plain and its transposed copy. The weight gradients of a layer go out
  // as one grouped launch where the shapes allow it, else product by product.
  void dxdw_bf16(const float* dY, const float* W, const float* X, float* dX, float* dW, int M, int N, int K, const void* saved_xt,
                 const float* relu_act, const float* fuse_mask) {
    WGradSide& sd = w.side;
    hipStream_t s = Ln.s;
    // Mk: the reduction length of the dW product (the rows; the bf16 kernel walks K in tiles of 64); Ml: the row stride of the
    // transposed operands that have a slot of their own (saved X^T, grouped dY^T)
    const int Mk = pad64(M), Ml = ldT(M);
    const auto wit = w.wc_off.find(W);
    const bool cached = wit != w.wc_off.end() && w.wcT.p;   // W^T was converted once per step
    const void* wT_cached = cached ? reinterpret_cast<const __half*>(w.wcT.p) + wit->second : nullptr;
    const size_t slot = WGradSide::slot_bytes(N, Ml);
    // the route, decided once. PRE: the previous call's dX product left this dY converted, rows + transposed copy in the group's
    // set (the room was checked when the slot was reserved); JOIN: convert into the group being collected; FLUSH_JOIN: send
    // that group off and start the next with this product; SINGLE: no group can take it (no saved X^T, no cached W^T, more
    // tiles or a larger dY^T than a group holds)
    enum { PRE, JOIN, FLUSH_JOIN, SINGLE } route = SINGLE;
    if (sd.pre_is(dY) && saved_xt && cached) route = PRE;
    else if (sd.pre_left()) { Ln.err = RPR_ERR_INVALID; set_error("dxdw: a pre-converted gradient was not consumed by the next product"); return; }
    else if (saved_xt && cached) {
      const WGradSide::Fit f = sd.fit(N, K, Mk, slot);
      route = f == WGradSide::FIT_OPEN ? JOIN : f == WGradSide::FIT_EMPTY ? FLUSH_JOIN : SINGLE;
    }
    if (route == FLUSH_JOIN || route == SINGLE) sd.flush(Ln);   // (SINGLE: keep the order of the side stream's work)
    if (Ln.err) return;
    if (route == SINGLE) {
      WGradSide::Set& t = sd.next_set(Ln);
      if (Ln.err) return;
      void *py = w.tA.p, *pyt = t.tY.p;
      const void *pxt = t.tX.p, *pwt = w.wT.p;
      Ln.run(RPR_K_OTHER, 0, (relu_act ? 12.0 : 8.0) * M * N, [&] { return launch_to_bf16_T(dY, M, N, N, Mk, pyt, py, s, relu_act); });
      if (saved_xt) pxt = saved_xt;                       // left behind by the forward pass
      else Ln.run(RPR_K_OTHER, 0, 6.0 * M * K, [&] { return launch_to_bf16_T(X, M, K, K, Mk, t.tX.p, nullptr, s); });
      if (cached) pwt = wT_cached;
      else Ln.run(RPR_K_OTHER, 0, 6.0 * N * K, [&] { return launch_to_bf16_T(W, N, K, K, N, w.wT.p, nullptr, s); });
      sd.run(Ln, t.sync, [&](Launcher& L2) { gemm_bf16(L2, pyt, Mk, pxt, saved_xt ? Ml : Mk, dW, K, N, K, Mk, nullptr, 0, &w.part2); });
      if (Ln.err) return;
      gemm_bf16(Ln, py, N, pwt, N, dX, K, M, K, N, nullptr, 0);
      return;
    }
    // grouped route: dY^T into this layer's set, the product into the group, dX on the main stream at once
    const void* py = w.tA.p;
    __half* pyt;
    if (route == PRE) { const WGradSide::Pre p = sd.take_pre(); py = p.py; pyt = p.pyt; }
    else {
      pyt = sd.reserve(slot);
      void* pyw = w.tA.p;
      Ln.run(RPR_K_OTHER, 0, (relu_act ? 12.0 : 8.0) * M * N, [&] { return launch_to_bf16_T(dY, M, N, N, Mk, pyt, pyw, s, relu_act, Ml); });
    }
    sd.add(pyt, saved_xt, dW, N, K, Mk, Ml);
    // the next product (dY = this dX, [M, K]) joins the same group: its dY^T slot is reserved now and this product's epilogue
    // fills it, with the rows for its dX product beside it. (The next product is dW2[K, N2]; N2 is not known here: its tiles
    // are bound by this one's N.)
    const size_t slot2 = WGradSide::slot_bytes(K, Ml);
    if (fuse_mask && fused_ok(c, M, K) && Mk == M && w.bfb.p && w.bfb.cap >= (size_t)M * K * sizeof(__half) &&
        sd.fit(K, N, Mk, slot2) == WGradSide::FIT_OPEN) {
      __half* pyt2 = sd.reserve(slot2);
      const BOut bo{w.bfb.p, pyt2, Ml, fuse_mask};
      gemm_bf16(Ln, py, N, wT_cached, N, nullptr, K, M, K, N, nullptr, 0, nullptr, &bo);
      sd.leave_pre(dX, w.bfb.p, pyt2);
      return;
    }
    gemm_bf16(Ln, py, N, wT_cached, N, dX, K, M, K, N, nullptr, 0);
  }
  // one read of dY gives its plain planes (for dX) and its transposed planes (for dW); W is transposed straight from the
  // fp32 weight. Mp: the reduction length of the dW product (the split kernel walks K in tiles of 32)
  void dxdw_f16x2(const float* dY, const float* W, const float* X, float* dX, float* dW, int M, int N, int K) {
    hipStream_t s = Ln.s;
    const int Mp = pad32(M);
    float* am = amax_slots(c, 3);
    if (!am) { Ln.err = RPR_ERR_INVALID; return; }
    WGradSide::Set& t = w.side.next_set(Ln);
    if (Ln.err) return;
    __half *py = P<__half>(w.tA), *pyt = P<__half>(t.tY), *pxt = P<__half>(t.tX), *pwt = P<__half>(w.wT);
    const float *am_x = am + 2, *am_w = am + 1;
    auto site = w.site_amax.find(W);
    if (site != w.site_amax.end()) {   // X and W are the forward GEMM's operands: their maxima are known
      am_x = site->second; am_w = site->second + 1;
      Ln.run(RPR_K_OTHER, 0, 4.0 * M * N, [&] { return launch_absmax2(dY, (size_t)M * N, nullptr, 0, am, s); });
    } else {
      Ln.run(RPR_K_OTHER, 0, 4.0 * M * N + 4.0 * N * K, [&] { return launch_absmax2(dY, (size_t)M * N, W, (size_t)N * K, am, s); });
      Ln.run(RPR_K_OTHER, 0, 4.0 * M * K, [&] { return launch_absmax2(X, (size_t)M * K, nullptr, 0, am + 2, s); });
    }
    Ln.run(RPR_K_OTHER, 0, 12.0 * M * N, [&] { return launch_split_dyn_T(dY, M, N, N, Mp, pyt, py, am, s); });
    Ln.run(RPR_K_OTHER, 0, 8.0 * M * K, [&] { return launch_split_dyn_T(X, M, K, K, Mp, pxt, nullptr, am_x, s); });
    Ln.run(RPR_K_OTHER, 0, 8.0 * N * K, [&] { return launch_split_dyn_T(W, N, K, K, N, pwt, nullptr, am_w, s); });
    w.side.run(Ln, t.sync, [&](Launcher& L2) {
      gemm_planes(L2, {pyt, (size_t)N * Mp, Mp, am}, {pxt, (size_t)K * Mp, Mp, am_x}, dW, K, N, K, Mp, nullptr, 0, &w.part2);
    });
    if (Ln.err) return;
    gemm_planes(Ln, {py, (size_t)M * N, N, am}, {pwt, (size_t)K * N, N, am_w}, dX, K, M, K, N, nullptr, 0);
  }
  void dxdw_f32(const float* dY, const float* W, const float* X, float* dX, float* dW, int M, int N, int K) {   // both on the main stream
    hipStream_t s = Ln.s;
    const int Mp = pad32(M);
    float* xT = w.side.main_stream_scratch();
    Ln.run(RPR_K_OTHER, 0, 8.0 * M * N, [&] { return launch_transpose_pad(dY, P<float>(w.tA), M, N, N, Mp, s); });
    Ln.run(RPR_K_OTHER, 0, 8.0 * M * K, [&] { return launch_transpose_pad(X, xT, M, K, K, Mp, s); });
    gemm(Ln, P<float>(w.tA), Mp, xT, Mp, dW, K, N, K, Mp);
    Ln.run(RPR_K_OTHER, 0, 8.0 * N * K, [&] { return launch_transpose_pad(W, P<float>(w.wT), N, K, K, N, s); });
    gemm(Ln, dY, N, P<float>(w.wT), N, dX, K, M, K, N);
  }
  void norm(const float* x, const float* ln, int rows, float post = 1.0f) {   // recompute the normalised input into w.h
    Ln.run(RPR_K_RMSNORM, 0, 8.0 * rows * D.dm, [&] { return launch_rmsnorm(x, ln, P<float>(w.h), rows, D.dm, D.eps, Ln.s, post); });
  }
  // The layer-norm weight gradient of a site is the column sum of its blocks' partials: the sites of a layer keep their
  // partials in separate regions of w_part and are summed by ONE launch at the end of the layer (flush_norms; 62 launches
  // of 10 us per step before)
  ColsumSites cs = {};
  void norm_bwd(const float* x, const float* ln, const float* dh, const float* dres, float* dx_out, float* dln, int rows,
                float post = 1.0f) {
    if (cs.n == ColsumSites::MAXS) flush_norms();
    const size_t region = ((size_t)(std::max(D.R, D.T) + 3) / 4) * D.dm;
    float* part = P<float>(w.w_part) + (size_t)cs.n * region;
    Ln.run(RPR_K_RMSNORM, 0, 16.0 * rows * D.dm, [&] {
      return launch_rmsnorm_bwd(x, ln, dh, dres, dx_out, part, nullptr, rows, D.dm, D.eps, post, 0, Ln.s);
    });
    cs.part[cs.n] = part; cs.out[cs.n] = dln; cs.nparts[cs.n] = rmsnorm_bwd_parts(rows); ++cs.n;
  }
  void flush_norms() {
    if (cs.n == 0 || Ln.err) return;
    const ColsumSites p = cs;
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_colsum_multi(p, D.dm, Ln.s); });
    cs.n = 0;
  }
};

// What follows the decoder stream: the ranking step's gold-code scores, the seq2seq cross-entropy head, or the dense first
// stage's dot products of the query and document representations (dense_head.hip)
enum Head { HEAD_GOLD, HEAD_CE, HEAD_DENSE };

int alloc_train(rpr_ctx* c, const rpr_model* m, const TrainDims& D, Head head) {
  if (!c->tws) c->tws = new TrainWs();
  TrainWs& w = *c->tws;
  const size_t f = sizeof(float), R = D.R, T = D.T, dm = D.dm, inner = D.inner, dff = D.dff;
  const size_t rows = std::max(R, T), rp = ((int)rows + 63) & ~63;   // rows padded to the K-tile of the bf16 kernel (64) / the split kernel (32)
  const size_t ffin = D.ff_in(), wide = std::max<size_t>(std::max<size_t>(ffin, 3 * inner), (size_t)D.xld);
  int e = 0;
  auto E = [&](DevBuf& b, size_t bytes) { if (!e) e = tensure(c, b, bytes); };
  const TrainLayout Y(D);
  E(w.enc_act, (size_t)D.ne * Y.enc.act_stride * f + T * dm * f);     // + the encoder's last stream
  E(w.dec_act, (size_t)D.nd * Y.dec.act_stride * f);
  E(w.enc_out, T * dm * f); E(w.xkv, T * (size_t)D.xld * f); E(w.x_last, R * dm * f);
  E(w.scores, R * f); E(w.margins, 8 * (size_t)D.bz * f); E(w.dscores, R * f);
  E(w.in_idx, R * 4); E(w.out_idx, R * 4);
  if (head == HEAD_CE) { E(w.hF, R * dm * f); E(w.dlog, R * (size_t)D.V * f); E(w.row_loss, R * f); }   // the seq2seq head
  if (head == HEAD_DENSE) { E(w.hF, R * dm * f); E(w.dense_codes, R * 4); }   // the dense head: dhF goes to dxa (rows x d_model, below)
  if (c->train_drop.rate > 0.f) { E(w.hF, R * dm * f); E(w.drop_dy, rows * dm * f); }   // dropout: the ranking step keeps hF too
  E(w.h, rows * dm * f); E(w.dxa, rows * dm * f); E(w.dxb, rows * dm * f); E(w.dbig, rows * wide * f);
  if (D.gated) E(w.dmid_ff, rows * dff * f);
  E(w.dattn, rows * inner * f); E(w.dxkv, T * (size_t)D.xld * f); E(w.denc, T * dm * f);
  E(w.tA, wide * rp * f);
  // grouped weight gradients (bf16 mode): dY^T of one layer's products, [N_out][pad64(rows)] bf16 each, 256-byte aligned
  const bool bf16 = c->precision == RPR_PREC_BF16;
  if (!e) e = w.side.create(c, wide * rp * f, bf16 ? Y.dyT_max() * sizeof(__half) + 8 * 256 : 0);
  if (bf16) { E(w.xT, Y.xt_total * sizeof(__half)); E(w.bfb, rp * dff * sizeof(__half)); }
  E(w.wT, std::max<size_t>(std::max<size_t>(ffin * dm, 3 * inner * dm), (size_t)D.xld * dm) * f);
  E(w.w_part, ColsumSites::MAXS * ((rows + 3) / 4) * dm * f);   // the partials of up to four norm sites (Bwd::norm_bwd)
  E(w.bias_part, std::max<size_t>((size_t)D.S, (size_t)D.bz) * D.H * D.buckets * f);
  E(w.fix, std::max<size_t>((size_t)m->d.vocab_size, (size_t)m->d.L * D.V) * dm * 8);
  E(w.gn_part, 1024 * 8); E(w.gn_out, 16); E(w.amax, AMAX_SLOTS * f); E(w.part, (size_t)16 << 20 << 2); E(w.part2, (size_t)16 << 20 << 2);   // split-K partials: 16 M floats per stream
  return e;
}

// gold: end with the gold-code scores of the ranking step (w.scores); else the decoder stream is left in w.x_last for the
// seq2seq head
void forward(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const TrainDims& D, const int32_t* ids, const int32_t* mask,
             const int32_t* codes, int32_t* last, const Drop& drop, bool gold = true) {
  TrainWs& w = *c->tws;
  const auto& d = m->d;
  hipStream_t s = Ln.s;
  const int T = D.T, R = D.R, dm = D.dm, inner = D.inner;
  float* h = P<float>(w.h);
  auto norm = [&](const float* x, const float* ln, float* out, int rows, float post = 1.0f) {
    Ln.run(RPR_K_RMSNORM, 0, 8.0 * rows * dm, [&] { return launch_rmsnorm(x, ln, out, rows, dm, D.eps, s, post); });
  };
  // out = act(norm(x) W^T): in bf16 mode the norm writes the product's bf16 operand and its transposed copy itself
  // (rmsnorm_bf16_T_kernel); otherwise norm into h, then gemm() converts.
  // next_xt: where the NEXT product (the one that reads C) wants C's transposed bf16 copy; when the shapes allow it (fused_ok)
  // this product's epilogue writes it, and C's bf16 rows into w.bfb: returns those rows (the next gemm()'s a_ready) or null
  auto norm_gemm = [&](const float* x, const float* ln, const float* W, float* C, int rows, int N, int relu, void* save_xt,
                       void* next_xt = nullptr) -> const void* {
    auto it = w.wc_off.find(W);
    if (c->precision == RPR_PREC_BF16 && save_xt && it != w.wc_off.end() && w.wc.p && dm <= 1024 && (dm & 63) == 0) {
      Ln.run(RPR_K_RMSNORM, 0, 8.0 * rows * dm, [&] {
        return launch_rmsnorm_bf16_T(x, ln, rows, dm, D.eps, 1.0f, w.tA.p, save_xt, pad64(rows), ldT(rows), s);
      });
      const bool fuse = next_xt && fused_ok(c, rows, N) && w.bfb.p && w.bfb.cap >= (size_t)rows * N * sizeof(__half) && pad64(rows) == rows;
      const BOut bo{w.bfb.p, next_xt, ldT(rows), nullptr};
      gemm_bf16(Ln, w.tA.p, dm, reinterpret_cast<const __half*>(w.wc.p) + it->second, dm, C, N, rows, N, dm, nullptr, relu, nullptr,
                fuse ? &bo : nullptr);
      return fuse ? w.bfb.p : nullptr;
    }
    norm(x, ln, h, rows);
    gemm(Ln, h, dm, W, dm, C, N, rows, N, dm, nullptr, relu, save_xt);
    return nullptr;
  };
  // y = x + mid(norm(x, ln) W_in^T) W_out^T, everything the backward needs kept. Only the middle op differs by kind; the FF
  // block hands its inner product's bf16 operands to the outer one (next_xt / a_ready)
  auto sub_fwd = [&](const Stack& k, int i, int j) {
    const SubBlock& b = k.lay.sub[j];
    const ParamSlot* p = k.params(i, j);
    const int rows = k.lay.rows;
    const bool ff = b.kind == SUB_FF && !D.gated;   // the ReLU FF: activation and operand hand-over in the inner product's epilogue
    float *x = k.x(i, j), *in = k.in(i, j), *mid = k.mid(i, j);
    const void* ready = norm_gemm(x, p[P_LN].ptr, p[P_WIN].ptr, in, rows, b.n_in, ff, k.xt_in(i, j), ff && !drop.on ? k.xt_out(i, j) : nullptr);
    const int site_mid = drop_site_mid(k.lay.dec, i, j);
    switch (b.kind) {
      case SUB_SELF: {
        if (drop.on) {
          Ln.run(RPR_K_ENC_ATTN, 0, 0, [&] {
            return launch_self_attn_drop_fwd(in, k.mask, k.rel_bias, k.bucket, mid, k.nseq, k.len, D.H, d.rel_buckets, k.causal,
                                             drop.attn(site_mid, k.len), s, d.d_kv);
          });
          break;
        }
        EncAttnArgs sa{in, k.mask, k.rel_bias, k.bucket, mid, k.nseq, k.len, D.H, d.rel_buckets, nullptr, 0, nullptr, nullptr, nullptr,
                       k.causal, 1, d.d_kv};
        Ln.run(RPR_K_ENC_ATTN, 0, 0, [&] { return launch_enc_attn(sa, s); });
        break;
      }
      case SUB_CROSS: {
        const float* xk = P<float>(w.xkv) + (size_t)i * 2 * inner;
        if (drop.on) {
          Ln.run(RPR_K_DEC_CROSS_ATTN, 0, 0, [&] {
            return launch_cross_attn_drop_fwd(in, xk, xk + inner, D.xld, mask, mid, D.bz, D.docs * D.L, D.Lq, D.H, drop.attn(site_mid, D.L), s,
                                              d.d_kv);
          });
          break;
        }
        DecCrossAttnArgs ca{in, xk, xk + inner, D.xld, mask, mid, D.bz, D.docs * D.L, D.H, D.Lq, nullptr, 0, last, nullptr, 0, nullptr,
                            nullptr, d.d_kv};
        // (the query's docs L decoder rows as 32-row tiles on the fp32-MFMA kernel of the search tail when Lq <= 64; 128-dim
        // heads: the block kernel)
        Ln.run(RPR_K_DEC_CROSS_ATTN, 0, 0, [&] { return launch_tail_cross_attn(ca, s); });
        break;
      }
      case SUB_FF:
        if (D.gated) {   // in = (g | u) stays as the product left it; mid = gelu_new(g) * u, and the dropout masks that product
          Ln.run(RPR_K_OTHER, 8.0 * rows * b.k_out, 12.0 * rows * b.k_out,
                 [&] { return launch_gated_gelu(in, rows, b.k_out, nullptr, mid, nullptr, 0, nullptr, s); });
          if (drop.on) drop.rows(Ln, k, mid, nullptr, mid, b.k_out, site_mid);
          break;
        }
        // the ReLU ran in the inner product's epilogue
        if (drop.on) drop.rows(Ln, k, in, nullptr, in, b.n_in, site_mid);
        break;
    }
    float* y = k.x(i, j + 1);
    gemm(Ln, mid, b.k_out, p[P_WOUT].ptr, b.k_out, y, dm, rows, dm, b.k_out, drop.on ? nullptr : x, 0, k.xt_out(i, j), ready);
    if (drop.on) drop.rows(Ln, k, y, x, y, dm, drop_site_sub_out(k.lay.dec, i, j));   // y = x + dropout(mid W_out^T)
  };
  auto stack_in = [&](const Stack& k) { if (drop.on) drop.rows(Ln, k, k.x(0, 0), nullptr, k.x(0, 0), dm, drop_site_input(k.lay.dec)); };
  auto stack_fwd = [&](const Stack& k) {
    for (int i = 0; i < k.lay.layers; ++i)
      for (int j = 0; j < k.lay.nsub; ++j) sub_fwd(k, i, j);
  };
  const TrainLayout Y(D);
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_mask_lengths(mask, last, D.bz, D.Lq, s, c->status + 1); });
  // ---- encoder over the padded [bz, Lq] layout (padded positions get no gradient: nothing downstream reads them)
  const Stack enc = enc_stack(c, m, D, Y, mask);
  Ln.run(RPR_K_OTHER, 0, 8.0 * T * dm, [&] { return launch_embed_rows(d.shared, ids, enc.x(0, 0), T, dm, d.vocab_size, s); });
  stack_in(enc);
  stack_fwd(enc);
  norm(enc.x_end, d.enc_final_ln, P<float>(w.enc_out), T);
  if (drop.on) drop.rows(Ln, enc, P<float>(w.enc_out), nullptr, P<float>(w.enc_out), dm, drop_site_output(0));
  gemm(Ln, P<float>(w.enc_out), dm, d.dec_xkv, dm, P<float>(w.xkv), D.xld, T, D.xld, dm, nullptr, 0, enc.xT ? enc.xT + Y.xt_xkv : nullptr);
  // ---- teacher-forced decoder over all positions of every smtid (ranking step: the positive and the negative)
  const Stack dec = dec_stack(c, m, D, Y);
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_train_indices(codes, P<int32_t>(w.in_idx), P<int32_t>(w.out_idx), D.S, D.L, D.V, s); });
  Ln.run(RPR_K_OTHER, 0, 8.0 * R * dm, [&] { return launch_train_dec_embed(d.start_embed, d.in_embeds, codes, dec.x(0, 0), D.S, D.L, dm, D.V, s); });
  stack_in(dec);
  stack_fwd(dec);
  if (!gold) return;
  if (drop.on) {   // hF = dropout(final norm) by its own launches, then the scores from it (gold_score_kernel fuses norm and score)
    norm(P<float>(w.x_last), d.dec_final_ln, P<float>(w.hF), R, D.post);
    drop.rows(Ln, dec, P<float>(w.hF), nullptr, P<float>(w.hF), dm, drop_site_output(1));
    Ln.run(RPR_K_OTHER, 0, 0, [&] {
      return launch_gold_rowdot(P<float>(w.hF), d.out_embeds, P<int32_t>(w.out_idx), P<float>(w.scores), nullptr, nullptr, nullptr, R, dm, s);
    });
    return;
  }
  Ln.run(RPR_K_OTHER, 0, 0, [&] {
    return launch_gold_scores(P<float>(w.x_last), d.dec_final_ln, d.out_embeds, codes, P<float>(w.scores), D.S, D.L, dm, D.V, D.eps,
                              D.post, s);
  });
}

// The seq2seq head after forward(gold = false): hF = the final RMSNorm of the decoder stream (times d^-0.5 under
// scaleup_output_hidden), then logits, log-softmax, cross-entropy and dlogits (train_kernels.hip, exact fp32 in every mode)
void s2s_head_forward(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const TrainDims& D, const int32_t* labels, float* out_loss,
                      float* out_label_lp, const Drop& drop) {
  TrainWs& w = *c->tws;
  const auto& d = m->d;
  hipStream_t s = Ln.s;
  Ln.run(RPR_K_RMSNORM, 0, 8.0 * D.R * D.dm, [&] {
    return launch_rmsnorm(P<float>(w.x_last), d.dec_final_ln, P<float>(w.hF), D.R, D.dm, D.eps, s, D.post);
  });
  if (drop.on) drop.rows(Ln, D.S, D.L, P<float>(w.hF), nullptr, P<float>(w.hF), D.dm, drop_site_output(1));
  Ln.run(RPR_K_OTHER, 2.0 * D.R * (double)D.V * D.dm, 4.0 * ((double)D.R * D.dm + (double)D.L * D.V * D.dm + (double)D.R * D.V), [&] {
    return launch_s2s_head_fwd(P<float>(w.hF), d.out_embeds, labels, P<float>(w.dlog), P<float>(w.row_loss), out_label_lp, out_loss,
                               D.bz, D.L, D.dm, D.V, s);
  });
}

// Gradient buckets for the data-parallel exchange (reference: DDP's bucketed all-reduce overlapped with the backward pass,
// tasks/trainer.py:486 wraps the model in DistributedDataParallel): one bucket per transformer layer — its nine (six)
// tensors are contiguous in the flat buffer — handed over the moment the layer's last gradient kernel has been ENQUEUED,
// plus one for everything that is only final at the end (embeddings, codebooks, cross K/V, final norms, bias tables).
// "Handed over" = the caller's communication stream is made to wait for the layer's producers on the main stream and on
// the weight-gradient side stream, then the host callback runs: it enqueues the bucket's all-reduce on that stream, where
// it overlaps the rest of the backward pass.
struct BucketHook {
  rpr_grad_bucket_cb cb; void* user; hipStream_t comm; int next = 0;
};

// head: HEAD_CE, the seq2seq cross-entropy head (s2s_head_forward ran) instead of the ranking step's gold scores; HEAD_DENSE, the
// dense head (dense_head_forward ran): dhF comes from the margins it kept, no codebook is touched
void backward(Launcher& Ln, rpr_ctx* c, rpr_model* m, const TrainDims& D, const int32_t* ids, const int32_t* mask, float* G,
              const Drop& drop, BucketHook* hook = nullptr, Head head = HEAD_GOLD) {
  TrainWs& w = *c->tws;
  const auto& d = m->d;
  hipStream_t s = Ln.s;
  auto bucket = [&](size_t off, size_t numel) {
    if (!hook || !hook->cb || Ln.err) return;
    while ((int)w.bucket_ev.size() <= hook->next) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { Ln.err = RPR_ERR_HIP; return; }
      w.bucket_ev.push_back(e);
    }
    hipEvent_t e0 = w.bucket_ev[(size_t)hook->next++];
    if (hipEventRecord(e0, s) != hipSuccess || hipStreamWaitEvent(hook->comm, e0, 0) != hipSuccess) { Ln.err = RPR_ERR_HIP; return; }
    // ... and for the weight gradients in flight on the side stream; the marks stay for the end-of-pass join
    w.side.wait_products(Ln, hook->comm, false);
    w.side.wait_groups(Ln, hook->comm, false);
    if (Ln.err) return;
    hook->cb(hook->user, (int64_t)off, (int64_t)numel);
  };
  const int T = D.T, R = D.R, dm = D.dm, inner = D.inner, H = D.H;
  w.side.reset();
  Bwd B{Ln, c, w, D};
  const TrainLayout Y(D);
  const Stack enc = enc_stack(c, m, D, Y, mask), dec = dec_stack(c, m, D, Y);
  const bool bf16 = c->precision == RPR_PREC_BF16;   // ReLU backward folded into the conversion of its result (dxdw)
  const bool saved = bf16;   // X^T kept by the forward: the normalised inputs are only recomputed for their weight-gradient products
  auto g = [&](int kind, int layer = -1) { return G + m->params.at(kind, layer).offset; };
  float *dxa = P<float>(w.dxa), *dxb = P<float>(w.dxb), *dbig = P<float>(w.dbig), *dattn = P<float>(w.dattn), *h = P<float>(w.h);
  unsigned long long* fix = P<unsigned long long>(w.fix);

  float* g_out = d.out_embeds != d.in_embeds ? g(K_OUT_EMB) : g(K_IN_EMB);
  if (head == HEAD_DENSE) {
    // ---- dense head: dhF = (g (d+ - d-) | g q | -g q) from the hF the forward kept -> final RMSNorm backward
    Ln.run(RPR_K_OTHER, 0, 24.0 * R * dm, [&] { return launch_dense_mse_head_bwd(P<float>(w.hF), P<float>(w.dscores), dxa, D.bz / 3, dm, s); });
  } else if (head == HEAD_CE) {
    // ---- cross-entropy head: dhF_i = dlogits_i E_i -> dxa, dE_i = dlogits_i^T hF_i stored into the codebook gradient (the
    // flat buffer is zero; with shared codebooks the input-embedding rows are added to it later) -> final RMSNorm backward
    Ln.run(RPR_K_OTHER, 4.0 * R * (double)D.V * dm, 4.0 * (2.0 * R * D.V + 2.0 * R * dm + 2.0 * (double)D.L * D.V * dm), [&] {
      return launch_s2s_head_bwd(P<float>(w.hF), d.out_embeds, P<float>(w.dlog), dxa, g_out, D.bz, D.L, dm, D.V, s);
    });
  } else {
    // ---- gold scores: dscore -> (dE rows, dhF) -> final RMSNorm backward
    Ln.run(RPR_K_OTHER, 0, 0, [&] {   // dE rows go to dxb, dhF to dxa
      if (drop.on)   // from the dropped-out hF the forward kept
        return launch_gold_rowdot(P<float>(w.hF), d.out_embeds, P<int32_t>(w.out_idx), nullptr, P<float>(w.dscores), dxa, dxb, R, dm, s);
      return launch_gold_score_bwd(P<float>(w.x_last), d.dec_final_ln, d.out_embeds, P<int32_t>(w.out_idx), P<float>(w.dscores), dxa, dxb,
                                   R, dm, D.eps, D.post, s);
    });
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_scatter_rows_fix(dxb, P<int32_t>(w.out_idx), fix, R, dm, s); });
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_fix_flush(fix, g_out, (size_t)d.L * D.V * dm, s); });
  }
  if (drop.on) drop.rows(Ln, dec, dxa, nullptr, dxa, dm, drop_site_output(1));
  B.norm_bwd(P<float>(w.x_last), d.dec_final_ln, dxa, nullptr, dxb, g(K_DEC_FLN), R, D.post);
  float *dx = dxb, *dx2 = dxa;   // dx = gradient w.r.t. the current sub-block's output stream, dx2 the buffer its input's goes to
  // y = x + mid(norm(x, ln) W_in^T) W_out^T backwards: dxdw of W_out -> the middle op's backward, into dbig -> (the norm again
  // when nothing was saved) -> dxdw of W_in into h (free by now) -> norm_bwd adds the residual path: dx2 = gradient w.r.t. x
  auto sub_bwd = [&](const Stack& k, int i, int j) {
    const SubBlock& b = k.lay.sub[j];
    const ParamSlot* p = k.params(i, j);
    const int rows = k.lay.rows;
    float *x = k.x(i, j), *in = k.in(i, j);
    const bool gated = b.kind == SUB_FF && D.gated;
    const float* relu = b.kind == SUB_FF && bf16 && !gated ? in : nullptr;   // ReLU FF: in = relu(norm(x) Wi^T), the mask of its own gradient
    float* dmid = gated ? P<float>(w.dmid_ff) : b.kind == SUB_FF ? dbig : dattn;
    // dropout: the W_out products see the masked dx, the residual path (norm_bwd below) the whole of it; the dropped-out `in` of
    // the FF block is positive exactly where its ReLU passed AND the element was kept, so it still gates its own gradient
    const int site_mid = drop_site_mid(k.lay.dec, i, j);
    const DropAttn da = drop.attn(site_mid, k.lay.dec && b.kind == SUB_CROSS ? D.L : k.len);
    const float* dy = dx;
    if (drop.on) { dy = P<float>(w.drop_dy); drop.rows(Ln, k, dx, nullptr, P<float>(w.drop_dy), dm, drop_site_sub_out(k.lay.dec, i, j)); }
    B.dxdw(dy, p[P_WOUT].ptr, k.mid(i, j), dmid, G + p[P_WOUT].offset, rows, dm, b.k_out, k.xt_out(i, j), nullptr, drop.on ? nullptr : relu);
    switch (b.kind) {
      case SUB_FF:
        if (gated) {   // dmid (masked like the product it belongs to) -> dgu = (dg | du) in dbig, one ordinary dY for the W_in products
          if (drop.on) drop.rows(Ln, k, dmid, nullptr, dmid, b.k_out, site_mid);
          Ln.run(RPR_K_OTHER, 0, 20.0 * rows * b.k_out, [&] { return launch_gated_gelu_bwd(in, dmid, rows, b.k_out, dbig, s); });
          break;
        }
        if (drop.on) drop.rows(Ln, k, dbig, nullptr, dbig, b.n_in, site_mid);
        if (!bf16) Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_relu_bwd(dbig, in, (size_t)rows * b.n_in, s); });
        break;
      case SUB_CROSS: {
        const float* xk = P<float>(w.xkv) + (size_t)i * 2 * inner;
        float* dxk = P<float>(w.dxkv) + (size_t)i * 2 * inner;
        Ln.run(RPR_K_DEC_CROSS_ATTN, 0, 0, [&] {   // dq into dbig (as [R, inner])
          return launch_cross_attn_bwd(in, xk, xk + inner, D.xld, mask, dattn, dbig, dxk, dxk + inner, D.bz, D.docs * D.L, D.Lq, H, s,
                                       drop.on ? &da : nullptr, d.d_kv);
        });
        break;
      }
      case SUB_SELF:
        Ln.run(RPR_K_ENC_ATTN, 0, 0, [&] {
          return launch_self_attn_bwd(in, dattn, k.mask, k.rel_bias, k.bucket, dbig, P<float>(w.bias_part),
                                      g(k.lay.dec ? K_DEC_REL : K_ENC_REL), k.nseq, k.len, H, d.rel_buckets, k.causal, s,
                                      drop.on ? &da : nullptr, d.d_kv);
        });
        break;
    }
    if (!saved) B.norm(x, p[P_LN].ptr, rows);
    B.dxdw(dbig, p[P_WIN].ptr, h, h, G + p[P_WIN].offset, rows, b.n_in, dm, k.xt_in(i, j), relu);
    B.norm_bwd(x, p[P_LN].ptr, h, dx, dx2, G + p[P_LN].offset, rows);
    std::swap(dx, dx2);
  };
  auto stack_bwd = [&](const Stack& k) {   // layers last to first
    for (int i = k.lay.layers - 1; i >= 0; --i) {
      for (int j = k.lay.nsub - 1; j >= 0; --j) sub_bwd(k, i, j);
      w.side.flush(Ln);                                               // the layer's weight gradients: one launch on the side stream
      B.flush_norms();                                               // ... and its layer-norm weight gradients
      size_t off, numel;
      m->params.bucket(k.lay, i, &off, &numel);
      bucket(off, numel);
    }
  };
  // ---- decoder
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return hipMemsetAsync(w.dxkv.p, 0, (size_t)T * D.xld * sizeof(float), s); });
  stack_bwd(dec);
  if (drop.on) drop.rows(Ln, dec, dx, nullptr, dx, dm, drop_site_input(1));
  // decoder input embeddings: codebook rows and the start embedding
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_scatter_rows_fix(dx, P<int32_t>(w.in_idx), fix, R, dm, s); });
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_fix_flush(fix, g(K_IN_EMB), (size_t)d.L * D.V * dm, s); });
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_sum_selected_rows(dx, P<int32_t>(w.in_idx), g(K_START), R, dm, s); });
  // ---- cross K/V projection and the encoder's final norm
  float* denc = P<float>(w.denc);
  B.dxdw(P<float>(w.dxkv), d.dec_xkv, P<float>(w.enc_out), denc, g(K_XKV), T, D.xld, dm, enc.xT ? enc.xT + Y.xt_xkv : nullptr);
  w.side.flush(Ln);
  if (drop.on) drop.rows(Ln, enc, denc, nullptr, denc, dm, drop_site_output(0));
  B.norm_bwd(enc.x_end, d.enc_final_ln, denc, nullptr, dxa, g(K_ENC_FLN), T);
  dx = dxa; dx2 = dxb;   // the ping-pong starts again
  stack_bwd(enc);
  if (drop.on) drop.rows(Ln, enc, dx, nullptr, dx, dm, drop_site_input(0));
  // token embeddings (the encoder's table is the shared one)
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_scatter_rows_fix(dx, ids, fix, T, dm, s); });
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_fix_flush(fix, g(K_SHARED), (size_t)d.vocab_size * dm, s); });
  // the weight gradients still in flight on the side stream belong to this pass: join
  w.side.wait_products(Ln, s, true);
  w.side.flush(Ln);
  B.flush_norms();                                                 // the encoder's final norm (the decoder's went with its last layer)
  w.side.wait_groups(Ln, s, true);
  bucket(0, m->params.at(K_ENC_LAYER, 0).offset);   // everything in front of the first layer: final only now
}

// Checks and workspaces shared by the training passes: docs decoder sequences of L positions per query
int train_setup(rpr_ctx* c, rpr_model* m, int32_t bz, int32_t Lq, int32_t L, int docs, TrainDims& D, Head head) {
  RPR_REQUIRE(m->ctx == c, "model belongs to another ctx");
  RPR_REQUIRE(bz >= 1 && Lq >= 1, "bz or Lq out of range");
  RPR_REQUIRE(Lq <= MAX_LQ, "Lq out of range: the training passes take queries of at most 256 tokens");
  RPR_REQUIRE(m->d.d_kv == DKV || m->d.d_kv == 128, "d_kv must be 64 (t5-base / t5-large) or 128 (t5-3b)");
  RPR_REQUIRE(L >= 1 && L <= m->d.L && L <= MAX_DEC_LEN, "smtid length exceeds the model's decoder length");
  RPR_HIP(hipSetDevice(c->device));
  const auto& d = m->d;
  D = train_dims(d, bz, Lq, L, docs, m->gated());
  // every attention launch of the step has a plan (attn_route.h, the training sites): 64-dim heads beyond the carve of a whole head
  // go on in tiles, 128-dim heads stop at the carve
  RPR_REQUIRE(train_attn_admitted(bz, Lq, L, docs, d.num_heads, d.rel_buckets, d.d_kv),
              "sequence lengths beyond the 160 KB of LDS the attention backward holds a head in: self-attention max(L, Lq) <= 91, "
              "cross-attention 130 (docs L + Lq) + 2 docs L (Lq + 1) + Lq floats <= 40960 (the same for 64- and 128-dim heads)");
  int e = alloc_train(c, m, D, head);
  if (e) return e;
  // the forward's cross-attention kernel needs the per-query key counts: reuse the search workspace's small buffers
  return ensure(c, c->ws.last, (size_t)bz * 4);
}

// per pass: fixed-point accumulators and amax slots zeroed, the bf16 weight copies refreshed (bf16 mode)
int train_begin(Launcher& Ln, rpr_ctx* c, rpr_model* m) {
  TrainWs& w = *c->tws;
  RPR_HIP(hipMemsetAsync(w.fix.p, 0, w.fix.cap, Ln.s));
  amax_reset(Ln);
  if (c->precision == RPR_PREC_BF16) return refresh_weight_cache(Ln, c, m);
  w.wc_off.clear(); w.wc_model = nullptr;   // the other modes convert per call
  return Ln.err;
}

}  // namespace

void rpr::train_forget_model(rpr_ctx* c, const rpr_model* m) {
  if (c && c->tws && c->tws->wc_model == m) { c->tws->wc_model = nullptr; c->tws->wc_off.clear(); }
  if (c && c->tws && c->tws->aw_model == m) c->tws->aw_model = nullptr;
}

void rpr::free_train_ws(rpr_ctx* c) {
  if (!c->tws) return;
  TrainWs& w = *c->tws;
  for (DevBuf* b : w.bufs) if (b->p) (void)hipFree(b->p);
  w.side.destroy();
  for (hipEvent_t e : w.bucket_ev) (void)hipEventDestroy(e);
  delete c->tws;
  c->tws = nullptr;
}

extern "C" {

int64_t rpr_param_count(rpr_model* m) { return m ? (int64_t)m->params.slots.size() : 0; }
int64_t rpr_param_total(rpr_model* m) { return m ? (int64_t)m->params.total : 0; }
int rpr_param_info(rpr_model* m, int64_t index, const float** ptr, int64_t* numel, int64_t* offset) {
  RPR_REQUIRE(m, "NULL model");
  RPR_REQUIRE(index >= 0 && index < (int64_t)m->params.slots.size(), "parameter index out of range");
  const auto& p = m->params.slots[(size_t)index];
  if (ptr) *ptr = p.ptr;
  if (numel) *numel = (int64_t)p.numel;
  if (offset) *offset = (int64_t)p.offset;
  return RPR_OK;
}

int rpr_lngknp_backward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lq,
                        const int32_t* doc_codes, int32_t L, const float* teacher_pos, const float* teacher_neg,
                        const int32_t* prefix_lens, int32_t n_prefix, float* out_losses, float* flat_grads, void* stream) {
  return rpr_lngknp_backward_buckets(c, m, input_ids, attention_mask, bz, Lq, doc_codes, L, teacher_pos, teacher_neg, prefix_lens,
                                     n_prefix, out_losses, flat_grads, stream, nullptr, nullptr, nullptr);
}

int rpr_lngknp_backward_buckets(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                                int32_t Lq, const int32_t* doc_codes, int32_t L, const float* teacher_pos, const float* teacher_neg,
                                const int32_t* prefix_lens, int32_t n_prefix, float* out_losses, float* flat_grads, void* stream,
                                void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && doc_codes && teacher_pos && teacher_neg && prefix_lens && out_losses &&
                  flat_grads, "NULL argument");
  RPR_REQUIRE(n_prefix >= 1 && n_prefix <= 8, "n_prefix out of range (1..8)");
  TrainDims D{};
  int e = train_setup(c, m, bz, Lq, L, 2, D, HEAD_GOLD);
  if (e) return e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  TrainWs& w = *c->tws;
  RPR_HIP(hipMemsetAsync(flat_grads, 0, m->params.total * sizeof(float), s));
  Launcher Ln{c, s};
  e = train_begin(Ln, c, m);
  if (e) return e;
  const Drop drop(c);
  forward(Ln, c, m, D, input_ids, attention_mask, doc_codes, P<int32_t>(c->ws.last), drop);
  if (Ln.err) return Ln.err;
  RPR_HIP(launch_margin_mse(P<float>(w.scores), teacher_pos, teacher_neg, prefix_lens, n_prefix, bz, L, out_losses, P<float>(w.margins), s));
  // total loss = sum of the task losses with weight 1 (reference arguments.py:109-119, trainer.py:228-240)
  RPR_HIP(launch_margin_mse_bwd(P<float>(w.margins), teacher_pos, teacher_neg, prefix_lens, n_prefix, bz, L, P<float>(w.dscores), s));
  BucketHook hook{on_bucket, user, reinterpret_cast<hipStream_t>(comm_stream)};
  backward(Ln, c, m, D, input_ids, attention_mask, flat_grads, drop, on_bucket ? &hook : nullptr);
  return Ln.err;
}

// ---- seq2seq docid cross-entropy step (reference T5SeqAQEncoderForSeq2Seq, modeling/t5_generative_retriever.py:968-1019) ----
// The same teacher-forced pass with one decoder sequence per query (decoder_input_ids = [-1, labels[:, :-1]]: the labels are the
// doc codes of the ranking step) and the cross-entropy head in place of the gold scores.
static int seq2seq_run(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lq,
                       const int32_t* labels, int32_t L, float* out_loss, float* out_label_lp, float* flat_grads, void* stream,
                       void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && labels && out_loss, "NULL argument");
  RPR_REQUIRE(s2s_head_smem_ok(m->d.V) && m->d.d_model % 32 == 0,
              "the cross-entropy head needs a codebook size V with V % 64 == 0 and V <= 1024, and d_model % 32 == 0");
  TrainDims D{};
  int e = train_setup(c, m, bz, Lq, L, 1, D, HEAD_CE);
  if (e) return e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  {  // labels outside [0, V) would index past a codebook: refused before anything is enqueued (one small copy + synchronisation)
    std::vector<int32_t> h((size_t)bz * L);
    RPR_HIP(hipMemcpyAsync(h.data(), labels, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RPR_HIP(hipStreamSynchronize(s));
    for (int32_t v : h) RPR_REQUIRE(v >= 0 && v < m->d.V, "a label is outside [0, V) of the codebooks");
  }
  if (flat_grads) RPR_HIP(hipMemsetAsync(flat_grads, 0, m->params.total * sizeof(float), s));
  Launcher Ln{c, s};
  e = train_begin(Ln, c, m);
  if (e) return e;
  const Drop drop = flat_grads ? Drop(c) : Drop();   // rpr_seq2seq_forward stays in evaluation mode
  forward(Ln, c, m, D, input_ids, attention_mask, labels, P<int32_t>(c->ws.last), drop, false);
  s2s_head_forward(Ln, c, m, D, labels, out_loss, out_label_lp, drop);
  if (Ln.err || !flat_grads) return Ln.err;
  BucketHook hook{on_bucket, user, reinterpret_cast<hipStream_t>(comm_stream)};
  backward(Ln, c, m, D, input_ids, attention_mask, flat_grads, drop, on_bucket ? &hook : nullptr, HEAD_CE);
  return Ln.err;
}

int rpr_seq2seq_forward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lq,
                        const int32_t* labels, int32_t L, float* out_loss, float* out_label_logprob, void* stream) {
  return seq2seq_run(c, m, input_ids, attention_mask, bz, Lq, labels, L, out_loss, out_label_logprob, nullptr, stream, nullptr, nullptr,
                     nullptr);
}

int rpr_seq2seq_backward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lq,
                         const int32_t* labels, int32_t L, float* out_loss, float* flat_grads, void* stream) {
  RPR_REQUIRE(flat_grads, "NULL argument");
  return seq2seq_run(c, m, input_ids, attention_mask, bz, Lq, labels, L, out_loss, nullptr, flat_grads, stream, nullptr, nullptr, nullptr);
}

int rpr_seq2seq_backward_buckets(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                                 int32_t Lq, const int32_t* labels, int32_t L, float* out_loss, float* flat_grads, void* stream,
                                 void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user) {
  RPR_REQUIRE(flat_grads, "NULL argument");
  return seq2seq_run(c, m, input_ids, attention_mask, bz, Lq, labels, L, out_loss, nullptr, flat_grads, stream, comm_stream, on_bucket,
                     user);
}

// ---- dense first-stage step (reference T5SeqPretrainEncoder, modeling/t5_generative_retriever.py:558-615 and :708-757 with one
// decoder position: decoder_input_ids = [-1], no commit loss) ----
// One teacher-forced pass over S = 3 bz sequences (queries | positive documents | negative documents), one decoder sequence of
// one position each, and the dense head in place of the gold scores. The query is encoded once and takes both gradient
// contributions (the reference encodes the same text twice).
static void dense_head_forward(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const TrainDims& D, const float* teacher_pos,
                               const float* teacher_neg, float* out_loss, const Drop& drop) {
  TrainWs& w = *c->tws;
  hipStream_t s = Ln.s;
  Ln.run(RPR_K_RMSNORM, 0, 8.0 * D.R * D.dm, [&] {
    return launch_rmsnorm(P<float>(w.x_last), m->d.dec_final_ln, P<float>(w.hF), D.R, D.dm, D.eps, s, D.post);
  });
  if (drop.on) drop.rows(Ln, D.S, D.L, P<float>(w.hF), nullptr, P<float>(w.hF), D.dm, drop_site_output(1));
  Ln.run(RPR_K_OTHER, 4.0 * D.R * D.dm, 4.0 * D.R * D.dm, [&] {
    return launch_dense_mse_head_fwd(P<float>(w.hF), teacher_pos, teacher_neg, P<float>(w.scores), P<float>(w.margins), P<float>(w.dscores),
                                     out_loss, D.bz / 3, D.dm, s);
  });
}

static int dense_run(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lt,
                     const float* teacher_pos, const float* teacher_neg, float* out_loss, float* out_scores, float* out_reps,
                     float* flat_grads, void* stream, void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && teacher_pos && teacher_neg && out_loss, "NULL argument");
  RPR_REQUIRE(bz >= 1 && bz <= (1 << 20), "bz out of range");
  TrainDims D{};
  int e = train_setup(c, m, 3 * bz, Lt, 1, 1, D, HEAD_DENSE);
  if (e) return e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  TrainWs& w = *c->tws;
  if (flat_grads) RPR_HIP(hipMemsetAsync(flat_grads, 0, m->params.total * sizeof(float), s));
  RPR_HIP(hipMemsetAsync(w.dense_codes.p, 0, (size_t)D.R * 4, s));
  Launcher Ln{c, s};
  e = train_begin(Ln, c, m);
  if (e) return e;
  const Drop drop = flat_grads ? Drop(c) : Drop();   // rpr_dense_mse_forward stays in evaluation mode
  forward(Ln, c, m, D, input_ids, attention_mask, P<int32_t>(w.dense_codes), P<int32_t>(c->ws.last), drop, false);
  dense_head_forward(Ln, c, m, D, teacher_pos, teacher_neg, out_loss, drop);
  if (Ln.err) return Ln.err;
  if (out_scores) RPR_HIP(hipMemcpyAsync(out_scores, w.scores.p, (size_t)2 * bz * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (out_reps) RPR_HIP(hipMemcpyAsync(out_reps, w.hF.p, (size_t)D.R * D.dm * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!flat_grads) return RPR_OK;
  BucketHook hook{on_bucket, user, reinterpret_cast<hipStream_t>(comm_stream)};
  backward(Ln, c, m, D, input_ids, attention_mask, flat_grads, drop, on_bucket ? &hook : nullptr, HEAD_DENSE);
  return Ln.err;
}

int rpr_dense_mse_forward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lt,
                          const float* teacher_pos, const float* teacher_neg, float* out_loss, float* out_scores, float* out_reps,
                          void* stream) {
  return dense_run(c, m, input_ids, attention_mask, bz, Lt, teacher_pos, teacher_neg, out_loss, out_scores, out_reps, nullptr, stream,
                   nullptr, nullptr, nullptr);
}

int rpr_dense_mse_backward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lt,
                           const float* teacher_pos, const float* teacher_neg, float* out_loss, float* flat_grads, void* stream) {
  RPR_REQUIRE(flat_grads, "NULL argument");
  return dense_run(c, m, input_ids, attention_mask, bz, Lt, teacher_pos, teacher_neg, out_loss, nullptr, nullptr, flat_grads, stream,
                   nullptr, nullptr, nullptr);
}

int rpr_dense_mse_backward_buckets(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                                   int32_t Lt, const float* teacher_pos, const float* teacher_neg, float* out_loss, float* flat_grads,
                                   void* stream, void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user) {
  RPR_REQUIRE(flat_grads, "NULL argument");
  return dense_run(c, m, input_ids, attention_mask, bz, Lt, teacher_pos, teacher_neg, out_loss, nullptr, nullptr, flat_grads, stream,
                   comm_stream, on_bucket, user);
}

int rpr_set_train_dropout(rpr_ctx* c, float rate, uint64_t seed, uint64_t step) {
  RPR_REQUIRE(c, "NULL ctx");
  RPR_REQUIRE(rate >= 0.f && rate < 1.f, "dropout rate outside [0, 1)");   // (a NaN fails both comparisons)
  c->train_drop.rate = rate; c->train_drop.seed = seed; c->train_drop.step = step;
  return RPR_OK;
}

// test hook: the activation mask of dropout.h over x [n_seq][n_pos][n_feat] (tests/test_gpu_dropout.py compares it bit for bit
// with the numpy restatement)
int rpr_op_dropout(rpr_ctx* c, const float* x, float* out, int64_t n_seq, int32_t n_pos, int32_t n_feat, float rate, uint64_t seed,
                   uint64_t step, int32_t site, void* stream) {
  RPR_REQUIRE(c && x && out, "NULL argument");
  RPR_REQUIRE(rate >= 0.f && rate < 1.f, "dropout rate outside [0, 1)");
  RPR_REQUIRE(n_seq >= 0 && n_pos >= 1 && n_pos <= 65536 && n_feat >= 1 && site >= 0 && site <= 0xffff, "shape or site out of range");
  RPR_HIP(hipSetDevice(c->device));
  const Drop d(rate, seed, step);
  RPR_HIP(launch_dropout_rows(x, nullptr, out, (size_t)n_seq, n_pos, n_feat, d.key, site, reinterpret_cast<hipStream_t>(stream)));
  return RPR_OK;
}

int rpr_adamw_step(rpr_ctx* c, rpr_model* m, const float* flat_grads, float* exp_avg, float* exp_avg_sq, int64_t step, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, float* out_grad_norm,
                   void* stream) {
  RPR_REQUIRE(c && m && flat_grads && exp_avg && exp_avg_sq, "NULL argument");
  RPR_REQUIRE(m->ctx == c && step >= 1, "bad model or step (1-based)");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!c->tws) c->tws = new TrainWs();
  TrainWs& w = *c->tws;
  int e = tensure(c, w.gn_part, 1024 * 8);
  if (!e) e = tensure(c, w.gn_out, 16);
  if (e) return e;
  RPR_HIP(launch_grad_norm(flat_grads, m->params.total, P<double>(w.gn_part), 1024, max_grad_norm, P<float>(w.gn_out), s));
  const float bc1 = 1.0f - (float)pow((double)beta1, (double)step);
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  // Weight decay follows HF 4.17's Trainer.create_optimizer (what the reference trains with, tasks/trainer.py:477):
  // every parameter decays except those of nn.LayerNorm modules and those whose name contains "bias". T5LayerNorm is
  // not an nn.LayerNorm in that version, so the T5 layer-norm weights DO decay; `relative_attention_bias.weight` is
  // excluded by its name. (Restated from memory of transformers 4.17 — its source is not available offline; the
  // reference's default weight_decay is 0, where the rule is moot.)
  if (w.aw_model != m) {   // tensor table: pointer, offset in the flat buffers, elements, decays?
    std::vector<AdamSeg> segs;
    std::vector<int> pref;
    int chunks = 0;
    for (const auto& p : m->params.slots) {
      if (!p.numel) continue;
      segs.push_back(AdamSeg{p.ptr, (unsigned long long)p.offset, (unsigned long long)p.numel,
                             (p.kind == K_ENC_REL || p.kind == K_DEC_REL) ? 0 : 1});
      pref.push_back(chunks);
      chunks += (int)((p.numel + 4095) / 4096);
    }
    e = tensure(c, w.aseg, segs.size() * sizeof(AdamSeg));
    if (!e) e = tensure(c, w.apref, pref.size() * sizeof(int));
    if (e) return e;
    RPR_HIP(hipMemcpyAsync(w.aseg.p, segs.data(), segs.size() * sizeof(AdamSeg), hipMemcpyHostToDevice, s));
    RPR_HIP(hipMemcpyAsync(w.apref.p, pref.data(), pref.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RPR_HIP(hipStreamSynchronize(s));              // the host vectors go out of scope
    w.aw_model = m; w.aw_nseg = (int)segs.size(); w.aw_chunks = chunks;
  }
  RPR_HIP(launch_adamw_multi(P<AdamSeg>(w.aseg), P<int>(w.apref), w.aw_nseg, w.aw_chunks, flat_grads, exp_avg, exp_avg_sq,
                             P<float>(w.gn_out), lr, beta1, beta2, eps, weight_decay, bc1, bc2s, s));
  if (out_grad_norm) RPR_HIP(hipMemcpyAsync(out_grad_norm, w.gn_out.p, 4, hipMemcpyDeviceToDevice, s));
  // the search / inference paths read the f16 planes of the weights: they are stale now and are re-split by the next call
  // that needs them (ensure_weight_planes) — a training loop never does, and the refresh costs a pass over every weight
  // plus a stream synchronisation per step
  m->planes_dirty = true;
  m->l0_valid = false;   // and so is the layer-0 Q/K/V table made from them (in_embeds, dec_ln0[0], dec_qkv[0])
  return RPR_OK;
}

}  // extern "C"
