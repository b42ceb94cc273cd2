// The forward passes of the product, as launches enqueued on one HIP stream (the C ABI that drives them is api.hip):
// the T5 encoder, the KV-cached decoder steps of a constrained beam search with their forks and teacher-forced tail
// passes (enqueue_search), and the teacher-forced forward of the ranking fine-tune step (enqueue_train_forward).
// The transformer layer all of them walk is written once (Pass); a pass keeps what is its own: the embedding, where
// Q/K/V go, its attention launches and what follows the last layer. No kernel lives here.
#include <cmath>
#include <vector>

#include "internal.h"

namespace rpr {

LinOut out_f32(float* p, int ld, int N, const float* resid, int relu) {
  LinOut o{};
  o.f[0] = o.f[1] = o.f[2] = p; o.ldo[0] = o.ldo[1] = o.ldo[2] = ld; o.split_n = N; o.resid = resid; o.relu = relu;
  return o;
}

namespace {

// The split-precision launch of one linear layer: what linear() hands to launch_gemm_h2 (and the layer-0 table's gate to
// the route planner).
GemmH2Args h2_args(const Launcher& L, const LinIn& A, const LinW& W, int M, const LinOut& O, const int* m_dev) {
  const rpr_ctx* c = L.c;
  const int Nh = W.Nh ? W.Nh : W.N;
  GemmH2Args g{};
  g.A = A.h; g.a_ps = A.ps; g.lda = A.ld; g.W = W.h; g.w_ps = W.ps ? W.ps : (size_t)W.N * W.K; g.ldw = W.K;
  g.resid = O.resid; g.ldr = O.ldo[0];
  for (int i = 0; i < 3; ++i) { g.out[i] = O.f[i]; g.ldo[i] = O.ldo[i]; }
  g.split_n = O.split_n; g.out_h = O.h; g.o_ps = O.ps; g.ldoh = O.ldh;
  g.M = M; g.N = Nh; g.K = W.K; g.relu = O.relu;
  g.rm_B = O.rm_B; g.rm_stride = O.rm_stride; g.rm_slot = O.rm_slot; g.rm_head = O.rm_head; g.rm_dshift = O.rm_dshift;
  g.m_dev = m_dev; g.acc_scale = 1.0f / (W_PLANE_SCALE * A.scale); g.plane_scale = O.plane_scale;
  g.row_ssq = A.ssq; g.inv_d_fix = A.inv_d_fix; g.eps = A.eps;
  g.resid_h = O.resid_h; g.r_ps = O.ps; g.ldrh = O.ldh; g.ssq_out = O.ssq_out;
  g.sat = c->status;
  g.cus = L.cus;
  g.small_live = m_dev ? L.small_live : 0;
  g.no_row_split = W.row_split_ok ? 0 : L.no_row_split;
  g.force_pp = W.force_pp ? 1 : 0;
  g.mfma16 = L.mfma16;
  if (!W.no_scratch) { g.part = P<float>(c->ws.part); g.part_cap = c->ws.part.cap / sizeof(float); g.mid_split = 1; }
  return g;
}

}  // namespace

void linear(Launcher& L, const LinIn& A, const LinW& W, int M, const LinOut& O, const int* m_dev, int m_acc) {
  const double Ma = m_acc >= 0 ? m_acc : M;
  const double fl = 2.0 * Ma * (double)W.N * W.K;
  const double by = 4.0 * (Ma * W.K + (double)W.N * W.K + Ma * W.N * ((O.resid || O.resid_h) ? 2 : 1));
  hipStream_t s = L.s;
  if (L.c->precision == RPR_PREC_F16X2) {
    GemmH2Args g = h2_args(L, A, W, M, O, m_dev);
    L.run(RPR_K_GEMM, fl, by, [&] { return launch_gemm_h2(g, s); }, &g.kernel_cls);
  } else {
    GemmArgs g{};
    g.A = A.f; g.lda = A.ld; g.W = W.f; g.ldw = W.K; g.resid = O.resid; g.ldr = O.ldo[0];
    for (int i = 0; i < 3; ++i) { g.out[i] = O.f[i]; g.ldo[i] = O.ldo[i]; }
    g.split_n = O.split_n; g.M = M; g.N = W.N; g.K = W.K; g.relu = O.relu;
    g.rm_B = O.rm_B; g.rm_stride = O.rm_stride; g.rm_slot = O.rm_slot; g.rm_head = O.rm_head; g.rm_dshift = O.rm_dshift;
    g.m_dev = m_dev;
    L.run(RPR_K_GEMM, fl, by, [&] { return launch_gemm(g, s); });
  }
}

int alloc_workspace(rpr_ctx* c, const rpr_model* m, const SearchPlan& plan) {
  const auto& d = m->d;
  const int Q = plan.Q, Lq = plan.Lq, B = plan.B, L = plan.L, nf = plan.n_forks;
  const int* forks = plan.forks;
  const size_t T = (size_t)Q * Lq, R = (size_t)Q * B, inner = m->inner(), dm = d.d_model, dff = d.d_ff;
  const size_t nd = d.num_decoder_layers, ne = d.num_layers, f = sizeof(float);
  Workspace& w = c->ws;
  // forced with extras: `pool` spare tail entries per fork = virtual queries behind the beam state of the stage (0 without forks)
  const size_t pool = (size_t)plan.pool, Qt = (size_t)Q + pool, Rv = Qt * B;
  int e = 0;
  auto E = [&](DevBuf& b, size_t bytes) { if (!e) e = ensure(c, b, bytes); };
  E(w.ids, T * 4); E(w.mask, T * 4); E(w.last, (size_t)Q * 4); E(w.offs, ((size_t)Q + 1) * 4); E(w.row_src, T * 4);
  E(w.ex, T * dm * f); E(w.eh, T * dm * f); E(w.eqkv, T * 3 * inner * f); E(w.eattn, T * inner * f);
  E(w.eff, T * dff * f); E(w.enc_out, T * dm * f); E(w.xkv, T * nd * 2 * inner * f);
  E(w.x, R * dm * f); E(w.h, R * dm * f); E(w.q, R * inner * f); E(w.attn, R * inner * f);
  E(w.ff, R * dff * f); E(w.logits, R * (size_t)m->Vp() * f);
  const size_t depth0 = nf ? (size_t)forks[0] : (size_t)L;   // stage 0 stops at the first fork
  E(w.kcache, nd * depth0 * R * inner * f); E(w.vcache, nd * depth0 * R * inner * f);
  E(w.lb, R * (size_t)m->Vp() * 4 * 2);   // start and end of every child's row range
  if (select_radix_wanted(B, m->Vp())) E(w.sel_rs, select_radix_ws_bytes(Q, B, m->Vp()));
  for (int i = 0; i < 2; ++i) {
    E(w.score[i], Rv * 8); E(w.lo[i], Rv * 4); E(w.hi[i], Rv * 4);
    E(w.tokens[i], Rv * (size_t)L * 2); E(w.anc[i], Rv * (size_t)L * 2);
  }
  E(w.o_tokens, R * (size_t)L * 4); E(w.o_scores, R * 4); E(w.o_lo, R * 8); E(w.o_hi, R * 8);
  for (int k = 0; k < plan.n_depths; ++k) {   // rpr_search_prefixes: staged outputs per prefix length
    E(w.d_tokens[k], R * (size_t)plan.depths[k] * 4); E(w.d_scores[k], R * 4); E(w.d_lo[k], R * 8); E(w.d_hi[k], R * 8);
  }
  if (plan.margins) { E(w.mg_valid, R * (size_t)m->Vp() / 8); E(w.o_margin, (size_t)Q * 8); }
  const size_t hb = sizeof(__half) * 2;  // two planes
  E(w.eattn_h, T * inner * hb); E(w.eff_h, T * dff * hb); E(w.enc_out_h, T * dm * hb);
  E(w.attn_h, R * inner * hb); E(w.ff_h, R * dff * hb);
  E(w.ex_h, T * dm * hb); E(w.x_h, R * dm * hb);
  E(w.ssq_e, (2 * ne + 1) * T * 8); E(w.ssq_d, (3 * nd + 1) * R * 8);
  // gated feed-forward: the fp32 result of the W_in product (gate | linear half), read by the gate kernel
  if (m->gated()) { E(w.egu, T * 2 * dff * f); E(w.gu, R * 2 * dff * f); }
  E(w.part, (size_t)9 << 20 << 2);   // split-K partials of the mid-size GEMM route: < 256 tiles of 128 x 64, up to 4 splits
  // forced-tail search: one compacted stage and one tail job per fork, tail activations for the longest tail
  for (int k = 0; k < nf; ++k) {
    const size_t depth = k + 1 < nf ? (size_t)forks[k + 1] : (size_t)L, Lt = (size_t)(L - forks[k]);
    StageBufs& sb = w.stage[k];
    E(sb.cnt, 16); E(sb.src, (size_t)Q * 4);
    if (!(plan.drop_last && k + 1 == nf)) {
      E(sb.qmap, (size_t)Q * 4); E(sb.offs, (size_t)Q * 4); E(sb.last, (size_t)Q * 4); E(sb.mask, T * 4);
      E(sb.kcache, nd * depth * R * inner * f); E(sb.vcache, nd * depth * R * inner * f);
      for (int i = 0; i < 2; ++i) {
        E(sb.score[i], Rv * 8); E(sb.lo[i], Rv * 4); E(sb.hi[i], Rv * 4);
        E(sb.tokens[i], Rv * (size_t)L * 2); E(sb.anc[i], Rv * (size_t)L * 2);
      }
    }
    TailBufs& tb = w.tail[k];
    E(tb.flag, (size_t)Q * 4); E(tb.flist, Qt * 4); E(tb.cnt, 16);
    E(tb.kvq, Qt * 4); E(tb.spare, ((size_t)Q + 1 + pool + pool * B) * 4);
    E(tb.qmap, Qt * 4); E(tb.offs, Qt * 4); E(tb.last, Qt * 4); E(tb.mask, Qt * Lq * 4);
    E(tb.tokens, Rv * (size_t)L * 2); E(tb.gold, Rv * Lt * f);
  }
  if (nf) {
    const size_t Rt = Rv * (size_t)(L - forks[0]);
    E(w.t_qkv, Rt * 3 * inner * f); E(w.t_q, Rt * inner * f);
    if (plan.prec == RPR_PREC_F16X2) {
      E(w.t_x_h, Rt * dm * hb); E(w.t_attn_h, Rt * inner * hb); E(w.t_ff_h, Rt * dff * hb); E(w.t_ssq, (3 * nd + 1) * Rt * 8);
    } else {
      E(w.t_x, Rt * dm * f); E(w.t_h, Rt * dm * f); E(w.t_attn, Rt * inner * f); E(w.t_ff, Rt * dff * f);
    }
    if (m->gated()) E(w.t_gu, Rt * 2 * dff * f);
    if (plan.log_softmax()) { E(w.t_h, Rt * dm * f); E(w.t_logits, Rt * (size_t)d.V * f); }   // normalised rows, V logits per row
  }
  return e;
}

namespace {

// Fused RMSNorm plumbing of the split-precision mode: the residual stream x lives in two f16 planes
// (hi + lo = 22 bits; operand of the next projection AND residual of the next producer) plus one fixed-point sum of
// squares per row and norm site; the projection that follows a norm runs on the x planes against W * diag(ln_weight)
// and scales its output rows by rsqrt(ssq / d + eps). Sites are numbered in program order; every site of a pass has
// its own ssq slot, zeroed by one small kernel per pass (site 0 is stored by the embedding kernel, the others are
// accumulated with integer atomics by the residual GEMMs' epilogues, so the sums do not depend on the order of
// arrival). The exact-fp32 mode keeps the fp32 stream and the separate RMSNorm kernel.
struct XStream {
  __half* x_h; size_t ps; unsigned long long* ssq; size_t rows; int dm; float eps;
  LinIn in(int site) const {
    LinIn a{nullptr, x_h, ps, dm, X_PLANE_SCALE};
    a.ssq = ssq + (size_t)site * rows; a.inv_d_fix = 1.0f / ((float)dm * SSQ_FIX); a.eps = eps;
    return a;
  }
  LinOut out(int site) const {          // x += projection (in place in the planes); the site's row sums
    LinOut o{};
    o.split_n = dm; o.h = x_h; o.ps = ps; o.ldh = dm; o.plane_scale = X_PLANE_SCALE;
    o.resid_h = x_h; o.ssq_out = ssq + (size_t)site * rows;
    return o;
  }
};

// Residual stream and layer intermediates of one pass (fp32 buffers of the exact mode, planes and row sums of the split mode)
struct PassBufs { const DevBuf &x, &h, &attn, &ff, &x_h, &attn_h, &ff_h, &ssq, &gu; };   // gu: gated models only

// The transformer layer every pass walks, in both precision modes: how a normalised input reaches a projection, where a
// residual projection lands, the FF block. A layer has `spl` norm sites (encoder 2: self-attention, FF; decoder 3: self-,
// cross-attention, FF): the k-th norm of a layer reads site layer * spl + k, the residual projection behind it
// accumulates the next one; site spl * layers is the input of the final norm. A pass builds one of these from its
// buffers and keeps what is its own: the embedding, the Q/K/V destination, the attention launches, the head.
struct Pass {
  Launcher& Ln;
  const rpr_model* const m; const bool dec;      // the model and the stack whose sub-blocks' weights the layers read (internal.h)
  const bool h2;                                // split-precision mode (fused norms); false: exact fp32
  const int spl, layers, dm, inner, dff;
  int M; const int* const m_dev; int m_acc;      // rows of the launches that follow (rows()), their device-side live count (nullable),
                                                 //   the rows their profile records account
  const int norm_acc;                            // rows the RMSNorm records account: as constructed (the decoder steps state
                                                 //   the whole stage's on the shared step 0 too)
  float *const x, *const h, *const attn, *const ff, *const gu; __half *const attn_h, *const ff_h;
  const size_t ps_i, ps_f;                       // plane strides of attn_h / ff_h (the x planes': xs.ps)
  const XStream xs;
  const float post;                              // scaleup_output_hidden: factor on the final norm of the decoder

  Pass(Launcher& Ln_, const rpr_model* m_, const PassBufs& b, bool dec_, int layers_, int rows_cap, const int* m_dev_, int m_acc_)
      : Ln(Ln_), m(m_), dec(dec_), h2(Ln_.c->precision == RPR_PREC_F16X2), spl(dec_ ? 3 : 2), layers(layers_), dm(m->d.d_model),
        inner(m->inner()), dff(m->d.d_ff), M(rows_cap), m_dev(m_dev_), m_acc(m_acc_), norm_acc(m_acc_), x(P<float>(b.x)), h(P<float>(b.h)),
        attn(P<float>(b.attn)), ff(P<float>(b.ff)), gu(P<float>(b.gu)), attn_h(P<__half>(b.attn_h)), ff_h(P<__half>(b.ff_h)),
        ps_i((size_t)rows_cap * inner), ps_f((size_t)rows_cap * dff),
        xs{P<__half>(b.x_h), (size_t)rows_cap * dm, P<unsigned long long>(b.ssq), (size_t)rows_cap, dm, m->d.layer_norm_eps},
        post(m->d.scaleup_output_hidden ? (float)pow((double)dm, -0.5) : 1.0f) {}

  void rows(int M_, int m_acc_) { M = M_; m_acc = m_acc_; }
  int site(int layer, int k) const { return layer * spl + k; }
  // every ssq slot of the pass starts at zero (split mode; once per pass, the decoder steps once per step). check: the slots
  // hold the totals of THIS call's previous step — test them against the stream's floor before they go (never the first
  // zeroing of a call: what it finds belongs to an earlier call, whose flags were read and cleared long ago)
  void zero_ssq(bool check = false) {
    if (!h2) return;
    const size_t n = (size_t)(spl * layers + 1) * xs.rows;
    if (check) Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_ssq_floor(xs.ssq, n, 1.0f / ((float)dm * SSQ_FIX), Ln.c->status, true, Ln.s); });
    else Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_zero_u64(xs.ssq, n, Ln.s); });
  }
  void check_ssq() {  // behind the last layer of a pass: a row total under the floor raises RPR_STATUS_SMALL_STREAM (common.h X_MS_FLOOR)
    if (h2) Ln.run(RPR_K_OTHER, 0, 0, [&] {
      return launch_ssq_floor(xs.ssq, (size_t)(spl * layers + 1) * xs.rows, 1.0f / ((float)dm * SSQ_FIX), Ln.c->status, false, Ln.s);
    });
  }
  XOut embed_out() const { return h2 ? XOut{xs.x_h, xs.ps, xs.ssq, Ln.c->status} : XOut{}; }   // where the embedding kernel puts x
  const __half* x_planes() const { return h2 ? xs.x_h : nullptr; }                             // for the kernels that read x themselves
  __half* attn_planes() const { return h2 ? attn_h : nullptr; }
  // input of the projection behind norm k of a layer: the x planes with the site's row sums (the norm weight is folded
  // into the projection's planes), or, exact fp32, the RMSNorm kernel's output
  LinIn normed(int layer, int k) { return normed(layer, k, m->ln(dec, layer, k)); }
  LinIn normed(int layer, int k, const float* ln, float post_scale = 1.0f) {   // (ln given: the final norm, layer = layers)
    if (h2) return xs.in(site(layer, k));
    Ln.run(RPR_K_RMSNORM, 0, 2.0 * norm_acc * dm * 4, [&] { return launch_rmsnorm(x, ln, h, M, dm, xs.eps, Ln.s, post_scale, nullptr, 0, m_dev); });
    return LinIn{h, nullptr, 0, dm};
  }
  // x += projection: destination of the residual projection behind norm k
  LinOut residual(int layer, int k) const { return h2 ? xs.out(site(layer, k) + 1) : out_f32(x, dm, dm, x); }
  void project(const LinIn& A, const LinW& W, const LinOut& O) { linear(Ln, A, W, M, O, m_dev, m_acc); }
  // the inner projection of sub-block k: norm, then W_in (Q/K/V, the cross-attention query)
  void project_in(int layer, int k, const LinOut& O) { project(normed(layer, k), m->weight(dec, layer, k, P_WIN), O); }
  // The model's layer-0 Q/K/V table stands in for this pass's layer-0 self-attention projection into O: split precision, the
  // table current (SearchPlan::l0), and the launch one the route planner sends whole to the ping-pong kernel — the kernel the table was made
  // by, whose K order does not depend on where a row sits, so the rows are the same bits (l0_mode 2: whatever the route).
  bool l0_replaces(const SearchPlan& plan, const LinOut& O) const {
    if (!h2 || !plan.l0) return false;
    if (plan.l0 >= 2) return true;
    return gemm_h2_pp_only(h2_args(Ln, xs.in(0), m->weight(true, 0, 0, P_WIN), M, O, m_dev));
  }
  void attn_out(int layer, int k) {   // o / xo: the attention output back into the stream
    project(LinIn{attn, attn_h, ps_i, inner}, m->weight(dec, layer, k, P_WOUT), residual(layer, k));
  }
  void ff_block(int layer, int k) {
    if (m->gated()) {   // W_in = wi_0 over wi_1 into gu (fp32, both modes), the gate kernel makes the W_out operand from it
      project_in(layer, k, out_f32(gu, 2 * dff, 2 * dff));
      Ln.run(RPR_K_OTHER, 8.0 * m_acc * dff, 12.0 * m_acc * dff, [&] {
        return launch_gated_gelu(gu, M, dff, m_dev, h2 ? nullptr : ff, h2 ? ff_h : nullptr, ps_f, Ln.c->status, Ln.s);
      });
      project(LinIn{ff, ff_h, ps_f, dff, FF_PLANE_SCALE}, m->weight(dec, layer, k, P_WOUT), residual(layer, k));
      return;
    }
    LinOut o = out_f32(ff, dff, dff, nullptr, 1);
    if (h2) { o.h = ff_h; o.ps = ps_f; o.ldh = dff; o.plane_scale = FF_PLANE_SCALE; }
    project_in(layer, k, o);
    project(LinIn{ff, ff_h, ps_f, dff, FF_PLANE_SCALE}, m->weight(dec, layer, k, P_WOUT), residual(layer, k));
  }
};

}  // namespace

// The layer-0 Q/K/V table of m (internal.h), made by the path it stands in for: the embedding copy of every table row into
// x planes with the site-0 row sums, then the layer-0 projection of those rows as ONE launch pinned to the ping-pong kernel.
// Saturation raises the ctx's sticky word like the launches it replaces. Scratch (x planes, row sums: 25 MB at the
// headline) lives for the call only. Not profiled: it is not part of a search.
int ensure_l0_table(rpr_ctx* c, rpr_model* m, hipStream_t s) {
  if (c->l0_mode <= 0 || effective_precision(c->precision, m->f32_only) != RPR_PREC_F16X2 || m->l0_state < 0 || m->l0_ready(c)) return RPR_OK;
  const auto& d = m->d;
  const size_t rows = m->l0_rows(), dm = d.d_model;
  if (!l0_table_fits(d.L, d.V, m->inner()) || rows >= ((size_t)1 << 30)) { m->l0_state = -1; return RPR_OK; }
  DevTmp x_h, ssq;
  if (!m->l0_table) {
    void* p = nullptr;
    if (hipMalloc(&p, m->l0_bytes()) != hipSuccess) { (void)hipGetLastError(); m->l0_state = -1; return RPR_OK; }
    m->owned.push_back(p);
    m->l0_table = reinterpret_cast<float*>(p);
  }
  if (x_h.alloc(rows * dm * 2 * sizeof(__half)) != hipSuccess || ssq.alloc(rows * 8) != hipSuccess) {
    (void)hipGetLastError();
    return RPR_OK;   // no scratch right now: this search keeps its GEMM, the next one tries again
  }
  struct Restore {
    rpr_ctx* c; int prec; bool prof;
    ~Restore() { c->precision = prec; c->profiling = prof; }
  } restore{c, c->precision, c->profiling};
  c->precision = RPR_PREC_F16X2; c->profiling = false;
  const DevBuf none{}, xb{x_h.p, rows * dm * 2 * sizeof(__half)}, sb{ssq.p, rows * 8};
  Launcher Ln{c, s};
  Pass p(Ln, m, {none, none, none, none, xb, none, none, sb, none}, true, 1, (int)rows, nullptr, (int)rows);
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_l0_table_embed(d.start_embed, d.in_embeds, (int)rows, (int)dm, s, p.embed_out()); });
  LinW w = m->weight(true, 0, 0, P_WIN);
  w.no_scratch = true; w.row_split_ok = true; w.force_pp = true;
  p.project(p.normed(0, 0), w, out_f32(m->l0_table, 3 * m->inner(), 3 * m->inner()));
  if (Ln.err) return Ln.err;
  RPR_HIP(hipStreamSynchronize(s));   // the scratch goes with this scope
  m->l0_valid = true; m->l0_epoch = c->l0_epoch; m->l0_state = 1;
  return RPR_OK;
}

// Encoder forward into ws.enc_out (reference generation.py:132-137 -> model.encoder(...)).
// packed = false: rows are [Q, Lq] padded (taps / rpr_encode return that layout).
// packed = true (the search path): only the positions before each query's last attended token exist, as rows
//   offs[q] .. offs[q] + last[q] - 1 (ws.offs / ws.last / ws.row_src, launch_pack_rows). The row count is only
//   known on the device, so every launch keeps its padded grid (hipGraph-safe) and tiles / rows past offs[Q] exit.
//   Padded positions are exp(-inf) keys and unused query rows in the padded layout, so results are identical.
void enqueue_encoder(Launcher& Ln, rpr_ctx* c, const rpr_model* m, int Q, int Lq, bool packed) {
  const auto& d = m->d;
  Workspace& w = c->ws;
  const int T = Q * Lq, inner = m->inner(), dm = d.d_model;
  hipStream_t s = Ln.s;
  float* qkv = P<float>(w.eqkv);
  const int32_t* offs = packed ? P<int32_t>(w.offs) : nullptr;
  const int* live = packed ? P<int>(w.offs) + Q : nullptr;   // device-side number of live rows
  const int Ta = T;                                            // rows accounted in the profile (flops / bytes)
  if (packed) {
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_pack_rows(P<int32_t>(w.last), P<int32_t>(w.offs), P<int32_t>(w.row_src), Q, Lq, s); });
  }
  Ln.account_live(live, T);   // profile pass: flops / bytes below are stated for T rows and scaled by the live count at flush
  Pass p(Ln, m, {w.ex, w.eh, w.eattn, w.eff, w.ex_h, w.eattn_h, w.eff_h, w.ssq_e, w.egu}, false, d.num_layers, T, live, Ta);
  p.zero_ssq();
  Ln.run(RPR_K_OTHER, 0, 2.0 * Ta * dm * 4, [&] {
    return launch_embed_rows(d.shared, P<int32_t>(w.ids), p.x, T, dm, d.vocab_size, s,
                             packed ? P<int32_t>(w.row_src) : nullptr, live, p.embed_out());
  });
  for (int i = 0; i < d.num_layers; ++i) {
    p.project_in(i, 0, out_f32(qkv, 3 * inner, 3 * inner));
    EncAttnArgs a{qkv, P<int32_t>(w.mask), d.enc_rel_bias, m->enc_bucket, p.attn, Q, Lq, d.num_heads, d.rel_buckets,
                  p.attn_planes(), p.ps_i, offs, P<int32_t>(w.last), c->status, 0};
    a.dkv = d.d_kv;
    Ln.run(RPR_K_ENC_ATTN, 4.0 * Q * d.num_heads * (double)Lq * Lq * d.d_kv * ((double)Ta / T) * ((double)Ta / T), 4.0 * Ta * 4 * inner,
           [&] { return launch_enc_attn(a, s); });
    p.attn_out(i, 0);
    p.ff_block(i, 1);
  }
  // final norm: fp32 copy always (taps / rpr_encode), planes for the cross-K/V GEMM in split mode
  Ln.run(RPR_K_RMSNORM, 0, 2.0 * Ta * dm * 4, [&] {
    return launch_rmsnorm(p.x, d.enc_final_ln, P<float>(w.enc_out), T, dm, p.xs.eps, s, 1.0f,
                          p.h2 ? P<__half>(w.enc_out_h) : nullptr, p.xs.ps, live, c->status, p.x_planes(), p.xs.ps);
  });
  p.check_ssq();
  c->enc_rows_accounted = Ta;
  Ln.account_live(nullptr, 0);
}

namespace {

BeamState beam_state(DevBuf (&score)[2], DevBuf (&lo)[2], DevBuf (&hi)[2], DevBuf (&tokens)[2], DevBuf (&anc)[2], int i, int L) {
  BeamState st;
  st.score = P<double>(score[i]); st.lo = P<int32_t>(lo[i]); st.hi = P<int32_t>(hi[i]);
  st.tokens = P<uint16_t>(tokens[i]); st.anc = P<uint16_t>(anc[i]); st.ld = L;
  return st;
}

// A batch of queries stepping through the decoder one position at a time: stage 0 = all queries of the call, later
// stages = the queries left over by a fork, compacted (live counts on the device, static launch geometry).
struct StageView {
  int Qcap;                        // query capacity = grid size of every launch
  const int* nq_dev;               // live queries / live rows (queries x beams) on the device; null = Qcap (stage 0)
  const int* nrows_dev;
  StageIO io;                      // qmap (null = identity), first encoder row (null = q * Lq), attended length, mask rows
  float* kcache; float* vcache;    // [nd][Qcap][H][depth][B][64] fp32: everything one (query, head) can touch is one
  int depth;                       //   contiguous depth*B*256-B region and the B rows of a position are adjacent
  BeamState st[2];                 // ping-pong by step parity
  size_t kv_q(int B, int inner) const { return (size_t)depth * B * inner; }
  int dkv = DKV;                   // head dim of the caches (64; 128 = t5-3b, which runs without forks)
  size_t kv_h(int B) const { return (size_t)depth * B * dkv; }
  size_t kv_layer(int B, int inner) const { return (size_t)Qcap * depth * B * inner; }
};

// Profile accounting of a compacted stage / tail job: the launches that follow state their flops and bytes for the
// static capacity `rows`; the record keeps the device counter and flush_profile scales by live / rows afterwards. Nothing
// is read back while the step is being enqueued (a synchronisation here would run the two lanes one after the other).
int live_count(Launcher& Ln, const int* dev, int rows) {
  Ln.account_live(dev, rows);
  return rows;
}

// index of prefix length p among the plan's (rpr_search_prefixes), -1 = not asked for
int depth_index(const SearchPlan& plan, int p) {
  for (int k = 0; k < plan.n_depths; ++k) if (plan.depths[k] == p) return k;
  return -1;
}

int xkv_ld(const rpr_model* m) { return m->d.num_decoder_layers * 2 * m->inner(); }   // row of ws.xkv: K | V of every decoder layer

// Decoder steps [t0, t1) of one stage: embed, nd x {self-attention over the beam's ancestry, cross-attention, FF},
// logits of position t, fused trie mask / top-B / beam expand (reference generation.py:423-526, one iteration per step).
void enqueue_steps(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const rpr_trie* tr, const SearchPlan& plan, const StageView& sv,
                   int t0, int t1, bool shared0, const rpr_debug_taps* taps) {
  const auto& d = m->d;
  Workspace& w = c->ws;
  const int Q = sv.Qcap, B = plan.B, L = plan.L, Lq = plan.Lq, R = Q * B, inner = m->inner(), dm = d.d_model, H = d.num_heads;
  const int nd = d.num_decoder_layers, V = d.V, Vp = m->Vp(), xld = xkv_ld(m);   // Vp: logits row / selection width (V padded to 64)
  hipStream_t s = Ln.s;
  float *qb = P<float>(w.q), *logits = P<float>(w.logits);
  const size_t layer_stride = sv.kv_layer(B, inner), kv_q = sv.kv_q(B, inner), kv_h = sv.kv_h(B), kv_pos = (size_t)B * sv.dkv, kv_slot = sv.dkv;
  int Rt = R, Bt = B;   // rows / beams per query of the current step's decoder pass
  const int Racc = live_count(Ln, sv.nrows_dev, R);   // rows the profile accounts for
  Pass p(Ln, m, {w.x, w.h, w.attn, w.ff, w.x_h, w.attn_h, w.ff_h, w.ssq_d, w.gu}, true, nd, R, sv.nrows_dev, Racc);
  if (Vp != V && !p.h2)   // exact-fp32 logits GEMM writes the V real columns of a row only: the padding must read as finite
    // (a kernel node: memset nodes captured into the search graph did not re-execute reliably on replay, see launch_zero_u64)
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_zero_u64(reinterpret_cast<unsigned long long*>(logits), (size_t)R * Vp / 2, s); });
  for (int t = t0; t < t1; ++t) {
    const BeamState cur = sv.st[t & 1], nxt = sv.st[(t + 1) & 1];
    Bt = (t == 0 && shared0) ? 1 : B; Rt = Q * Bt;
    const int Ma = (Bt == B) ? Racc : Rt;
    p.rows(Rt, Ma);
    p.zero_ssq(t > t0);
    Ln.run(RPR_K_OTHER, 0, 2.0 * Ma * dm * 4, [&] {
      return launch_dec_embed(d.start_embed, d.in_embeds, cur.tokens, L, p.x, Rt, dm, V, t, s, p.embed_out(), sv.nrows_dev);
    });
    for (int i = 0; i < nd; ++i) {
      float* kc = sv.kcache + i * layer_stride;
      float* vc = sv.vcache + i * layer_stride;
      {  // q -> qb, k/v -> cache row block of position t
        LinOut o{};
        o.f[0] = qb; o.f[1] = kc + (size_t)t * kv_pos; o.f[2] = vc + (size_t)t * kv_pos;
        o.ldo[0] = o.ldo[1] = o.ldo[2] = inner; o.split_n = inner;
        o.rm_B = Bt; o.rm_stride = kv_q; o.rm_slot = kv_slot; o.rm_head = kv_h; o.rm_dshift = sv.dkv == 128 ? 7 : 6;
        if (i == 0 && p.l0_replaces(plan, o))   // the row's q | k | v from the model's table, landing where the epilogue puts them
          Ln.run(RPR_K_OTHER, 0, 2.0 * Ma * 3 * inner * 4, [&] {
            return launch_dec_l0_qkv(m->l0_table, cur.tokens, L, Rt, V, d.L * V, t, inner, o.f[0], o.f[1], o.f[2], o.rm_B, o.rm_stride,
                                     o.rm_slot, o.rm_head, o.rm_dshift, sv.nrows_dev, s);
          });
        else
          p.project_in(i, 0, o);
      }
      {
        DecSelfAttnArgs a{qb, kc, vc, kv_q, kv_h, kv_pos, kv_slot, cur.anc, L, d.dec_rel_bias, m->dec_bucket, p.attn, Q, Bt, H, t,
                          p.attn_planes(), p.ps_i, c->status, sv.nq_dev};
        a.dkv = d.d_kv;
        Ln.run(RPR_K_DEC_SELF_ATTN, 4.0 * Ma * H * (double)(t + 1) * d.d_kv,
               4.0 * ((double)Ma * inner * 2 + 2.0 * Ma * (double)(t + 1) * inner), [&] { return launch_dec_self_attn(a, s); });
      }
      p.attn_out(i, 0);
      p.project_in(i, 1, out_f32(qb, inner, inner));
      {
        const float* xk = P<float>(w.xkv) + (size_t)i * 2 * inner;
        DecCrossAttnArgs a{qb, xk, xk + inner, xld, sv.io.mask, p.attn, Q, Bt, H, Lq, p.attn_planes(), p.ps_i,
                           sv.io.last, sv.io.offs, 0, c->status, sv.nq_dev};
        a.dkv = d.d_kv;
        Ln.run(RPR_K_DEC_CROSS_ATTN, 4.0 * Ma * H * (double)Lq * d.d_kv,
               4.0 * ((double)Ma * inner * 2 + 2.0 * (Ma / Bt) * (double)Lq * inner), [&] { return launch_step_cross_attn(a, s); });
      }
      p.attn_out(i, 1);
      p.ff_block(i, 2);
    }
    // logits of position t only (the reference computes every position and keeps [-1])
    float* lg = (taps && taps->step_logits) ? taps->step_logits + (size_t)t * R * V : logits;   // taps: V == Vp (rpr_search)
    {
      // codebook t (rpr_model::w_codebook: V fp32 rows, planes of Vp rows). The split kernel writes whole rows of Vp logits,
      // the exact-fp32 kernel the V real columns (the pad stays 0). The split-K scratch is not lent and the launcher's no-row-split state does not apply:
      // this product has never taken the mid-size split-K route nor set no_row_split, whoever calls enqueue_steps.
      // Its profile record is stated on V columns.
      LinW wt = m->w_codebook(t);
      wt.no_scratch = true; wt.row_split_ok = true;
      p.project(p.normed(nd, 0, d.dec_final_ln, p.post), wt, out_f32(lg, Vp, p.h2 ? Vp : V));
    }
    SelectArgs sa{};
    sa.logits = lg; sa.codes = tr->codes; sa.Lc = tr->L; sa.cur = cur; sa.nxt = nxt;
    sa.lb_scratch = P<int32_t>(w.lb); sa.Q = Q; sa.B = B; sa.V = Vp; sa.Vreal = V; sa.t = t;
    if (tr->lvl_V == tr->V) {
      sa.lvl0 = tr->lvl0; sa.lvl1 = tr->lvl1; sa.lvl_V = tr->lvl_V;
      sa.idx2 = tr->idx2; sa.n_deep = tr->n_deep;
      for (int i = 0; i < tr->n_deep; ++i) { sa.d_start[i] = tr->d_start[i]; sa.d_tok[i] = tr->d_tok[i]; sa.d_n[i] = tr->d_n[i]; }
    }
    if (w.sel_rs.p && select_radix_wanted(B, Vp) && w.sel_rs.cap >= select_radix_ws_bytes(Q, B, Vp))
      select_radix_carve(sa.rs, w.sel_rs.p, P<int32_t>(w.lb) + (size_t)R * Vp, Q, B, Vp);
    sa.log_softmax = plan.log_softmax() ? 1 : 0;
    sa.shared0 = (Bt != B) ? 1 : 0;
    sa.nq_dev = sv.nq_dev;
    if (taps) {
      sa.tap_scores = taps->step_scores ? taps->step_scores + (size_t)t * R : nullptr;
      sa.tap_tokens = taps->step_tokens ? taps->step_tokens + (size_t)t * R : nullptr;
      sa.tap_parent = taps->step_parent ? taps->step_parent + (size_t)t * R : nullptr;
      sa.tap_valid = taps->step_valid ? reinterpret_cast<unsigned long long*>(taps->step_valid) + (size_t)t * ((size_t)R * V / 64) : nullptr;
    }
    // the bitmap of this step, for the margin kernel (the shared step 0 needs none: every beam stands on the root)
    if (plan.margins && !sa.tap_valid && !sa.shared0) sa.tap_valid = P<unsigned long long>(w.mg_valid);
    Ln.run(RPR_K_SELECT, 0, (double)Ma * V * 4 + (double)Ma * 40, [&] { return launch_select(sa, s); });
    if (plan.margins) {
      // pruning margin of the step (rpr_search_margins): one more pass over the step's candidates, behind the selection
      MarginArgs ma{lg, cur.score, nxt.score, sa.tap_valid, tr->codes, tr->L, t, cur.lo, cur.hi, Q, B, Vp, V, sa.log_softmax,
                    sa.shared0, sv.nq_dev, sv.io.qmap, P<double>(w.o_margin)};
      Ln.run(RPR_K_SELECT, 0, (double)Ma * V * 4, [&] { return launch_prune_margin(ma, s); });
    }
    // a prefix length of the plan (rpr_search_prefixes): the beams of the queries walking in this stage after selection step
    // t are those of a search of length t + 1 — finalize's rule on them, into that length's staged outputs (before a fork
    // at this depth classifies: every query of the stage is still here)
    if (const int k = depth_index(plan, t + 1); k >= 0) {
      FinalizeArgs fa{nxt, Q, B, t + 1, P<int32_t>(w.d_tokens[k]), P<float>(w.d_scores[k]), P<int64_t>(w.d_lo[k]), P<int64_t>(w.d_hi[k]),
                      sv.nq_dev, sv.io.qmap};
      Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_finalize(fa, s); });
    }
  }
  if (t1 > t0) p.check_ssq();    // the last step's totals (the earlier steps': zero_ssq)
  Ln.account_live(nullptr, 0);   // the live counter of this stage scales THIS stage's records only (fork, tail, finalize follow)
}

// The fork after step T-1 of stage `sv`: which of its queries are forced (tail job `tb`), the others compacted into
// the next stage (`nb` / returned view): beam state, the K/V of the T positions walked so far, the cross-attention inputs.
// compact = false (optimistic mode, last fork): nobody walks on — a query that is not forced here only raises the ctx's
// sticky RPR_STATUS_TAIL_LEFTOVER word and the caller repeats the batch in the exact mode.
StageView enqueue_fork(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const rpr_trie* tr, const SearchPlan& plan, const StageView& sv,
                       int T, int next_depth, TailBufs& tb, StageBufs& nb, bool compact) {
  const auto& d = m->d;
  const int Q = sv.Qcap, B = plan.B, L = plan.L, Lq = plan.Lq, inner = m->inner(), nd = d.num_decoder_layers, H = d.num_heads;
  hipStream_t s = Ln.s;
  const BeamState st = sv.st[T & 1];
  // No masked candidate may overtake a valid one during the remaining n = L - T steps. With |logit| <= bound
  // (rpr_model::logit_bound) the valid candidates of a step are >= smin - n*bound and the masked ones
  // <= smax + n*bound - 1e9, so forced requires (smax - smin) + 2*n*bound < 1e9; a tenth of that is demanded.
  // Log-softmax scores: a step adds a log-probability in [-(2*bound + ln V), 0] instead of a logit in [-bound, bound].
  const double per_step = plan.log_softmax() ? 2.0 * (double)m->logit_bound + log((double)d.V) : 2.0 * (double)m->logit_bound;
  const double spread_max = 1e8 - (double)(L - T) * per_step;
  const int extras = plan.extras, pool = plan.pool;   // forced with extras (common.h: ForkScanArgs): the budget per query, the stage's spare tail entries
  ForkArgs fa{st, tr->codes, tr->L, Q, sv.nq_dev, B, T, L, spread_max, P<int32_t>(tb.flag), extras};
  Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_fork_classify(fa, s); });
  const ForkScanArgs fs{P<int32_t>(tb.flag), Q, sv.nq_dev, B, L - T, P<int32_t>(tb.flist), P<int32_t>(tb.cnt), P<int32_t>(nb.src),
                        P<int32_t>(nb.cnt), P<int32_t>(tb.kvq), P<int32_t>(tb.spare), pool};
  Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_fork_scan(fs, s); });
  if (pool > 0) {
    const ForkExtrasArgs fe{st, tr->codes, tr->L, Q, B, T, L, pool, P<int32_t>(tb.spare)};
    Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_fork_extras(fe, s); });
  }
  // tail job: per-entry inputs (a spare entry: its owner's) and the full token rows of the forced beams
  Ln.run(RPR_K_FORK, 0, 0, [&] {
    return launch_gather_stage_io(sv.io, StageOut{P<int32_t>(tb.qmap), P<int32_t>(tb.offs), P<int32_t>(tb.last), P<int32_t>(tb.mask)},
                                  P<int32_t>(tb.kvq), P<int>(tb.cnt), Q + pool, Lq, s);
  });
  Ln.run(RPR_K_FORK, 0, 0, [&] {
    return launch_tail_tokens(st, tr->codes, tr->L, P<int32_t>(tb.flist), P<int>(tb.cnt), Q + pool, B, T, L, P<uint16_t>(tb.tokens), s);
  });
  // next stage
  StageView nv{};
  if (!compact) {
    Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_flag_nonzero(P<int>(nb.cnt), c->status + 2, s); });
    return nv;
  }
  nv.Qcap = Q; nv.nq_dev = P<int>(nb.cnt); nv.nrows_dev = P<int>(nb.cnt) + 1;
  nv.io = StageIO{P<int32_t>(nb.qmap), P<int32_t>(nb.offs), P<int32_t>(nb.last), P<int32_t>(nb.mask)};
  nv.kcache = P<float>(nb.kcache); nv.vcache = P<float>(nb.vcache); nv.depth = next_depth; nv.dkv = sv.dkv;
  for (int i = 0; i < 2; ++i) nv.st[i] = beam_state(nb.score, nb.lo, nb.hi, nb.tokens, nb.anc, i, L);
  Ln.run(RPR_K_FORK, 0, 0, [&] {
    return launch_gather_stage_io(sv.io, StageOut{P<int32_t>(nb.qmap), P<int32_t>(nb.offs), P<int32_t>(nb.last), P<int32_t>(nb.mask)},
                                  P<int32_t>(nb.src), nv.nq_dev, Q, Lq, s);
  });
  Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_compact_beams(st, nv.st[T & 1], P<int32_t>(nb.src), nv.nq_dev, Q, B, T, s); });
  KvCopyArgs kc{sv.kcache, sv.vcache, nv.kcache, nv.vcache, sv.kv_layer(B, inner), sv.kv_q(B, inner), sv.kv_h(B),
                nv.kv_layer(B, inner), nv.kv_q(B, inner), nv.kv_h(B), P<int32_t>(nb.src), nv.nq_dev, Q, nd, H, T * B * sv.dkv};
  Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_kv_copy(kc, s); });
  return nv;
}

// Tail pass of one fork: the remaining positions T..L-1 of every forced beam in ONE teacher-forced decoder pass
// (rows = forced queries x beams x (L - T), sequence-major), then the replay of the selection order and finalize.
// Same layer arithmetic as the sequential steps; self-attention reads the positions < T from the fork stage's KV cache
// through the beams' ancestry and the positions >= T from this pass's own K/V rows; the B*(L-T) rows of a query share
// its encoder K/V in cross-attention; instead of V logits per row only the logit of the row's (only valid) token is
// computed, in exact fp32 (tail_gold_kernel).
void enqueue_tail(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const rpr_trie* tr, const SearchPlan& plan, const StageView& sv, int T,
                  TailBufs& tb) {
  const auto& d = m->d;
  Workspace& w = c->ws;
  const int pool = plan.pool;
  const int Q = sv.Qcap + pool;   // tail entries: the stage's queries and the spare entries of those forced with extras
  const int B = plan.B, L = plan.L, Lq = plan.Lq, Lt = L - T, S = Q * B, R = S * Lt;
  const int inner = m->inner(), dm = d.d_model, H = d.num_heads, nd = d.num_decoder_layers, V = d.V, xld = xkv_ld(m);
  hipStream_t s = Ln.s;
  const int* nf_dev = P<int>(tb.cnt);
  const int* nseq_dev = nf_dev + 1;
  const int* nrows_dev = nf_dev + 2;
  const int Ra = live_count(Ln, nrows_dev, R);
  float *qkv = P<float>(w.t_qkv), *qb = P<float>(w.t_q);
  Pass p(Ln, m, {w.t_x, w.t_h, w.t_attn, w.t_ff, w.t_x_h, w.t_attn_h, w.t_ff_h, w.t_ssq, w.t_gu}, true, nd, R, nrows_dev, Ra);
  p.zero_ssq();
  // MFMA shape of the pass's 256x256 GEMM launches (SearchPlan::mfma16). A tail pass scores sequences that are already chosen:
  // its rounding reaches the returned scores, never which sequences survive the steps — those launches (encoder, steps, the
  // layer-0 table) keep the 32x32x16 arithmetic, and so does the layer-0 projection the table stands in for, below.
  // One exception: a query forced WITH EXTRAS (plan.extras > 0) brings B + extras sequences, and tail_rank_extras keeps the best
  // B of them by this pass's scores — that one pruning decision sees the pass's rounding (a few 1e-6 on either shape).
  Launcher::Mfma16Scope tail_shape(Ln, plan.mfma16);
  Ln.run(RPR_K_OTHER, 0, 2.0 * Ra * dm * 4, [&] {
    return launch_tail_embed(d.in_embeds, P<uint16_t>(tb.tokens), p.x, R, nrows_dev, T, L, dm, V, s, p.embed_out());
  });
  const size_t kv_pos = (size_t)B * sv.dkv;
  for (int i = 0; i < nd; ++i) {
    const LinOut o_qkv = out_f32(qkv, 3 * inner, 3 * inner);
    if (i == 0) {   // layer 0 on the table's arithmetic: the gate asks the planner about the launch that would run, flag included
      Launcher::Mfma16Scope l0_shape(Ln, 0);
      if (p.l0_replaces(plan, o_qkv))   // the rows of the model's (position, token) table instead of the projection
        Ln.run(RPR_K_OTHER, 0, 2.0 * Ra * 3 * inner * 4, [&] {
          return launch_tail_l0_qkv(m->l0_table, P<uint16_t>(tb.tokens), qkv, R, nrows_dev, T, L, V, 3 * inner, s);
        });
      else
        p.project_in(i, 0, o_qkv);
    } else
      p.project_in(i, 0, o_qkv);
    {
      const size_t ls = sv.kv_layer(B, inner);
      TailSelfAttnArgs a{qkv, sv.kcache + i * ls, sv.vcache + i * ls, sv.kv_q(B, inner), sv.kv_h(B), kv_pos, (size_t)sv.dkv,
                         sv.st[T & 1].anc, L, P<int32_t>(tb.flist), nseq_dev, d.dec_rel_bias, m->dec_bucket, p.attn,
                         p.attn_planes(), p.ps_i, c->status, S, B, H, T, L};
      a.dkv = d.d_kv;
      a.kvq = P<int32_t>(tb.kvq);
      Ln.run(RPR_K_TAIL_SELF_ATTN, 2.0 * Ra * H * (double)(L + T + 1) * sv.dkv, 4.0 * ((double)Ra * 4 * inner + 2.0 * (Ra / Lt) * (double)T * inner),
             [&] { return launch_tail_self_attn(a, s); });
    }
    p.attn_out(i, 0);
    p.project_in(i, 1, out_f32(qb, inner, inner));
    {
      const float* xk = P<float>(w.xkv) + (size_t)i * 2 * inner;
      DecCrossAttnArgs a{qb, xk, xk + inner, xld, P<int32_t>(tb.mask), p.attn, Q, B * Lt, H, Lq, p.attn_planes(), p.ps_i,
                         P<int32_t>(tb.last), P<int32_t>(tb.offs), 0, c->status, nf_dev};
      a.dkv = d.d_kv;
      Ln.run(RPR_K_DEC_CROSS_ATTN, 4.0 * Ra * H * (double)Lq * sv.dkv, 4.0 * ((double)Ra * inner * 2 + 2.0 * (Ra / (B * Lt)) * (double)Lq * inner),
             [&] { return launch_tail_cross_attn(a, s); });
    }
    p.attn_out(i, 1);
    p.ff_block(i, 2);
  }
  p.check_ssq();
  if (plan.log_softmax()) {
    // the score of a position is the log-probability of its token: final RMSNorm of every row, the V logits of the rows
    // of one position per launch of the exact-fp32 GEMM (rows of a position are Lt apart; its codebook is out_embeds[pos]),
    // then log_softmax at the token (tail_logprob_kernel)
    float* lg = P<float>(w.t_logits);
    Ln.run(RPR_K_RMSNORM, 0, 2.0 * Ra * dm * 4, [&] {
      return launch_rmsnorm(p.x, d.dec_final_ln, p.h, R, dm, p.xs.eps, s, p.post, nullptr, 0, nrows_dev, nullptr, p.x_planes(), p.xs.ps);
    });
    for (int pos = T; pos < L; ++pos) {
      GemmArgs g{};
      g.A = p.h + (size_t)(pos - T) * dm; g.lda = Lt * dm;
      g.W = d.out_embeds + (size_t)pos * V * dm; g.ldw = dm;
      for (int i = 0; i < 3; ++i) { g.out[i] = lg + (size_t)(pos - T) * V; g.ldo[i] = Lt * V; }
      g.split_n = V; g.M = S; g.N = V; g.K = dm; g.m_dev = nseq_dev;
      Ln.run(RPR_K_GEMM_SMALL, 2.0 * (Ra / Lt) * (double)V * dm, 4.0 * ((double)(Ra / Lt) * (dm + V) + (double)V * dm),
             [&] { return launch_gemm(g, s); });
    }
    Ln.run(RPR_K_OTHER, 0, 4.0 * Ra * V, [&] {
      return launch_tail_logprob(lg, P<uint16_t>(tb.tokens), P<float>(tb.gold), R, nrows_dev, T, L, V, s);
    });
  } else {
    Ln.run(RPR_K_OTHER, 2.0 * Ra * dm, 4.0 * 2 * Ra * dm, [&] {
      return launch_tail_gold(p.x, d.dec_final_ln, d.out_embeds, P<uint16_t>(tb.tokens), P<float>(tb.gold), R, nrows_dev, T, L, dm, V, p.xs.eps,
                              p.post, s, p.x_planes(), p.xs.ps);
    });
  }
  TailRankArgs ra{sv.st[T & 1], P<int32_t>(tb.flist), P<int32_t>(tb.qmap), nf_dev + 3, P<uint16_t>(tb.tokens), P<float>(tb.gold), sv.Qcap, B, T, L,
                  P<int32_t>(w.o_tokens), P<float>(w.o_scores), P<int64_t>(w.o_lo), P<int64_t>(w.o_hi)};
  ra.spare = P<int32_t>(tb.spare); ra.pool = pool; ra.codes = tr->codes; ra.Lc = tr->L;
  Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_tail_rank(ra, s); });
  // the prefix lengths behind this fork (rpr_search_prefixes): the same rule stopped at p, on the same gold scores
  for (int k = 0; k < plan.n_depths; ++k) {
    if (plan.depths[k] <= T) continue;
    TailRankArgs rp = ra;
    rp.Lr = plan.depths[k];
    rp.out_tokens = P<int32_t>(w.d_tokens[k]); rp.out_scores = P<float>(w.d_scores[k]);
    rp.out_lo = P<int64_t>(w.d_lo[k]); rp.out_hi = P<int64_t>(w.d_hi[k]);
    Ln.run(RPR_K_FORK, 0, 0, [&] { return launch_tail_rank(rp, s); });
  }
  Ln.account_live(nullptr, 0);
}

}  // namespace

// Everything between the staged inputs (ws.ids/ws.mask) and the staged outputs (ws.o_*).
void enqueue_search(Launcher& Ln, rpr_ctx* c, const rpr_model* m, const rpr_trie* tr, const SearchPlan& plan, const rpr_debug_taps* taps) {
  const auto& d = m->d;
  Workspace& w = c->ws;
  const int Q = plan.Q, Lq = plan.Lq, B = plan.B, L = plan.L, nf = plan.n_forks;
  const int* forks = plan.forks;
  const int T = Q * Lq, dm = d.d_model, xld = xkv_ld(m);
  hipStream_t s = Ln.s;
  Ln.cus = plan.cus;
  // index of the last attended key + 1 per query: row packing of the encoder and the cross-attention loop bound
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_mask_lengths(P<int32_t>(w.mask), P<int32_t>(w.last), Q, Lq, s, c->status + 1); });
  const bool packed = !taps;   // taps return the padded [Q, Lq, d] encoder output
  Ln.no_row_split = packed ? 1 : 0;   // the packed rows' capacity says nothing about the live rows (reset below, after the cross-K/V product)
  enqueue_encoder(Ln, c, m, Q, Lq, packed);
  if (taps && taps->encoder_out && !Ln.err) {
    hipError_t e = hipMemcpyAsync(taps->encoder_out, w.enc_out.p, (size_t)T * dm * 4, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { Ln.err = hip_fail(e, "tap copy", __FILE__, __LINE__); return; }
  }
  // cross-attention K/V of every decoder layer in one GEMM (shared by the B beams of a query;
  // the reference recomputes them for every beam at every step)
  Ln.account_live(packed ? P<int>(w.offs) + Q : nullptr, T);
  linear(Ln, {P<float>(w.enc_out), P<__half>(w.enc_out_h), (size_t)T * dm, dm}, m->w_xkv(), T,
         out_f32(P<float>(w.xkv), xld, xld), packed ? P<int>(w.offs) + Q : nullptr, c->enc_rows_accounted);
  Ln.account_live(nullptr, 0);
  Ln.no_row_split = 0;

  StageView sv{};
  sv.Qcap = Q;
  sv.io = StageIO{nullptr, packed ? P<int32_t>(w.offs) : nullptr, P<int32_t>(w.last), P<int32_t>(w.mask)};
  sv.kcache = P<float>(w.kcache); sv.vcache = P<float>(w.vcache); sv.depth = nf ? forks[0] : L; sv.dkv = d.d_kv;
  for (int i = 0; i < 2; ++i) sv.st[i] = beam_state(w.score, w.lo, w.hi, w.tokens, w.anc, i, L);
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_init_beams(sv.st[0], Q, B, tr->N, s); });
  if (plan.margins) Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_margin_init(P<double>(w.o_margin), Q, s); });
  if (w.sel_rs.p && select_radix_wanted(B, m->Vp()) && w.sel_rs.cap >= select_radix_ws_bytes(Q, B, m->Vp())) {
    RadixWs rs;   // the radix selection's histograms and counters start at zero (every step leaves them so)
    select_radix_carve(rs, w.sel_rs.p, nullptr, Q, B, m->Vp());
    Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_select_radix_reset(rs, Q, s); });
  }

  // Step 0: every beam of a query starts from the same start embedding and the same encoder states, so the
  // decoder pass is computed once per query (Q rows, "one beam") and select reads the shared logits row; the
  // position-0 K/V exist in slot 0 only and every beam's ancestry points there. (The reference recomputes
  // the B identical rows; beams 1..B-1 differ only by their -1e9 initial score, generation.py:418-420.)
  // Off when debug taps are requested (they expect [Q*B, V] logits per step).
  const bool shared0 = !taps && B > 1;
  // Stages: stage 0 (all queries) walks steps [0, forks[0]); at every fork the forced queries get their tail pass and
  // the others are compacted into the next stage, which walks on to the next fork (or to L); finalize ranks whoever is
  // still stepping at L. Without forks this is the plain loop of the reference.
  // Everything after the first fork works on what that fork left over — usually a handful of queries in buffers sized for
  // all of them: those GEMMs are enqueued as large-tile / small-tile pairs gated on the live count (GemmH2Args.small_live)
  constexpr int small_live_rows = 1024;
  int t0 = 0;
  for (int k = 0; k <= nf; ++k) {
    const int t1 = k < nf ? forks[k] : L;
    Ln.small_live = k >= 1 ? small_live_rows : 0;
    enqueue_steps(Ln, c, m, tr, plan, sv, t0, t1, shared0, taps);
    if (k < nf) {
      const int next_depth = k + 1 < nf ? forks[k + 1] : L;
      const bool last_dropped = plan.drop_last && k + 1 == nf;
      const StageView nv = enqueue_fork(Ln, c, m, tr, plan, sv, t1, next_depth, w.tail[k], w.stage[k], !last_dropped);
      enqueue_tail(Ln, c, m, tr, plan, sv, t1, w.tail[k]);
      if (last_dropped) return;   // every query was finished by a tail pass (or flagged)
      sv = nv;
    }
    t0 = t1;
  }
  FinalizeArgs fa{sv.st[L & 1], sv.Qcap, B, L, P<int32_t>(w.o_tokens), P<float>(w.o_scores),
                  P<int64_t>(w.o_lo), P<int64_t>(w.o_hi), sv.nq_dev, sv.io.qmap};
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_finalize(fa, s); });
}

// Teacher-forced forward of the prefix-oriented ranking fine-tune step: reference
// T5SeqAQEncoderForLngKnpMarginMSE.forward (modeling/t5_generative_retriever.py:902-966). The encoder runs once per
// query (the positive and the negative example of a row carry the same query text, dataset/dataset.py:502-503: the
// reference encodes it twice); the decoder runs over all L positions of the n_docs smtids of every query at once:
// rows (q, doc, position) = bz * n_docs * L, causal block self-attention per (sequence, head), cross-attention with
// the n_docs * L rows of a query sharing its encoder K/V. Output: the gold-code score of every position.
void enqueue_train_forward(Launcher& Ln, rpr_ctx* c, const rpr_model* m, int bz, int Lq, int ndoc, int L,
                           const int32_t* codes /*[bz, ndoc, L]*/, float* pos_scores /*[bz, ndoc, L]*/, float* hidden) {
  const auto& d = m->d;
  Workspace& w = c->ws;
  const int T = bz * Lq, S = bz * ndoc, R = S * L, inner = m->inner(), dm = d.d_model, H = d.num_heads;
  const int nd = d.num_decoder_layers, V = d.V;
  hipStream_t s = Ln.s;
  Ln.run(RPR_K_OTHER, 0, 0, [&] { return launch_mask_lengths(P<int32_t>(w.mask), P<int32_t>(w.last), bz, Lq, s, c->status + 1); });
  Ln.no_row_split = 1;
  enqueue_encoder(Ln, c, m, bz, Lq, true);
  const int xld = xkv_ld(m);
  linear(Ln, {P<float>(w.enc_out), P<__half>(w.enc_out_h), (size_t)T * dm, dm}, m->w_xkv(), T,
         out_f32(P<float>(w.xkv), xld, xld), P<int>(w.offs) + bz, c->enc_rows_accounted);
  Ln.account_live(nullptr, 0);
  Ln.no_row_split = 0;

  float *qkv = P<float>(w.tr_x), *qb = P<float>(w.q);
  Pass p(Ln, m, {w.x, w.h, w.attn, w.ff, w.x_h, w.attn_h, w.ff_h, w.ssq_d, w.gu}, true, nd, R, nullptr, R);   // every row is live
  p.zero_ssq();
  Ln.run(RPR_K_OTHER, 0, 2.0 * R * dm * 4, [&] {
    return launch_train_dec_embed(d.start_embed, d.in_embeds, codes, p.x, S, L, dm, V, s, p.embed_out());
  });
  for (int i = 0; i < nd; ++i) {
    p.project_in(i, 0, out_f32(qkv, 3 * inner, 3 * inner));
    {  // causal self-attention of every sequence over its own L positions (decoder relative-position table)
      EncAttnArgs a{qkv, nullptr, d.dec_rel_bias, m->dec_bucket, p.attn, S, L, H, d.rel_buckets,
                    p.attn_planes(), p.ps_i, nullptr, nullptr, c->status, 1, 0, d.d_kv};
      Ln.run(RPR_K_ENC_ATTN, 2.0 * S * H * (double)L * L * d.d_kv, 4.0 * R * 4 * inner, [&] { return launch_enc_attn(a, s); });
    }
    p.attn_out(i, 0);
    p.project_in(i, 1, out_f32(qb, inner, inner));
    {
      const float* xk = P<float>(w.xkv) + (size_t)i * 2 * inner;
      DecCrossAttnArgs a{qb, xk, xk + inner, xld, P<int32_t>(w.mask), p.attn, bz, ndoc * L, H, Lq, p.attn_planes(), p.ps_i,
                         P<int32_t>(w.last), P<int32_t>(w.offs), 0, c->status, nullptr, d.d_kv};
      Ln.run(RPR_K_DEC_CROSS_ATTN, 4.0 * R * H * (double)Lq * d.d_kv, 4.0 * ((double)R * inner * 2 + 2.0 * bz * (double)Lq * inner),
             [&] { return launch_dec_cross_attn(a, s); });
    }
    p.attn_out(i, 1);
    p.ff_block(i, 2);
  }
  p.check_ssq();
  // decoder_last_hidden_state (final RMSNorm, scaleup factor) dotted with the gold codes' OUTPUT codebook rows — or, for
  // rpr_embed, written out as it is
  Ln.run(RPR_K_OTHER, 2.0 * R * dm, 4.0 * 2 * R * dm, [&] {
    return launch_gold_scores(p.x, d.dec_final_ln, d.out_embeds, codes, pos_scores, S, L, dm, V, p.xs.eps, p.post, s,
                              p.x_planes(), p.xs.ps, hidden);
  });
}

int alloc_train_workspace(rpr_ctx* c, const rpr_model* m, int bz, int Lq, int ndoc, int L) {
  // the search workspace for bz queries with ndoc * L "beams" of one position covers every shared buffer
  int e = alloc_workspace(c, m, plain_plan(bz, Lq, ndoc * L, 1));
  if (e) return e;
  const size_t R = (size_t)bz * ndoc * L;
  e = ensure(c, c->ws.tr_x, R * 3 * m->inner() * sizeof(float));
  if (e) return e;
  return ensure(c, c->ws.tr_misc, R * sizeof(float) + R * sizeof(int32_t) + 4096);
}

}  // namespace rpr
