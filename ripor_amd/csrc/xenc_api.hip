// C ABI of the cross-encoder teacher: rpr_xenc_load / rpr_xenc_free / rpr_xenc_score and the opt-in f16 mode,
// rpr_xenc_set_precision. One layer walk (xenc_forward) over two modes: fp32 (kernels in xenc_kernels.hip, the products
// through the exact-fp32 GEMM of gemm_f32.hip) and f16 operands (xenc_half.hip); DESIGN.md §9f.
#include <new>
#include <vector>

#include "internal.h"

using namespace rpr;

struct rpr_xenc {
  rpr_ctx* ctx;
  rpr_xenc_desc d;
  int device;                    // of ctx, kept here: the model may outlive a look at its ctx
  int precision = RPR_XENC_F32;
  __half* wh = nullptr;          // f16 copies of qkv_w | ao_w | ff1_w | ff2_w (one allocation, made by the first switch to f16)
  const __half *qkv_h = nullptr, *ao_h = nullptr, *ff1_h = nullptr, *ff2_h = nullptr;
};

namespace {

// What the steps of one rpr_xenc_score call share. A mode (below) adds its weights and says how a step is launched and
// what it costs; the walk (xenc_forward) owns the order, the buffers and the weight offsets.
template <class E>
struct XencCall {
  using Elem = E;                  // of QKV, CTX and FF
  Launcher Ln;
  const rpr_xenc_desc& d;
  int T, H, F, dh, ntiles;
  double Td, qk_pairs;             // rows; pairs of keys a query tile meets: 64 x len per tile (an upper bound on a sequence's last)
  float *X, *TMP;                  // hidden states (the residual stream), a product's raw result
  Elem *QKV, *CTX, *FF;            // q | k | v, attention output, feed-forward intermediate
  __half* Xh;                      // f16 mode: the hidden states once more
  const int2* tiles;
  const int32_t* off_dev;
};

// fp32: the exact GEMM has no epilogue, so the biases are added by attention, bias_gelu and add_ln
struct XencF32 : XencCall<float> {
  using Call = XencCall<float>;
  static constexpr bool HALF_X = false;
  const float *qkv_w, *ao_w, *ff1_w, *ff2_w;
  XencF32(const Call& k, const rpr_xenc* x) : Call(k), qkv_w(x->d.qkv_w), ao_w(x->d.ao_w), ff1_w(x->d.ff1_w), ff2_w(x->d.ff2_w) {}

  void gemm(const float* A, const float* W, int N, int K, float* out) {
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K;
    g.out[0] = out; g.ldo[0] = N; g.split_n = N;
    g.M = T; g.N = N; g.K = K;
    Ln.run(RPR_K_GEMM, 2.0 * Td * N * K, 4.0 * (Td * (N + K) + (double)N * K), [&] { return launch_gemm(g, Ln.s); });
  }
  void embed(const XencEmbedArgs& ea) {
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, 4.0 * 4 * Td * H, [&] { return launch_xenc_embed_ln(ea, nullptr, Ln.s); });
  }
  void project_qkv(const float* W, const float*) { gemm(X, W, 3 * H, H, QKV); }
  void attend(const float* bias) {
    XencAttnArgs aa{QKV, bias, off_dev, tiles, ntiles, H, d.heads, CTX};
    Ln.run(RPR_K_ENC_ATTN, 4.0 * qk_pairs * H, 4.0 * 4 * Td * H, [&] { return launch_xenc_attn(aa, dh, Ln.s); });
  }
  void project_add_ln(const float* A, const float* W, const float* bias, int K, const float* ln_w, const float* ln_b) {
    gemm(A, W, H, K, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, 4.0 * 3 * Td * H,
           [&] { return launch_xenc_add_ln(TMP, bias, X, ln_w, ln_b, d.ln_eps, T, H, X, nullptr, Ln.s); });
  }
  void project_gelu(const float* W, const float* bias) {
    gemm(X, W, F, H, FF);
    Ln.run(RPR_K_OTHER, 10.0 * Td * F, 4.0 * 2 * Td * F, [&] { return launch_xenc_bias_gelu(FF, bias, T, F, Ln.s); });
  }
};

// f16 operands: bias, GELU and the residual sit in the GEMM epilogues; X stays fp32, Xh feeds the products
struct XencF16 : XencCall<__half> {
  using Call = XencCall<__half>;
  static constexpr bool HALF_X = true;
  const __half *qkv_w, *ao_w, *ff1_w, *ff2_w;
  XencF16(const Call& k, const rpr_xenc* x) : Call(k), qkv_w(x->qkv_h), ao_w(x->ao_h), ff1_w(x->ff1_h), ff2_w(x->ff2_h) {}

  // bytes: f16 operands; out_b = bytes per output element written (+ read, for the residual)
  void gemm(int epi, const __half* A, const __half* W, const float* bias, int N, int K, __half* outh, float* outf) {
    const double out_b = epi == XENC_EPI_RESID ? 8.0 : 2.0;
    Ln.run(RPR_K_GEMM, 2.0 * Td * N * K, 2.0 * (Td * K + (double)N * K) + out_b * Td * N,
           [&] { return launch_xenc_gemm_h(epi, A, W, bias, epi == XENC_EPI_RESID ? X : nullptr, outh, outf, T, N, K, Ln.s); });
  }
  void embed(const XencEmbedArgs& ea) {
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, (4.0 * 4 + 2.0) * Td * H, [&] { return launch_xenc_embed_ln(ea, Xh, Ln.s); });
  }
  void project_qkv(const __half* W, const float* bias) { gemm(XENC_EPI_BIAS, Xh, W, bias, 3 * H, H, QKV, nullptr); }
  void attend(const float*) {
    Ln.run(RPR_K_ENC_ATTN, 4.0 * qk_pairs * H, 2.0 * 4 * Td * H,
           [&] { return launch_xenc_attn_h(QKV, off_dev, tiles, ntiles, H, d.heads, dh, CTX, Ln.s); });
  }
  void project_add_ln(const __half* A, const __half* W, const float* bias, int K, const float* ln_w, const float* ln_b) {
    gemm(XENC_EPI_RESID, A, W, bias, H, K, nullptr, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, (4.0 * 2 + 2.0) * Td * H,
           [&] { return launch_xenc_add_ln(TMP, nullptr, nullptr, ln_w, ln_b, d.ln_eps, T, H, X, Xh, Ln.s); });
  }
  void project_gelu(const __half* W, const float* bias) { gemm(XENC_EPI_BIAS_GELU, Xh, W, bias, F, H, FF, nullptr); }
};

// the forward over a packed batch, once for both modes: meta = the attention kernel's tile list, then the sequence offsets
template <class Mode>
int xenc_forward(rpr_ctx* c, const rpr_xenc* x, const int32_t* input_ids, const int32_t* token_type_ids, const int32_t* position_ids,
                 const int32_t* seq_off, int32_t bz, const std::vector<int32_t>& meta, int ntiles, float* out_scores, hipStream_t s) {
  const rpr_xenc_desc& d = x->d;
  const int H = d.hidden, F = d.d_ff, T = seq_off[bz];
  Workspace& w = c->ws;
  using Elem = typename Mode::Elem;
  const size_t TH = (size_t)T * H, el = sizeof(Elem);
  const struct { DevBuf& buf; size_t n, size; } need[] = {
      {w.xe_x, TH, sizeof(float)}, {w.xe_qkv, 3 * TH, el}, {w.xe_ctx, TH, el}, {w.xe_tmp, TH, sizeof(float)}, {w.xe_ff, (size_t)T * F, el},
      {w.xe_meta, meta.size(), sizeof(int32_t)}, {w.xe_xh, Mode::HALF_X ? TH : 0, sizeof(__half)}};
  for (const auto& r : need)
    if (const int e = ensure(c, r.buf, r.n * r.size)) return e;

  double qk_pairs = 0.0;
  for (int b = 0; b < bz; ++b) { const double len = seq_off[b + 1] - seq_off[b]; qk_pairs += len * len; }
  Mode m(typename Mode::Call{Launcher{c, s}, d, T, H, F, H / d.heads, ntiles, (double)T, qk_pairs, P<float>(w.xe_x), P<float>(w.xe_tmp),
                             P<Elem>(w.xe_qkv), P<Elem>(w.xe_ctx), P<Elem>(w.xe_ff), P<__half>(w.xe_xh), P<int2>(w.xe_meta),
                             P<int32_t>(w.xe_meta) + (size_t)2 * ntiles},
         x);
  Launcher& Ln = m.Ln;
  Ln.run(RPR_K_OTHER, 0, 4.0 * meta.size(), [&] { return launch_xenc_meta(meta.data(), (int)meta.size(), P<int32_t>(w.xe_meta), s); });
  m.embed(XencEmbedArgs{input_ids, token_type_ids, position_ids, T, H, d.vocab_size, d.type_vocab, d.max_pos,
                        d.word_emb, d.type_emb, d.pos_emb, d.emb_ln_w, d.emb_ln_b, d.ln_eps, m.X});
  for (int l = 0; l < d.layers; ++l) {
    const size_t HH = (size_t)H * H, FH = (size_t)F * H, lH = (size_t)l * H;
    m.project_qkv(m.qkv_w + l * 3 * HH, d.qkv_b + 3 * lH);
    m.attend(d.qkv_b + 3 * lH);
    m.project_add_ln(m.CTX, m.ao_w + l * HH, d.ao_b + lH, H, d.ln1_w + lH, d.ln1_b + lH);
    m.project_gelu(m.ff1_w + l * FH, d.ff1_b + (size_t)l * F);
    m.project_add_ln(m.FF, m.ff2_w + l * FH, d.ff2_b + lH, F, d.ln2_w + lH, d.ln2_b + lH);
  }
  Ln.run(RPR_K_OTHER, 2.0 * bz * ((double)H * H + H), 4.0 * ((double)H * H + 2.0 * bz * H), [&] {
    return launch_xenc_head(m.X, m.off_dev, bz, H, d.pool_w, d.pool_b, d.cls_w, d.cls_b, out_scores, s);
  });
  return Ln.err;
}

}  // namespace

extern "C" {

int rpr_xenc_load(rpr_ctx* c, const rpr_xenc_desc* d, rpr_xenc** out) {
  RPR_REQUIRE(c && d && out, "NULL argument");
  RPR_REQUIRE(d->vocab_size >= 1 && d->hidden >= 1 && d->layers >= 1 && d->heads >= 1 && d->d_ff >= 1 && d->max_pos >= 1 &&
              d->type_vocab >= 1, "a dimension of the cross-encoder is below 1");
  RPR_REQUIRE(d->hidden % d->heads == 0, "hidden is not a multiple of heads");
  RPR_REQUIRE(d->ln_eps >= 0.f, "ln_eps is negative");
  RPR_REQUIRE(d->word_emb && d->pos_emb && d->type_emb && d->emb_ln_w && d->emb_ln_b && d->qkv_w && d->qkv_b && d->ao_w && d->ao_b &&
              d->ln1_w && d->ln1_b && d->ff1_w && d->ff1_b && d->ff2_w && d->ff2_b && d->ln2_w && d->ln2_b && d->pool_w && d->pool_b &&
              d->cls_w && d->cls_b, "NULL weight pointer");
  rpr_xenc* x = new rpr_xenc{};
  x->ctx = c; x->d = *d; x->device = c->device;
  *out = x;
  return RPR_OK;
}

void rpr_xenc_free(rpr_xenc* x) {
  if (!x) return;
  if (x->wh) {
    (void)hipSetDevice(x->device);
    (void)hipFree(x->wh);
  }
  delete x;
}

int rpr_xenc_get_precision(const rpr_xenc* x) { return x ? x->precision : RPR_ERR_INVALID; }

int rpr_xenc_set_precision(rpr_ctx* c, rpr_xenc* x, int precision, void* stream) {
  RPR_REQUIRE(c && x, "NULL argument");
  RPR_REQUIRE(x->ctx == c, "the cross-encoder belongs to another ctx");
  RPR_REQUIRE(precision == RPR_XENC_F32 || precision == RPR_XENC_F16, "precision is neither 0 (fp32) nor 1 (f16 operands)");
  if (precision == RPR_XENC_F16 && !x->wh) {
    const rpr_xenc_desc& d = x->d;
    const size_t HH = (size_t)d.hidden * d.hidden, FH = (size_t)d.d_ff * d.hidden, L = (size_t)d.layers;
    const size_t n_qkv = L * 3 * HH, n_ao = L * HH, n_ff = L * FH;   // (each a multiple of 8 halves when hidden % 32 == 0)
    RPR_HIP(hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    __half* wh = nullptr;
    RPR_HIP(hipMalloc(&wh, (n_qkv + n_ao + 2 * n_ff) * sizeof(__half)));
    const float* src[4] = {d.qkv_w, d.ao_w, d.ff1_w, d.ff2_w};
    const size_t n[4] = {n_qkv, n_ao, n_ff, n_ff};
    Launcher Ln{c, s};
    size_t at = 0;
    for (int i = 0; i < 4; ++i) {
      __half* dst = wh + at;
      Ln.run(RPR_K_OTHER, 0, 6.0 * n[i], [&] { return launch_xenc_f32_to_f16(src[i], dst, n[i], s); });
      at += n[i];
    }
    if (Ln.err) { (void)hipFree(wh); return Ln.err; }
    x->wh = wh;
    x->qkv_h = wh; x->ao_h = wh + n_qkv; x->ff1_h = wh + n_qkv + n_ao; x->ff2_h = wh + n_qkv + n_ao + n_ff;
  }
  x->precision = precision;
  return RPR_OK;
}

int rpr_xenc_score(rpr_ctx* c, rpr_xenc* x, const int32_t* input_ids, const int32_t* token_type_ids, const int32_t* position_ids,
                   const int32_t* seq_off, int32_t bz, float* out_scores, void* stream) {
  RPR_REQUIRE(c && x && input_ids && token_type_ids && position_ids && seq_off && out_scores, "NULL argument");
  RPR_REQUIRE(x->ctx == c, "the cross-encoder belongs to another ctx");
  const rpr_xenc_desc& d = x->d;
  const int H = d.hidden, F = d.d_ff, dh = H / d.heads;
  RPR_REQUIRE(dh == 32 || dh == 64, "the attention kernel is built for heads of 32 or 64 dims");
  RPR_REQUIRE(H % 32 == 0 && F % 32 == 0, "hidden and d_ff must be multiples of 32 (exact-fp32 GEMM: K % 32 == 0)");
  RPR_REQUIRE(H <= 4096, "hidden above 4096 (the pooler head keeps two rows in LDS)");
  RPR_REQUIRE(bz >= 1 && bz <= (1 << 20), "bz out of range (1 .. 2^20)");
  RPR_REQUIRE(seq_off[0] == 0, "seq_off[0] must be 0");
  const int max_len = d.max_pos < 512 ? d.max_pos : 512;
  // the tile list of the attention kernel, then the sequence offsets: one int32 array
  std::vector<int32_t> meta;
  int ntiles = 0;
  try {   // (no exception crosses the C boundary)
    meta.reserve((size_t)4 * bz + 1);
    for (int b = 0; b < bz; ++b) {
      const int64_t len = (int64_t)seq_off[b + 1] - seq_off[b];
      RPR_REQUIRE(len >= 1, "an empty sequence (the pooled token is its first row)");
      RPR_REQUIRE(len <= max_len, "a sequence is longer than min(max_pos, 512)");
      for (int q0 = 0; q0 < (int)len; q0 += 64) { meta.push_back(b); meta.push_back(q0); }
    }
    ntiles = (int)(meta.size() / 2);
    meta.insert(meta.end(), seq_off, seq_off + bz + 1);
  } catch (const std::bad_alloc&) {
    set_error("out of host memory for the tile list");
    return RPR_ERR_OOM;
  }

  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return x->precision == RPR_XENC_F16
             ? xenc_forward<XencF16>(c, x, input_ids, token_type_ids, position_ids, seq_off, bz, meta, ntiles, out_scores, s)
             : xenc_forward<XencF32>(c, x, input_ids, token_type_ids, position_ids, seq_off, bz, meta, ntiles, out_scores, s);
}

}  // extern "C"
