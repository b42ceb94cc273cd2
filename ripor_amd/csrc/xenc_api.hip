// C ABI of the cross-encoder teacher: rpr_xenc_load / rpr_xenc_free / rpr_xenc_score (kernels in xenc_kernels.hip, the
// products through the exact-fp32 GEMM of gemm_f32.hip) and its opt-in f16 mode, rpr_xenc_set_precision (kernels in
// xenc_half.hip); DESIGN.md §9f.
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

// the f16 mode of rpr_xenc_score: the same layer walk with f16 operands. X stays fp32; Xh, QKV, CTX and FF are f16.
int score_f16(rpr_ctx* c, rpr_xenc* x, const int32_t* input_ids, const int32_t* token_type_ids, const int32_t* position_ids,
              const int32_t* seq_off, int32_t bz, const std::vector<int32_t>& meta, int ntiles, float* out_scores, hipStream_t s) {
  const rpr_xenc_desc& d = x->d;
  const int H = d.hidden, F = d.d_ff, dh = H / d.heads, T = seq_off[bz];
  Workspace& w = c->ws;
  int e = ensure(c, w.xe_x, (size_t)T * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_tmp, (size_t)T * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_meta, meta.size() * sizeof(int32_t));
  if (!e) e = ensure(c, w.xe_xh, (size_t)T * H * sizeof(__half));
  if (!e) e = ensure(c, w.xe_qkvh, (size_t)T * 3 * H * sizeof(__half));
  if (!e) e = ensure(c, w.xe_ctxh, (size_t)T * H * sizeof(__half));
  if (!e) e = ensure(c, w.xe_ffh, (size_t)T * F * sizeof(__half));
  if (e) return e;
  float *X = P<float>(w.xe_x), *TMP = P<float>(w.xe_tmp);
  __half *Xh = P<__half>(w.xe_xh), *QKVh = P<__half>(w.xe_qkvh), *CTXh = P<__half>(w.xe_ctxh), *FFh = P<__half>(w.xe_ffh);
  const int2* tiles = P<int2>(w.xe_meta);
  const int32_t* off_dev = P<int32_t>(w.xe_meta) + (size_t)2 * ntiles;

  Launcher Ln{c, s};
  const double Td = (double)T;
  Ln.run(RPR_K_OTHER, 0, 4.0 * meta.size(), [&] { return launch_xenc_meta(meta.data(), (int)meta.size(), P<int32_t>(w.xe_meta), s); });
  XencEmbedArgs ea{input_ids, token_type_ids, position_ids, T, H, d.vocab_size, d.type_vocab, d.max_pos,
                   d.word_emb, d.type_emb, d.pos_emb, d.emb_ln_w, d.emb_ln_b, d.ln_eps, X};
  Ln.run(RPR_K_OTHER, 10.0 * Td * H, (4.0 * 4 + 2.0) * Td * H, [&] { return launch_xenc_embed_ln_h(ea, Xh, s); });
  // bytes: f16 operands; out_b = bytes per output element written (+ read, for the residual)
  auto gemm = [&](int epi, const __half* A, const __half* W, const float* bias, int N, int K, __half* outh, float* outf) {
    const double out_b = epi == XENC_EPI_RESID ? 8.0 : 2.0;
    Ln.run(RPR_K_GEMM, 2.0 * Td * N * K, 2.0 * (Td * K + (double)N * K) + out_b * Td * N,
           [&] { return launch_xenc_gemm_h(epi, A, W, bias, epi == XENC_EPI_RESID ? X : nullptr, outh, outf, T, N, K, s); });
  };
  double qk_pairs = 0.0;
  for (int b = 0; b < bz; ++b) { const double len = seq_off[b + 1] - seq_off[b]; qk_pairs += len * len; }
  for (int l = 0; l < d.layers; ++l) {
    const size_t HH = (size_t)H * H, FH = (size_t)F * H;
    gemm(XENC_EPI_BIAS, Xh, x->qkv_h + l * 3 * HH, d.qkv_b + (size_t)l * 3 * H, 3 * H, H, QKVh, nullptr);
    Ln.run(RPR_K_ENC_ATTN, 4.0 * qk_pairs * H, 2.0 * 4 * Td * H,
           [&] { return launch_xenc_attn_h(QKVh, off_dev, tiles, ntiles, H, d.heads, dh, CTXh, s); });
    gemm(XENC_EPI_RESID, CTXh, x->ao_h + l * HH, d.ao_b + (size_t)l * H, H, H, nullptr, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, (4.0 * 2 + 2.0) * Td * H, [&] {
      return launch_xenc_ln_h(TMP, d.ln1_w + (size_t)l * H, d.ln1_b + (size_t)l * H, d.ln_eps, T, H, X, Xh, s);
    });
    gemm(XENC_EPI_BIAS_GELU, Xh, x->ff1_h + l * FH, d.ff1_b + (size_t)l * F, F, H, FFh, nullptr);
    gemm(XENC_EPI_RESID, FFh, x->ff2_h + l * FH, d.ff2_b + (size_t)l * H, H, F, nullptr, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, (4.0 * 2 + 2.0) * Td * H, [&] {
      return launch_xenc_ln_h(TMP, d.ln2_w + (size_t)l * H, d.ln2_b + (size_t)l * H, d.ln_eps, T, H, X, Xh, s);
    });
  }
  Ln.run(RPR_K_OTHER, 2.0 * bz * ((double)H * H + H), 4.0 * ((double)H * H + 2.0 * bz * H), [&] {
    return launch_xenc_head(X, off_dev, bz, H, d.pool_w, d.pool_b, d.cls_w, d.cls_b, out_scores, s);
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
  const int T = seq_off[bz];

  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (x->precision == RPR_XENC_F16)
    return score_f16(c, x, input_ids, token_type_ids, position_ids, seq_off, bz, meta, ntiles, out_scores, s);
  Workspace& w = c->ws;
  int e = ensure(c, w.xe_x, (size_t)T * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_qkv, (size_t)T * 3 * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_ctx, (size_t)T * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_tmp, (size_t)T * H * sizeof(float));
  if (!e) e = ensure(c, w.xe_ff, (size_t)T * F * sizeof(float));
  if (!e) e = ensure(c, w.xe_meta, meta.size() * sizeof(int32_t));
  if (e) return e;
  float *X = P<float>(w.xe_x), *QKV = P<float>(w.xe_qkv), *CTX = P<float>(w.xe_ctx), *TMP = P<float>(w.xe_tmp), *FF = P<float>(w.xe_ff);
  const int2* tiles = P<int2>(w.xe_meta);
  const int32_t* off_dev = P<int32_t>(w.xe_meta) + (size_t)2 * ntiles;

  Launcher Ln{c, s};
  const double Td = (double)T;
  Ln.run(RPR_K_OTHER, 0, 4.0 * meta.size(), [&] { return launch_xenc_meta(meta.data(), (int)meta.size(), P<int32_t>(w.xe_meta), s); });
  XencEmbedArgs ea{input_ids, token_type_ids, position_ids, T, H, d.vocab_size, d.type_vocab, d.max_pos,
                   d.word_emb, d.type_emb, d.pos_emb, d.emb_ln_w, d.emb_ln_b, d.ln_eps, X};
  Ln.run(RPR_K_OTHER, 10.0 * Td * H, 4.0 * 4 * Td * H, [&] { return launch_xenc_embed_ln(ea, s); });
  auto gemm = [&](const float* A, const float* W, int N, int K, float* out) {
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K;
    g.out[0] = out; g.ldo[0] = N; g.split_n = N;
    g.M = T; g.N = N; g.K = K;
    Ln.run(RPR_K_GEMM, 2.0 * Td * N * K, 4.0 * (Td * (N + K) + (double)N * K), [&] { return launch_gemm(g, s); });
  };
  // pairs of keys a query tile meets: 64 x len per tile (an upper bound on the last tile of a sequence)
  double qk_pairs = 0.0;
  for (int b = 0; b < bz; ++b) { const double len = seq_off[b + 1] - seq_off[b]; qk_pairs += len * len; }
  for (int l = 0; l < d.layers; ++l) {
    const size_t HH = (size_t)H * H, FH = (size_t)F * H;
    gemm(X, d.qkv_w + l * 3 * HH, 3 * H, H, QKV);
    XencAttnArgs aa{QKV, d.qkv_b + (size_t)l * 3 * H, off_dev, tiles, ntiles, H, d.heads, CTX};
    Ln.run(RPR_K_ENC_ATTN, 4.0 * qk_pairs * H, 4.0 * 4 * Td * H, [&] { return launch_xenc_attn(aa, dh, s); });
    gemm(CTX, d.ao_w + l * HH, H, H, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, 4.0 * 3 * Td * H, [&] {
      return launch_xenc_bias_resid_ln(TMP, d.ao_b + (size_t)l * H, X, d.ln1_w + (size_t)l * H, d.ln1_b + (size_t)l * H, d.ln_eps, T, H, X, s);
    });
    gemm(X, d.ff1_w + l * FH, F, H, FF);
    Ln.run(RPR_K_OTHER, 10.0 * Td * F, 4.0 * 2 * Td * F, [&] { return launch_xenc_bias_gelu(FF, d.ff1_b + (size_t)l * F, T, F, s); });
    gemm(FF, d.ff2_w + l * FH, H, F, TMP);
    Ln.run(RPR_K_OTHER, 10.0 * Td * H, 4.0 * 3 * Td * H, [&] {
      return launch_xenc_bias_resid_ln(TMP, d.ff2_b + (size_t)l * H, X, d.ln2_w + (size_t)l * H, d.ln2_b + (size_t)l * H, d.ln_eps, T, H, X, s);
    });
  }
  Ln.run(RPR_K_OTHER, 2.0 * bz * ((double)H * H + H), 4.0 * ((double)H * H + 2.0 * bz * H), [&] {
    return launch_xenc_head(X, off_dev, bz, H, d.pool_w, d.pool_b, d.cls_w, d.cls_b, out_scores, s);
  });
  return Ln.err;
}

}  // extern "C"
