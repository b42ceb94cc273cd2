// Docid creation behind the C ABI: rpr_rq_train / rpr_rq_encode (kernels in gemm_f32.hip, buffers in the search workspace),
// rpr_rq_encode_beam (kernels in rq_beam.hip),
// the search over the codes they produce: rpr_rq_search (kernels in rq_search.hip),
// and the exact search over the embeddings themselves: rpr_flat_search (kernels in flat_search.hip).
#include <vector>

#include "internal.h"

using namespace rpr;

extern "C" {

// ---- residual quantization: docid creation (reference: faiss.IndexResidualQuantizer in tasks/evaluator.py:405-421) ------
// Greedy residual k-means, DESIGN.md "Residual quantization": Lloyd iterations of the fused assign kernel and the
// deterministic centroid update (gemm_f32.hip) per level, the residuals of the training rows in the ctx workspace.

static int rq_check(rpr_ctx* c, const float* x, int64_t n, int32_t d, int32_t M, int32_t K, const void* out) {
  RPR_REQUIRE(c && x && out, "NULL argument");
  RPR_REQUIRE(n >= 1 && n <= (int64_t)1 << 30, "row count out of range (1 .. 2^30 per call)");
  RPR_REQUIRE(d >= 32 && d % 32 == 0, "d must be a positive multiple of 32");
  RPR_REQUIRE(K >= 64 && K % 64 == 0 && K <= RQ_MAX_K, "K must be a multiple of 64 and at most 1024");
  RPR_REQUIRE(M >= 1 && M <= 4096, "M out of range");
  return RPR_OK;
}

static int rq_ws(rpr_ctx* c, int64_t n, int32_t d, int32_t M, int32_t K, bool train) {
  Workspace& w = c->ws;
  const size_t nblk = (size_t)((n + RQ_BM - 1) / RQ_BM), nb = (size_t)((n + RQ_SORT_ROWS - 1) / RQ_SORT_ROWS);
  int e = ensure(c, w.rq_r, (size_t)n * d * sizeof(float));
  if (!e) e = ensure(c, w.rq_cnorm, (size_t)M * K * sizeof(float));
  if (!e) e = ensure(c, w.rq_part, (size_t)M * nblk * sizeof(double));
  if (train) {
    if (!e) e = ensure(c, w.rq_code, (size_t)n * sizeof(uint16_t));
    if (!e) e = ensure(c, w.rq_hist, ((size_t)K * nb + 1) * sizeof(int));
    if (!e) e = ensure(c, w.rq_order, (size_t)n * sizeof(int));
    if (!e) e = ensure(c, w.rq_idx, (size_t)M * K * sizeof(int));
  }
  return e;
}

// sum of the per-block |r|^2 partials of every level, block by block (host, fp64)
static int rq_level_sums(rpr_ctx* c, int64_t n, int32_t M, double* out, hipStream_t s) {
  const size_t nblk = (size_t)((n + RQ_BM - 1) / RQ_BM);
  std::vector<double> part((size_t)M * nblk);
  RPR_HIP(hipMemcpyAsync(part.data(), c->ws.rq_part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  RPR_HIP(hipStreamSynchronize(s));
  for (int m = 0; m < M; ++m) {
    double t = 0.0;
    for (size_t b = 0; b < nblk; ++b) t += part[(size_t)m * nblk + b];
    out[m] = t;
  }
  return RPR_OK;
}

int rpr_rq_train(rpr_ctx* c, const float* x, int64_t n, int32_t d, int32_t M, int32_t K, int32_t niter, const int32_t* init_idx,
                 float* codebooks, double* level_mse, void* stream) {
  { const int e = rq_check(c, x, n, d, M, K, codebooks); if (e) return e; }
  RPR_REQUIRE(init_idx, "NULL init_idx");
  RPR_REQUIRE(n >= K, "fewer training rows than codewords");
  RPR_REQUIRE(niter >= 0 && niter <= 10000, "niter out of range");
  for (int64_t i = 0; i < (int64_t)M * K; ++i) RPR_REQUIRE(init_idx[i] >= 0 && init_idx[i] < n, "init_idx entry out of range");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  { const int e = rq_ws(c, n, d, M, K, true); if (e) return e; }
  Workspace& w = c->ws;
  float* R = static_cast<float*>(w.rq_r.p);
  uint16_t* code = static_cast<uint16_t*>(w.rq_code.p);
  float* cnorm = static_cast<float*>(w.rq_cnorm.p);
  int* idx = static_cast<int*>(w.rq_idx.p);
  const size_t nblk = (size_t)((n + RQ_BM - 1) / RQ_BM);
  RPR_HIP(hipMemcpyAsync(R, x, (size_t)n * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(idx, init_idx, (size_t)M * K * sizeof(int), hipMemcpyHostToDevice, s));
  RPR_HIP(hipStreamSynchronize(s));   // init_idx is the caller's
  for (int m = 0; m < M; ++m) {
    float* Cm = codebooks + (size_t)m * K * d;
    RPR_HIP(launch_rq_gather(R, d, idx + (size_t)m * K, K, Cm, s));
    RPR_HIP(launch_rq_norms(Cm, K, d, cnorm, s));
    RqAssignArgs a{R, (int)n, d, Cm, cnorm, K, code, 1, nullptr};
    for (int it = 0; it < niter; ++it) {
      RPR_HIP(launch_rq_assign(a, s));
      RPR_HIP(launch_rq_update(R, (int)n, d, code, K, static_cast<int*>(w.rq_hist.p), static_cast<int*>(w.rq_order.p), Cm, cnorm, s));
    }
    a.part = static_cast<double*>(w.rq_part.p) + (size_t)m * nblk;   // final assignment, R -= C_m[code]
    RPR_HIP(launch_rq_assign(a, s));
  }
  if (level_mse) {
    { const int e = rq_level_sums(c, n, M, level_mse, s); if (e) return e; }
    for (int m = 0; m < M; ++m) level_mse[m] /= (double)n;
  }
  return RPR_OK;
}

int rpr_rq_encode(rpr_ctx* c, const float* x, int64_t n, int32_t d, const float* codebooks, int32_t M, int32_t K, uint16_t* codes,
                  double* level_sse, void* stream) {
  { const int e = rq_check(c, x, n, d, M, K, codebooks); if (e) return e; }
  RPR_REQUIRE(codes, "NULL codes");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  { const int e = rq_ws(c, n, d, M, K, false); if (e) return e; }
  Workspace& w = c->ws;
  float* R = static_cast<float*>(w.rq_r.p);
  float* cnorm = static_cast<float*>(w.rq_cnorm.p);
  const size_t nblk = (size_t)((n + RQ_BM - 1) / RQ_BM);
  RPR_HIP(hipMemcpyAsync(R, x, (size_t)n * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  RPR_HIP(launch_rq_norms(codebooks, M * K, d, cnorm, s));
  for (int m = 0; m < M; ++m) {
    RqAssignArgs a{R, (int)n, d, codebooks + (size_t)m * K * d, cnorm + (size_t)m * K, K, codes + m, M,
                   static_cast<double*>(w.rq_part.p) + (size_t)m * nblk};
    RPR_HIP(launch_rq_assign(a, s));
  }
  if (level_sse) return rq_level_sums(c, n, M, level_sse, s);
  return RPR_OK;
}

// Beam encoding (kernels in rq_beam.hip). Level m turns the b_m beam entries of every row (b_0 = 1: the row
// itself, read from x) into T children: T = beam, and 1 at the last level, where only slot 0 is asked for. The planes
// alternate: a parent is read by several children, so a level cannot run in place.
int rpr_rq_encode_beam(rpr_ctx* c, const float* x, int64_t n, int32_t d, const float* codebooks, int32_t M, int32_t K, int32_t beam,
                       uint16_t* codes, double* level_sse, void* stream) {
  { const int e = rq_check(c, x, n, d, M, K, codebooks); if (e) return e; }
  RPR_REQUIRE(codes, "NULL codes");
  RPR_REQUIRE(beam >= 1 && beam <= RQ_MAX_BEAM, "beam out of range (1 .. 8)");
  static_assert(RQ_MAX_BEAM == 8, "the message above names the limit");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Workspace& w = c->ws;
  const size_t nblk = (size_t)((n + RQ_BM - 1) / RQ_BM), ent = (size_t)n * beam;   // beam entries of a level
  const size_t par_bytes = ((size_t)M * ent + 255) & ~(size_t)255;
  int e = ensure(c, w.rq_r, ent * d * sizeof(float));
  if (!e) e = ensure(c, w.rq_r2, ent * d * sizeof(float));
  if (!e) e = ensure(c, w.rq_bnorm, 2 * ent * sizeof(float));
  if (!e) e = ensure(c, w.rq_cand, ent * beam * (sizeof(float) + sizeof(uint16_t)));
  if (!e) e = ensure(c, w.rq_bhist, par_bytes + (size_t)M * ent * sizeof(uint16_t));
  if (!e) e = ensure(c, w.rq_cnorm, (size_t)M * K * sizeof(float));
  if (!e) e = ensure(c, w.rq_part, (size_t)M * nblk * sizeof(double));
  if (e) return e;
  float* plane[2] = {P<float>(w.rq_r), P<float>(w.rq_r2)};
  float* rnorm[2] = {P<float>(w.rq_bnorm), P<float>(w.rq_bnorm) + ent};
  float* cand_v = P<float>(w.rq_cand);
  uint16_t* cand_k = reinterpret_cast<uint16_t*>(cand_v + ent * beam);
  unsigned char* par = P<unsigned char>(w.rq_bhist);
  uint16_t* code = reinterpret_cast<uint16_t*>(par + par_bytes);
  float* cnorm = P<float>(w.rq_cnorm);
  RPR_HIP(launch_rq_norms(codebooks, M * K, d, cnorm, s));
  const float* Rin = x;
  const float* rn_in = nullptr;   // one parent: its |r|^2 orders nothing
  int b = 1;
  for (int m = 0; m < M; ++m) {
    const float* Cm = codebooks + (size_t)m * K * d;
    const int T = m == M - 1 ? 1 : beam;
    RqTopTArgs t{Rin, (long long)n * b, d, Cm, cnorm + (size_t)m * K, K, T, cand_v, cand_k};
    RPR_HIP(launch_rq_topt(t, s));
    RqMergeArgs g{Rin, rn_in, (long long)n, b, d, T, cand_v, cand_k, Cm, plane[m & 1], rnorm[m & 1],
                  par + (size_t)m * ent, code + (size_t)m * ent, beam, P<double>(w.rq_part) + (size_t)m * nblk};
    RPR_HIP(launch_rq_merge(g, s));
    Rin = plane[m & 1]; rn_in = rnorm[m & 1]; b = T;
  }
  RPR_HIP(launch_rq_backtrack(par, code, (long long)n, M, beam, codes, s));
  if (level_sse) return rq_level_sums(c, n, M, level_sse, s);
  return RPR_OK;
}

// ---- top-k inner-product search over the codes (reference: AddictvieQuantizeIndexer.search, tasks/evaluator.py:423-443) --
// DESIGN.md §9d. Per chunk of queries: one exact-fp32 GEMM fills the LUT [Qc, M * K], then the radix selection of
// rq_search.hip recomputes the scores from it pass by pass. Scratch per query: the LUT row, 4 KB of histogram and a 64 KB
// candidate list; a chunk is sized to stay under 60 MB of it.
int rpr_rq_search(rpr_ctx* c, const float* queries, int32_t Q, int32_t d, const float* codebooks, int32_t M, int32_t K,
                  const uint16_t* codes, int64_t N, int32_t topk, int64_t* out_idx, float* out_scores, void* stream) {
  RPR_REQUIRE(c, "NULL argument");
  RPR_REQUIRE(Q >= 1, "Q must be at least 1");
  RPR_REQUIRE(d >= 32 && d % 32 == 0, "d must be a positive multiple of 32");
  RPR_REQUIRE(K >= 64 && K % 64 == 0 && K <= RQ_MAX_K, "K must be a multiple of 64 and at most 1024");
  RPR_REQUIRE(M >= 1 && M <= 64, "M out of range (1 .. 64)");
  RPR_REQUIRE(N >= 1 && N <= (int64_t)0x7fffffff, "N out of range (1 .. 2^31 - 1)");
  RPR_REQUIRE(topk >= 1 && topk <= 2048, "topk out of range (1 .. 2048)");
  RPR_REQUIRE(queries && codebooks && codes && out_idx && out_scores, "NULL argument");   // after the limits: an empty tensor has no address
  static_assert(RQS_CAP >= 2048, "the candidate list holds the largest topk");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int cus = 0;
  RPR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  const size_t MK = (size_t)M * K;
  const size_t per_q = MK * sizeof(float) + RQS_BINS * sizeof(unsigned) + RQS_CAP * sizeof(unsigned long long) + sizeof(RqSelState) +
                       sizeof(unsigned);
  const int G = rq_search_group(M, K);
  int64_t qc = (int64_t)(((size_t)60 << 20) / per_q) / G * G;
  qc = qc < G ? G : qc;
  qc = qc > Q ? Q : qc;
  Workspace& w = c->ws;
  { const int e = ensure(c, w.rq_lut, (size_t)qc * MK * sizeof(float)); if (e) return e; }
  { const int e = ensure(c, w.rq_sel, (size_t)qc * (per_q - MK * sizeof(float)) + 64); if (e) return e; }
  RqScanArgs a{};
  a.lut = P<float>(w.rq_lut);
  a.codes = codes; a.N = N; a.M = M; a.K = K;
  a.cand = P<unsigned long long>(w.rq_sel);                                   // 8-byte items first
  a.st = reinterpret_cast<RqSelState*>(a.cand + (size_t)qc * RQS_CAP);
  a.hist = reinterpret_cast<unsigned*>(a.st + qc);
  a.cand_n = a.hist + (size_t)qc * RQS_BINS;
  for (int64_t q0 = 0; q0 < Q; q0 += qc) {
    const int nq = (int)(Q - q0 < qc ? Q - q0 : qc);
    GemmArgs g{};
    g.A = queries + (size_t)q0 * d; g.lda = d;
    g.W = codebooks; g.ldw = d;
    g.out[0] = P<float>(w.rq_lut); g.ldo[0] = (int)MK; g.split_n = (int)MK;
    g.M = nq; g.N = (int)MK; g.K = d;
    RPR_HIP(launch_gemm(g, s));
    a.Q = nq;
    RPR_HIP(launch_rq_select(a, topk, out_idx + (size_t)q0 * topk, out_scores + (size_t)q0 * topk, cus, s));
  }
  return RPR_OK;
}

// ---- exact top-k inner-product search over the embeddings (reference: faiss.IndexFlatIP.search, --task=retrieve) --------
// DESIGN.md §9e. Per chunk of queries and per sub-block of rows: the exact-fp32 GEMM fills the score scratch [Qc, rows]
// (at most FLAT_SCRATCH_BYTES), flat_search.hip selects the sub-block's top-k and merges it into io_*. The row in every
// compared value is the global one, so neither the sub-block size nor the caller's blocks change a bit of the result.
int rpr_flat_search(rpr_ctx* c, const float* queries, int32_t Q, int32_t d, const float* x, int64_t n, int64_t row_base,
                    int32_t topk, int64_t* io_idx, float* io_scores, int32_t merge, void* stream) {
  RPR_REQUIRE(c, "NULL argument");
  RPR_REQUIRE(Q >= 1, "Q must be at least 1");
  RPR_REQUIRE(d >= 32 && d % 32 == 0, "d must be a positive multiple of 32");
  RPR_REQUIRE(n >= 1, "n must be at least 1");
  RPR_REQUIRE(row_base >= 0, "row_base must be at least 0");
  RPR_REQUIRE(n <= (int64_t)0x7fffffff && row_base <= (int64_t)0x7fffffff - n, "row_base + n out of range (at most 2^31 - 1)");
  RPR_REQUIRE(topk >= 1 && topk <= 2048, "topk out of range (1 .. 2048)");
  RPR_REQUIRE(merge == 0 || merge == 1, "merge must be 0 or 1");
  RPR_REQUIRE(queries && x && io_idx && io_scores, "NULL argument");   // after the limits: an empty tensor has no address
  static_assert(RQS_CAP >= 2048, "the candidate list holds the largest topk");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int cus = 0;
  RPR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  // queries are chunked as rpr_rq_search chunks them: the per-query selection scratch (plus the sub-block's sorted list) under 60 MB
  const size_t per_q = RQS_BINS * sizeof(unsigned) + RQS_CAP * sizeof(unsigned long long) + sizeof(RqSelState) + sizeof(unsigned) +
                       (size_t)topk * (sizeof(int64_t) + sizeof(float));
  int64_t qc = (int64_t)(((size_t)60 << 20) / per_q);
  qc = qc > Q ? Q : qc;
  // rows of a sub-block: whole 128-row GEMM tiles, Qc x rows x 4 bytes within the scratch constant
  int64_t rows = (int64_t)(FLAT_SCRATCH_BYTES / sizeof(float)) / qc / 128 * 128;
  rows = rows < 128 ? 128 : rows;
  const int64_t ld = rows < n ? rows : (n + 3) / 4 * 4;
  Workspace& w = c->ws;
  { const int e = ensure(c, w.flat_sc, (size_t)qc * ld * sizeof(float)); if (e) return e; }
  { const int e = ensure(c, w.rq_sel, (size_t)qc * per_q + 64); if (e) return e; }
  FlatScanArgs a{};
  a.sc = P<float>(w.flat_sc); a.ld = ld;
  a.b.cand = P<unsigned long long>(w.rq_sel);                                 // 8-byte items first
  int64_t* tmp_idx = reinterpret_cast<int64_t*>(a.b.cand + (size_t)qc * RQS_CAP);
  a.b.st = reinterpret_cast<RqSelState*>(tmp_idx + (size_t)qc * topk);
  a.b.hist = reinterpret_cast<unsigned*>(a.b.st + qc);
  a.b.cand_n = a.b.hist + (size_t)qc * RQS_BINS;
  float* tmp_scores = reinterpret_cast<float*>(a.b.cand_n + qc);
  if (!merge) RPR_HIP(launch_flat_clear(io_idx, io_scores, (long long)Q * topk, s));
  for (int64_t q0 = 0; q0 < Q; q0 += qc) {
    const int nq = (int)(Q - q0 < qc ? Q - q0 : qc);
    a.Q = nq;
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t nr = n - r0 < rows ? n - r0 : rows;
      GemmArgs g{};
      g.A = queries + (size_t)q0 * d; g.lda = d;
      g.W = x + (size_t)r0 * d; g.ldw = d;
      g.out[0] = P<float>(w.flat_sc); g.ldo[0] = (int)ld; g.split_n = (int)nr;
      g.M = nq; g.N = (int)nr; g.K = d;
      RPR_HIP(launch_gemm(g, s));
      a.n = nr; a.row0 = row_base + r0;
      a.io_idx = io_idx + (size_t)q0 * topk; a.io_scores = io_scores + (size_t)q0 * topk; a.topk = topk;
      RPR_HIP(launch_flat_select(a, topk, tmp_idx, tmp_scores, cus, s));
      RPR_HIP(launch_flat_merge(tmp_idx, tmp_scores, nq, topk, io_idx + (size_t)q0 * topk, io_scores + (size_t)q0 * topk, s));
    }
  }
  return RPR_OK;
}

}  // extern "C"
