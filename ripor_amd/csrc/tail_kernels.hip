// Forced-tail evaluation of the trie-constrained beam search (gfx950, wave64): the fork (which queries can no longer
// be pruned, compaction of the others into the next stage) and the kernels of the teacher-forced tail pass that are
// not shared with the sequential steps. Orchestration: passes.hip::enqueue_search.
//
// Semantics preserved (reference t5_pretrainer/tasks/generation.py): per step, candidate = ((double)logit_f32 +
// (valid ? 0 : -1e9)) + beam_score in float64 (:453-463); the first B of the sorted candidates become the new beams in
// that order, ties by ascending flat index beam*V + token (:484-503); finalize ranks by float64 sum/(L+1) descending
// with exact ties in reverse slot order and stores float32 (:532-540). For a forced query every beam has exactly one
// valid child per step, so the B winners of a step are those B candidates (fork_classify_kernel proves that no masked
// candidate can reach them) and only their ORDER has to be replayed: tail_rank_kernel.
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "kernel_utils.h"

namespace rpr {

// ------------------------------------------------------------------------------------ fork
// One wave per stage query. forced <=> every beam is live (non-empty trie range), its range holds one distinct
// sequence over the columns T..L-1 (first row == last row there: the rows are sorted), and the spread of the beam
// scores is small enough that B valid continuations stay above every masked candidate for all remaining steps.
// Rows [r, hi) are sorted and share the columns [0, T): the first row behind r that differs from row r in the columns
// [T, L), or hi — the end of the run of r's sequence (duplicated smtids: many rows, one sequence).
__device__ inline int seq_run_end(const uint16_t* __restrict__ codes, int Lc, int r, int hi, int T, int L) {
  const uint16_t* a = codes + (size_t)r * Lc;
  int lo = r + 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const uint16_t* m = codes + (size_t)mid * Lc;
    bool same = true;
    for (int p = T; p < L; ++p)
      if (a[p] != m[p]) { same = false; break; }
    if (same) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// a.E > 0: a beam whose range holds several sequences does not fail the query by itself; the sequences beyond the first are
// counted (one binary search per sequence, given up beyond E + 1) and the query is forced with 1..E of them over all beams.
__global__ __launch_bounds__(256) void fork_classify_kernel(ForkArgs a) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= a.Qcap || (a.nq_dev && q >= *a.nq_dev)) return;
  const int r0 = q * a.B;
  bool ok = true;
  int extras = 0;
  double smin = INFINITY, smax = -INFINITY;
  for (int b = lane; b < a.B; b += 64) {
    const int lo = a.st.lo[r0 + b], hi = a.st.hi[r0 + b];
    const double s = a.st.score[r0 + b];
    smin = fmin(smin, s); smax = fmax(smax, s);
    if (lo >= hi) { ok = false; continue; }
    if (hi - lo > 1) {
      const uint16_t* first = a.codes + (size_t)lo * a.Lc;
      const uint16_t* last = a.codes + (size_t)(hi - 1) * a.Lc;
      bool one = true;
      for (int p = a.T; p < a.L; ++p)
        if (first[p] != last[p]) { one = false; break; }
      if (!one) {
        if (a.E <= 0) { ok = false; continue; }
        int n = 0;
        for (int r = lo; r < hi && n <= a.E + 1; ++n) r = seq_run_end(a.codes, a.Lc, r, hi, a.T, a.L);
        extras += n - 1;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    smin = fmin(smin, __shfl_xor(smin, o, 64));
    smax = fmax(smax, __shfl_xor(smax, o, 64));
  }
  if (a.E > 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) extras += __shfl_xor(extras, o, 64);
  }
  const bool all_ok = __all(ok) && extras <= a.E;
  if (lane == 0) a.flag[q] = (all_ok && (smax - smin) < a.spread_max) ? 1 + extras : 0;   // NaN scores compare false: not forced
}

hipError_t launch_fork_classify(const ForkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fork_classify_kernel, dim3((a.Qcap + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

// One block: the two lists in query order (forced -> flist, the others -> src) and the live counts of the tail pass
// and of the next stage. pool > 0: the queries flagged with extras take the spare entries in query order first (a query
// that finds the pool empty is not forced), and the spare entries in use follow the own entries in flist.
__device__ inline void block_scan_1024(int* part, int tid) {   // Hillis-Steele inclusive scan of part[0..1023]
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int add = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void fork_scan_kernel(ForkScanArgs a) {
  __shared__ int part[1024];
  __shared__ int carry, carry_x;
  const int tid = threadIdx.x, Qcap = a.Qcap;
  const int n = a.nq_dev ? min(*a.nq_dev, Qcap) : Qcap;
  int32_t* sp_of = a.spare;
  int32_t* owner = a.spare + Qcap + 1;
  if (tid == 0) { carry = 0; carry_x = 0; }
  __syncthreads();
  for (int q0 = 0; q0 < n; q0 += 1024) {
    const int q = q0 + tid;
    const int fl = q < n ? a.flag[q] : 0;
    int k = -1;                                      // spare entry of q
    if (a.pool > 0) {                                // (block-uniform)
      const int x = fl > 1 ? 1 : 0;
      part[tid] = x;
      block_scan_1024(part, tid);
      const int kx = carry_x + part[tid] - x;
      if (x && kx < a.pool) k = kx;
      __syncthreads();
      if (tid == 1023) carry_x += part[1023];
      __syncthreads();
    }
    const int v = (fl == 1 || k >= 0) ? 1 : 0;
    part[tid] = v;
    block_scan_1024(part, tid);
    if (q < n) {
      const int nf_before = carry + part[tid] - v;   // forced queries before q
      if (v) {
        a.flist[nf_before] = q; a.kvq[nf_before] = q; sp_of[nf_before] = k;
        if (k >= 0) owner[k] = q;
      } else {
        a.src[q - nf_before] = q;
      }
    }
    __syncthreads();
    if (tid == 1023) carry += part[1023];
    __syncthreads();
  }
  const int nf = carry, used = min(carry_x, a.pool);
  for (int k = tid; k < used; k += 1024) { a.flist[nf + k] = Qcap + k; a.kvq[nf + k] = owner[k]; }
  if (tid == 0) {
    const int ne = nf + used, nu = n - nf;
    a.tail_cnt[0] = ne; a.tail_cnt[1] = ne * a.B; a.tail_cnt[2] = ne * a.B * a.Lt; a.tail_cnt[3] = nf;
    a.next_cnt[0] = nu; a.next_cnt[1] = nu * a.B; a.next_cnt[2] = 0; a.next_cnt[3] = 0;
    a.spare[Qcap] = used;
  }
}

hipError_t launch_fork_scan(const ForkScanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fork_scan_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

// One block per spare entry in use: the extra sequences of its owner in (beam, row) order become the slots of the virtual
// query Qcap + k — parent beam's score, tokens and ancestry of the positions < T, the sequence's own row range; the
// remaining slots are copies of the owner's beam 0 (computed like any sequence, ignored by the ranking).
__global__ __launch_bounds__(64) void fork_extras_kernel(ForkExtrasArgs a) {
  const int k = blockIdx.x, tid = threadIdx.x, B = a.B, T = a.T;
  if (k >= a.spare[a.Qcap]) return;
  __shared__ int pb[32], plo[32], phi[32];
  const int q = a.spare[a.Qcap + 1 + k];
  const size_t r0 = (size_t)q * B, v0 = (size_t)(a.Qcap + k) * B;
  int32_t* parent = a.spare + a.Qcap + 1 + a.pool + (size_t)k * B;
  if (tid == 0) {
    int s = 0;
    for (int b = 0; b < B && s < B; ++b) {
      const int lo = a.st.lo[r0 + b], hi = a.st.hi[r0 + b];
      if (lo >= hi) continue;
      for (int r = seq_run_end(a.codes, a.Lc, lo, hi, T, a.L); r < hi && s < B; ++s) {
        const int e = seq_run_end(a.codes, a.Lc, r, hi, T, a.L);
        pb[s] = b; plo[s] = r; phi[s] = e;
        r = e;
      }
    }
    for (; s < B; ++s) { pb[s] = -1; plo[s] = a.st.lo[r0]; phi[s] = a.st.hi[r0]; }
  }
  __syncthreads();
  for (int s = tid; s < B; s += 64) {
    const size_t src = r0 + (pb[s] > 0 ? pb[s] : 0);
    a.st.score[v0 + s] = a.st.score[src];
    a.st.lo[v0 + s] = plo[s];
    a.st.hi[v0 + s] = phi[s];
    parent[s] = pb[s];
  }
  for (int i = tid; i < B * T; i += 64) {
    const int s = i / T, p = i - s * T;
    const size_t src = r0 + (pb[s] > 0 ? pb[s] : 0);
    a.st.tokens[(v0 + s) * a.st.ld + p] = a.st.tokens[src * a.st.ld + p];
    a.st.anc[(v0 + s) * a.st.ld + p] = a.st.anc[src * a.st.ld + p];
  }
}

hipError_t launch_fork_extras(const ForkExtrasArgs& a, hipStream_t s) {
  if (a.pool <= 0) return hipSuccess;
  if (a.B > 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fork_extras_kernel, dim3(a.pool), dim3(64), 0, s, a);
  return hipGetLastError();
}

// one wave per destination query
__global__ __launch_bounds__(256) void gather_stage_io_kernel(StageIO src, StageOut dst, const int32_t* __restrict__ list,
                                                               const int* __restrict__ n_dev, int Qcap, int Lq) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= Qcap || i >= *n_dev) return;
  const int q = list[i];
  if (lane == 0) {
    dst.qmap[i] = src.qmap ? src.qmap[q] : q;
    dst.offs[i] = src.offs ? src.offs[q] : q * Lq;
    dst.last[i] = src.last[q];
  }
  for (int j = lane; j < Lq; j += 64) dst.mask[(size_t)i * Lq + j] = src.mask[(size_t)q * Lq + j];
}

hipError_t launch_gather_stage_io(const StageIO& src, const StageOut& dst, const int32_t* list, const int* n_dev, int Qcap, int Lq,
                                  hipStream_t s) {
  hipLaunchKernelGGL(gather_stage_io_kernel, dim3((Qcap + 3) / 4), dim3(256), 0, s, src, dst, list, n_dev, Qcap, Lq);
  return hipGetLastError();
}

// one block per destination query
__global__ __launch_bounds__(256) void compact_beams_kernel(BeamState from, BeamState to, const int32_t* __restrict__ src,
                                                             const int* __restrict__ n_dev, int B, int T) {
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= *n_dev) return;
  const int q = src[i];
  const size_t rf = (size_t)q * B, rt = (size_t)i * B;
  for (int b = tid; b < B; b += 256) {
    to.score[rt + b] = from.score[rf + b];
    to.lo[rt + b] = from.lo[rf + b];
    to.hi[rt + b] = from.hi[rf + b];
  }
  for (int k = tid; k < B * T; k += 256) {
    const int b = k / T, p = k - b * T;
    to.tokens[(rt + b) * to.ld + p] = from.tokens[(rf + b) * from.ld + p];
    to.anc[(rt + b) * to.ld + p] = from.anc[(rf + b) * from.ld + p];
  }
}

hipError_t launch_compact_beams(const BeamState& from, const BeamState& to, const int32_t* src, const int* n_dev, int Qcap, int B, int T,
                                hipStream_t s) {
  hipLaunchKernelGGL(compact_beams_kernel, dim3(Qcap), dim3(256), 0, s, from, to, src, n_dev, B, T);
  return hipGetLastError();
}

// block (i, layer * H + head): the first n floats of the (layer, query, head) region [depth][B][64] — positions < T
__global__ __launch_bounds__(256) void kv_copy_kernel(KvCopyArgs a) {
  const int i = blockIdx.x;
  if (i >= *a.n_dev) return;
  const int lh = blockIdx.y, layer = lh / a.H, h = lh - layer * a.H;
  const size_t of = (size_t)layer * a.layer_from + (size_t)a.src[i] * a.q_from + (size_t)h * a.h_from;
  const size_t ot = (size_t)layer * a.layer_to + (size_t)i * a.q_to + (size_t)h * a.h_to;
  const float4* kf = reinterpret_cast<const float4*>(a.k_from + of);
  const float4* vf = reinterpret_cast<const float4*>(a.v_from + of);
  float4* kt = reinterpret_cast<float4*>(a.k_to + ot);
  float4* vt = reinterpret_cast<float4*>(a.v_to + ot);
  for (int k = threadIdx.x; k < (a.n >> 2); k += 256) { kt[k] = kf[k]; vt[k] = vf[k]; }
}

hipError_t launch_kv_copy(const KvCopyArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(kv_copy_kernel, dim3(a.Qcap, a.nd * a.H), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------ tail pass
// one block per forced query: the whole token row of each of its beams
__global__ __launch_bounds__(256) void tail_tokens_kernel(BeamState st, const uint16_t* __restrict__ codes, int Lc,
                                                           const int32_t* __restrict__ flist, const int* __restrict__ nf_dev,
                                                           int B, int T, int L, uint16_t* __restrict__ tokens) {
  const int i = blockIdx.x;
  if (i >= *nf_dev) return;
  const int q = flist[i];
  for (int k = threadIdx.x; k < B * L; k += 256) {
    const int b = k / L, p = k - b * L;
    const size_t r = (size_t)q * B + b;
    tokens[((size_t)i * B + b) * L + p] = p < T ? st.tokens[r * st.ld + p] : codes[(size_t)st.lo[r] * Lc + p];
  }
}

hipError_t launch_tail_tokens(const BeamState& st, const uint16_t* codes, int Lc, const int32_t* flist, const int* nf_dev, int Qcap,
                              int B, int T, int L, uint16_t* tokens, hipStream_t s) {
  hipLaunchKernelGGL(tail_tokens_kernel, dim3(Qcap), dim3(256), 0, s, st, codes, Lc, flist, nf_dev, B, T, L, tokens);
  return hipGetLastError();
}

// decoder input embeddings of the tail rows (reference t5_generative_retriever.py:194-214: position p >= 1 takes
// list_decoder_embeds[p-1][token p-1]); one wave per row
__global__ __launch_bounds__(256) void tail_embed_kernel(const float* __restrict__ in_embeds, const uint16_t* __restrict__ tokens,
                                                          float* __restrict__ out, int rows, const int* __restrict__ rows_dev,
                                                          int T, int L, int d, int V, XOut xo) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || row >= *rows_dev) return;
  const int Lt = L - T, seq = row / Lt, p = T + (row - seq * Lt);
  const int tok = tokens[(size_t)seq * L + (p - 1)];
  copy_row_x(reinterpret_cast<const float4*>(in_embeds + ((size_t)(p - 1) * V + tok) * d), out, row, d, lane, xo);
}

hipError_t launch_tail_embed(const float* in_embeds, const uint16_t* tokens, float* out, int rows, const int* rows_dev, int T, int L,
                             int d, int V, hipStream_t s, XOut xo) {
  if (rows <= 0 || T < 1) return rows <= 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(tail_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in_embeds, tokens, out, rows, rows_dev, T, L, d, V, xo);
  return hipGetLastError();
}

// Layer-0 Q/K/V of the tail rows from the model's table (t5_kernels.hip: l0_table_embed_kernel) instead of the projection:
// row r copies table row (p - 1) * V + token(p - 1) into qkv[r], 16 bytes per lane and piece; rows past the live count exit
// like tail_embed_kernel's. One wave per row.
__global__ __launch_bounds__(256) void tail_l0_qkv_kernel(const float* __restrict__ table, const uint16_t* __restrict__ tokens,
                                                           float* __restrict__ qkv, int rows, const int* __restrict__ rows_dev,
                                                           int T, int L, int V, int n4) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || row >= *rows_dev) return;
  const int Lt = L - T, seq = row / Lt, p = T + (row - seq * Lt);
  const int tok = tokens[(size_t)seq * L + (p - 1)];
  const float4* src = reinterpret_cast<const float4*>(table) + ((size_t)(p - 1) * V + tok) * n4;
  float4* dst = reinterpret_cast<float4*>(qkv) + (size_t)row * n4;
#pragma unroll 4
  for (int i = lane; i < n4; i += 64) dst[i] = src[i];
}

hipError_t launch_tail_l0_qkv(const float* table, const uint16_t* tokens, float* qkv, int rows, const int* rows_dev, int T, int L,
                              int V, int n3, hipStream_t s) {
  if (rows <= 0 || T < 1 || (n3 & 3)) return rows <= 0 ? hipSuccess : hipErrorInvalidValue;
  hipLaunchKernelGGL(tail_l0_qkv_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, table, tokens, qkv, rows, rows_dev, T, L, V, n3 >> 2);
  return hipGetLastError();
}

// Gold-code score of a tail row: final RMSNorm of the row's stream (times d_model^-0.5 under scaleup_output_hidden)
// dotted with the OUTPUT codebook row of the token at that position = the logit the sequential step's GEMM would give
// the beam's only valid child (reference get_lm_logits, t5_generative_retriever.py:250-262), in exact fp32.
__global__ __launch_bounds__(256) void tail_gold_kernel(const float* __restrict__ x, const float* __restrict__ ln,
                                                         const float* __restrict__ out_embeds, const uint16_t* __restrict__ tokens,
                                                         float* __restrict__ gold, int rows, const int* __restrict__ rows_dev, int T,
                                                         int L, int d, int V, float eps, float post, const __half* __restrict__ x_h,
                                                         size_t x_ps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || row >= *rows_dev) return;
  const int Lt = L - T, seq = row / Lt, p = T + (row - seq * Lt);
  const int tok = tokens[(size_t)seq * L + p];
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * d);   // only dereferenced when x_h == nullptr
  const float4* wr = reinterpret_cast<const float4*>(ln);
  const float4* er = reinterpret_cast<const float4*>(out_embeds + ((size_t)p * V + tok) * d);
  const int n4 = d >> 2;
  auto load4 = [&](int k) -> float4 {
    if (!x_h) return xr[k];
    const size_t idx = (size_t)row * d + 4 * (size_t)k;
    const uint2 hh = *reinterpret_cast<const uint2*>(x_h + idx), ll = *reinterpret_cast<const uint2*>(x_h + x_ps + idx);
    const __half* h = reinterpret_cast<const __half*>(&hh); const __half* l = reinterpret_cast<const __half*>(&ll);
    return make_float4(x_from_planes(h[0], l[0]), x_from_planes(h[1], l[1]), x_from_planes(h[2], l[2]), x_from_planes(h[3], l[3]));
  };
  float ss = 0.f;
  for (int k = lane; k < n4; k += 64) {
    const float4 v = load4(k);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = wave_sum(ss);
  const float rs = rsqrtf(ss / (float)d + eps);
  float acc = 0.f;
  for (int k = lane; k < n4; k += 64) {
    const float4 v = load4(k), g = wr[k], e = er[k];
    float4 hd = make_float4(g.x * (v.x * rs), g.y * (v.y * rs), g.z * (v.z * rs), g.w * (v.w * rs));
    if (post != 1.0f) { hd.x *= post; hd.y *= post; hd.z *= post; hd.w *= post; }
    acc += (hd.x * e.x + hd.y * e.y) + (hd.z * e.z + hd.w * e.w);
  }
  acc = wave_sum(acc);
  if (lane == 0) gold[row] = acc;
}

hipError_t launch_tail_gold(const float* x, const float* ln, const float* out_embeds, const uint16_t* tokens, float* gold, int rows,
                            const int* rows_dev, int T, int L, int d, int V, float eps, float post, hipStream_t s, const __half* x_h,
                            size_t x_ps) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(tail_gold_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, ln, out_embeds, tokens, gold, rows, rows_dev, T, L, d, V,
                     eps, post, x_h, x_ps);
  return hipGetLastError();
}

// RPR_FLAG_LOG_SOFTMAX: the score of a position is the log-probability of its token (reference generation.py:453-455:
// log_softmax over the V logits of the position in fp32). One wave per tail row: logits = the row's V exact-fp32 logits
// (one GEMM per position, passes.hip::enqueue_tail), arithmetic as select_kernel's: (x - max) - log(sum exp(x - max)).
__global__ __launch_bounds__(256) void tail_logprob_kernel(const float* __restrict__ logits, const uint16_t* __restrict__ tokens,
                                                            float* __restrict__ gold, int rows, const int* __restrict__ rows_dev, int T,
                                                            int L, int V) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || row >= *rows_dev) return;
  const int Lt = L - T, seq = row / Lt, p = T + (row - seq * Lt);
  const int tok = tokens[(size_t)seq * L + p];
  const float* lr = logits + (size_t)row * V;
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, lr[c]);
  mx = wave_max(mx);
  float sm = 0.f;
  for (int c = lane; c < V; c += 64) sm += expf(lr[c] - mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);      // the reduction order of select_kernel
  if (lane == 0) gold[row] = (lr[tok] - mx) - logf(sm);
}

hipError_t launch_tail_logprob(const float* logits, const uint16_t* tokens, float* gold, int rows, const int* rows_dev, int T, int L,
                               int V, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(tail_logprob_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, tokens, gold, rows, rows_dev, T, L, V);
  return hipGetLastError();
}

// A query forced with extras (own entry i, spare entry k): the reference's loop (generation.py:453-503, :532-540) on its
// B + extras enumerated candidates. Candidate c < B = the first sequence of beam c (tail sequence i * B + c), candidate
// B + s = slot s of the spare entry (parent beam parent[s]). At step t every current slot expands into the distinct next
// tokens of its surviving members; a group of members with the same token is one candidate of the step, scored with its
// lowest-index member's logit (members that share a prefix share its logits): ((double)gold + 0.0) + slot score. The
// candidates are ranked by (score desc, slot * V + token asc), the first B become the new slots in that order and the
// members of the others are dropped. Every slot keeps at least one member, so at least B candidates exist at every step.
// Then finalize's rule on the B survivors. One block; a thread per candidate (at most 2 B <= 62).
__device__ void tail_rank_extras(const TailRankArgs& a, int i, int k) {
  constexpr int CM = 64;
  __shared__ double S[2][32], sc[CM];
  __shared__ int slot[CM], lead[CM], flat[CM], nslot[CM], cseq[CM], alive[CM], orank[CM];
  const int tid = threadIdx.x, nt = blockDim.x, B = a.B, T = a.T, L = a.L, Lt = L - T, C = 2 * B;
  const int q = a.flist[i], es = *a.nf_dev + k;
  const size_t r0 = (size_t)q * B, v0 = (size_t)(a.Qcap + k) * B;
  const int32_t* parent = a.spare + a.Qcap + 1 + a.pool + (size_t)k * B;
  if (tid < C) {
    const int pb = tid < B ? tid : parent[tid - B];
    alive[tid] = pb >= 0;
    slot[tid] = pb >= 0 ? pb : 0;
    cseq[tid] = tid < B ? i * B + tid : es * B + (tid - B);
    orank[tid] = -1;
  }
  if (tid < B) S[0][tid] = a.st.score[r0 + tid];
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < Lt; ++t) {
    const int p = T + t;
    if (tid < C && alive[tid]) {
      const int tok = a.tokens[(size_t)cseq[tid] * L + p], j = slot[tid];
      int ld = tid;
      for (int c = 0; c < tid; ++c)
        if (alive[c] && slot[c] == j && a.tokens[(size_t)cseq[c] * L + p] == tok) { ld = c; break; }
      lead[tid] = ld;
      if (ld == tid) {
        sc[tid] = ((double)a.gold[(size_t)cseq[tid] * Lt + t] + 0.0) + S[cur][j];
        flat[tid] = j * 65536 + tok;                       // (tokens are 16 bits: the order of slot * V + token)
      }
    }
    __syncthreads();
    if (tid < C && alive[tid] && lead[tid] == tid) {
      const double s = sc[tid];
      const int fl = flat[tid];
      int rk = 0;
      for (int c = 0; c < C; ++c) rk += (alive[c] && lead[c] == c) && (sc[c] > s || (sc[c] == s && flat[c] < fl));
      nslot[tid] = rk < B ? rk : -1;
      if (rk < B) S[cur ^ 1][rk] = s;
    }
    __syncthreads();
    if (tid < C && alive[tid]) {
      const int ns = nslot[lead[tid]];
      if (ns < 0) alive[tid] = 0; else slot[tid] = ns;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (tid < C && alive[tid]) {
    bool first = true;                                     // (distinct sequences never share a slot at the end)
    for (int c = 0; c < tid; ++c) first = first && !(alive[c] && slot[c] == slot[tid]);
    if (first) {
      const int pb = slot[tid];
      const double s = S[cur][pb] / (double)(L + 1);
      int rk = 0;
      for (int c = 0; c < C; ++c) {
        if (!alive[c] || c == tid) continue;
        const double o = S[cur][slot[c]] / (double)(L + 1);
        rk += (o > s) || (o == s && slot[c] > pb);
      }
      if (rk < B) {
        const size_t o = (size_t)a.qmap[i] * B + rk;
        orank[tid] = rk;
        a.out_scores[o] = (float)s;
        if (tid < B) {
          const int lo = a.st.lo[r0 + tid];
          a.out_lo[o] = lo;
          a.out_hi[o] = seq_run_end(a.codes, a.Lc, lo, a.st.hi[r0 + tid], T, L);
        } else {
          a.out_lo[o] = a.st.lo[v0 + tid - B];
          a.out_hi[o] = a.st.hi[v0 + tid - B];
        }
      }
    }
  }
  __syncthreads();
  const size_t o0 = (size_t)a.qmap[i] * B;
  for (int x = tid; x < C * L; x += nt) {
    const int c = x / L, p = x - c * L;
    if (orank[c] >= 0) a.out_tokens[(o0 + orank[c]) * L + p] = (int32_t)a.tokens[(size_t)cseq[c] * L + p];
  }
}

// One block per forced query: replay of the remaining L - T selection steps and the finalize step on the B forced
// candidates. Per step the B winners are the beams' single valid children; new slot order = (cumulative score desc,
// parent slot asc) — the sort order of the sequential select_kernel restricted to those candidates. Then
// finalize_kernel's rule: rank by float64 sum/(L+1) desc, exact ties in reverse slot order, float32 store.
// The slot order of the intermediate steps only ever decides exact ties, so the kernel first sums the scores (same
// additions in the same order), ranks the final values once and replays the L - T steps only if two of them are equal
// (B = 1000: the replay was 28 x B^2 comparisons = 9 ms for one query; the single ranking pass is 30 us).
__global__ __launch_bounds__(1024) void tail_rank_kernel(TailRankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int i = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (i >= *a.nf_dev) return;
  if (a.pool > 0 && a.spare[i] >= 0) { tail_rank_extras(a, i, a.spare[i]); return; }   // block-uniform
  const int B = a.B, T = a.T, L = a.L, Lt = L - T;
  const int Lr = a.Lr ? a.Lr : L, n = Lr - T;            // report length (TailRankArgs::Lr): the first n of the Lt remaining steps
  double* S = reinterpret_cast<double*>(smem_raw);       // [B] cumulative score of the beam that started in slot b
  int* pos = reinterpret_cast<int*>(S + B);              // [B] its current slot
  int* npos = pos + B;                                   // [B]
  __shared__ int tie;
  const int q = a.flist[i];
  const size_t r0 = (size_t)q * B;
  if (tid == 0) tie = a.replay;
  for (int b = tid; b < B; b += nt) {
    double s = a.st.score[r0 + b];
    const float* g = a.gold + ((size_t)i * B + b) * Lt;
    for (int t = 0; t < n; ++t) s = ((double)g[t] + 0.0) + s;
    S[b] = s / (double)(Lr + 1);
    pos[b] = b;
  }
  __syncthreads();
  for (int b = tid; b < B; b += nt) {
    const double s = S[b];
    int gt = 0, eq = 0;
    for (int k = 0; k < B; ++k) { const double o = S[k]; gt += o > s; eq += o == s; }
    npos[b] = gt;
    if (eq > 1) tie = 1;                                 // benign race: every writer stores 1
  }
  __syncthreads();
  if (tie) {                                             // block-uniform: exact ties -> the full replay decides them
    for (int b = tid; b < B; b += nt) S[b] = a.st.score[r0 + b];
    __syncthreads();
    for (int t = 0; t < n; ++t) {
      for (int b = tid; b < B; b += nt) S[b] = ((double)a.gold[((size_t)i * B + b) * Lt + t] + 0.0) + S[b];
      __syncthreads();
      for (int b = tid; b < B; b += nt) {
        const double s = S[b];
        const int pb = pos[b];
        int rk = 0;
        for (int k = 0; k < B; ++k) rk += (S[k] > s) || (S[k] == s && pos[k] < pb);
        npos[b] = rk;
      }
      __syncthreads();
      for (int b = tid; b < B; b += nt) pos[b] = npos[b];
      __syncthreads();
    }
    for (int b = tid; b < B; b += nt) S[b] = S[b] / (double)(Lr + 1);
    __syncthreads();
    for (int b = tid; b < B; b += nt) {
      const double s = S[b];
      const int pb = pos[b];
      int rk = 0;
      for (int k = 0; k < B; ++k) rk += (S[k] > s) || (S[k] == s && pos[k] > pb);
      npos[b] = rk;
    }
    __syncthreads();
  }
  const size_t o0 = (size_t)a.qmap[i] * B;
  for (int b = tid; b < B; b += nt) {
    const int rk = npos[b];
    a.out_scores[o0 + rk] = (float)S[b];
    a.out_lo[o0 + rk] = a.st.lo[r0 + b];
    a.out_hi[o0 + rk] = a.st.hi[r0 + b];
  }
  for (int k = tid; k < B * Lr; k += nt) {
    const int b = k / Lr, p = k - b * Lr;
    a.out_tokens[(o0 + npos[b]) * Lr + p] = (int32_t)a.tokens[((size_t)i * B + b) * L + p];
  }
}

hipError_t launch_tail_rank(const TailRankArgs& a_in, hipStream_t s) {
  const char* rp = getenv("RPR_TAIL_RANK_REPLAY");          // tests: always take the tie path (read per call)
  const int replay = rp ? atoi(rp) : 0;
  TailRankArgs a = a_in;
  if (replay) a.replay = 1;
  if (a.pool > 0 && (a.B >= 32 || !a.spare || !a.codes)) return hipErrorInvalidValue;
  if (a.Lr && (a.pool > 0 || a.Lr <= a.T || a.Lr > a.L)) return hipErrorInvalidValue;
  const size_t smem = (size_t)a.B * (sizeof(double) + 2 * sizeof(int)) + 16;
  hipLaunchKernelGGL(tail_rank_kernel, dim3(a.Qcap), dim3(a.B > 256 ? 1024 : 256), smem, s, a);
  return hipGetLastError();
}

__global__ void flag_nonzero_kernel(const int* __restrict__ cnt, unsigned int* __restrict__ flag) {
  if (threadIdx.x == 0 && *cnt != 0) *flag = 1u;
}

hipError_t launch_flag_nonzero(const int* cnt, unsigned int* flag, hipStream_t s) {
  hipLaunchKernelGGL(flag_nonzero_kernel, dim3(1), dim3(64), 0, s, cnt, flag);
  return hipGetLastError();
}

// max over rows of || E[r] (*) w ||_2, as the bit pattern of a non-negative float through atomicMax (out zeroed)
__global__ __launch_bounds__(256) void max_row_norm_kernel(const float* __restrict__ E, const float* __restrict__ w, int rows, int d,
                                                            float* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float ss = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float v = E[(size_t)row * d + k] * (w ? w[k] : 1.0f);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    float n = sqrtf(ss);
    if (!(n >= 0.f)) n = INFINITY;   // NaN: no bound
    atomicMax(reinterpret_cast<unsigned int*>(out), __float_as_uint(n));
  }
}

hipError_t launch_max_row_norm(const float* E, const float* w, int rows, int d, float* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(max_row_norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, E, w, rows, d, out);
  return hipGetLastError();
}

hipError_t init_tail_kernel_attributes() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(tail_rank_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
}

}  // namespace rpr
