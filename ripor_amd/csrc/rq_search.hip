// Top-k inner-product search over residual-quantizer codes (rpr_rq_search). Replaces
// faiss.IndexResidualQuantizer.search with METRIC_INNER_PRODUCT (reference tasks/evaluator.py:423-443).
//
// score[q][n] = ((LUT[q][0][c_n0] + LUT[q][1][c_n1]) + ...) in fp32, LUT = queries x codebooks^T from the exact-fp32 GEMM.
// The Q x N scores are never stored: a score costs M LDS reads, so the selection recomputes it in every pass.
//
// Scan kernel. A block keeps the LUTs of G queries in LDS, interleaved [m][k][G] (G = 4 at M 32 / K 256: 128 KB, one
// 16-byte LDS read serves a code for four queries; G = 2 / 1 for larger tables, and a table over the LDS budget is read
// from global memory with G = 1). Every lane owns four rows of a 1024-row chunk at a time, loads their codes in 16-byte
// pieces and sums the M gathered values of every query in registers in level order. Blocks of different query groups walk
// the chunks in the same order, so the code matrix is streamed from HBM about once per pass and served from the caches
// to the other groups.
//
// Selection. Every (score, row) pair maps to a unique 63-bit value c = key(score) << 31 | (2^31 - 1 - n): key is the
// order-preserving 32-bit image of the float (-0.0 = +0.0), so "c descending" is "score descending, ties to the smaller
// row". A radix select over c, ten bits at a time from the top (select_radix.hip's pattern): a histogram pass counts the
// next digit of the values that match the prefix found so far (integer LDS atomics, one global integer atomic per
// non-empty bin), a locate kernel finds the bin of the topk-th value. A query stops refining as soon as the values at or
// above its prefix number at most RQS_CAP; the collect pass then appends exactly those to the query's candidate list and
// a finish kernel sorts the list by c and writes topk rows. Equal scores in excess of the list (all scores equal, N >>
// topk) simply take more digits: the later ones are bits of the row index. Every count is an integer and every candidate
// value is unique, so the result does not depend on the order in which atomics land.
//
// The key helpers, the selection state, the pass schedule (rq_select_passes) and the init / locate / finish launchers are
// declared in common.h: flat_search.hip runs the same selection over a score matrix with a scan kernel of its own.
#include "common.h"

namespace rpr {

namespace {

constexpr int RQS_THREADS = 256, RQS_ROWS = 4, RQS_CHUNK = RQS_THREADS * RQS_ROWS;
constexpr size_t RQS_LDS = 160 * 1024;

template <int G>
__device__ __forceinline__ void rqs_add(float (&acc)[G], const float* e) {
  if constexpr (G == 4) {
    const float4 v = *reinterpret_cast<const float4*>(e);
    acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
  } else if constexpr (G == 2) {
    const float2 v = *reinterpret_cast<const float2*>(e);
    acc[0] += v.x; acc[1] += v.y;
  } else {
    acc[0] += e[0];
  }
}

// collect == 0: histogram of the width-bit digit at `shift` over the values whose bits above the digit equal the prefix;
// collect == 1: append every c >= prefix to the query's candidate list
template <int G, bool LDS, bool VEC>
__global__ __launch_bounds__(RQS_THREADS) void rq_scan_kernel(RqScanArgs a, int collect, int shift, int width) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int MK = a.M * a.K, K = a.K, M = a.M;
  float* lut_s = reinterpret_cast<float*>(smem_raw);
  unsigned* hist_s = reinterpret_cast<unsigned*>(smem_raw + (LDS ? (size_t)G * MK * sizeof(float) : 0));
  const int tid = threadIdx.x;
  const int group = blockIdx.x % a.ngroups, slot = blockIdx.x / a.ngroups, nslots = gridDim.x / a.ngroups;
  const int q0 = group * G;

  bool act[G];
  unsigned long long prefix[G];
  unsigned actmask = 0u;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    act[g] = q0 + g < a.Q && (collect || !a.st[q0 + g].done);
    prefix[g] = act[g] ? a.st[q0 + g].prefix : 0ull;
    actmask |= act[g] ? 1u << g : 0u;
  }
  if (!actmask) return;   // the same for every thread of the block

  const float* lutp;
  if (LDS) {
    for (int i = tid; i < MK; i += RQS_THREADS)
#pragma unroll
      for (int g = 0; g < G; ++g) lut_s[(size_t)i * G + g] = q0 + g < a.Q ? a.lut[(size_t)(q0 + g) * MK + i] : 0.f;
    lutp = lut_s;
  } else {
    lutp = a.lut + (size_t)q0 * MK;   // G == 1: [m][k][1] is the GEMM's own row
  }
  if (!collect)
    for (int i = tid; i < G * RQS_BINS; i += RQS_THREADS) hist_s[i] = 0u;
  __syncthreads();

  const int hi_shift = shift + width;   // <= 63
  const unsigned long long dmask = (1ull << width) - 1;
  const long long nchunks = (a.N + RQS_CHUNK - 1) / RQS_CHUNK;
  for (long long chunk = slot; chunk < nchunks; chunk += nslots) {
    long long n[RQS_ROWS];
    const uint16_t* rowp[RQS_ROWS];
#pragma unroll
    for (int r = 0; r < RQS_ROWS; ++r) {
      n[r] = chunk * RQS_CHUNK + r * RQS_THREADS + tid;
      rowp[r] = a.codes + (size_t)(n[r] < a.N ? n[r] : a.N - 1) * M;   // rows past the end re-read the last row
    }
    float acc[RQS_ROWS][G];
#pragma unroll
    for (int r = 0; r < RQS_ROWS; ++r)
#pragma unroll
      for (int g = 0; g < G; ++g) acc[r][g] = 0.f;
    if (VEC) {   // M % 8 == 0, rows 16-byte aligned
      for (int m0 = 0; m0 < M; m0 += 8) {
        uint4 cw[RQS_ROWS];
#pragma unroll
        for (int r = 0; r < RQS_ROWS; ++r) cw[r] = *reinterpret_cast<const uint4*>(rowp[r] + m0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float* base = lutp + (size_t)(m0 + j) * K * G;
#pragma unroll
          for (int r = 0; r < RQS_ROWS; ++r) {
            const unsigned w = j < 2 ? cw[r].x : j < 4 ? cw[r].y : j < 6 ? cw[r].z : cw[r].w;
            const int c = min((int)((w >> (16 * (j & 1))) & 0xffffu), K - 1);
            rqs_add<G>(acc[r], base + (size_t)c * G);
          }
        }
      }
    } else {
      for (int m = 0; m < M; ++m) {
        const float* base = lutp + (size_t)m * K * G;
#pragma unroll
        for (int r = 0; r < RQS_ROWS; ++r) {
          const int c = min((int)rowp[r][m], K - 1);
          rqs_add<G>(acc[r], base + (size_t)c * G);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RQS_ROWS; ++r) {
      if (n[r] >= a.N) continue;
      const unsigned long long low = 0x7fffffffull - (unsigned long long)n[r];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (!act[g]) continue;
        const unsigned long long c = ((unsigned long long)rqs_key(acc[r][g]) << 31) | low;
        if (!collect) {
          if ((c >> hi_shift) == (prefix[g] >> hi_shift))
            atomicAdd(&hist_s[g * RQS_BINS + (int)((c >> shift) & dmask)], 1u);
        } else if (c >= prefix[g]) {
          const unsigned pos = atomicAdd(&a.cand_n[q0 + g], 1u);
          if (pos < (unsigned)RQS_CAP) a.cand[(size_t)(q0 + g) * RQS_CAP + pos] = c;
        }
      }
    }
  }
  if (collect) return;
  __syncthreads();
  for (int i = tid; i < G * RQS_BINS; i += RQS_THREADS) {
    const unsigned v = hist_s[i];
    const int g = i / RQS_BINS;
    if (v && ((actmask >> g) & 1u)) atomicAdd(&a.hist[(size_t)(q0 + g) * RQS_BINS + (i - g * RQS_BINS)], v);
  }
}

__global__ void rq_sel_init_kernel(RqSelState* st, int Q, unsigned need, int done) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < Q) st[q] = RqSelState{0ull, need, 0u, done, 0};
}

// One block per query: the bin (from the top) that holds the need-th value among those matching the prefix
__global__ __launch_bounds__(RQS_BINS) void rq_locate_kernel(RqSelState* st, unsigned* hist, int shift) {
  __shared__ unsigned sc[RQS_BINS];
  const int q = blockIdx.x, t = threadIdx.x;
  const RqSelState cur = st[q];
  if (cur.done) return;
  unsigned* hq = hist + (size_t)q * RQS_BINS;
  const int bin = RQS_BINS - 1 - t;
  const unsigned h = hq[bin];
  hq[bin] = 0u;   // ready for the next digit
  sc[t] = h;
  __syncthreads();
  for (int o = 1; o < RQS_BINS; o <<= 1) {   // inclusive scan over the bins in descending order
    const unsigned v = t >= o ? sc[t - o] : 0u;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  const unsigned incl = sc[t], excl = incl - h;
  if (t == RQS_BINS - 1 && incl < cur.need) {
    // fewer values were counted than asked for: a scan that leaves out values under a lower bound (flat_search.hip; never
    // rpr_rq_search, whose first pass counts all N >= need). They all fit the candidate list: collect them, take them all
    RqSelState nx = cur;
    nx.need = incl;
    nx.done = 1;
    st[q] = nx;
  }
  if (excl < cur.need && cur.need <= incl) {
    RqSelState nx = cur;
    nx.prefix = cur.prefix | ((unsigned long long)bin << shift);
    nx.above = cur.above + excl;
    nx.need = cur.need - excl;
    nx.done = (nx.above + h <= (unsigned)RQS_CAP || shift == 0) ? 1 : 0;
    st[q] = nx;
  }
}

// One block per query: bitonic sort of the candidate list by c descending, then the first topk rows
__global__ __launch_bounds__(1024) void rq_finish_kernel(const unsigned long long* cand, const unsigned* cand_n, int topk,
                                                         int64_t* out_idx, float* out_scores) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned long long* s = reinterpret_cast<unsigned long long*>(smem_raw);
  const int q = blockIdx.x, t = threadIdx.x;
  const int n = (int)min(cand_n[q], (unsigned)RQS_CAP);
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = t; i < P; i += 1024) s[i] = i < n ? cand[(size_t)q * RQS_CAP + i] : 0ull;   // 0 is below every real value
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int i = t; i < P; i += 1024) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long u = s[i], v = s[x];
          if (((i & k) == 0) ? (u < v) : (u > v)) { s[i] = v; s[x] = u; }
        }
      }
      __syncthreads();
    }
  for (int i = t; i < topk; i += 1024) {
    const bool ok = i < n;
    const unsigned long long c = ok ? s[i] : 0ull;
    out_idx[(size_t)q * topk + i] = ok ? (int64_t)(0x7fffffffull - (c & 0x7fffffffull)) : (int64_t)-1;
    out_scores[(size_t)q * topk + i] = ok ? rqs_unkey((unsigned)(c >> 31)) : -INFINITY;
  }
}

template <int G, bool LDS, bool VEC>
hipError_t scan_launch(const RqScanArgs& a, int collect, int shift, int width, int blocks, size_t smem, hipStream_t s) {
  static bool attr_done = false;   // the attribute is per kernel; set once (same value every time)
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rq_scan_kernel<G, LDS, VEC>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)RQS_LDS);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  hipLaunchKernelGGL((rq_scan_kernel<G, LDS, VEC>), dim3(blocks), dim3(RQS_THREADS), smem, s, a, collect, shift, width);
  return hipGetLastError();
}

}  // namespace

int rq_search_group(int M, int K) {
  const size_t mk = (size_t)M * K * sizeof(float), hist = RQS_BINS * sizeof(unsigned);
  if (4 * (mk + hist) <= RQS_LDS) return 4;
  if (2 * (mk + hist) <= RQS_LDS) return 2;
  return 1;
}

hipError_t launch_rq_scan(RqScanArgs a, int collect, int shift, int width, int cus, hipStream_t s) {
  const int G = rq_search_group(a.M, a.K);
  const size_t mk = (size_t)a.M * a.K * sizeof(float), hist = RQS_BINS * sizeof(unsigned);
  const bool lds = G * (mk + hist) <= RQS_LDS;
  const bool vec = a.M % 8 == 0 && reinterpret_cast<uintptr_t>(a.codes) % 16 == 0;
  const size_t smem = (size_t)G * ((lds ? mk : 0) + hist);
  a.ngroups = (a.Q + G - 1) / G;
  // enough blocks to fill the chip (as many per CU as the LDS allows, at most 4), every group the same number of slots
  const int per_cu = RQS_LDS / smem < 4 ? (int)(RQS_LDS / smem) : 4;
  const long long nchunks = (a.N + RQS_CHUNK - 1) / RQS_CHUNK;
  long long nslots = ((long long)cus * per_cu + a.ngroups - 1) / a.ngroups;
  nslots = nslots < 1 ? 1 : (nslots > nchunks ? nchunks : nslots);
  const int blocks = (int)(a.ngroups * nslots);
#define RPR_RQS(Gv, Lv) \
  return vec ? scan_launch<Gv, Lv, true>(a, collect, shift, width, blocks, smem, s) \
             : scan_launch<Gv, Lv, false>(a, collect, shift, width, blocks, smem, s)
  if (G == 4) { RPR_RQS(4, true); }
  if (G == 2) { RPR_RQS(2, true); }
  if (lds) { RPR_RQS(1, true); }
  RPR_RQS(1, false);
#undef RPR_RQS
}

hipError_t launch_rq_sel_init(RqSelState* st, int Q, unsigned need, int done, hipStream_t s) {
  hipLaunchKernelGGL(rq_sel_init_kernel, dim3((Q + 255) / 256), dim3(256), 0, s, st, Q, need, done);
  return hipGetLastError();
}

hipError_t launch_rq_locate(RqSelState* st, unsigned* hist, int Q, int shift, hipStream_t s) {
  hipLaunchKernelGGL(rq_locate_kernel, dim3(Q), dim3(RQS_BINS), 0, s, st, hist, shift);
  return hipGetLastError();
}

hipError_t launch_rq_finish(const unsigned long long* cand, const unsigned* cand_n, int Q, int topk, int64_t* out_idx,
                            float* out_scores, hipStream_t s) {
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rq_finish_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, RQS_CAP * (int)sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  hipLaunchKernelGGL(rq_finish_kernel, dim3(Q), dim3(1024), RQS_CAP * sizeof(unsigned long long), s, cand, cand_n, topk, out_idx,
                     out_scores);
  return hipGetLastError();
}

hipError_t launch_rq_select(const RqScanArgs& a, int topk, int64_t* out_idx, float* out_scores, int cus, hipStream_t s) {
  const RqSelBufs b{a.st, a.hist, a.cand, a.cand_n};
  return rq_select_passes(b, a.Q, a.N, topk, out_idx, out_scores, s,
                          [&](int collect, int shift, int width) { return launch_rq_scan(a, collect, shift, width, cus, s); });
}

}  // namespace rpr
