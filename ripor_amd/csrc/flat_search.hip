// Exact top-k inner-product search over an fp32 embedding matrix (rpr_flat_search). Replaces
// faiss.IndexFlatIP.search (reference tasks/dense_indexer.py / evaluate.py --task=retrieve).
//
// The host entry (rq_api.hip) walks the rows in sub-blocks: the exact-fp32 GEMM writes the scores of one (query chunk,
// sub-block) into a scratch matrix [Q, ld], the kernels here select the sub-block's top-k from it and fold them into the
// caller's running [Q, topk] state.
//
// Selection: rq_search.hip's radix select over the 63-bit value rqs_value(score, global row) (common.h: key helpers, state,
// pass schedule, locate and finish kernels are shared; only the scan differs). Here a score is one coalesced 16-byte read
// of the query's row of the scratch matrix instead of M LDS gathers. The row in the value is the GLOBAL row, so the
// sorted list a sub-block yields merges with any other list by the same value and the result does not depend on how the
// collection was cut.
//
// Lower bound: once a query's running list is full, its last value bounds the result from below, and the scans of the
// later sub-blocks leave out everything under it: almost every value, so their histogram passes add next to nothing and
// the locate kernel, finding fewer values than asked for, has them all collected (rq_locate_kernel).
//
// Merge: one block per query holds both sorted lists (<= 2048 values each) in LDS; an element's output slot is its own
// position plus the number of elements of the other list above it (binary search). Values are unique — rows of different
// blocks differ — so every slot is written once.
#include "common.h"

namespace rpr {

namespace {

constexpr int FLS_THREADS = 256, FLS_CHUNK = FLS_THREADS * 4;
constexpr int FLS_MAX_TOPK = 2048;

__global__ __launch_bounds__(FLS_THREADS) void flat_scan_kernel(FlatScanArgs a, int collect, int shift, int width) {
  __shared__ unsigned hist_s[RQS_BINS];
  const int tid = threadIdx.x;
  const int q = blockIdx.x % a.Q, slot = blockIdx.x / a.Q, nslots = gridDim.x / a.Q;
  const RqSelState st = a.b.st[q];
  if (!collect && st.done) return;   // the same for every thread of the block
  const unsigned long long prefix = st.prefix;
  // the value of the state's last entry (0 while the list is not full): nothing below it can enter the result. The state
  // is written by the merge that follows this selection on the stream, not during it.
  const int64_t last = a.io_idx[(size_t)q * a.topk + a.topk - 1];
  const unsigned long long floor_c = last < 0 ? 0ull : rqs_value(a.io_scores[(size_t)q * a.topk + a.topk - 1], last);
  if (!collect) {
    for (int i = tid; i < RQS_BINS; i += FLS_THREADS) hist_s[i] = 0u;
    __syncthreads();
  }
  const int hi_shift = shift + width;   // <= 63
  const unsigned long long dmask = (1ull << width) - 1;
  const float* row = a.sc + (size_t)q * a.ld;
  for (long long j0 = (long long)slot * FLS_CHUNK + tid * 4; j0 < a.n; j0 += (long long)nslots * FLS_CHUNK) {
    const float4 v = *reinterpret_cast<const float4*>(row + j0);   // ld % 4 == 0: the four columns lie inside the row
    const float sv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (j0 + r >= a.n) continue;
      const unsigned long long c = rqs_value(sv[r], a.row0 + j0 + r);
      if (c < floor_c) continue;
      if (!collect) {
        if ((c >> hi_shift) == (prefix >> hi_shift)) atomicAdd(&hist_s[(int)((c >> shift) & dmask)], 1u);
      } else if (c >= prefix) {
        const unsigned pos = atomicAdd(&a.b.cand_n[q], 1u);
        if (pos < (unsigned)RQS_CAP) a.b.cand[(size_t)q * RQS_CAP + pos] = c;
      }
    }
  }
  if (collect) return;
  __syncthreads();
  for (int i = tid; i < RQS_BINS; i += FLS_THREADS) {
    const unsigned v = hist_s[i];
    if (v) atomicAdd(&a.b.hist[(size_t)q * RQS_BINS + i], v);
  }
}

__device__ __forceinline__ unsigned long long fls_load(const int64_t* idx, const float* sc, size_t i) {
  const int64_t r = idx[i];
  return r < 0 ? 0ull : rqs_value(sc[i], r);   // 0 is below every real value
}

// number of values of the descending list s[0 .. n) that are > c (strict) or >= c
__device__ __forceinline__ int fls_above(const unsigned long long* s, int n, unsigned long long c, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (or_equal ? s[mid] >= c : s[mid] > c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(FLS_THREADS) void flat_merge_kernel(const int64_t* tmp_idx, const float* tmp_scores, int topk,
                                                                 int64_t* io_idx, float* io_scores) {
  __shared__ unsigned long long sa[FLS_MAX_TOPK], sb[FLS_MAX_TOPK];   // the state, the sub-block's list
  __shared__ int cnt[2];
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)q * topk;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  int na = 0, nb = 0;
  for (int i = tid; i < topk; i += FLS_THREADS) {
    const unsigned long long u = fls_load(io_idx, io_scores, base + i), v = fls_load(tmp_idx, tmp_scores, base + i);
    sa[i] = u; sb[i] = v;
    na += u != 0ull; nb += v != 0ull;
  }
  if (na) atomicAdd(&cnt[0], na);
  if (nb) atomicAdd(&cnt[1], nb);
  __syncthreads();   // both lists are in LDS: io may be overwritten from here on
  na = cnt[0]; nb = cnt[1];
  // both lists are sorted by value, so their ignored entries (value 0) are the last ones: the live ones are [0, na), [0, nb)
  for (int i = tid; i < topk; i += FLS_THREADS) {
    if (i < na) {
      const unsigned long long c = sa[i];
      const int pos = i + fls_above(sb, nb, c, false);
      if (pos < topk) { io_idx[base + pos] = (int64_t)(0x7fffffffull - (c & 0x7fffffffull)); io_scores[base + pos] = rqs_unkey((unsigned)(c >> 31)); }
    }
    if (i < nb) {
      const unsigned long long c = sb[i];
      const int pos = i + fls_above(sa, na, c, true);
      if (pos < topk) { io_idx[base + pos] = (int64_t)(0x7fffffffull - (c & 0x7fffffffull)); io_scores[base + pos] = rqs_unkey((unsigned)(c >> 31)); }
    }
    if (i >= na + nb) { io_idx[base + i] = -1; io_scores[base + i] = -INFINITY; }
  }
}

__global__ void flat_clear_kernel(int64_t* idx, float* scores, long long count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) { idx[i] = -1; scores[i] = -INFINITY; }
}

}  // namespace

hipError_t launch_flat_select(const FlatScanArgs& a, int topk, int64_t* tmp_idx, float* tmp_scores, int cus, hipStream_t s) {
  // enough blocks to fill the chip (8 of these small blocks fit a CU), every query the same number of slots
  const long long nchunks = (a.n + FLS_CHUNK - 1) / FLS_CHUNK;
  long long nslots = ((long long)cus * 8 + a.Q - 1) / a.Q;
  nslots = nslots < 1 ? 1 : (nslots > nchunks ? nchunks : nslots);
  const int blocks = (int)(a.Q * nslots);
  return rq_select_passes(a.b, a.Q, a.n, topk, tmp_idx, tmp_scores, s, [&](int collect, int shift, int width) {
    hipLaunchKernelGGL(flat_scan_kernel, dim3(blocks), dim3(FLS_THREADS), 0, s, a, collect, shift, width);
    return hipGetLastError();
  });
}

hipError_t launch_flat_merge(const int64_t* tmp_idx, const float* tmp_scores, int Q, int topk, int64_t* io_idx, float* io_scores,
                             hipStream_t s) {
  if (topk > FLS_MAX_TOPK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(flat_merge_kernel, dim3(Q), dim3(FLS_THREADS), 0, s, tmp_idx, tmp_scores, topk, io_idx, io_scores);
  return hipGetLastError();
}

hipError_t launch_flat_clear(int64_t* idx, float* scores, long long count, hipStream_t s) {
  hipLaunchKernelGGL(flat_clear_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, idx, scores, count);
  return hipGetLastError();
}

}  // namespace rpr
