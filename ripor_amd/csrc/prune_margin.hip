// Pruning margin of a selection step (gfx950, wave64): how far the last kept candidate of a query (rank B-1 of the step's
// sorted candidates) is from the first dropped live one (rank B). Launched behind launch_select by rpr_search_margins only;
// the selection kernels are not touched (they export the child bitmap they work from through SelectArgs::tap_valid).
//
// Candidates and their float64 keys are those of the selection (beam_kernels.hip, select_radix.hip):
//   key = ((double)logit_f32 + (valid ? 0 : -1e9)) + beam_score, the logit being the fp32 log-softmax value when the search
//   runs with log-softmax scores (same reduction order as select_kernel / row_lstat); padding columns Vreal..V-1 of a logits
//   row are no candidates; a candidate is LIVE iff key > -1e8 (masked tokens and dead beams carry -1e9).
// With k = the smallest score among the B new slots (= rank B-1, whatever path selected them):
//   k <= -1e8                        fewer than B live candidates: rank B is dead as well, the step contributes +inf;
//   more than B candidates >= k      rank B ties with rank B-1: gap 0;
//   else                             gap = k - max{live keys < k} (+inf if there is none) — the same double subtraction
//                                    numpy does on the sorted keys, so the result is bit-identical to the restatement.
// One block per live query of the stage over its B * V candidates (one wave per beam), folded into the query's running
// minimum: a query has one writer per step and the steps of a search are ordered on its stream, so a plain load / store.
// The shared step 0 (SelectArgs::shared0: one logits row per query, every beam on the root range) has no exported bitmap —
// the radix path's step-0 kernel never builds the B copies — so the block finds the root's children itself, one binary
// search per token over the beam's row range (what the selection's own fallback does), and uses that row for every beam.
#include "common.h"

namespace rpr {

__global__ void margin_init_kernel(double* __restrict__ out, int Q) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < Q) out[q] = INFINITY;
}

hipError_t launch_margin_init(double* out, int Q, hipStream_t s) {
  hipLaunchKernelGGL(margin_init_kernel, dim3((Q + 255) / 256), dim3(256), 0, s, out, Q);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void prune_margin_kernel(MarginArgs a) {
  __shared__ double red_d[4];
  __shared__ int red_c[4];
  __shared__ unsigned long long root[MARGIN_MAX_V / 64];   // shared step 0: children of the root range
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.nq_dev && q >= *a.nq_dev) return;   // compacted stage: block-uniform
  const int B = a.B, V = a.V, Vr = a.Vreal > 0 ? a.Vreal : V;
  const size_t r0 = (size_t)q * B;

  // rank B-1 of the step: the smallest score among the new slots
  double k = INFINITY;
  for (int j = tid; j < B; j += 256) k = fmin(k, a.nxt_score[r0 + j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = fmin(k, __shfl_xor(k, o, 64));
  if (lane == 0) red_d[wave] = k;
  __syncthreads();
  k = fmin(fmin(red_d[0], red_d[1]), fmin(red_d[2], red_d[3]));
  __syncthreads();                          // red_d is reused below
  if (!(k > -1e8)) return;                  // block-uniform: rank B-1 is dead, so is rank B

  const float* lg_q = a.logits + (a.shared0 ? (size_t)q * V : r0 * V);
  const unsigned long long* valid_q = a.shared0 ? root : a.valid + (size_t)q * ((size_t)B * V >> 6);
  if (a.shared0) {                          // block-uniform
    const int lo = a.cur_lo[r0], hi = a.cur_hi[r0], Lc = a.Lc, t = a.t;
    for (int c = tid; c < V; c += 256) {    // V % 64 == 0: whole waves
      bool ok = false;
      if (t < Lc && lo < hi) {
        int l = lo, h = hi;
        while (l < h) {
          const int mid = (int)(((unsigned)l + (unsigned)h) >> 1);
          if ((int)a.codes[(size_t)mid * Lc + t] < c) l = mid + 1; else h = mid;
        }
        ok = l < hi && (int)a.codes[(size_t)l * Lc + t] == c;
      }
      const unsigned long long m = __ballot(ok);
      if (lane == 0) root[c >> 6] = m;
    }
    __syncthreads();
  }
  int cnt = 0;                              // candidates >= k (all of them live: k > -1e8)
  double below = -INFINITY;                 // best live candidate < k
  for (int b = wave; b < B; b += 4) {       // one wave per beam; V % 64 == 0: a wave reads one bitmap word per round
    const float* row = a.shared0 ? lg_q : lg_q + (size_t)b * V;
    const double bs = a.cur_score[r0 + b];
    float mx = 0.f, lsum = 0.f;
    if (a.log_softmax) {                    // fp32 log_softmax statistics of the row, as the selection computes them
      mx = -INFINITY;
      for (int c = lane; c < Vr; c += 64) mx = fmaxf(mx, row[c]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float sm = 0.f;
      for (int c = lane; c < Vr; c += 64) sm += expf(row[c] - mx);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
      lsum = logf(sm);
    }
    for (int c0 = 0; c0 < V; c0 += 64) {
      const int c = c0 + lane;
      if (c >= Vr) continue;
      const unsigned long long word = valid_q[a.shared0 ? (size_t)(c0 >> 6) : ((size_t)b * V + c0) >> 6];
      float lg = row[c];
      if (a.log_softmax) lg = (lg - mx) - lsum;
      const bool ok = (word >> lane) & 1ull;
      const double s = ((double)lg + (ok ? 0.0 : -1e9)) + bs;
      if (s >= k) ++cnt;
      else if (s > -1e8) below = fmax(below, s);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    below = fmax(below, __shfl_xor(below, o, 64));
  }
  if (lane == 0) { red_c[wave] = cnt; red_d[wave] = below; }
  __syncthreads();
  if (tid == 0) {
    cnt = red_c[0] + red_c[1] + red_c[2] + red_c[3];
    below = fmax(fmax(red_d[0], red_d[1]), fmax(red_d[2], red_d[3]));
    const double gap = cnt > B ? 0.0 : (below > -INFINITY ? k - below : INFINITY);
    double* o = a.out + (a.qmap ? a.qmap[q] : q);
    *o = fmin(*o, gap);
  }
}

hipError_t launch_prune_margin(const MarginArgs& a, hipStream_t s) {
  if (a.V % 64 != 0 || a.V > MARGIN_MAX_V || a.Q <= 0 || (!a.shared0 && !a.valid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prune_margin_kernel, dim3((unsigned)a.Q), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace rpr
