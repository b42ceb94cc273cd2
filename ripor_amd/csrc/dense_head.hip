// Head of the dense first-stage step (loss_type t5seq_pretrain_margin_mse; reference T5SeqPretrainEncoder.forward with one
// decoder position, modeling/t5_generative_retriever.py:708-757 and get_rank_loss :575-615). hF [3 bz, d] holds the
// representations of the queries (rows 0 .. bz), the positive documents (bz .. 2 bz) and the negative documents (2 bz .. 3 bz):
//   score_b = (<q_b, d+_b>, <q_b, d-_b>),  margin_b = score_b[0] - score_b[1],  loss = mean_b (margin_b - (t+_b - t-_b))^2,
//   g_b = 2 (margin_b - t_b) / bz,  dq_b = g_b (d+_b - d-_b),  dd+_b = g_b q_b,  dd-_b = -g_b q_b.
// Exact fp32 in every precision mode (the loss sum in double, as the ranking step's margin_mse_kernel); every reduction adds
// strided shares and then walks a fixed LDS tree: two calls give the same bits.
#include "common.h"

namespace rpr {

// one block per example: the two dot products, the margin and g
__global__ __launch_bounds__(256) void dense_mse_scores_kernel(const float* __restrict__ hF, const float* __restrict__ teacher_pos,
                                                                const float* __restrict__ teacher_neg, float* __restrict__ scores,
                                                                float* __restrict__ margins, float* __restrict__ g, int bz, int d) {
  __shared__ float red[2][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* q = hF + (size_t)b * d;
  const float* dp = hF + ((size_t)bz + b) * d;
  const float* dn = hF + ((size_t)2 * bz + b) * d;
  float sp = 0.f, sn = 0.f;
  for (int k = tid; k < d; k += 256) { const float qv = q[k]; sp += qv * dp[k]; sn += qv * dn[k]; }
  red[0][tid] = sp; red[1][tid] = sn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float m = red[0][0] - red[1][0];
    scores[2 * b] = red[0][0]; scores[2 * b + 1] = red[1][0];
    margins[b] = m;
    g[b] = 2.0f / (float)bz * (m - (teacher_pos[b] - teacher_neg[b]));
  }
}

// loss = mean_b (margin_b - teacher margin_b)^2 (torch.nn.MSELoss): one block, float64 sum in a fixed order
__global__ __launch_bounds__(256) void dense_mse_loss_kernel(const float* __restrict__ margins, const float* __restrict__ teacher_pos,
                                                              const float* __restrict__ teacher_neg, int bz, float* __restrict__ loss) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double part = 0.0;
  for (int b = tid; b < bz; b += 256) {
    const float dlt = margins[b] - (teacher_pos[b] - teacher_neg[b]);
    part += (double)(dlt * dlt);
  }
  red[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(red[0] / (double)bz);
}

// dhF rows of example b (one block per example; hF is what the forward kept, dropped out when the step drops out)
__global__ __launch_bounds__(256) void dense_mse_bwd_kernel(const float* __restrict__ hF, const float* __restrict__ g,
                                                             float* __restrict__ dhF, int bz, int d) {
  const int b = blockIdx.x;
  const size_t rq = (size_t)b * d, rp = ((size_t)bz + b) * d, rn = ((size_t)2 * bz + b) * d;
  const float gb = g[b];
  for (int k = threadIdx.x; k < d; k += 256) {
    const float qv = hF[rq + k];
    dhF[rq + k] = gb * (hF[rp + k] - hF[rn + k]);
    dhF[rp + k] = gb * qv;
    dhF[rn + k] = -gb * qv;
  }
}

hipError_t launch_dense_mse_head_fwd(const float* hF, const float* teacher_pos, const float* teacher_neg, float* scores, float* margins,
                                     float* g, float* loss, int bz, int d, hipStream_t s) {
  if (bz <= 0 || d <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dense_mse_scores_kernel, dim3(bz), dim3(256), 0, s, hF, teacher_pos, teacher_neg, scores, margins, g, bz, d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dense_mse_loss_kernel, dim3(1), dim3(256), 0, s, margins, teacher_pos, teacher_neg, bz, loss);
  return hipGetLastError();
}

hipError_t launch_dense_mse_head_bwd(const float* hF, const float* g, float* dhF, int bz, int d, hipStream_t s) {
  if (bz <= 0 || d <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dense_mse_bwd_kernel, dim3(bz), dim3(256), 0, s, hF, g, dhF, bz, d);
  return hipGetLastError();
}

}  // namespace rpr
