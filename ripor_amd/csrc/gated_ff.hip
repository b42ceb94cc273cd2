// The gate of the gated-GELU feed-forward block (T5 v1.1 / Flan-T5 / mT5: wo(gelu_new(wi_0 x) * wi_1 x)) and its backward.
// The W_in product of such a block is an ordinary GEMM launch into an fp32 buffer gu [rows, 2 F] (columns 0..F-1 = g, the
// wi_0 half; F..2F-1 = u, the wi_1 half); the forward kernel turns it into the W_out product's operand y = gelu_new(g) * u,
// fp32 [rows, F] in the exact mode or the two f16 planes at FF_PLANE_SCALE in the split mode; the backward kernel turns the
// W_out product's input gradient dmid [rows, F] into dgu [rows, 2 F], the dY of the W_in products. Elementwise and
// bandwidth-bound: one wave per row at a time, 16-byte loads, a grid sized from the row count (capped; the waves stride).
//
// gelu_new(g) = 0.5 g (1 + tanh z), z = c (g + 0.044715 g^3). 0.5 (1 + tanh z) is the logistic function of 2 z: written as
// s = 1 / (1 + e^(-2z)) it has no cancellation where tanh z -> -1 (g < -4: 1 + tanhf(z) keeps one or two bits there), and with
// e = exp(-2 |z|) <= 1 nothing overflows: s = 1 / (1 + e) for z >= 0, e / (1 + e) below. The derivative
// 0.5 (1 + t) + 0.5 g (1 - t^2) c (1 + 3 * 0.044715 g^2) is s + 2 g s (1 - s) c (1 + 0.134145 g^2) in the same terms.
#include <hip/hip_runtime.h>

#include "kernel_utils.h"

namespace rpr {

namespace {

constexpr float GELU_C = 0.7978845608028654f, GELU_A = 0.044715f;
constexpr int GATE_THREADS = 256, GATE_WAVES = GATE_THREADS / 64, GATE_MAX_BLOCKS = 4096;

// s = 0.5 (1 + tanh z) and q = 1 - s for z = c (g + a g^3)
__device__ __forceinline__ void gelu_gate(float g, float& s, float& q) {
  const float z = GELU_C * (g + GELU_A * g * g * g);
  const float e = expf(-2.0f * fabsf(z));   // in [0, 1]
  const float r = 1.0f / (1.0f + e);
  const float big = r, small = e * r;
  s = z >= 0.f ? big : small;
  q = z >= 0.f ? small : big;
}
__device__ __forceinline__ float gelu_new_mul(float g, float u) {
  float s, q;
  gelu_gate(g, s, q);
  return (g * s) * u;
}
// dg = d u gelu_new'(g), du = d gelu_new(g)
__device__ __forceinline__ void gelu_new_bwd(float g, float u, float d, float& dg, float& du) {
  float s, q;
  gelu_gate(g, s, q);
  const float dz = GELU_C * (1.0f + 3.0f * GELU_A * g * g);
  const float ds = s + 2.0f * g * (s * q) * dz;
  dg = (d * u) * ds;
  du = d * (g * s);
}

// rows [0, min(*m_dev, M)) (m_dev null: M). F4 = F / 4 column groups per row; plane row stride F, plane stride o_ps.
__global__ __launch_bounds__(GATE_THREADS) void gated_gelu_kernel(const float* __restrict__ gu, int M, int F4, const int* __restrict__ m_dev,
                                                                 float* __restrict__ out_f, __half* __restrict__ out_h, size_t o_ps,
                                                                 unsigned int* sat) {
  int Ml = M;
  if (m_dev) { const int live = *m_dev; Ml = live < M ? (live > 0 ? live : 0) : M; }
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * GATE_WAVES + (threadIdx.x >> 6), nwaves = gridDim.x * GATE_WAVES;
  for (int r = wave; r < Ml; r += nwaves) {
    const float4* g4 = reinterpret_cast<const float4*>(gu + (size_t)r * 8 * F4);
    const float4* u4 = g4 + F4;
    for (int j = lane; j < F4; j += 64) {
      const float4 g = g4[j], u = u4[j];
      const float4 y = make_float4(gelu_new_mul(g.x, u.x), gelu_new_mul(g.y, u.y), gelu_new_mul(g.z, u.z), gelu_new_mul(g.w, u.w));
      const size_t idx = ((size_t)r * F4 + j) * 4;
      if (out_f) *reinterpret_cast<float4*>(out_f + idx) = y;
      if (out_h) store_planes4(out_h, o_ps, idx, y, sat, FF_PLANE_SCALE);
    }
  }
}

__global__ __launch_bounds__(GATE_THREADS) void gated_gelu_bwd_kernel(const float* __restrict__ gu, const float* __restrict__ dmid, int M, int F4,
                                                                     float* __restrict__ dgu) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * GATE_WAVES + (threadIdx.x >> 6), nwaves = gridDim.x * GATE_WAVES;
  for (int r = wave; r < M; r += nwaves) {
    const float4* g4 = reinterpret_cast<const float4*>(gu + (size_t)r * 8 * F4);
    const float4* u4 = g4 + F4;
    const float4* d4 = reinterpret_cast<const float4*>(dmid + (size_t)r * 4 * F4);
    float4* og = reinterpret_cast<float4*>(dgu + (size_t)r * 8 * F4);
    float4* ou = og + F4;
    for (int j = lane; j < F4; j += 64) {
      const float4 g = g4[j], u = u4[j], d = d4[j];
      float4 dg, du;
      gelu_new_bwd(g.x, u.x, d.x, dg.x, du.x); gelu_new_bwd(g.y, u.y, d.y, dg.y, du.y);
      gelu_new_bwd(g.z, u.z, d.z, dg.z, du.z); gelu_new_bwd(g.w, u.w, d.w, dg.w, du.w);
      og[j] = dg; ou[j] = du;
    }
  }
}

inline unsigned gate_blocks(int M) {
  const int b = (M + GATE_WAVES - 1) / GATE_WAVES;
  return (unsigned)(b < GATE_MAX_BLOCKS ? b : GATE_MAX_BLOCKS);
}

}  // namespace

hipError_t launch_gated_gelu(const float* gu, int M, int F, const int* m_dev, float* out_f, __half* out_h, size_t o_ps, unsigned int* sat,
                             hipStream_t s) {
  if (M <= 0 || F <= 0) return hipSuccess;
  if ((F & 3) || (!out_f && !out_h)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gated_gelu_kernel, dim3(gate_blocks(M)), dim3(GATE_THREADS), 0, s, gu, M, F / 4, m_dev, out_f, out_h, o_ps, sat);
  return hipGetLastError();
}

hipError_t launch_gated_gelu_bwd(const float* gu, const float* dmid, int M, int F, float* dgu, hipStream_t s) {
  if (M <= 0 || F <= 0) return hipSuccess;
  if (F & 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gated_gelu_bwd_kernel, dim3(gate_blocks(M)), dim3(GATE_THREADS), 0, s, gu, dmid, M, F / 4, dgu);
  return hipGetLastError();
}

}  // namespace rpr
