// Device code the two precisions of the BERT cross-encoder share (xenc_kernels.hip, xenc_half.hip): the erf
// GELU and the attention kernel, written once over an operand-traits struct per precision.
#pragma once
#include "kernel_utils.h"

namespace rpr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// Attention of one (64-query tile of a sequence, head): softmax(q k^T / sqrt(DH)) v over the rows of that sequence. 4 waves,
// 16 query rows each; keys and values walk through LDS in tiles of 64 rows with an online softmax in fp32. Both products are
// 16x16 MFMAs of the operand type (lane l, c = l & 15, g = l >> 4) with the C/D map [row = 4 g + reg][col = c]:
//   S = Q K^T: A = Q rows (registers, loaded once), B = K rows of the tile: four independent accumulators (16 keys each).
//   O += P V:  P leaves the S accumulators in the C map and is needed in the A map: through a private LDS strip per wave.
// The C maps of S and O share the row, so the running maximum / sum of a row and the rescaling of O stay in the lane's own
// registers; a row's 64 scores sit in 16 lanes x 4 accumulators and are reduced with the xor-shuffles 1, 2, 4, 8.
// What makes it correct: a tile always holds at least one key of the sequence (k0 < len, the first holds key 0), so the
// running maximum is finite after the first tile; keys past the end get -inf before the softmax and weigh exactly 0 (their
// K / V rows are zeros); query rows past the end compute on q = 0 and are not stored.
//
// Tr<DH> supplies the operand side (XencAttnF32 in xenc_kernels.hip, XencAttnF16 in xenc_half.hip):
//   Elem, Args (qkv, seq_off, tiles, H, out), the fragment types QFrag and PFrag, the LDS sizes LDK (K row stride), V_ELEMS
//   and LDP (P row stride), the MFMA steps KS over a head's dims and PS over a tile's 64 keys (PU of them unrolled), NB
//   load_q   fragment kk of query row qrow (zeros past the end)
//   stage    K / V rows k0 .. k0 + 63 of the sequence into LDS (zeros past the end)
//   qk       acc + Q fragment kk . K[16 j .. 16 j + 15]^T
//   load_p   fragment kk of the wave's P rows
//   pv       acc + P fragment kk . V[:, 16 n .. 16 n + 15]
//   cvt      a probability or an output as it is stored
// Fragments travel by value: handing the register arrays to the traits by reference made the compiler lay this kernel out
// differently.
template <int DH, template <int> class Tr>
__global__ __launch_bounds__(256) void xenc_attn_kernel(typename Tr<DH>::Args a) {
  using T = Tr<DH>;
  using Elem = typename T::Elem;
  constexpr int NB = T::NB;
  __shared__ __attribute__((aligned(16))) Elem k_s[64 * T::LDK];
  __shared__ __attribute__((aligned(16))) Elem v_s[T::V_ELEMS];
  __shared__ __attribute__((aligned(16))) Elem p_s[4 * 16 * T::LDP];
  const int2 t = a.tiles[blockIdx.x];   // (sequence, first query row of the tile inside it)
  const int head = blockIdx.y;
  const int s0 = a.seq_off[t.x], len = a.seq_off[t.x + 1] - s0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const size_t ld = (size_t)3 * a.H;
  const Elem* qb = a.qkv + (size_t)s0 * ld + (size_t)head * DH;   // q of the sequence's first row; k at + H, v at + 2 H
  const float scale = 1.0f / sqrtf((float)DH);
  const bool wave_live = t.y + wave * 16 < len;

  typename T::QFrag qf[T::KS];
  {
    const int qrow = t.y + wave * 16 + c;
#pragma unroll
    for (int kk = 0; kk < T::KS; ++kk) qf[kk] = T::load_q(a, qb, ld, head, qrow, len, g, kk);
  }
  f32x4 o[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
  Elem* pw = p_s + wave * 16 * T::LDP;

  for (int k0 = 0; k0 < len; k0 += 64) {
    __syncthreads();   // the previous tile's K, V and P have been read
    T::stage(k_s, v_s, a, qb, ld, head, k0, len, tid);
    __syncthreads();
    if (wave_live) {
      f32x4 s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < T::KS; ++kk)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = T::qk(qf[kk], k_s, j, kk, c, g, s[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = k0 + 16 * j + c < len;
#pragma unroll
        for (int r = 0; r < 4; ++r) s[j][r] = ok ? s[j][r] * scale : -INFINITY;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
        const float m_new = fmaxf(m_run[r], mx);        // finite: the tile holds a key of the sequence
        const float alpha = expf(m_run[r] - m_new);     // first tile: exp(-inf) = 0
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = expf(s[j][r] - m_new);
          sum += p;
          pw[(4 * g + r) * T::LDP + 16 * j + c] = T::cvt(p);
        }
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) sum += __shfl_xor(sum, sh, 64);
        l_run[r] = l_run[r] * alpha + sum;
        m_run[r] = m_new;
#pragma unroll
        for (int n = 0; n < NB; ++n) o[n][r] *= alpha;
      }
    }
    __syncthreads();   // P is in the wave's strip
    if (wave_live) {
#pragma unroll T::PU
      for (int kk = 0; kk < T::PS; ++kk) {
        const typename T::PFrag pa = T::load_p(pw, c, g, kk);
#pragma unroll
        for (int n = 0; n < NB; ++n) o[n] = T::pv(pa, v_s, n, kk, c, g, o[n]);
      }
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = t.y + wave * 16 + 4 * g + r;
    if (qrow >= len) continue;
    const float inv = 1.0f / l_run[r];
    Elem* dst = a.out + (size_t)(s0 + qrow) * a.H + (size_t)head * DH + c;
#pragma unroll
    for (int n = 0; n < NB; ++n) dst[16 * n] = T::cvt(o[n][r] * inv);
  }
}

// dh = 32 or 64; a grid of (64-query tiles, heads)
template <template <int> class Tr, class Args>
hipError_t launch_xenc_attn_as(const Args& a, int dh, hipStream_t s) {
  if (a.ntiles <= 0 || a.heads <= 0 || a.H != a.heads * dh) return hipErrorInvalidValue;
  if (dh == 32) hipLaunchKernelGGL((xenc_attn_kernel<32, Tr>), dim3(a.ntiles, a.heads), dim3(256), 0, s, a);
  else if (dh == 64) hipLaunchKernelGGL((xenc_attn_kernel<64, Tr>), dim3(a.ntiles, a.heads), dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace rpr
