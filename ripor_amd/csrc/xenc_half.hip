// The f16 mode of the BERT cross-encoder (rpr_xenc_set_precision(RPR_XENC_F16)): the arithmetic of the
// reference's fp16 autocast. Matrix operands are f16, every accumulation is fp32, the residual stream, LayerNorm and the
// softmax stay fp32. Packed rows as in xenc_kernels.hip.
//
//   xenc_f32_to_f16            round-to-nearest-even copy of a weight stack
//   xenc_gemm_h<EPI>           C[M, N] = A[M, K] (f16) . W[N, K]^T (f16) on v_mfma_f32_32x32x16_f16, epilogues
//                                0: + bias -> f16         (QKV: attention adds no bias)
//                                1: + bias, erf GELU -> f16 (FF1)
//                                2: + bias + fp32 residual -> fp32 (attention output, FF2; LayerNorm follows)
//   xenc_attn<DH, XencAttnF16> softmax(q k^T / sqrt(DH)) v per (sequence, head) on v_mfma_f32_16x16x32_f16 -> CTX f16
//
// The embedding and the LayerNorm are the row kernels of xenc_kernels.hip with their f16 copy compiled in.
// f16 stores are plain conversions: a value beyond +-65504 becomes +-inf, as under autocast. Every reduction has a fixed
// order (no atomics): a call repeated gives the same bits.
#include "xenc_device.h"

namespace rpr {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void xenc_f32_to_f16_kernel(const float* src, __half* dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = __float2half_rn(src[i]);
}

// ---- GEMM ----------------------------------------------------------------------------------------------------------------
// Block = 128 x 128 outputs, 4 waves as 2 x 2, a wave 64 x 64 = 2 x 2 accumulators of v_mfma_f32_32x32x16_f16 (64
// registers). Lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r] = W[col r][8 h + j],
// j = 0 .. 7: both operands are K-contiguous, a fragment is one 16-byte LDS read. K walks in steps of 64 (16 MFMAs per
// wave) through one LDS stage; the next step's global loads (eight 16-byte pieces per thread, 8 lanes = 128 contiguous
// bytes of a row) are issued before the step's MFMAs and land in registers while they run. LDS rows are 64 + 8 halves =
// 144 bytes = 9 slots of 16 bytes: the 32 rows of a fragment read land on slots 9 r + h (mod 16), at most two lanes of a
// 16-lane group on one slot. Rows past M, weight rows past N and the k pieces past K are loaded as zeros, nothing past M
// or N is stored: M is anything >= 1, N and K any multiples of 32.
constexpr int GH_BM = 128, GH_BN = 128, GH_BK = 64, GH_LD = GH_BK + 8;

struct XencGemmHArgs {
  const __half* A;      // [M, K]
  const __half* W;      // [N, K]
  const float* bias;    // [N]
  const float* resid;   // [M, N] (epilogue 2)
  __half* outh;         // [M, N] (epilogues 0, 1)
  float* outf;          // [M, N] (epilogue 2)
  int M, N, K;
};

template <int EPI>
__global__ __launch_bounds__(256) void xenc_gemm_h_kernel(XencGemmHArgs g) {
  __shared__ __attribute__((aligned(16))) __half sm[(GH_BM + GH_BN) * GH_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * GH_BN, m0 = blockIdx.y * GH_BM;
  // staging: thread t moves the piece (t & 7) of the rows (t >> 3) + 32 i, i = 0 .. 3, of the A tile and of the W tile
  const int srow = tid >> 3, sc8 = (tid & 7) * 8;
  const __half* ap = g.A + (size_t)(m0 + srow) * g.K + sc8;
  const __half* wp = g.W + (size_t)(n0 + srow) * g.K + sc8;
  uint4 st[8];
  auto fetch = [&](int k0) {
    const bool kin = k0 + sc8 < g.K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      st[i] = kin && m0 + srow + 32 * i < g.M ? *reinterpret_cast<const uint4*>(ap + (size_t)32 * i * g.K + k0) : make_uint4(0u, 0u, 0u, 0u);
      st[4 + i] = kin && n0 + srow + 32 * i < g.N ? *reinterpret_cast<const uint4*>(wp + (size_t)32 * i * g.K + k0) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const __half* as = &sm[(wm * 64 + r) * GH_LD + 8 * h];
  const __half* bs = &sm[(GH_BM + wn * 64 + r) * GH_LD + 8 * h];
  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += GH_BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4*>(&sm[(srow + 32 * i) * GH_LD + sc8]) = st[i];
      *reinterpret_cast<uint4*>(&sm[(GH_BM + srow + 32 * i) * GH_LD + sc8]) = st[4 + i];
    }
    __syncthreads();
    if (k0 + GH_BK < g.K) fetch(k0 + GH_BK);
#pragma unroll
    for (int ks = 0; ks < GH_BK / 16; ++ks) {
      f16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const f16x8*>(as + 32 * i * GH_LD + 16 * ks);
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f16x8*>(bs + 32 * j * GH_LD + 16 * ks);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();   // the stage has been read: the next step may overwrite it
  }
  // C/D map of the 32x32 forms: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn * 64 + 32 * j + r;
    if (col >= g.N) continue;
    const float bias = g.bias[col];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row >= g.M) continue;
        const size_t at = (size_t)row * g.N + col;
        const float v = acc[i][j][e] + bias;
        if (EPI == 0) g.outh[at] = __float2half_rn(v);
        else if (EPI == 1) g.outh[at] = __float2half_rn(gelu_erf(v));
        else g.outf[at] = v + g.resid[at];
      }
  }
}

// ---- attention -----------------------------------------------------------------------------------------------------------
// The f16 operands of xenc_attn_kernel (xenc_device.h): v_mfma_f32_16x16x32_f16, A[row c][k = 8 g + j], B[k = 8 g + j][col c];
// q | k | v carry their biases already.
//   S: A = Q[row c][d = 32 kk + 8 g + j], B = K[key 16 j' + c][d = 32 kk + 8 g + j] from row-major K rows of DH + 8 halves; a
//      head of 32 dims is one instruction deep.
//   O: P is rounded to f16 into the strip and read back in the A map (8 consecutive keys per lane).
//      B = V[key 32 kk + 8 g + j][d = 16 n + c] needs 8 keys of one column per lane, so V is stored TRANSPOSED in LDS
//      ([d][key], rows of 64 + 8 halves) when the tile is filled.
// Every fragment is one aligned 16-byte read; row strides of 80 / 144 bytes put 16 consecutive rows on 16 different
// 16-byte slots.
struct XencAttnHArgs {
  const __half* qkv;         // [T, 3 H]: q | k | v of every row, biases included
  const int32_t* seq_off;    // [dev, bz + 1]
  const int2* tiles;         // [dev, ntiles]
  int ntiles, H, heads;
  __half* out;               // [T, H]
};

template <int DH>
struct XencAttnF16 {
  using Elem = __half;
  using Args = XencAttnHArgs;
  using QFrag = f16x8;
  using PFrag = f16x8;
  static constexpr int LDK = DH + 8, LDV = 64 + 8, V_ELEMS = DH * LDV, LDP = 64 + 8, KS = DH / 32, PS = 2, PU = 2, NB = DH / 16, C8 = DH / 8;

  static __device__ __forceinline__ f16x8 load_q(const Args&, const __half* qb, size_t ld, int, int qrow, int len, int g, int kk) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (qrow < len) v = *reinterpret_cast<const uint4*>(qb + (size_t)qrow * ld + 32 * kk + 8 * g);
    return *reinterpret_cast<const f16x8*>(&v);
  }
  static __device__ __forceinline__ void stage(__half* k_s, __half* vt_s, const Args& a, const __half* qb, size_t ld, int, int k0,
                                               int len, int tid) {
    for (int idx = tid; idx < 64 * C8; idx += 256) {
      const int r = idx / C8, c8 = (idx - r * C8) * 8;
      uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;
      if (k0 + r < len) {
        const __half* src = qb + (size_t)(k0 + r) * ld + c8;
        kv = *reinterpret_cast<const uint4*>(src + a.H);
        vv = *reinterpret_cast<const uint4*>(src + 2 * a.H);
      }
      *reinterpret_cast<uint4*>(&k_s[r * LDK + c8]) = kv;
      const __half* ve = reinterpret_cast<const __half*>(&vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) vt_s[(c8 + j) * LDV + r] = ve[j];
    }
  }
  static __device__ __forceinline__ f32x4 qk(f16x8 q, const __half* k_s, int j, int kk, int c, int g, f32x4 acc) {
    const f16x8 kf = *reinterpret_cast<const f16x8*>(&k_s[(16 * j + c) * LDK + 32 * kk + 8 * g]);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(q, kf, acc, 0, 0, 0);
  }
  static __device__ __forceinline__ f16x8 load_p(const __half* pw, int c, int g, int kk) {
    return *reinterpret_cast<const f16x8*>(&pw[c * LDP + 32 * kk + 8 * g]);
  }
  static __device__ __forceinline__ f32x4 pv(f16x8 p, const __half* vt_s, int n, int kk, int c, int g, f32x4 acc) {
    const f16x8 vb = *reinterpret_cast<const f16x8*>(&vt_s[(16 * n + c) * LDV + 32 * kk + 8 * g]);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(p, vb, acc, 0, 0, 0);
  }
  static __device__ __forceinline__ __half cvt(float v) { return __float2half_rn(v); }
};

}  // namespace

hipError_t launch_xenc_f32_to_f16(const float* src, __half* dst, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(xenc_f32_to_f16_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, src, dst, n);
  return hipGetLastError();
}

hipError_t launch_xenc_gemm_h(int epilogue, const __half* A, const __half* W, const float* bias, const float* resid, __half* outh,
                              float* outf, int M, int N, int K, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0 || (N & 31) || (K & 31) || !A || !W || !bias) return hipErrorInvalidValue;
  if (epilogue == XENC_EPI_RESID ? !(resid && outf) : !outh) return hipErrorInvalidValue;
  const dim3 grid((N + GH_BN - 1) / GH_BN, (M + GH_BM - 1) / GH_BM);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  XencGemmHArgs g{A, W, bias, resid, outh, outf, M, N, K};
  if (epilogue == XENC_EPI_BIAS) hipLaunchKernelGGL(xenc_gemm_h_kernel<0>, grid, dim3(256), 0, s, g);
  else if (epilogue == XENC_EPI_BIAS_GELU) hipLaunchKernelGGL(xenc_gemm_h_kernel<1>, grid, dim3(256), 0, s, g);
  else if (epilogue == XENC_EPI_RESID) hipLaunchKernelGGL(xenc_gemm_h_kernel<2>, grid, dim3(256), 0, s, g);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_xenc_attn_h(const __half* qkv, const int32_t* seq_off, const int2* tiles, int ntiles, int H, int heads, int dh,
                              __half* out, hipStream_t s) {
  return launch_xenc_attn_as<XencAttnF16>(XencAttnHArgs{qkv, seq_off, tiles, ntiles, H, heads, out}, dh, s);
}

}  // namespace rpr
