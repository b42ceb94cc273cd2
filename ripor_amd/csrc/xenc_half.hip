// The f16 mode of the BERT cross-encoder (rpr_xenc_set_precision(RPR_XENC_F16)): the arithmetic of the
// reference's fp16 autocast. Matrix operands are f16, every accumulation is fp32, the residual stream, LayerNorm and the
// softmax stay fp32. Packed rows as in xenc_kernels.hip.
//
//   xenc_f32_to_f16        round-to-nearest-even copy of a weight stack
//   xenc_embed_ln_h        LayerNorm(word[id] + type[tt] + pos[p]) -> X fp32 and Xh f16
//   xenc_gemm_h<EPI>       C[M, N] = A[M, K] (f16) . W[N, K]^T (f16) on v_mfma_f32_32x32x16_f16, epilogues
//                            0: + bias -> f16         (QKV: attention adds no bias)
//                            1: + bias, erf GELU -> f16 (FF1)
//                            2: + bias + fp32 residual -> fp32 (attention output, FF2; xenc_ln_h follows)
//   xenc_ln_h              LayerNorm(y) -> X fp32 and Xh f16
//   xenc_attn_h<DH>        softmax(q k^T / sqrt(DH)) v per (sequence, head) on v_mfma_f32_16x16x32_f16 -> CTX f16
//
// f16 stores are plain conversions: a value beyond +-65504 becomes +-inf, as under autocast. Every reduction has a fixed
// order (no atomics): a call repeated gives the same bits.
#include "common.h"

namespace rpr {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__global__ __launch_bounds__(256) void xenc_f32_to_f16_kernel(const float* src, __half* dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = __float2half_rn(src[i]);
}

// LayerNorm of the row held un-normalised in out[0 .. H) (written by this wave: lane l owns the float4 pieces l, l + 64,
// ...): the arithmetic of row_layernorm in xenc_kernels.hip, and an f16 copy of the result
__device__ __forceinline__ void row_layernorm_h(float* out, __half* outh, int H, float sum, const float* w, const float* b, float eps,
                                                int lane) {
  const float mean = wave_sum(sum) / (float)H;
  float ss = 0.f;
  for (int i = lane * 4; i < H; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(out + i);
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    ss += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)H + eps);
  for (int i = lane * 4; i < H; i += 256) {
    float4 v = *reinterpret_cast<const float4*>(out + i);
    const float4 g = *reinterpret_cast<const float4*>(w + i), bb = *reinterpret_cast<const float4*>(b + i);
    v.x = (v.x - mean) * rstd * g.x + bb.x; v.y = (v.y - mean) * rstd * g.y + bb.y;
    v.z = (v.z - mean) * rstd * g.z + bb.z; v.w = (v.w - mean) * rstd * g.w + bb.w;
    *reinterpret_cast<float4*>(out + i) = v;
    __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
    uint2 pk;
    pk.x = *reinterpret_cast<const unsigned*>(&lo); pk.y = *reinterpret_cast<const unsigned*>(&hi);
    *reinterpret_cast<uint2*>(outh + i) = pk;
  }
}

// one wave per row, 4 rows per block; H % 4 == 0; ids clamped into their tables (memory safety only)
__global__ __launch_bounds__(256) void xenc_embed_ln_h_kernel(XencEmbedArgs a, __half* outh) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.T) return;
  const int id = min(max(a.ids[row], 0), a.vocab - 1), tt = min(max(a.types[row], 0), a.type_vocab - 1),
            p = min(max(a.pos[row], 0), a.max_pos - 1);
  const float* we = a.word + (size_t)id * a.H;
  const float* te = a.typew + (size_t)tt * a.H;
  const float* pe = a.posw + (size_t)p * a.H;
  float* out = a.out + (size_t)row * a.H;
  float sum = 0.f;
  for (int i = lane * 4; i < a.H; i += 256) {
    const float4 x = *reinterpret_cast<const float4*>(we + i), y = *reinterpret_cast<const float4*>(te + i),
                 z = *reinterpret_cast<const float4*>(pe + i);
    float4 v;
    v.x = (x.x + y.x) + z.x; v.y = (x.y + y.y) + z.y; v.z = (x.z + y.z) + z.z; v.w = (x.w + y.w) + z.w;
    *reinterpret_cast<float4*>(out + i) = v;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  row_layernorm_h(out, outh + (size_t)row * a.H, a.H, sum, a.ln_w, a.ln_b, a.eps, lane);
}

// y already holds product + bias + residual (epilogue 2 of the GEMM)
__global__ __launch_bounds__(256) void xenc_ln_h_kernel(const float* y, const float* w, const float* b, float eps, int T, int H,
                                                        float* outp, __half* outh) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* yr = y + (size_t)row * H;
  float* out = outp + (size_t)row * H;
  float sum = 0.f;
  for (int i = lane * 4; i < H; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(yr + i);
    *reinterpret_cast<float4*>(out + i) = v;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  row_layernorm_h(out, outh + (size_t)row * H, H, sum, w, b, eps, lane);
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
// One block per (64 query rows of a sequence, head), 4 waves x 16 query rows, keys and values in tiles of 64 through LDS,
// online softmax in fp32. v_mfma_f32_16x16x32_f16, lane l (c = l & 15, g = l >> 4): A[row c][k = 8 g + j],
// B[k = 8 g + j][col c], C/D[row 4 g + reg][col c].
//   S = Q K^T: A = Q[row c][d = 32 kk + 8 g + j] (registers, loaded once), B = K[key 16 j' + c][d = 32 kk + 8 g + j] from
//     row-major K rows of DH + 8 halves; a head of 32 dims is one instruction deep. Scaled by 1 / sqrt(DH) in fp32.
//   O += P V: P leaves the S accumulators in the C map, is rounded to f16 into a private strip per wave and read back in
//     the A map (8 consecutive keys per lane). B = V[key 32 kk + 8 g + j][d = 16 n + c] needs 8 keys of one column per
//     lane, so V is stored TRANSPOSED in LDS ([d][key], rows of 64 + 8 halves) when the tile is filled.
// Every fragment is one aligned 16-byte read; row strides of 80 / 144 bytes put 16 consecutive rows on 16 different
// 16-byte slots. Keys past the end get -inf before the softmax (weight exactly 0) and their K / V rows are zeros; query
// rows past the end compute on q = 0 and are not stored; the first tile always holds key 0, so the running maximum is
// finite from the first tile on.
struct XencAttnHArgs {
  const __half* qkv;         // [T, 3 H]: q | k | v of every row, biases included
  const int32_t* seq_off;    // [dev, bz + 1]
  const int2* tiles;         // [dev, ntiles]
  int ntiles, H, heads;
  __half* out;               // [T, H]
};

template <int DH>
__global__ __launch_bounds__(256) void xenc_attn_h_kernel(XencAttnHArgs a) {
  constexpr int LDK = DH + 8, LDV = 64 + 8, LDP = 64 + 8, KS = DH / 32, NB = DH / 16, C8 = DH / 8;
  __shared__ __attribute__((aligned(16))) __half k_s[64 * LDK];
  __shared__ __attribute__((aligned(16))) __half vt_s[DH * LDV];
  __shared__ __attribute__((aligned(16))) __half p_s[4 * 16 * LDP];
  const int2 t = a.tiles[blockIdx.x];
  const int head = blockIdx.y;
  const int s0 = a.seq_off[t.x], len = a.seq_off[t.x + 1] - s0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const size_t ld = (size_t)3 * a.H;
  const __half* qb = a.qkv + (size_t)s0 * ld + (size_t)head * DH;
  const float scale = 1.0f / sqrtf((float)DH);
  const bool wave_live = t.y + wave * 16 < len;

  f16x8 qf[KS];
  {
    const int qrow = t.y + wave * 16 + c;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (qrow < len) v = *reinterpret_cast<const uint4*>(qb + (size_t)qrow * ld + 32 * kk + 8 * g);
      qf[kk] = *reinterpret_cast<const f16x8*>(&v);
    }
  }
  f32x4 o[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
  __half* pw = p_s + wave * 16 * LDP;

  for (int k0 = 0; k0 < len; k0 += 64) {
    __syncthreads();   // the previous tile's K, V and P have been read
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
    __syncthreads();
    if (wave_live) {
      f32x4 s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f16x8 kf = *reinterpret_cast<const f16x8*>(&k_s[(16 * j + c) * LDK + 32 * kk + 8 * g]);
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[kk], kf, s[j], 0, 0, 0);
        }
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
        const float m_new = fmaxf(m_run[r], mx);
        const float alpha = expf(m_run[r] - m_new);     // first tile: exp(-inf) = 0
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = expf(s[j][r] - m_new);
          sum += p;
          pw[(4 * g + r) * LDP + 16 * j + c] = __float2half_rn(p);
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
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const f16x8 pa = *reinterpret_cast<const f16x8*>(&pw[c * LDP + 32 * kk + 8 * g]);
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const f16x8 vb = *reinterpret_cast<const f16x8*>(&vt_s[(16 * n + c) * LDV + 32 * kk + 8 * g]);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, vb, o[n], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = t.y + wave * 16 + 4 * g + r;
    if (qrow >= len) continue;
    const float inv = 1.0f / l_run[r];
    __half* dst = a.out + (size_t)(s0 + qrow) * a.H + (size_t)head * DH + c;
#pragma unroll
    for (int n = 0; n < NB; ++n) dst[16 * n] = __float2half_rn(o[n][r] * inv);
  }
}

}  // namespace

hipError_t launch_xenc_f32_to_f16(const float* src, __half* dst, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(xenc_f32_to_f16_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, src, dst, n);
  return hipGetLastError();
}

hipError_t launch_xenc_embed_ln_h(const XencEmbedArgs& a, __half* outh, hipStream_t s) {
  if (a.T <= 0 || a.H <= 0 || (a.H & 3) || !outh) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xenc_embed_ln_h_kernel, dim3((a.T + 3) / 4), dim3(256), 0, s, a, outh);
  return hipGetLastError();
}

hipError_t launch_xenc_ln_h(const float* y, const float* ln_w, const float* ln_b, float eps, int T, int H, float* out, __half* outh,
                            hipStream_t s) {
  if (T <= 0 || H <= 0 || (H & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xenc_ln_h_kernel, dim3((T + 3) / 4), dim3(256), 0, s, y, ln_w, ln_b, eps, T, H, out, outh);
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
  if (ntiles <= 0 || heads <= 0 || H != heads * dh) return hipErrorInvalidValue;
  XencAttnHArgs a{qkv, seq_off, tiles, ntiles, H, heads, out};
  if (dh == 32) hipLaunchKernelGGL(xenc_attn_h_kernel<32>, dim3(ntiles, heads), dim3(256), 0, s, a);
  else if (dh == 64) hipLaunchKernelGGL(xenc_attn_h_kernel<64>, dim3(ntiles, heads), dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace rpr
