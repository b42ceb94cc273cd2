// BERT cross-encoder forward over a PACKED batch (rpr_xenc_score in xenc_api.hip). Replaces the HF
// BertForSequenceClassification pass of the reference's teacher (modeling/cross_encoder.py, tasks/reranker.py).
//
// Packed: only attended tokens exist. Row t of every [T, .] matrix is one token, sequence b owns the rows
// seq_off[b] .. seq_off[b + 1] - 1, and a row carries its original position id. Attention runs per (sequence, head) over
// that sequence's rows, so there is no key mask and padding costs nothing. The fp32 mode runs on these kernels and the
// exact-fp32 GEMM of gemm_f32.hip (no bias, no activation: those live here); the f16 mode (xenc_half.hip) shares the row
// kernels, which then also write an f16 copy of the hidden states, and the head.
//
//   xenc_embed_ln<HALF_COPY>     LayerNorm(word[id] + type[tt] + pos[p])
//   xenc_attn<DH, XencAttnF32>   softmax((q + b_q)(k + b_k)^T / sqrt(DH)) (v + b_v), DH = 32 or 64 (skeleton: xenc_device.h)
//   xenc_add_ln<ADD, HALF_COPY>  LayerNorm(y + bias + residual), or LayerNorm(y) after a GEMM that has added both
//   xenc_bias_gelu               bias + exact (erf) GELU, in place
//   xenc_head                    tanh(pool_w x_first + pool_b) . cls_w + cls_b of every sequence's first row
//
// Every reduction has a fixed order (shuffles inside a wave, no atomics): a call repeated gives the same bits.
#include "xenc_device.h"

namespace rpr {

namespace {

// LayerNorm of one row held as out[0 .. H) (already written by this wave: lane l owns the float4 pieces l, l + 64, ...),
// biased variance, two passes over the row; HALF_COPY: the result goes to outh[0 .. H) in f16 as well
template <bool HALF_COPY>
__device__ __forceinline__ void row_layernorm(float* out, __half* outh, int H, float sum, const float* w, const float* b, float eps,
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
    if constexpr (HALF_COPY) {
      __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
      uint2 pk;
      pk.x = *reinterpret_cast<const unsigned*>(&lo); pk.y = *reinterpret_cast<const unsigned*>(&hi);
      *reinterpret_cast<uint2*>(outh + i) = pk;
    }
  }
}

// one wave per row, 4 rows per block; H % 4 == 0. Ids outside their tables are clamped (memory safety only: the Python
// boundary refuses them before the call).
template <bool HALF_COPY>
__global__ __launch_bounds__(256) void xenc_embed_ln_kernel(XencEmbedArgs a, __half* outh) {
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
    float4 v;   // HF BertEmbeddings: (inputs_embeds + token_type_embeddings) + position_embeddings
    v.x = (x.x + y.x) + z.x; v.y = (x.y + y.y) + z.y; v.z = (x.z + y.z) + z.z; v.w = (x.w + y.w) + z.w;
    *reinterpret_cast<float4*>(out + i) = v;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  row_layernorm<HALF_COPY>(out, outh + (size_t)row * a.H, a.H, sum, a.ln_w, a.ln_b, a.eps, lane);
}

// LayerNorm(y + bias + resid) when ADD, LayerNorm(y) otherwise (the f16 GEMM's epilogue has added both). out may be resid
// or y (in place): a lane reads its pieces before it writes them
template <bool ADD, bool HALF_COPY>
__global__ __launch_bounds__(256) void xenc_add_ln_kernel(const float* y, const float* bias, const float* resid, const float* w,
                                                          const float* b, float eps, int T, int H, float* outp, __half* outh) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* yr = y + (size_t)row * H;
  const float* rr = resid + (size_t)row * H;
  float* out = outp + (size_t)row * H;
  float sum = 0.f;
  for (int i = lane * 4; i < H; i += 256) {
    float4 v = *reinterpret_cast<const float4*>(yr + i);
    if constexpr (ADD) {
      const float4 bb = *reinterpret_cast<const float4*>(bias + i), r = *reinterpret_cast<const float4*>(rr + i);
      v.x = (v.x + bb.x) + r.x; v.y = (v.y + bb.y) + r.y; v.z = (v.z + bb.z) + r.z; v.w = (v.w + bb.w) + r.w;
    }
    *reinterpret_cast<float4*>(out + i) = v;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  row_layernorm<HALF_COPY>(out, outh + (size_t)row * H, H, sum, w, b, eps, lane);
}

// x [rows, N] in place; N % 4 == 0, n4 = rows * N / 4
__global__ __launch_bounds__(256) void xenc_bias_gelu_kernel(float* x, const float* bias, long long n4, int N) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = reinterpret_cast<float4*>(x)[i];
  const float4 b = *reinterpret_cast<const float4*>(bias + (int)((i * 4) % N));
  v.x = gelu_erf(v.x + b.x); v.y = gelu_erf(v.y + b.y); v.z = gelu_erf(v.z + b.z); v.w = gelu_erf(v.w + b.w);
  reinterpret_cast<float4*>(x)[i] = v;
}

// The fp32 operands of xenc_attn_kernel (xenc_device.h): v_mfma_f32_16x16x4_f32, A[i = c][k = g], B[k = g][j = c]; the
// q | k | v biases are added while loading.
//   S: A = Q[row c][d = 4 kk + g], B = K[key 16 j + c][d = 4 kk + g]; K rows of DH + 4 floats: the 64 lanes of a B read hit
//      64 different banks.
//   O: A = P[row c][key 4 kk + g] (strip rows of 64 + 4), B = V[key 4 kk + g][d = 16 n + c], V rows of DH + 16: again 64
//      different banks.
template <int DH>
struct XencAttnF32 {
  using Elem = float;
  using Args = XencAttnArgs;
  using QFrag = float;
  using PFrag = float;
  static constexpr int LDK = DH + 4, LDV = DH + 16, V_ELEMS = 64 * LDV, LDP = 64 + 4, KS = DH / 4, PS = 16, PU = 4, NB = DH / 16, C4 = DH / 4;

  static __device__ __forceinline__ float load_q(const Args& a, const float* qb, size_t ld, int head, int qrow, int len, int g, int kk) {
    const float* bq = a.bias + head * DH;
    return qrow < len ? qb[(size_t)qrow * ld + 4 * kk + g] + bq[4 * kk + g] : 0.f;
  }
  static __device__ __forceinline__ void stage(float* k_s, float* v_s, const Args& a, const float* qb, size_t ld, int head, int k0,
                                               int len, int tid) {
    const float* bq = a.bias + head * DH;
    for (int idx = tid; idx < 64 * C4; idx += 256) {
      const int r = idx / C4, c4 = (idx - r * C4) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (k0 + r < len) {
        const float* src = qb + (size_t)(k0 + r) * ld + c4;
        kv = *reinterpret_cast<const float4*>(src + a.H);
        vv = *reinterpret_cast<const float4*>(src + 2 * a.H);
        const float4 bk = *reinterpret_cast<const float4*>(bq + a.H + c4), bv = *reinterpret_cast<const float4*>(bq + 2 * a.H + c4);
        kv.x += bk.x; kv.y += bk.y; kv.z += bk.z; kv.w += bk.w;
        vv.x += bv.x; vv.y += bv.y; vv.z += bv.z; vv.w += bv.w;
      }
      *reinterpret_cast<float4*>(&k_s[r * LDK + c4]) = kv;
      *reinterpret_cast<float4*>(&v_s[r * LDV + c4]) = vv;
    }
  }
  static __device__ __forceinline__ f32x4 qk(float q, const float* k_s, int j, int kk, int c, int g, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(q, k_s[(16 * j + c) * LDK + 4 * kk + g], acc, 0, 0, 0);
  }
  static __device__ __forceinline__ float load_p(const float* pw, int c, int g, int kk) { return pw[c * LDP + 4 * kk + g]; }
  static __device__ __forceinline__ f32x4 pv(float p, const float* v_s, int n, int kk, int c, int g, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(p, v_s[(4 * kk + g) * LDV + 16 * n + c], acc, 0, 0, 0);
  }
  static __device__ __forceinline__ float cvt(float v) { return v; }
};

// one block per sequence: x = its first row; pooled[j] = tanh(pool_w[j] . x + pool_b[j]) (a wave per j, fixed order), then
// the classifier row. Dynamic LDS: 2 H floats.
__global__ __launch_bounds__(256) void xenc_head_kernel(const float* x, const int32_t* seq_off, int H, const float* pool_w,
                                                        const float* pool_b, const float* cls_w, const float* cls_b, float* out) {
  extern __shared__ float hs[];
  float* xs = hs;
  float* pooled = hs + H;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xr = x + (size_t)seq_off[b] * H;
  for (int i = tid; i < H; i += 256) xs[i] = xr[i];
  __syncthreads();
  for (int j = wave; j < H; j += 4) {
    const float* wr = pool_w + (size_t)j * H;
    float acc = 0.f;
    for (int i = lane; i < H; i += 64) acc = fmaf(wr[i], xs[i], acc);
    acc = wave_sum(acc);
    if (lane == 0) pooled[j] = tanhf(acc + pool_b[j]);
  }
  __syncthreads();
  if (wave == 0) {
    float acc = 0.f;
    for (int i = lane; i < H; i += 64) acc = fmaf(cls_w[i], pooled[i], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[b] = acc + cls_b[0];
  }
}

__global__ void xenc_meta_kernel(XencMetaChunk ch, int n, int32_t* dst) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = ch.v[i];
}

}  // namespace

hipError_t launch_xenc_meta(const int32_t* host, int n, int32_t* dst, hipStream_t s) {
  // through kernel arguments: they are copied when the launch is enqueued, so the caller's array is free on return and no
  // host-to-device copy (pageable memory: a synchronisation) is needed
  for (int i0 = 0; i0 < n; i0 += XencMetaChunk::N) {
    XencMetaChunk ch;
    const int m = n - i0 < XencMetaChunk::N ? n - i0 : XencMetaChunk::N;
    for (int i = 0; i < m; ++i) ch.v[i] = host[i0 + i];
    for (int i = m; i < XencMetaChunk::N; ++i) ch.v[i] = 0;
    hipLaunchKernelGGL(xenc_meta_kernel, dim3(1), dim3(XencMetaChunk::N), 0, s, ch, m, dst + i0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_xenc_embed_ln(const XencEmbedArgs& a, __half* outh, hipStream_t s) {
  if (a.T <= 0 || a.H <= 0 || (a.H & 3)) return hipErrorInvalidValue;
  if (outh) hipLaunchKernelGGL(xenc_embed_ln_kernel<true>, dim3((a.T + 3) / 4), dim3(256), 0, s, a, outh);
  else hipLaunchKernelGGL(xenc_embed_ln_kernel<false>, dim3((a.T + 3) / 4), dim3(256), 0, s, a, outh);
  return hipGetLastError();
}

hipError_t launch_xenc_attn(const XencAttnArgs& a, int dh, hipStream_t s) { return launch_xenc_attn_as<XencAttnF32>(a, dh, s); }

hipError_t launch_xenc_add_ln(const float* y, const float* bias, const float* resid, const float* ln_w, const float* ln_b, float eps,
                              int T, int H, float* out, __half* outh, hipStream_t s) {
  if (T <= 0 || H <= 0 || (H & 3)) return hipErrorInvalidValue;
  const dim3 grid((T + 3) / 4);
  // the two forms the walk has: fp32 adds while loading, f16 has added in the GEMM and wants the f16 copy
  if (bias && resid && !outh)
    hipLaunchKernelGGL((xenc_add_ln_kernel<true, false>), grid, dim3(256), 0, s, y, bias, resid, ln_w, ln_b, eps, T, H, out, outh);
  else if (!bias && !resid && outh)
    hipLaunchKernelGGL((xenc_add_ln_kernel<false, true>), grid, dim3(256), 0, s, y, bias, resid, ln_w, ln_b, eps, T, H, out, outh);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_xenc_bias_gelu(float* x, const float* bias, int rows, int N, hipStream_t s) {
  if (rows <= 0 || N <= 0 || (N & 3)) return hipErrorInvalidValue;
  const long long n4 = (long long)rows * N / 4;
  hipLaunchKernelGGL(xenc_bias_gelu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, bias, n4, N);
  return hipGetLastError();
}

hipError_t launch_xenc_head(const float* x, const int32_t* seq_off, int bz, int H, const float* pool_w, const float* pool_b,
                            const float* cls_w, const float* cls_b, float* out, hipStream_t s) {
  if (bz <= 0 || H <= 0 || (size_t)2 * H * sizeof(float) > 48 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xenc_head_kernel, dim3(bz), dim3(256), 2 * H * sizeof(float), s, x, seq_off, H, pool_w, pool_b, cls_w, cls_b, out);
  return hipGetLastError();
}

}  // namespace rpr
