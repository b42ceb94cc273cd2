// BERT cross-encoder forward over a PACKED batch (rpr_xenc_score in xenc_api.hip). Replaces the HF
// BertForSequenceClassification pass of the reference's teacher (modeling/cross_encoder.py, tasks/reranker.py).
//
// Packed: only attended tokens exist. Row t of every [T, .] matrix is one token, sequence b owns the rows
// seq_off[b] .. seq_off[b + 1] - 1, and a row carries its original position id. Attention runs per (sequence, head) over
// that sequence's rows, so there is no key mask and padding costs nothing. Everything is fp32; the matrix products are the
// exact-fp32 GEMM of gemm_f32.hip (no bias, no activation: those live here).
//
//   xenc_embed_ln       LayerNorm(word[id] + type[tt] + pos[p])
//   xenc_attn<DH>       softmax((q + b_q)(k + b_k)^T / sqrt(DH)) (v + b_v), DH = 32 or 64, v_mfma_f32_16x16x4_f32 for both products
//   xenc_bias_resid_ln  LayerNorm(y + bias + residual)
//   xenc_bias_gelu      bias + exact (erf) GELU, in place
//   xenc_head           tanh(pool_w x_first + pool_b) . cls_w + cls_b of every sequence's first row
//
// Every reduction has a fixed order (shuffles inside a wave, no atomics): a call repeated gives the same bits.
#include "common.h"

namespace rpr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LayerNorm of one row held as out[0 .. H) (already written by this wave: lane l owns the float4 pieces l, l + 64, ...),
// biased variance, two passes over the row
__device__ __forceinline__ void row_layernorm(float* out, int H, float sum, const float* w, const float* b, float eps, int lane) {
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
  }
}

// one wave per row, 4 rows per block; H % 4 == 0. Ids outside their tables are clamped (memory safety only: the Python
// boundary refuses them before the call).
__global__ __launch_bounds__(256) void xenc_embed_ln_kernel(XencEmbedArgs a) {
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
  row_layernorm(out, a.H, sum, a.ln_w, a.ln_b, a.eps, lane);
}

// out may be resid (in place): a lane reads its pieces of the residual before it writes them
__global__ __launch_bounds__(256) void xenc_bias_resid_ln_kernel(const float* y, const float* bias, const float* resid, const float* w,
                                                                 const float* b, float eps, int T, int H, float* outp) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* yr = y + (size_t)row * H;
  const float* rr = resid + (size_t)row * H;
  float* out = outp + (size_t)row * H;
  float sum = 0.f;
  for (int i = lane * 4; i < H; i += 256) {
    const float4 x = *reinterpret_cast<const float4*>(yr + i), bb = *reinterpret_cast<const float4*>(bias + i),
                 r = *reinterpret_cast<const float4*>(rr + i);
    float4 v;
    v.x = (x.x + bb.x) + r.x; v.y = (x.y + bb.y) + r.y; v.z = (x.z + bb.z) + r.z; v.w = (x.w + bb.w) + r.w;
    *reinterpret_cast<float4*>(out + i) = v;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  row_layernorm(out, H, sum, w, b, eps, lane);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// x [rows, N] in place; N % 4 == 0, n4 = rows * N / 4
__global__ __launch_bounds__(256) void xenc_bias_gelu_kernel(float* x, const float* bias, long long n4, int N) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = reinterpret_cast<float4*>(x)[i];
  const float4 b = *reinterpret_cast<const float4*>(bias + (int)((i * 4) % N));
  v.x = gelu_erf(v.x + b.x); v.y = gelu_erf(v.y + b.y); v.z = gelu_erf(v.z + b.z); v.w = gelu_erf(v.w + b.w);
  reinterpret_cast<float4*>(x)[i] = v;
}

// Attention of one (64-query tile of a sequence, head). 4 waves, 16 query rows each; keys and values walk through LDS in
// tiles of 64 rows with an online softmax. MFMA 16x16x4 f32 operand maps (lane l, c = l & 15, g = l >> 4):
//   A[i = c][k = g], B[k = g][j = c], C/D[row = 4 g + reg][col = c].
// S = Q K^T: A = Q[row c][d = 4 kk + g] (registers, loaded once), B = K[key 16 j + c][d = 4 kk + g]: four independent
//   accumulators (j) per wave. LDS row stride DH + 4 floats: the 64 lanes of a B read hit 64 different banks.
// O += P V:  P leaves the S accumulators in the C map and is needed in the A map: through a private LDS strip per wave
//   (row stride 64 + 4). B = V[key 4 kk + g][d = 16 n + c], row stride DH + 16: again 64 different banks.
// The C map of S and of O share the row (4 g + reg), so the running maximum / sum of a row and the rescaling of O stay in
// the lane's own registers; a row's 64 scores sit in 16 lanes x 4 accumulators: reduced with 4 xor-shuffles.
// A tile always holds at least one key of the sequence (k0 < len), so the running maximum is finite after the first
// tile; keys past the end get -inf and weigh exactly 0. Query rows past the end compute on q = 0 and are not stored.
template <int DH>
__global__ __launch_bounds__(256) void xenc_attn_kernel(XencAttnArgs a) {
  constexpr int LDK = DH + 4, LDV = DH + 16, LDP = 64 + 4, KS = DH / 4, NB = DH / 16, C4 = DH / 4;
  __shared__ __attribute__((aligned(16))) float k_s[64 * LDK];
  __shared__ __attribute__((aligned(16))) float v_s[64 * LDV];
  __shared__ float p_s[4 * 16 * LDP];
  const int2 t = a.tiles[blockIdx.x];   // (sequence, first query row of the tile inside it)
  const int head = blockIdx.y;
  const int s0 = a.seq_off[t.x], len = a.seq_off[t.x + 1] - s0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const size_t ld = (size_t)3 * a.H;
  const float* qb = a.qkv + (size_t)s0 * ld + (size_t)head * DH;
  const float* bq = a.bias + head * DH;
  const float scale = 1.0f / sqrtf((float)DH);
  const bool wave_live = t.y + wave * 16 < len;

  float qf[KS];
  {
    const int qrow = t.y + wave * 16 + c;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) qf[kk] = qrow < len ? qb[(size_t)qrow * ld + 4 * kk + g] + bq[4 * kk + g] : 0.f;
  }
  f32x4 o[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
  float* pw = p_s + wave * 16 * LDP;

  for (int k0 = 0; k0 < len; k0 += 64) {
    __syncthreads();   // the previous tile's K, V and P have been read
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
    __syncthreads();
    if (wave_live) {
      f32x4 s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          s[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kk], k_s[(16 * j + c) * LDK + 4 * kk + g], s[j], 0, 0, 0);
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
          pw[(4 * g + r) * LDP + 16 * j + c] = p;
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
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const float pa = pw[c * LDP + 4 * kk + g];
#pragma unroll
        for (int n = 0; n < NB; ++n)
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, v_s[(4 * kk + g) * LDV + 16 * n + c], o[n], 0, 0, 0);
      }
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = t.y + wave * 16 + 4 * g + r;
    if (qrow >= len) continue;
    const float inv = 1.0f / l_run[r];
    float* dst = a.out + (size_t)(s0 + qrow) * a.H + (size_t)head * DH + c;
#pragma unroll
    for (int n = 0; n < NB; ++n) dst[16 * n] = o[n][r] * inv;
  }
}

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

hipError_t launch_xenc_embed_ln(const XencEmbedArgs& a, hipStream_t s) {
  if (a.T <= 0 || a.H <= 0 || (a.H & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xenc_embed_ln_kernel, dim3((a.T + 3) / 4), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_xenc_attn(const XencAttnArgs& a, int dh, hipStream_t s) {
  if (a.ntiles <= 0 || a.heads <= 0 || a.H != a.heads * dh) return hipErrorInvalidValue;
  if (dh == 32) hipLaunchKernelGGL(xenc_attn_kernel<32>, dim3(a.ntiles, a.heads), dim3(256), 0, s, a);
  else if (dh == 64) hipLaunchKernelGGL(xenc_attn_kernel<64>, dim3(a.ntiles, a.heads), dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_xenc_bias_resid_ln(const float* y, const float* bias, const float* resid, const float* ln_w, const float* ln_b,
                                     float eps, int T, int H, float* out, hipStream_t s) {
  if (T <= 0 || H <= 0 || (H & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xenc_bias_resid_ln_kernel, dim3((T + 3) / 4), dim3(256), 0, s, y, bias, resid, ln_w, ln_b, eps, T, H, out);
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
