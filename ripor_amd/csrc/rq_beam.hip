// Beam encoding of the residual quantizer (rpr_rq_encode_beam in rq_api.hip; DESIGN.md §9c, tests/rq_beam_ref.py).
//
// A row keeps up to B candidate encodings (its beam) through the levels. Per level, three launches:
//   rq_topt_kernel   every beam entry is a residual row; its T smallest |c_k|^2 - 2 r.c_k with their k, in (score, k) order;
//   rq_merge_kernel  per original row the best T of the b * T candidates by (|r_s|^2 + score, parent slot s, k), the
//                    children's residuals r_s - c_k into the other residual plane, their |r|^2, parent slot and code;
// and after the last level rq_backtrack_kernel walks the parent slots back from slot 0 and writes codes [n, M].
// With B = 1 every step is the greedy chain of rq_assign_kernel (gemm_f32.hip), bit for bit: the dot products are the same
// MFMA chain, the residual update and the |r|^2 sums the same expressions in the same order.
#include "common.h"

namespace rpr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BK = 32, LDSP = BK + 4;   // the operand tiles of gemm_f32.hip

// one (v, k) into a list sorted ascending, the last entry falls out. LEX = false: by v alone, an equal value goes behind
// the entries already there (arrival order); LEX = true: by (v, k).
template <bool LEX>
__device__ __forceinline__ void topt_insert(float (&lv)[RQ_MAX_BEAM], int (&li)[RQ_MAX_BEAM], float v, int k) {
  bool below = false;   // the entry before this one already moved down
  float pv = 0.f;
  int pi = 0;
#pragma unroll
  for (int t = 0; t < RQ_MAX_BEAM; ++t) {
    const bool here = v < lv[t] || (LEX && v == lv[t] && k < li[t]);
    const float ov = lv[t];
    const int oi = li[t];
    lv[t] = here ? (below ? pv : v) : ov;
    li[t] = here ? (below ? pi : k) : oi;
    below = here; pv = ov; pi = oi;
  }
}

}  // namespace

// The main loop is rq_assign_kernel's, unchanged (128-row tile, 32x32x2 fp32 MFMA, double-buffered operands, every
// codeword tile of BN rows walked by the block): a running minimum per accumulator register does not extend to the T
// smallest, since a lane sees only K / 64 codewords of a row. Instead, after a codeword tile's last MFMA the operand
// buffers are dead and receive the tile's 128 x BN scores, row-major with an odd stride; two threads per row (the row's
// two halves of BN / 2 columns) each scan their half in increasing k into a sorted list of RQ_MAX_BEAM (score, k) pairs
// in registers with a strict '<', so equal scores keep the smaller k in front. After the last tile the two lists of a row
// are merged in (score, k) order and its first T entries written.
template <int BN, bool FULL>
__global__ __launch_bounds__(256, 2) void rq_topt_kernel(RqTopTArgs g) {
  constexpr int BM = RQ_BM;
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int PA = BM / 32, PW = BN / 32;
  constexpr int TILE = (BM + BN) * LDSP;
  constexpr int SS = BN + 1;                      // score row stride: the 32 rows of a lane group in 32 distinct banks
  static_assert(BM * SS <= 2 * TILE, "the score tile fits the operand buffers");
  static_assert(BM * RQ_MAX_BEAM * 2 <= 2 * TILE, "so do the lists of the upper halves");
  __shared__ __attribute__((aligned(16))) float smem[2 * TILE];

  const long long bm = (long long)blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int c4 = (tid & 7) * 4, r0 = tid >> 3;
  const int frow = lane & 31, fk = (lane >> 5) * 4;
  const int a_off = (wm * (BM / 2) + frow) * LDSP + fk;
  const int w_off = (BM + wn * (BN / 2) + frow) * LDSP + fk;
  const size_t step = (size_t)32 * g.d;
  const float* Ab = g.R + (size_t)(bm + r0) * g.d + c4;
  const int nkt = g.d / BK;
  const int srow = tid & (BM - 1), shalf = tid >> 7;   // the scan: row and half of its columns

  float lv[RQ_MAX_BEAM];
  int li[RQ_MAX_BEAM];
#pragma unroll
  for (int t = 0; t < RQ_MAX_BEAM; ++t) { lv[t] = INFINITY; li[t] = 0; }

  for (int bn = 0; bn < g.K; bn += BN) {   // K % BN == 0: every codeword tile is full
    const float* Wb = g.C + (size_t)(bn + r0) * g.d + c4;
    float4 ra[PA], rw[PW];
    auto gload = [&](int k0) {
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        if (FULL || bm + r0 + 32 * i < g.rows) ra[i] = *reinterpret_cast<const float4*>(Ab + i * step + k0);
        else ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < PW; ++i) rw[i] = *reinterpret_cast<const float4*>(Wb + i * step + k0);
    };
    auto lstore = [&](float* buf) {
#pragma unroll
      for (int i = 0; i < PA; ++i) *reinterpret_cast<float4*>(&buf[(r0 + 32 * i) * LDSP + c4]) = ra[i];
#pragma unroll
      for (int i = 0; i < PW; ++i) *reinterpret_cast<float4*>(&buf[(BM + r0 + 32 * i) * LDSP + c4]) = rw[i];
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    auto compute = [&](const float* cur) {
#pragma unroll
      for (int kk = 0; kk < BK / 8; ++kk) {
        float4 a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const float4*>(cur + a_off + i * 32 * LDSP + kk * 8);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const float4*>(cur + w_off + j * 32 * LDSP + kk * 8);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
          }
      }
    };
    gload(0);
    lstore(smem);
    __syncthreads();
    for (int kt = 0; kt + 1 < nkt; ++kt) {
      gload((kt + 1) * BK);
      compute(smem + (kt & 1) * TILE);
      lstore(smem + ((kt + 1) & 1) * TILE);
      __syncthreads();
    }
    compute(smem + ((nkt - 1) & 1) * TILE);
    __syncthreads();   // every wave is done reading operand tiles: the buffers take the scores
    // MFMA result layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of a 32 x 32 block
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * (BN / 2) + j * 32 + frow;
      const float cn = g.cnorm[bn + col];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          smem[row * SS + col] = cn - 2.0f * acc[i][j][r];
        }
    }
    __syncthreads();
    {
      const float* sp = smem + srow * SS + shalf * (BN / 2);
      const int k0 = bn + shalf * (BN / 2);
#pragma unroll 8
      for (int c = 0; c < BN / 2; ++c) {
        const float v = sp[c];
        if (v < lv[RQ_MAX_BEAM - 1]) topt_insert<false>(lv, li, v, k0 + c);
      }
    }
    __syncthreads();   // the next codeword tile overwrites the scores
  }

  // the upper half's list joins the lower half's in (score, k) order
  float* mv = smem;                                              // [BM][RQ_MAX_BEAM]
  int* mi = reinterpret_cast<int*>(smem + BM * RQ_MAX_BEAM);     // [BM][RQ_MAX_BEAM]
  if (shalf == 1) {
#pragma unroll
    for (int t = 0; t < RQ_MAX_BEAM; ++t) { mv[srow * RQ_MAX_BEAM + t] = lv[t]; mi[srow * RQ_MAX_BEAM + t] = li[t]; }
  }
  __syncthreads();
  if (shalf == 1 || (!FULL && bm + srow >= g.rows)) return;
#pragma unroll
  for (int u = 0; u < RQ_MAX_BEAM; ++u) topt_insert<true>(lv, li, mv[srow * RQ_MAX_BEAM + u], mi[srow * RQ_MAX_BEAM + u]);
  float* ov = g.cand_v + (size_t)(bm + srow) * g.T;
  uint16_t* ok = g.cand_k + (size_t)(bm + srow) * g.T;
#pragma unroll
  for (int t = 0; t < RQ_MAX_BEAM; ++t)
    if (t < g.T) { ov[t] = lv[t]; ok[t] = (uint16_t)li[t]; }
}

template <int BN>
static hipError_t launch_rq_topt_bn(const RqTopTArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.rows + RQ_BM - 1) / RQ_BM);
  if (a.rows % RQ_BM == 0) hipLaunchKernelGGL((rq_topt_kernel<BN, true>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rq_topt_kernel<BN, false>), dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rq_topt(const RqTopTArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.d <= 0 || a.d % BK || a.K <= 0 || a.K % 64 || a.K > RQ_MAX_K || a.T < 1 || a.T > RQ_MAX_BEAM) return hipErrorInvalidValue;
  return a.K % 128 == 0 ? launch_rq_topt_bn<128>(a, s) : launch_rq_topt_bn<64>(a, s);
}

// One block per RQ_BM original rows (the blocks of rq_assign_kernel's epilogue, so that the per-block fp64 partials are
// the greedy ones at B = 1). A thread per row merges the b sorted candidate lists of its parents: T times the smallest
// head by (total, s), total = |r_s|^2 + score added in fp64 (exact for all but absurd exponent gaps, so that the order
// inside a parent stays the (score, k) order of its list). Then one wave per (row, child): r_s - c_k in 16-byte pieces into
// the other plane, the new |r|^2 as a lane-strided fp32 chain and an fp64 butterfly, exactly as the greedy epilogue.
__global__ __launch_bounds__(256) void rq_merge_kernel(RqMergeArgs g) {
  __shared__ uint16_t sel_code[RQ_BM * RQ_MAX_BEAM];
  __shared__ unsigned char sel_par[RQ_BM * RQ_MAX_BEAM];
  __shared__ double wsum[4];
  const long long bm = (long long)blockIdx.x * RQ_BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < RQ_BM && bm + tid < g.n) {
    const size_t e0 = (size_t)(bm + tid) * g.b;     // the row's first beam entry
    unsigned heads = 0;                             // 4 bits per parent: candidates of its list already taken
    for (int t = 0; t < g.T; ++t) {
      double bt = 0.0;
      int bs = -1;
      for (int s = 0; s < g.b; ++s) {
        const int p = (heads >> (4 * s)) & 15;
        const double tot = (g.rnorm ? (double)g.rnorm[e0 + s] : 0.0) + (double)g.cand_v[(e0 + s) * g.T + p];
        if (bs < 0 || tot < bt) { bt = tot; bs = s; }
      }
      const int p = (heads >> (4 * bs)) & 15;
      const int k = g.cand_k[(e0 + bs) * g.T + p];
      heads += 1u << (4 * bs);
      sel_par[tid * RQ_MAX_BEAM + t] = (unsigned char)bs;
      sel_code[tid * RQ_MAX_BEAM + t] = (uint16_t)k;
      g.par[(size_t)(bm + tid) * g.hstride + t] = (unsigned char)bs;
      g.code[(size_t)(bm + tid) * g.hstride + t] = (uint16_t)k;
    }
  }
  __syncthreads();
  double acc_w = 0.0;
  for (int row = wave; row < RQ_BM; row += 4) {
    if (bm + row >= g.n) break;
    for (int t = 0; t < g.T; ++t) {
      const float* rp = g.Rin + ((size_t)(bm + row) * g.b + sel_par[row * RQ_MAX_BEAM + t]) * g.d;
      const float* cp = g.C + (size_t)sel_code[row * RQ_MAX_BEAM + t] * g.d;
      float* op = g.Rout + ((size_t)(bm + row) * g.T + t) * g.d;
      float ss = 0.f;
      for (int off = lane * 4; off < g.d; off += 256) {
        float4 x = *reinterpret_cast<const float4*>(rp + off);
        const float4 c = *reinterpret_cast<const float4*>(cp + off);
        x.x -= c.x; x.y -= c.y; x.z -= c.z; x.w -= c.w;
        *reinterpret_cast<float4*>(op + off) = x;
        ss = fmaf(x.x, x.x, ss); ss = fmaf(x.y, x.y, ss); ss = fmaf(x.z, x.z, ss); ss = fmaf(x.w, x.w, ss);
      }
      double sd = ss;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) sd += __shfl_xor(sd, m);
      if (lane == 0) g.rnorm_out[(size_t)(bm + row) * g.T + t] = (float)sd;
      if (t == 0) acc_w += sd;
    }
  }
  if (lane == 0) wsum[wave] = acc_w;
  __syncthreads();
  if (tid == 0) g.part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

hipError_t launch_rq_merge(const RqMergeArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (a.d <= 0 || a.d % 4 || a.b < 1 || a.b > RQ_MAX_BEAM || a.T < 1 || a.T > RQ_MAX_BEAM || a.hstride < a.T) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rq_merge_kernel, dim3((unsigned)((a.n + RQ_BM - 1) / RQ_BM)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// codes[row][m] = the level-m code on the path that ends in slot 0 after the last level
__global__ __launch_bounds__(256) void rq_backtrack_kernel(const unsigned char* par, const uint16_t* code, long long n, int M,
                                                           int hstride, uint16_t* codes) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const size_t plane = (size_t)n * hstride;
  int s = 0;
  for (int m = M - 1; m >= 0; --m) {
    const size_t e = (size_t)m * plane + (size_t)row * hstride + s;
    codes[(size_t)row * M + m] = code[e];
    s = par[e];
  }
}

hipError_t launch_rq_backtrack(const unsigned char* par, const uint16_t* code, long long n, int M, int hstride, uint16_t* codes,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rq_backtrack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, par, code, n, M, hstride, codes);
  return hipGetLastError();
}

}  // namespace rpr
