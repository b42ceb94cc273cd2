// Split-precision linear layer on the gfx950 matrix cores: C[M,N] = act(A[M,K] @ W[N,K]^T) (+ residual)
// with fp32-equivalent accuracy from f16 MFMA.
//
// Every fp32 operand x is carried as two f16 planes  s*x = hi + lo,  hi = f16(s*x), lo = f16(s*x - hi), with a
// power-of-two scale s per tensor class (weights 2^8, activations 2^4, FF intermediate 2^-4; common.h) that keeps
// lo out of the f16 subnormals and the FF intermediate inside the f16 range: 22 significant bits,
// |s*x - hi - lo| <= 2^-22 |s*x|. A product is evaluated as  hi*hi + hi*lo + lo*hi  with three
// v_mfma_f32_32x32x16_f16 accumulating in fp32 (the dropped lo*lo term is <= 2^-22 |xy|); the epilogue multiplies
// the accumulators by 1/(s_A s_W) (exact). Measured on the t5-base golden model (tools/precision_probe.py): logits
// differ from the exact-fp32 path by <= 7.4e-5 (mean 1.2e-5; two fp32 summation orders differ by <= 4e-5), beam
// scores by <= 5e-6 — inside the 1e-4 parity bar — while the matrix pipe runs at the f16 rate: 3 MFMAs of 32
// cycles instead of 8 fp32 MFMAs of 64 cycles per 32x32x16 block = 5.3x the fp32-MFMA roof. The exact fp32 kernel
// (gemm_f32.hip) stays selectable (RPR_PRECISION=f32) as the numerical reference.
//
// Planes are produced where the data is written (RMSNorm, attention and ReLU epilogues emit hi/lo
// planes; weights are split once at rpr_load_model), so this kernel only moves 16-bit data:
// operand traffic is 4 B/element, the same as fp32.
//
// Kernels: gemm_h2_pp_kernel (256x256x32 tiles, 8 waves, ping-pong schedule; the default whenever a launch has
// >= 112 such tiles) and gemm_h2_dma_kernel (128x128 / 128x64 tiles, 4 waves) for smaller launches; both stage
// K-tiles with LDS-DMA into unpadded XOR-swizzled rows. Earlier variants (register staging, in-phase software
// pipelining) are in the history and in DESIGN.md §5 / §8 with their measured numbers.
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <hip/hip_fp16.h>

#include <cstdlib>

#include "common.h"
#include "gemm_route.h"

#include <algorithm>
#include <vector>

namespace rpr {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// A wave's accumulators as the epilogue takes them: TM x TN tiles of 32 x 32 (v_mfma_f32_32x32x16_*), or, M16, the same
// outputs as 2 TM x 2 TN tiles of 16 x 16 (v_mfma_f32_16x16x32_f16: the tail passes' 256x256 kernel)
template <bool M16, int TM, int TN> struct H2Acc { typedef f32x16 type[TM][TN]; };
template <int TM, int TN> struct H2Acc<true, TM, TN> { typedef f32x4 type[2 * TM][2 * TN]; };

// the LDS-transposed epilogue of the tile kernels (defined behind gemm_h2_dma_kernel)
template <bool FULL, int TM, int TN, int WM, int WN, int BM, int BN, bool BOUT = false, bool M16 = false>
__device__ __forceinline__ void h2_epilogue_256(const GemmH2Args& g, typename H2Acc<M16, TM, TN>::type& acc, __half* smem, int wave, int lane, int bm,
                                                int bn, int wm, int wn, const float* rs_tile, float acc_scale);



// ---- LDS-DMA variant -------------------------------------------------------------------------------
// Same math, but the K-tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (no staging VGPRs, no
// ds_write pass — the ds_write_b128 of the register-staged kernel cost as many LDS cycles as all the
// fragment reads and made the LDS co-critical with the matrix pipe). LDS is double-buffered; the DMA
// of tile t+1 is issued before the MFMAs of tile t and drained by the single barrier that ends the
// iteration. An LDS-DMA instruction writes wave-uniform base + lane*16 B, so rows are stored
// unpadded (64 B) and the 16-byte segments of a row are XOR-swizzled with (row>>2)&3 on the SOURCE
// address and again on the fragment read: the 16-lane groups of ds_read_b128 then hit 16 distinct
// 4-bank slots.
// STAGES = LDS buffers. 2: one K-tile of prefetch, several blocks per CU hide the rest (large launches).
// 4: launches with fewer tiles than CUs (small in-flight batches) — one block per CU walks its whole K alone, and
// with one tile of prefetch every K-tile paid a full L2/HBM latency (~1.2 us x 24 K-tiles per GEMM); three tiles
// in flight and a counted s_waitcnt make the walk bandwidth-bound instead.
// BF16 = false: the split-precision f16 hi/lo planes (3 MFMAs per product, K-tile of 32). BF16 = true: ONE bf16 plane per
// operand and one v_mfma_f32_32x32x16_bf16 per product with fp32 accumulation — the arithmetic of the reference's bf16
// autocast for the training GEMMs (RPR_PREC_BF16; main.py:152, tasks/trainer.py:229), except that the result is not
// rounded to bf16. The LDS layout is the same: where the split kernel keeps the lo planes, this one keeps the NEXT 32
// columns of K, so a K-tile is 64 deep (16 MFMAs per wave and barrier for the 128x128 tile instead of 8).
template <int BM, int BN, int WM, int WN, bool FULL, int STAGES = 2, bool BF16 = false>
__global__ __launch_bounds__(64 * WM * WN, STAGES > 2 ? 1 : (WM * WN) / 4 * ((BM * BN >= 256 * 256) ? 1 : 2))
void gemm_h2_dma_kernel(GemmH2Args g, int tiles_m, int tiles_n) {
  // per-tensor dynamic plane scales (training): read from the device; g itself must stay untouched — a kernel that writes
  // to its by-value argument struct gets a private copy of all 320 bytes in scratch (measured: +20 % per launch)
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  constexpr int NW = WM * WN;                    // waves per block
  constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);  // MFMA 32x32 tiles per wave
  constexpr int ROWS = 2 * (BM + BN);            // LDS rows of 32 halves (64 B) per buffer
  constexpr int KSTEP = BF16 ? 2 * HBK : HBK;    // K columns per tile
  constexpr int NINST = ROWS / 16;               // DMA wave-instructions per K-tile (16 rows each)
  constexpr int PER_WAVE = NINST / NW;
  static_assert(NINST % NW == 0, "tile rows must split evenly over the waves");
  __shared__ __attribute__((aligned(16))) __half smem[STAGES * ROWS * HBK];
  __shared__ float rs_tile[BM];                      // fused RMSNorm: rsqrt(mean(x^2) + eps) of the tile's rows (split-precision launches)
  static_assert(64 * WM * WN >= BM, "one thread per tile row fills rs_tile");

  int nt = tiles_m * tiles_n;
  int bid = blockIdx.x;
  if (g.m_dev) {   // packed encoder: only the tiles holding live rows are distributed (evenly) over the XCDs
    const int live = max(0, min(*g.m_dev - g.m_base, g.M));
    if (g.live_hi > 0 && (*g.m_dev <= g.live_lo || *g.m_dev > g.live_hi)) return;   // the other kernel of the pair runs
    nt = ((live + BM - 1) / BM) * tiles_n;
    if (bid >= nt) return;
  }
  {
    const int q = nt >> 3, r = nt & 7, x = bid & 7, k = bid >> 3;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
  }
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int bm = tm * BM, bn = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  if (!BF16 && g.row_ssq && tid < BM) {   // read by the epilogue, behind the K-loop's barriers
    const int m = bm + tid;
    rs_tile[tid] = (m < g.M) ? ssq_rsqrt(g.row_ssq[m], g.inv_d_fix, g.eps) : 1.f;
  }
  // split-K (training weight gradients: few output tiles, K = thousands of rows): blockIdx.y walks its own range of
  // K-tiles and stores a partial result at out + blockIdx.y * part_stride; splitk_reduce_kernel adds them in order
  int nkt = g.K / KSTEP, kbeg = 0;
  if (g.ksplit > 1) {
    const int per = (nkt + g.ksplit - 1) / g.ksplit;
    kbeg = blockIdx.y * per;
    nkt = min(per, nkt - kbeg);
  }

  // per-instruction source pointers (k0 = 0): instruction j of this wave covers LDS rows
  // [16*(wave + NW*j), +16); lane -> row (lane>>2), physical segment (lane&3)
  const __half* src[PER_WAVE];
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int lrow = 16 * (wave + NW * j) + (lane >> 2);          // LDS row within the buffer
    const int seg = (lane & 3) ^ ((lrow >> 2) & 3);               // logical segment fetched into this slot
    const __half* base;
    int trow, limit;
    size_t ld;
    const size_t second = BF16 ? (size_t)HBK : 0;                   // the "second plane" of the bf16 mode: the next 32 columns
    if (lrow < BM) { base = g.A; trow = bm + lrow; limit = g.M; ld = g.lda; }
    else if (lrow < 2 * BM) { base = g.A + (BF16 ? second : g.a_ps); trow = bm + lrow - BM; limit = g.M; ld = g.lda; }
    else if (lrow < 2 * BM + BN) { base = g.W; trow = bn + lrow - 2 * BM; limit = g.N; ld = g.ldw; }
    else { base = g.W + (BF16 ? second : g.w_ps); trow = bn + lrow - 2 * BM - BN; limit = g.N; ld = g.ldw; }
    if (!FULL && trow >= limit) trow = limit - 1;                  // ragged tile: duplicate a valid row
    src[j] = base + (size_t)trow * ld + seg * 8 + (size_t)kbeg * KSTEP;
  }
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {
      __half* dst = smem + (size_t)buf * ROWS * HBK + 16 * (wave + NW * j) * HBK;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + k0),
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment address: row = tile row, 16-B segment (2c + lane>>5) ^ swizzle(row); all row offsets used
  // below are multiples of 16, so swizzle(row) = (lane>>2)&3 for every fragment of this lane
  const int frow = lane & 31, sw = (lane >> 2) & 3, hf = lane >> 5;
  const int a_row = wm * (BM / WM) + frow, w_row = 2 * BM + wn * (BN / WN) + frow;

  auto compute = [&](int buf) {
    const __half* base = smem + (size_t)buf * ROWS * HBK;
#pragma unroll
    for (int c = 0; c < HBK / 16; ++c) {
      const int so = ((2 * c + hf) ^ sw) * 8;
      if (BF16) {   // columns k .. k+31 in the first row groups, k+32 .. k+63 in the second
        bf16x8 a0[TM], a1[TM], b0[TN], b1[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          a0[i] = *reinterpret_cast<const bf16x8*>(base + (a_row + i * 32) * HBK + so);
          a1[i] = *reinterpret_cast<const bf16x8*>(base + (BM + a_row + i * 32) * HBK + so);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          b0[j] = *reinterpret_cast<const bf16x8*>(base + (w_row + j * 32) * HBK + so);
          b1[j] = *reinterpret_cast<const bf16x8*>(base + (BN + w_row + j * 32) * HBK + so);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
        continue;
      }
      f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const f16x8*>(base + (a_row + i * 32) * HBK + so);
        al[i] = *reinterpret_cast<const f16x8*>(base + (BM + a_row + i * 32) * HBK + so);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const f16x8*>(base + (w_row + j * 32) * HBK + so);
        bl[j] = *reinterpret_cast<const f16x8*>(base + (BN + w_row + j * 32) * HBK + so);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
  };

  if (STAGES == 2) {
    stage(0, 0);
    __syncthreads();  // drains the DMA (vmcnt(0)) and publishes buffer 0
    for (int kt = 0; kt + 1 < nkt; ++kt) {
      stage((kt + 1) & 1, (kt + 1) * KSTEP);
      compute(kt & 1);
      __syncthreads();
    }
    compute((nkt - 1) & 1);
  } else {
    constexpr int AHEAD = STAGES - 1;                          // tiles requested before the first compute
    static_assert(PER_WAVE * (AHEAD - 1) <= 63, "vmcnt is a 6-bit counter");
    // vmcnt(N) immediate: bits [3:0] = N & 15, [15:14] = N >> 4; expcnt/lgkmcnt fields left at "no wait"
    constexpr int KEEP = PER_WAVE * (AHEAD - 1);
    constexpr int WAIT_KEEP = (KEEP & 15) | ((KEEP >> 4) << 14) | 0x0f70;
    constexpr int WAIT_NONE = 0x0f70;
#pragma unroll
    for (int t = 0; t < AHEAD; ++t)
      if (t < nkt) stage(t, t * KSTEP);
    for (int kt = 0; kt < nkt; ++kt) {
      // this wave's pieces of tile kt have landed once at most the pieces of the AHEAD-1 younger tiles are pending
      // (fewer tiles are in flight at the tail: wait for everything there)
      if (kt + AHEAD - 1 < nkt) __builtin_amdgcn_s_waitcnt(WAIT_KEEP); else __builtin_amdgcn_s_waitcnt(WAIT_NONE);
      __builtin_amdgcn_s_barrier();                            // everyone's pieces landed; compute(kt-1) is over everywhere
      __builtin_amdgcn_sched_barrier(0);
      if (kt + AHEAD < nkt) stage((kt + AHEAD) % STAGES, (kt + AHEAD) * KSTEP);   // refills the buffer of tile kt-1
      compute(kt % STAGES);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if (BF16) {
    // bf16 training GEMMs (fp32 output, optional fp32 residual and ReLU, nothing else fused: launch_gemm_h2 checks): the wave's
    // (BM / WM) x (BN / WN) outputs go through a private LDS strip (the operand buffers are free) and leave row-wise with
    // 16-byte accesses, every residual piece requested before the first store. Straight from the MFMA layout (below) a wave
    // issued 64 four-byte stores per 32 x 32 block and as many residual loads, each batch waiting behind the stores before it.
    constexpr int SH = BM / WM, SW = BN / WN;             // strip rows x columns (floats)
    static_assert((size_t)BM * BN * sizeof(float) <= sizeof(smem), "the strips of all waves fit the operand buffers");
    __syncthreads();                                      // every wave is done reading operand tiles
    float* stg = reinterpret_cast<float*>(smem) + (size_t)wave * (SH * SW);
    const int ncol_ = lane & 31, rsub_ = 4 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) stg[(i * 32 + (r & 3) + 8 * (r >> 2) + rsub_) * SW + j * 32 + ncol_] = acc[i][j][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);                   // lgkmcnt(0): the wave's own LDS writes have landed
    __builtin_amdgcn_wave_barrier();
    constexpr int LPR = SW / 4, RPI = 64 / LPR, NK = SH / RPI;   // lanes per staged row, rows per instruction, instructions
    const int rrow = lane / LPR, rc4 = (lane % LPR) * 4;
    const int mrow0 = bm + wm * SH, n0 = bn + wn * SW + rc4;
    const bool ncol_ok = FULL || n0 < g.N;
    float* outp = g.out[0] + (size_t)blockIdx.y * g.part_stride;   // split-K: this block's partial result
    const int ldo = g.ldo[0];
    const float relu_lo = g.relu ? 0.f : -INFINITY;
    float4 res[NK];
    if (g.resid) {
#pragma unroll
      for (int k = 0; k < NK; ++k) {   // clamped, unconditional: a branch around a load brings the conservative vmcnt(0) back
        const int m = min(mrow0 + k * RPI + rrow, g.M - 1), nc = ncol_ok ? n0 : 0;
        res[k] = *reinterpret_cast<const float4*>(g.resid + (size_t)m * g.ldr + nc);
      }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int rl = k * RPI + rrow, m = mrow0 + rl;
      float4 v = *reinterpret_cast<const float4*>(stg + rl * SW + rc4);
      v.x = fmaxf(v.x * acc_scale, relu_lo); v.y = fmaxf(v.y * acc_scale, relu_lo);
      v.z = fmaxf(v.z * acc_scale, relu_lo); v.w = fmaxf(v.w * acc_scale, relu_lo);
      if (g.resid) { v.x = res[k].x + v.x; v.y = res[k].y + v.y; v.z = res[k].z + v.z; v.w = res[k].w + v.w; }
      if (ncol_ok && (FULL || m < g.M)) *reinterpret_cast<float4*>(outp + (size_t)m * ldo + n0) = v;
    }
    return;
  }
  // split-precision launches (a few hundred to a few thousand rows in flight; every fused extra of the search path): the
  // LDS-transposed epilogue of the 256x256 kernels on this kernel's tile shape — 16-byte plane / fp32 stores, residual pieces
  // requested before the first store, row scales from LDS. (Until round 4 this kernel stored straight from the MFMA result
  // layout: two-byte plane stores and four-byte loads, 64 of each per 32 x 32 block.)
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  h2_epilogue_256<FULL, TM, TN, WM, WN, BM, BN>(g, acc, smem, wave, lane_e, bm, bn, wm, wn, g.row_ssq ? rs_tile : nullptr, acc_scale);
}

// ---- shared epilogue of the 256x256 kernels: transpose through LDS, then row-wise 16-byte global accesses --
// A wave stages 64 rows at a time: the strips of the 8 waves fill both operand buffers (128 KB).
// One strip (64 rows of a wave's 128 x 64 outputs) of the epilogue below. The strip index is a template parameter: the
// accumulators are indexed with it, and a strip loop the compiler declines to unroll — it did once the output paths had
// grown — puts all 128 of them into scratch.
template <bool FULL, int TM, int TN, int WM, int WN, int strip, int BM = 256, int BN = 256, bool BOUT = false, bool M16 = false>
__device__ __forceinline__ void h2_epilogue_strip(const GemmH2Args& g, typename H2Acc<M16, TM, TN>::type& acc, float* stg, int lane, int bm, int bn,
                                                  int wm, int wn, const float* rs_tile, float acc_scale, int Mlim) {
  constexpr int SH = 64, SW = TN * 32;
  const int ncol = lane & 31, rsub = 4 * (lane >> 5);
  if constexpr (M16) {   // the 16 x 16 C/D map with the fp32 column map of the body (column 4 c + j): lane = rows 4 (lane >> 4) + r,
    const int c16 = lane & 15, r16 = 4 * (lane >> 4);   // its four tiles = four consecutive floats of a staged row
#pragma unroll
    for (int ii = 0; ii < SH / 16; ++ii)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<f32x4*>(stg + (ii * 16 + r16 + r) * SW + 4 * c16) =
            f32x4{acc[strip * (SH / 16) + ii][0][r], acc[strip * (SH / 16) + ii][1][r], acc[strip * (SH / 16) + ii][2][r], acc[strip * (SH / 16) + ii][3][r]};
  } else
#pragma unroll
    for (int ii = 0; ii < SH / 32; ++ii)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stg[(ii * 32 + (r & 3) + 8 * (r >> 2) + rsub) * SW + j * 32 + ncol] = acc[strip * (SH / 32) + ii][j][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): the wave's own LDS writes have landed
    __builtin_amdgcn_wave_barrier();
    const int mrow0 = bm + wm * (BM / WM) + strip * SH;
    // How the output paths are written matters more than what they compute (ISA of the first version, measured with the
    // per-tile stamps of tools/gemm_tile_timeline.py: 6 us per tile on an idle chip, 10-14 us in a full launch, where the
    // same stores take 2.5 us in tools/store_probe.hip):
    //  * vmcnt counts loads AND stores in issue order. The residual pieces used to be loaded behind runtime branches in the
    //    same loop as the stores; at every join the compiler no longer knows what is pending and waits for vmcnt(0) — and
    //    it kept that wait on the path WITHOUT a residual too: each of the 32 stores of a wave waited for the previous
    //    one's write acknowledgement from the L2. Now the variants with and without a residual are separate
    //    instantiations (RES), a variant without one contains no global load at all, and one with a residual requests every
    //    piece of the strip with unconditional loads before the strip's first store. (Requesting strip 1's pieces before
    //    strip 0's stores as well — they otherwise complete behind them — needs registers the kernel does not have: all
    //    of them spill 120-290 B, half of them fits and measured -0.2 % same-box.)
    //  * every LDS read of a batch (staged rows, row scales) is issued before the first use (explicit arrays + a scheduling
    //    barrier; the compiler otherwise sinks each read next to its use behind an lgkmcnt(0)).
    auto planes_path = [&](auto res_tag) __attribute__((always_inline)) {
      // ---- f16-plane output (FF intermediate, residual stream): 8 columns per lane, 8 rows per pass
      constexpr bool RES = decltype(res_tag)::value;
      constexpr int LPR = SW / 8, RPI = 64 / LPR, NK = SH / RPI, KB = RES ? 2 : 4;   // (the residual pieces hold 64 registers)
      const int rrow = lane / LPR, rc8 = (lane % LPR) * 8;
      const int n0 = bn + wn * (BN / WN) + rc8;
      const bool ncol_ok = FULL || (n0 < g.N);          // N % 32 == 0
      const float ps = g.plane_scale;
      float amax = 0.f;                                 // split_f16's range check: one max per element, one compare per strip
      uint4 rh[RES ? NK : 1], rl_[RES ? NK : 1];
      if (RES) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          // unconditional loads from a clamped (always valid) address: a branch around a load brings the conservative
          // vmcnt(0) back; rows / columns past the limits are never stored
          const int m = min(mrow0 + k * RPI + rrow, Mlim - 1), nc = ncol_ok ? n0 : 0;
          rh[k] = *reinterpret_cast<const uint4*>(g.resid_h + (size_t)m * g.ldrh + nc);
          rl_[k] = *reinterpret_cast<const uint4*>(g.resid_h + g.r_ps + (size_t)m * g.ldrh + nc);
        }
      }
#pragma unroll
      for (int kb = 0; kb < NK; kb += KB) {
        float4 sa[KB], sb[KB];
        float scs[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow;
          sa[k] = *reinterpret_cast<const float4*>(stg + rl * SW + rc8);
          sb[k] = *reinterpret_cast<const float4*>(stg + rl * SW + rc8 + 4);
          scs[k] = rs_tile ? rs_tile[wm * (BM / WM) + strip * SH + rl] : 1.0f;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow, m = mrow0 + rl;
          const bool ok = ncol_ok && (FULL || m < Mlim);
          const float sc = rs_tile ? acc_scale * scs[k] : acc_scale;
          // pairs of columns as 2-vectors: gfx950 multiplies / adds / fmas two fp32 per instruction (v_pk_*_f32) and
          // converts two floats to a packed f16 pair in one (v_cvt_pk_f16_f32, round to nearest) — about half the VALU
          // work of the element-by-element form, which also spent a shift + or per pair on packing
          f32x2 v[4];
          *reinterpret_cast<float4*>(&v[0]) = sa[k];
          *reinterpret_cast<float4*>(&v[2]) = sb[k];
          f16x2 h[4], l[4];
          f32x2 ss2 = {0.f, 0.f};
          float am = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f32x2 x = v[e] * sc;
            if (g.relu) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); }
            if (RES) {   // the residual from its planes: (hi + lo) / X_PLANE_SCALE, both steps exact in fp32
              x += (__builtin_convertvector(reinterpret_cast<const f16x2*>(&rh[RES ? kb + k : 0])[e], f32x2) +
                    __builtin_convertvector(reinterpret_cast<const f16x2*>(&rl_[RES ? kb + k : 0])[e], f32x2)) * (1.0f / X_PLANE_SCALE);
            }
            ss2 += x * x;
            f32x2 xs = x * ps;
            am = fmaxf(am, fmaxf(fabsf(xs.x), fabsf(xs.y)));
            xs.x = __builtin_amdgcn_fmed3f(xs.x, -65504.f, 65504.f);
            xs.y = __builtin_amdgcn_fmed3f(xs.y, -65504.f, 65504.f);
            h[e] = __builtin_convertvector(xs, f16x2);
            l[e] = __builtin_convertvector(xs - __builtin_convertvector(h[e], f32x2), f16x2);
          }
          float ss = ss2.x + ss2.y;
          if (ok) {
            *reinterpret_cast<uint4*>(g.out_h + (size_t)m * g.ldoh + n0) = *reinterpret_cast<uint4*>(h);
            *reinterpret_cast<uint4*>(g.out_h + g.o_ps + (size_t)m * g.ldoh + n0) = *reinterpret_cast<uint4*>(l);
            amax = fmaxf(amax, am);
          }
          if (g.ssq_out) {   // the LPR lanes of a staged row hold this wave's 64 columns of output row m
            if (!ok) ss = 0.f;
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
            if ((lane % LPR) == 0 && (FULL || m < Mlim)) atomicAdd(g.ssq_out + m, ssq_to_fix(ss, g.sat));
          }
        }
      }
      if (amax > 65504.f && g.sat) *g.sat = 1u;
    };
    auto fp32_path = [&](auto res_tag, auto kv_tag) __attribute__((always_inline)) {
      // ---- fp32 output (q, K/V cache rows, logits, fp32 residual stream of callers without planes). KVMAP: the K/V-cache
      // element map of the sequential steps (an integer division per store); the variant without it keeps the store loop
      // free of branches (ReLU as a max against 0 or -inf, the row scale always multiplied): ~10 instructions per store
      // instead of ~30 with five branches
      constexpr bool RES = decltype(res_tag)::value, KVMAP = decltype(kv_tag)::value;
      const float relu_lo = g.relu ? 0.f : -INFINITY;
      constexpr int LPR = SW / 4, RPI = 64 / LPR, NK = SH / RPI, KB = RES ? 4 : 8;   // lanes per staged row, rows per read instruction
      const int rrow = lane / LPR, rc4 = (lane % LPR) * 4;
      const int n0 = bn + wn * (BN / WN) + rc4;           // first of this lane's 4 consecutive output columns
      const bool ncol_ok = FULL || (n0 < g.N);            // N % 4 == 0 is guaranteed (N % 32 == 0)
      const int oi = ncol_ok ? n0 / g.split_n : 0, on = n0 - oi * g.split_n;
      // (selects, not g.out[oi]: a variable index into the by-value argument struct makes the compiler keep a private copy
      // of all of it in scratch)
      float* outp = (oi == 0 ? g.out[0] : oi == 1 ? g.out[1] : g.out[2]) + (size_t)blockIdx.y * g.part_stride;   // split-K: this block's partial result
      const int ldo = oi == 0 ? g.ldo[0] : oi == 1 ? g.ldo[1] : g.ldo[2];
      float4 res[RES ? NK : 1];
      if (RES) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const int m = min(mrow0 + k * RPI + rrow, Mlim - 1), nc = ncol_ok ? n0 : 0;   // clamped, unconditional (see planes_path)
          res[k] = *reinterpret_cast<const float4*>(g.resid + (size_t)m * g.ldr + nc);
        }
      }
#pragma unroll
      for (int kb = 0; kb < NK; kb += KB) {
        float4 st[KB];
        float scs[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow;
          st[k] = *reinterpret_cast<const float4*>(stg + rl * SW + rc4);
          scs[k] = rs_tile ? rs_tile[wm * (BM / WM) + strip * SH + rl] : 1.0f;   // fused RMSNorm row scale
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow, m = mrow0 + rl;
          float4 v = st[k];
          const float sc = acc_scale * scs[k];
          v.x = fmaxf(v.x * sc, relu_lo); v.y = fmaxf(v.y * sc, relu_lo); v.z = fmaxf(v.z * sc, relu_lo); v.w = fmaxf(v.w * sc, relu_lo);
          if (RES) { const float4 r = res[RES ? kb + k : 0]; v.x = r.x + v.x; v.y = r.y + v.y; v.z = r.z + v.z; v.w = r.w + v.w; }
          if (ncol_ok && (FULL || m < Mlim)) {
            const size_t off = KVMAP ? out_off(g, oi, m, ldo, on) : (size_t)m * ldo + on;
            *reinterpret_cast<float4*>(outp + off) = v;
          }
        }
      }
    };
    // ---- bf16 outputs (BOUT instantiations = the bf16 256x256 kernel of the training step; GemmH2Args::out_b / out_bt):
    // the staged rows leave as bf16 rows (8 columns = one 16-byte store per lane) and, after the final values have gone back
    // into the strip, as the transposed copy: a lane owns one column of a 32-row half of the strip (conflict-free 4-byte LDS
    // reads, bank = column), packs row pairs and stores 4 x 16 bytes; the two halves complete a column's 128-byte line.
    auto bf16_path = [&](auto mask_tag) __attribute__((always_inline)) {
      constexpr bool MASK = decltype(mask_tag)::value;
      constexpr int LPR = SW / 8, RPI = 64 / LPR, NK = SH / RPI, KB = MASK ? 2 : 4;
      const int rrow = lane / LPR, rc8 = (lane % LPR) * 8;
      const int n0 = bn + wn * (BN / WN) + rc8;
      const float relu_lo = g.relu ? 0.f : -INFINITY;
      __bf16* ob = reinterpret_cast<__bf16*>(g.out_b);
      float* of = g.out[0];
      float4 ma[MASK ? NK : 1], mb[MASK ? NK : 1];
      if (MASK) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {   // every mask piece of the strip requested before the first store (see planes_path)
          const float* mp = g.mask_src + (size_t)(mrow0 + k * RPI + rrow) * g.ldmask + n0;
          ma[k] = *reinterpret_cast<const float4*>(mp);
          mb[k] = *reinterpret_cast<const float4*>(mp + 4);
        }
      }
#pragma unroll
      for (int kb = 0; kb < NK; kb += KB) {
        float4 sa[KB], sb[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow;
          sa[k] = *reinterpret_cast<const float4*>(stg + rl * SW + rc8);
          sb[k] = *reinterpret_cast<const float4*>(stg + rl * SW + rc8 + 4);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const int rl = (kb + k) * RPI + rrow, m = mrow0 + rl;
          float v[8] = {sa[k].x, sa[k].y, sa[k].z, sa[k].w, sb[k].x, sb[k].y, sb[k].z, sb[k].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e] * acc_scale, relu_lo);
          if (MASK) {
            const float mk[8] = {ma[MASK ? kb + k : 0].x, ma[MASK ? kb + k : 0].y, ma[MASK ? kb + k : 0].z, ma[MASK ? kb + k : 0].w,
                                 mb[MASK ? kb + k : 0].x, mb[MASK ? kb + k : 0].y, mb[MASK ? kb + k : 0].z, mb[MASK ? kb + k : 0].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = mk[e] > 0.f ? v[e] : 0.f;
          }
          if (g.out_bt) {   // the final values back into the strip for the transposed pass
            *reinterpret_cast<float4*>(stg + rl * SW + rc8) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(stg + rl * SW + rc8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
          }
          if (ob) {
            __bf16 b[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) b[e] = (__bf16)v[e];
            *reinterpret_cast<uint4*>(ob + (size_t)m * g.ldob + n0) = *reinterpret_cast<uint4*>(b);
          }
          if (of) {
            *reinterpret_cast<float4*>(of + (size_t)m * g.ldo[0] + n0) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(of + (size_t)m * g.ldo[0] + n0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
          }
        }
      }
      if (g.out_bt) {
        __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0): the rewritten strip has landed
        __builtin_amdgcn_wave_barrier();
        __bf16* obt = reinterpret_cast<__bf16*>(g.out_bt);
        const int c = lane & 31, hrow = 32 * (lane >> 5);
#pragma unroll
        for (int cc = 0; cc < SW; cc += 32) {
          float col[32];
#pragma unroll
          for (int r = 0; r < 32; ++r) col[r] = stg[(hrow + r) * SW + cc + c];
          __bf16 b[32];
#pragma unroll
          for (int r = 0; r < 32; ++r) b[r] = (__bf16)col[r];
          __bf16* dst = obt + (size_t)(bn + wn * (BN / WN) + cc + c) * g.ldobt + mrow0 + hrow;
#pragma unroll
          for (int j = 0; j < 4; ++j) reinterpret_cast<uint4*>(dst)[j] = reinterpret_cast<const uint4*>(b)[j];
        }
      }
    };
    if (BOUT && (g.out_b || g.out_bt)) {
      if (g.mask_src) bf16_path(std::true_type{}); else bf16_path(std::false_type{});
    } else if (!M16 && g.out_h) {   // (M16: plane outputs never come here, h2_epilogue_256)
      if (g.resid_h) planes_path(std::true_type{}); else planes_path(std::false_type{});
    } else {
      if (g.rm_B) { if (g.resid) fp32_path(std::true_type{}, std::true_type{}); else fp32_path(std::false_type{}, std::true_type{}); }
      else if (g.resid) fp32_path(std::true_type{}, std::false_type{});      // (training GEMMs with an fp32 residual)
      else fp32_path(std::false_type{}, std::false_type{});
    }
    __builtin_amdgcn_wave_barrier();                  // stg is rewritten by the next strip
}

// ---- register epilogue of the 16x16x32 body (gemm_h2_pp_kernel<FULL, false, true>): rows from the accumulators -------------
// The 16 x 16 C/D map gives lane (c = lane & 15, gq = lane >> 4) rows 4 gq .. 4 gq + 3 of ONE column per tile — and which W
// row a tile's column c is, is decided where the W rows are DMA'd into LDS (PP_SRC_SETUP, gemm_h2_pp_body.inc), not by the
// product. The body loads them so that a lane's four W tiles j are neighbouring columns, and the per-element arithmetic below
// (planes_path's / fp32_path's of h2_epilogue_strip) runs on the accumulators where they are: no LDS write, read-back or wave
// barrier (the row scales still come from rs_tile), the same 32 16-byte stores per wave with the staged path's store pattern.
//   fp32 outputs:  column 4 c + j. acc[it][0..3][r] are four consecutive floats of row 16 it + 4 gq + r; the 16 lanes of a
//                  group write its 256 contiguous bytes, a store instruction four whole rows (as fp32_path: 16 lanes per row).
//   plane outputs: column 8 (c & 7) + 4 (c >> 3) + j. Lanes c and c ^ 8 hold the two halves of the 8-column piece c & 7 in
//                  every row; per row pair (2p, 2p + 1) they trade one half (DPP row_ror:8, no LDS): lane c < 8 ends with the
//                  8 columns of row 2p, lane c >= 8 with those of row 2p + 1 — one 16-byte store per plane, eight lanes per
//                  128-byte row, eight rows per instruction (as planes_path). The row sums are added over those eight lanes
//                  in planes_path's order (lane xor 4, 2, 1), with DPP.
// (Feeding the W fragment as the MFMA's FIRST operand instead — a lane then holds four consecutive columns of one row without
// any of this — was built and measured first: neighbouring lanes then hold different ROWS, every lane's 16 bytes is a memory
// request of its own, and the headline fell by 1.9 %; profiles/r17_direct_epilogue_ab.txt.)
// Residual pieces (RES) are requested with unconditional clamped loads one A tile at a time and three tiles ahead: the wait
// for a tile's pieces leaves the stores of the two tiles before it in flight (vmcnt counts loads and stores in issue order;
// rule (1) of the strip's comment). Three tiles are 48 registers beside the 128 accumulators; four spilled.
template <int CTRL>
__device__ __forceinline__ float h2_dpp(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
constexpr int DPP_ROR8 = 0x128, DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_XOR3 = 0x1B, DPP_HALF_MIRROR = 0x141;   // (half mirror = xor 7)

template <bool FULL, bool RES>
__device__ __forceinline__ void h2_direct16_planes(const GemmH2Args& g, f32x4 (&acc)[8][4], int lane, int bm, int bn, int wm, int wn,
                                                   const float* rs_tile, float acc_scale, int Mlim) {
  const int c = lane & 15, gq = lane >> 4;
  const bool hi = c >= 8;                              // this lane ends with the odd row of a pair
  const int lrow0 = wm * 128 + 4 * gq + (hi ? 1 : 0), mrow0 = bm + lrow0;   // row pair p of A tile it: + 16 it + 2 p
  const int n0 = bn + wn * 64 + 8 * (c & 7);
  const bool ncol_ok = FULL || (n0 < g.N);             // N % 32 == 0
  const float ps = g.plane_scale;
  float amax = 0.f;
  float scs[16];   // row scales: read with the residual pieces, a batch ahead of their use
  auto load = [&](auto it_c, uint4 (&q)[4]) __attribute__((always_inline)) {
    constexpr int it = decltype(it_c)::value;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      scs[2 * it + p] = rs_tile ? rs_tile[lrow0 + 16 * it + 2 * p] : 1.0f;
      if (RES) {
        const int m = min(mrow0 + 16 * it + 2 * p, Mlim - 1), nc = ncol_ok ? n0 : 0;   // clamped, unconditional (see planes_path)
        q[2 * p] = *reinterpret_cast<const uint4*>(g.resid_h + (size_t)m * g.ldrh + nc);
        q[2 * p + 1] = *reinterpret_cast<const uint4*>(g.resid_h + g.r_ps + (size_t)m * g.ldrh + nc);
      }
    }
  };
  auto tile = [&](auto it_c, const uint4 (&q)[4]) __attribute__((always_inline)) {
    constexpr int it = decltype(it_c)::value;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      // the half this lane does not keep goes to lane c ^ 8, whose other half comes back
      f32x4 v0, v1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float got = h2_dpp<DPP_ROR8>(hi ? acc[it][j][2 * p] : acc[it][j][2 * p + 1]);
        v0[j] = hi ? got : acc[it][j][2 * p];
        v1[j] = hi ? acc[it][j][2 * p + 1] : got;
      }
      const int m = mrow0 + 16 * it + 2 * p;
      const bool ok = ncol_ok && (FULL || m < Mlim);
      const float sc = rs_tile ? acc_scale * scs[2 * it + p] : acc_scale;
      f32x2 v[4] = {{v0[0], v0[1]}, {v0[2], v0[3]}, {v1[0], v1[1]}, {v1[2], v1[3]}};
      f16x2 h[4], l[4];
      f32x2 ss2 = {0.f, 0.f};
      float am = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f32x2 x = v[e] * sc;
        if (g.relu) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); }
        if (RES) {   // the residual from its planes: (hi + lo) / X_PLANE_SCALE, both steps exact in fp32
          x += (__builtin_convertvector(reinterpret_cast<const f16x2*>(&q[2 * p])[e], f32x2) +
                __builtin_convertvector(reinterpret_cast<const f16x2*>(&q[2 * p + 1])[e], f32x2)) * (1.0f / X_PLANE_SCALE);
        }
        ss2 += x * x;
        f32x2 xs = x * ps;
        am = fmaxf(am, fmaxf(fabsf(xs.x), fabsf(xs.y)));
        xs.x = __builtin_amdgcn_fmed3f(xs.x, -65504.f, 65504.f);
        xs.y = __builtin_amdgcn_fmed3f(xs.y, -65504.f, 65504.f);
        h[e] = __builtin_convertvector(xs, f16x2);
        l[e] = __builtin_convertvector(xs - __builtin_convertvector(h[e], f32x2), f16x2);
      }
      float ss = ss2.x + ss2.y;
      if (ok) {
        *reinterpret_cast<uint4*>(g.out_h + (size_t)m * g.ldoh + n0) = *reinterpret_cast<uint4*>(h);
        *reinterpret_cast<uint4*>(g.out_h + g.o_ps + (size_t)m * g.ldoh + n0) = *reinterpret_cast<uint4*>(l);
        amax = fmaxf(amax, am);
      }
      if (g.ssq_out) {   // the eight lanes c & 8 .. + 7 hold this wave's 64 columns of output row m
        if (!ok) ss = 0.f;
        ss += h2_dpp<DPP_XOR3>(h2_dpp<DPP_HALF_MIRROR>(ss));   // lane ^ 4
        ss += h2_dpp<DPP_XOR2>(ss);
        ss += h2_dpp<DPP_XOR1>(ss);
        if ((c & 7) == 0 && (FULL || m < Mlim)) atomicAdd(g.ssq_out + m, ssq_to_fix(ss, g.sat));
      }
    }
  };
  // (amax is pinned after every tile: the compiler otherwise sinks each tile's range check to the single use of amax
  // behind the last tile and keeps all 128 scaled values alive until then — they spilled)
#define H2_PIN_AMAX() asm volatile("" : "+v"(amax)); __builtin_amdgcn_sched_barrier(0)
  using std::integral_constant;
  uint4 qa[4], qb[4], qc[4];   // three A tiles of residual pieces in flight
#define H2_T(it, q) tile(integral_constant<int, it>{}, q); H2_PIN_AMAX()
#define H2_L(it, q) load(integral_constant<int, it>{}, q); __builtin_amdgcn_sched_barrier(0)
  H2_L(0, qa); H2_L(1, qb); H2_L(2, qc);
  H2_T(0, qa); H2_L(3, qa);
  H2_T(1, qb); H2_L(4, qb);
  H2_T(2, qc); H2_L(5, qc);
  H2_T(3, qa); H2_L(6, qa);
  H2_T(4, qb); H2_L(7, qb);
  H2_T(5, qc); H2_T(6, qa); H2_T(7, qb);
#undef H2_T
#undef H2_L
#undef H2_PIN_AMAX
  if (amax > 65504.f && g.sat) *g.sat = 1u;
}

// fp32 outputs without residual or K/V map (q / k / v of a fused-norm input): fp32_path's arithmetic and store pattern.
template <bool FULL>
__device__ __forceinline__ void h2_direct16_fp32(const GemmH2Args& g, f32x4 (&acc)[8][4], int lane, int bm, int bn, int wm, int wn,
                                                 const float* rs_tile, float acc_scale, int Mlim) {
  const int c = lane & 15, gq = lane >> 4;
  const int lrow0 = wm * 128 + 4 * gq, mrow0 = bm + lrow0;   // row r of A tile it: + 16 it + r
  const float relu_lo = g.relu ? 0.f : -INFINITY;
  const int n0 = bn + wn * 64 + 4 * c;                  // first of this lane's 4 consecutive output columns
  const bool ncol_ok = FULL || (n0 < g.N);
  const int oi = ncol_ok ? n0 / g.split_n : 0, on = n0 - oi * g.split_n;
  // (selects, not g.out[oi]: see fp32_path)
  float* outp = (oi == 0 ? g.out[0] : oi == 1 ? g.out[1] : g.out[2]) + (size_t)blockIdx.y * g.part_stride;
  const int ldo = oi == 0 ? g.ldo[0] : oi == 1 ? g.ldo[1] : g.ldo[2];
#pragma unroll
  for (int ib = 0; ib < 8; ib += 4) {
    f32x4 scs[4];   // fused RMSNorm row scales of four A tiles: the lane's four rows of a tile are one 16-byte read
#pragma unroll
    for (int k = 0; k < 4; ++k)
      scs[k] = rs_tile ? *reinterpret_cast<const f32x4*>(rs_tile + lrow0 + 16 * (ib + k)) : f32x4{1.f, 1.f, 1.f, 1.f};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mrow0 + 16 * (ib + k) + r;
        const float sc = acc_scale * scs[k][r];
        f32x4 v = {acc[ib + k][0][r], acc[ib + k][1][r], acc[ib + k][2][r], acc[ib + k][3][r]};
        v[0] = fmaxf(v[0] * sc, relu_lo); v[1] = fmaxf(v[1] * sc, relu_lo); v[2] = fmaxf(v[2] * sc, relu_lo); v[3] = fmaxf(v[3] * sc, relu_lo);
        if (ncol_ok && (FULL || m < Mlim)) *reinterpret_cast<f32x4*>(outp + (size_t)m * ldo + on) = v;
      }
  }
}

template <bool FULL, int TM, int TN, int WM, int WN, int BM, int BN, bool BOUT, bool M16>
__device__ __forceinline__ void h2_epilogue_256(const GemmH2Args& g, typename H2Acc<M16, TM, TN>::type& acc, __half* smem, int wave,
                                                int lane, int bm, int bn, int wm, int wn, const float* rs_tile,
                                                float acc_scale) {
  constexpr int SH = 64;
  // The MFMA C layout gives a lane one column and 16 scattered rows per tile, so a direct epilogue is
  // 128 dword stores (+128 dword residual loads) per lane in 16-load batches, each batch exposing a full
  // memory latency: ~12 us per tile without and ~30 us with the residual, against ~55 us of K-loop at
  // K = 768. Here each wave stages SH x 64 outputs at a time in its private strip of the (now idle)
  // operand LDS and streams them out row-wise with 16-byte accesses. The epilogue is bound by the NUMBER of
  // memory instructions and by its VALU work, not by bytes (measured: two extra 8-byte plane stores per float4
  // tripled it; ~20 VALU ops per plane element cost ~5 us per tile; a global load of the fused-RMSNorm row scales
  // cost a full memory latency per half), so the f16-plane outputs give a lane 8 consecutive columns = one 16-byte
  // store per plane, the row scales come from LDS (rs_tile, filled before the K-loop) and the saturation check is
  // one max per element plus one compare per half.
  // That layout is a property of which W row sits in which column of an MFMA tile, not of the product: the 16x16x32 body
  // (M16) has its W rows DMA'd into LDS in an order that puts a lane's four tiles side by side, and its outputs leave from
  // the accumulators with the same row-wise 16-byte accesses and no strips (h2_direct16_planes / h2_direct16_fp32 above).
  // The 32 x 32 map (a lane = one column, 16 rows per tile, two tiles per wave row) has no such order: two tiles give a lane
  // two columns, and it carries the bits of the search's steps and of training — it keeps the strips.
  __syncthreads();                                   // all waves are done reading operand tiles
  const int Mlim = g.m_dev ? min(*g.m_dev - g.m_base, g.M) : g.M;   // packed encoder: rows past the live count are never stored
  if constexpr (M16) {
    // The 16x16x32 body chooses its output-column map so that the outputs a tail pass writes leave from registers (above).
    // The K/V scatter and the fp32 residual (not used by a tail pass; rpr_op_linear_h2 can ask for them) take the strips
    // below, from the fp32 column map.
    if (g.out_h) {
      if (g.resid_h) h2_direct16_planes<FULL, true>(g, acc, lane, bm, bn, wm, wn, rs_tile, acc_scale, Mlim);
      else h2_direct16_planes<FULL, false>(g, acc, lane, bm, bn, wm, wn, rs_tile, acc_scale, Mlim);
      return;
    }
    if (!g.rm_B && !g.resid) {
      h2_direct16_fp32<FULL>(g, acc, lane, bm, bn, wm, wn, rs_tile, acc_scale, Mlim);
      return;
    }
  }
  constexpr int SW = TN * 32;                         // staged row width (floats)
  constexpr int NS = TM * 32 / SH;                    // strips per wave
  float* stg = reinterpret_cast<float*>(smem) + wave * (SH * SW);
  const int ncol = lane & 31, rsub = 4 * (lane >> 5);
  static_assert(NS == 1 || NS == 2, "one or two strips of 64 rows per wave");
  (void)ncol; (void)rsub;
  h2_epilogue_strip<FULL, TM, TN, WM, WN, 0, BM, BN, BOUT, M16>(g, acc, stg, lane, bm, bn, wm, wn, rs_tile, acc_scale, Mlim);
  if (NS == 2) h2_epilogue_strip<FULL, TM, TN, WM, WN, NS - 1, BM, BN, BOUT, M16>(g, acc, stg, lane, bm, bn, wm, wn, rs_tile, acc_scale, Mlim);
}

// ---- ping-pong 256x256 variant -------------------------------------------------------------------------
// 256x256x32 tiles, LDS-DMA feed into two 64-KB operand buffers, LDS-transposed epilogue. The 8 waves are two groups of
// four (wm = 0 / 1), one wave of each group per SIMD. A K-tile is two phases (one per 16-column k-chunk), each phase = a
// load segment (4 W + 8 A fragment ds_reads) and an MFMA segment (24 MFMAs), separated by raw s_barriers:
//       L_p | barrier | M_p | barrier | L_p+1 | ...
// Group 1 runs one barrier behind group 0, so on every SIMD one wave is in its MFMA segment while the other
// issues its loads: the LDS read latency (which an in-phase kernel pays with the MFMA pipe idle) is hidden behind the
// other group's MFMAs. The 8 LDS-DMA pieces of tile t+1 are issued in the MFMA shadows of M_0 of tile t, retired by
// `s_waitcnt vmcnt(0)` at the end of L_1 and first read in L_0 of tile t+1 (one phase after the wait, as the staggered
// groups need one barrier more); each L ends with lgkmcnt(0) BEFORE its barrier, so a buffer's last reads are retired
// before the other group starts overwriting it. (Rounds 1-3 ran four phases of 12 MFMAs: twice the barriers, 5076 instead
// of 4224 cycles per K-tile.)
// BF16 = true (training GEMMs, RPR_PREC_BF16): one bf16 plane per operand; the LDS rows of the lo planes hold the NEXT
// 32 columns of K instead, a K-tile is 64 deep and a phase issues 8 v_mfma_f32_32x32x16_bf16 (slice 0 x slice 0 and
// slice 1 x slice 1) on the same fragment reads — see gemm_h2_dma_kernel.
// Schedules that were measured and removed (DESIGN.md "tried and rejected"; the code is in the history): a phase skew
// between the persistent blocks, a per-round barrier between the blocks of an XCD, and the next tile's first K-tile
// prefetched under the epilogue — all of them slower or equal on the power-capped headline step. Also measured and not
// taken: the 32x32x16 body with the three products of an accumulator back to back (below, M16): registers only it ran 0.5 %
// SLOWER than the interleaved order in every round (tools/mfma_chain_probe.hip, profiles/r29_mfma_chain_summary.txt).
// The body is textually shared by two kernels (gemm_h2_pp_body.inc): gemm_h2_pp_kernel (one product, its arguments by value)
// and gemm_h2_pp_group_kernel (a table of products in device memory, blockIdx.y = product; see there).
// M16 = true (the launches of a search's tail passes, GemmH2Args::mfma16; f16x2 only): the same tiles, LDS layout, LDS-DMA feed and barrier
// schedule with the K-loop on v_mfma_f32_16x16x32_f16 — 48 MFMAs of 16 cycles per phase instead of 24 of 32, a phase per half
// of the wave's A rows instead of per k-chunk. A product's 32 columns of a K-tile are then summed inside one MFMA, so the
// results differ from the 32x32x16 body's in the last bits. Issue order: the 32x32x16 body walks its eight
// accumulators three times (all lo*hi, all hi*lo, all hi*hi: an accumulator's products are eight MFMAs apart); the M16 body
// gives each of a phase's sixteen accumulators its lo*hi, hi*lo, hi*hi BACK TO BACK (chained triples, A tile outer, W tile
// inner), so two of three C operands come from the previous MFMA's result instead of the register file: the same bits, less
// register-file traffic per MFMA, a higher clock under the power cap (+2.1 % on the headline step).
template <bool FULL, bool BF16 = false, bool M16 = false>
__global__ __launch_bounds__(512, 2) void gemm_h2_pp_kernel(GemmH2Args g, int tiles_m, int tiles_n) {
  static_assert(!(BF16 && M16), "the 16x16x32 body is the split-precision kernel's");
#include "gemm_h2_pp_body.inc"
}

// Grouped launch (bf16 training GEMMs): the weight-gradient products of one transformer layer, dW[N, K] = dY^T X for its six
// (encoder: four) linear layers, are 9 .. 36 output tiles each with a reduction over all rows of the batch. One launch per
// product cannot fill the chip without split-K (5-K-tile loops, fp32 partials, a reduce pass: 240 TF/s, and every
// 252-block launch takes the whole chip from the input-gradient chain on the main stream); here ONE launch walks all
// products of the layer, one block per tile (at most 384 tiles), each running the whole reduction of its tile in a single
// K-loop (t5-base decoder layer: 126 tiles x 128 K-tiles of 64 rows). A block reads (product, tile) from an assignment
// table and its product's argument struct from a table in device memory (scalar loads; a struct assembled in the kernel
// from by-value arrays stayed in scratch, 344 bytes per lane, because the epilogue indexes out[] / ldo[] at run time).
// Both tables are written by gemm_group_table_kernel from by-value arguments on the same stream, directly in front of the
// product launch: no host memory whose lifetime would have to outlast the enqueue.
// Assignment (launch_gemm_h2_group): workgroup i of a 1-D grid runs on XCD i % 8. Every product's tile grid is cut into
// super-tiles of up to 4 x 4 tiles, the tiles are listed super-tile by super-tile and every XCD takes an equal run of that
// list: the blocks of a super-tile run side by side on one XCD and share their A and W panels in its L2 (a 4 x 3 super-tile
// streams 7 panels for 12 tiles). With the products' tiles in
// plain row-major order over the XCDs the launch fetched 773 MB from the fabric for 276 MB of distinct operands
// (rocprofv3 FETCH_SIZE; 1.03 GB go through LDS).
template <bool FULL>
__global__ __launch_bounds__(512, 2) void gemm_h2_pp_group_kernel(const GemmH2Args* __restrict__ table, const int* __restrict__ assign) {
  constexpr bool BF16 = true, M16 = false;
  const int asg = assign[blockIdx.x];
  if (asg < 0) return;
  const GemmH2Args& g = table[asg >> 16];
  const int tiles_m = (g.M + 255) >> 8, tiles_n = (g.N + 255) >> 8;
#define PP_GROUP_TILE (asg & 0xffff)
#include "gemm_h2_pp_body.inc"
#undef PP_GROUP_TILE
}

struct GroupAssign { int n; int v[GemmGroupArgs::MAX_BLOCKS]; };
__global__ void gemm_group_table_kernel(GemmGroupArgs p, GroupAssign a, GemmH2Args* __restrict__ table, int* __restrict__ assign) {
  const int i = threadIdx.x;
  for (int k = i; k < a.n; k += blockDim.x) assign[k] = a.v[k];
  if (i >= p.n) return;
  GemmH2Args g{};
  g.A = p.A[i]; g.W = p.W[i]; g.lda = p.lda; g.ldw = p.ldw;
  g.out[0] = g.out[1] = g.out[2] = p.out[i];
  g.ldo[0] = g.ldo[1] = g.ldo[2] = p.ldo[i];
  g.M = p.M[i]; g.N = p.N[i]; g.K = p.K; g.split_n = p.N[i];
  g.acc_scale = 1.0f; g.plane_scale = 1.0f; g.bf16 = 1;
  table[i] = g;
}

// ---- pieces shared by the small-tile kernels (gemm_h2_skinny16_kernel, gemm_h2_wsplit_kernel, splitk_epilogue_kernel) ----
// Live rows of a launch: M, or for a compacted stage / tail job (m_dev) the device-side live count capped at M. -1: this
// kernel of a gated group does not run (the count is outside (live_lo, live_hi]), so every row tile exits.
__device__ __forceinline__ int live_rows(const GemmH2Args& g) {
  if (!g.m_dev) return g.M;
  const int md = *g.m_dev;
  if (g.live_hi > 0 && (md <= g.live_lo || md > g.live_hi)) return -1;
  return min(md, g.M);
}

// Epilogue operands of one output: the fused-RMSNorm sum of squares of its row and its residual (the planes as raw f16 bits).
struct EpiIn { unsigned long long ssq; float rf; unsigned int rh, rl; };

// mok / nok: row m / column n exists (what does not exist reads as 0). g by value, here and in epi_fetch: through a reference
// hipcc re-read ldr / ldrh / r_ps from the kernel arguments in every row's load block, one scalar-load wait each.
__device__ __forceinline__ EpiIn epi_load(const GemmH2Args g, int m, int n, bool mok, bool nok) {
  EpiIn e;
  e.ssq = (g.row_ssq && mok) ? g.row_ssq[m] : 0ull;
  e.rf = (g.resid && mok && nok) ? g.resid[(size_t)m * g.ldr + n] : 0.f;
  e.rh = (g.resid_h && mok && nok) ? (unsigned int)reinterpret_cast<const unsigned short*>(g.resid_h)[(size_t)m * g.ldrh + n] : 0u;
  e.rl = (g.resid_h && mok && nok) ? (unsigned int)reinterpret_cast<const unsigned short*>(g.resid_h)[g.r_ps + (size_t)m * g.ldrh + n] : 0u;
  return e;
}

// The operands of the R outputs of column n in rows row(0) .. row(R - 1). The tile kernels request them BEFORE the K walk
// so that the memory latency passes under it (a launch is a chain of latencies: ~1.5 us each for the row scales and for the
// residual planes when they were loaded after the reduction). One plain array per operand, the residual planes in one
// 32-bit register each: as __half pairs, as an array of EpiIn or as one struct of the four arrays, hipcc converted every
// operand on arrival, i.e. waited for each load before requesting the next (R serial latencies in front of the K walk).
template <int R, typename RowOf>
__device__ __forceinline__ void epi_fetch(const GemmH2Args g, unsigned long long (&ssq)[R], float (&rf)[R], unsigned int (&rh)[R],
                                          unsigned int (&rl)[R], int n, bool nok, int Mlive, RowOf row) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const EpiIn x = epi_load(g, row(r), n, row(r) < Mlive, nok);
    ssq[r] = x.ssq; rf[r] = x.rf; rh[r] = x.rh; rl[r] = x.rl;
  }
}

// The fused epilogue of output (m, n) = column on of out[oi] (outp = out[oi], ldo = ldo[oi]: read once by the caller, not
// per element): accumulator scale, fused-RMSNorm row scale, ReLU, fp32 residual, residual planes, then an f16-plane or fp32
// store (ok: the output exists). Returns the value stored — for planes the value they carry — for the caller's row sums.
__device__ __forceinline__ float epi_apply(const GemmH2Args& g, float acc, float acc_scale, const EpiIn& e, int m, int n, bool mok,
                                           bool ok, float* outp, int ldo, int oi, int on) {
  float v = acc * acc_scale;
  if (g.row_ssq && mok) v *= ssq_rsqrt(e.ssq, g.inv_d_fix, g.eps);
  if (g.relu) v = fmaxf(v, 0.f);
  if (g.resid && ok) v = e.rf + v;
  if (g.resid_h && ok) v = x_from_planes(__ushort_as_half((unsigned short)e.rh), __ushort_as_half((unsigned short)e.rl)) + v;
  if (ok) {
    if (g.out_h) {
      __half hi, lo;
      split_f16(v * g.plane_scale, hi, lo, g.sat);
      g.out_h[(size_t)m * g.ldoh + n] = hi;
      g.out_h[g.o_ps + (size_t)m * g.ldoh + n] = lo;
      v = (__half2float(hi) + __half2float(lo)) / g.plane_scale;
    } else {
      outp[out_off(g, oi, m, ldo, on)] = v;
    }
  }
  return v;
}

// ---- skinny variant for at most 32 rows (ONE query in flight: the beams of a step, its encoder tokens) ------------------
// The 32 x 32 wave-split tile (gemm_h2_wsplit_kernel<1, 1, 4>) gives a 768 x 768 weight 24 blocks, and a wave's ring holds
// three of its six K-tiles (8-KB stages: 32 activation + 32 weight rows, two planes): two memory round trips per launch,
// 11 us, 413 launches = 85 % of a single-query search. Here a block is a 16 x 16 output tile (v_mfma_f32_16x16x32_f16: a
// K-tile of 32 is ONE MFMA per product term): twice the blocks, 4-KB stages, six stages per wave = all of K = 768 in flight
// at once (K = 3072: a ring of six). blockIdx.y = 16-row tile (one for a step's 10 beams, two for an encoder of 17 .. 32
// tokens). Same K split over the four waves, same fixed-order reduction, same fused epilogue (epi_apply) as the 32-row tile.
template <bool FULL>
__global__ __launch_bounds__(256, 1) void gemm_h2_skinny16_kernel(GemmH2Args g, int tiles_n) {
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  constexpr int BT = 16, ST = 6, ROWS = 4 * BT, PIECES = ROWS / 16;   // 4 KB per stage: A hi, A lo, W hi, W lo x 16 rows
  __shared__ __attribute__((aligned(16))) __half smem[4 * ST * ROWS * HBK];   // 96 KB
  const int bn = blockIdx.x * BT, bm = blockIdx.y * BT;
  const int Mlive = live_rows(g);
  if (bm >= Mlive) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __half* wsm = smem + (size_t)wave * ST * ROWS * HBK;
  // epilogue operands of wave 0, requested before the K walk: lane = column bn + lane % 16, rows 4 (lane / 16) + r
  const int n = bn + (lane & 15), rsub = 4 * (lane >> 4);
  const bool nok = FULL || n < g.N;
  const auto row = [&](int r) { return bm + rsub + r; };
  unsigned long long e_ssq[4];
  float e_rf[4];
  unsigned int e_rh[4], e_rl[4];
  if (wave == 0) epi_fetch(g, e_ssq, e_rf, e_rh, e_rl, n, nok, Mlive, row);
  const __half* src[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int lrow = 16 * j + (lane >> 2);
    const int seg = (lane & 3) ^ ((lrow >> 2) & 3);
    const bool is_a = j < 2, second = (j & 1) != 0;
    const __half* base = is_a ? g.A : g.W;
    const size_t plane = second ? (is_a ? g.a_ps : g.w_ps) : 0;
    const int limit = is_a ? g.M : g.N;
    const size_t ld = is_a ? (size_t)g.lda : (size_t)g.ldw;
    int trow = (is_a ? bm : bn) + (lane >> 2);
    if (trow >= limit) trow = limit - 1;                 // activation rows past M: clamped, their outputs are never stored
    src[j] = base + plane + (size_t)trow * ld + seg * 8;
  }
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + k0),
                                       (__attribute__((address_space(3))) void*)(wsm + (size_t)buf * ROWS * HBK + 16 * j * HBK),
                                       16, 0, 0);
  };
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, kg = lane >> 4;
  const int so = (kg ^ ((frow >> 2) & 3)) * 8;           // the lane's 8 k values of its row: one swizzled 16-byte segment
  auto compute = [&](int buf) {
    const __half* base = wsm + (size_t)buf * ROWS * HBK + frow * HBK + so;
    const f16x8 ah = *reinterpret_cast<const f16x8*>(base);
    const f16x8 al = *reinterpret_cast<const f16x8*>(base + BT * HBK);
    const f16x8 bh = *reinterpret_cast<const f16x8*>(base + 2 * BT * HBK);
    const f16x8 bl = *reinterpret_cast<const f16x8*>(base + 3 * BT * HBK);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
  };
  const int nkt = g.K / HBK;
  const int mine = wave < nkt ? (nkt - wave + 3) / 4 : 0;         // K-tiles wave, wave + 4, ...
  constexpr int KEEP = PIECES * (ST - 2);                         // pieces of the younger tiles that may be pending
  constexpr int WAIT_KEEP = (KEEP & 15) | ((KEEP >> 4) << 14) | 0x0f70, WAIT_NONE = 0x0f70;
#pragma unroll
  for (int t = 0; t < ST - 1; ++t)
    if (t < mine) stage(t, (wave + 4 * t) * HBK);
  for (int i = 0; i < mine; ++i) {
    if (i + ST - 2 < mine) __builtin_amdgcn_s_waitcnt(WAIT_KEEP); else __builtin_amdgcn_s_waitcnt(WAIT_NONE);
    __builtin_amdgcn_sched_barrier(0);
    if (i + ST - 1 < mine) stage((i + ST - 1) % ST, (wave + 4 * (i + ST - 1)) * HBK);   // buffer of tile i-1: its reads are done
    compute(i % ST);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    acc[r] = ((red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane]) + red[(2 * 4 + r) * 64 + lane]) + red[(3 * 4 + r) * 64 + lane];
  const int oi = nok ? n / g.split_n : 0, on = n - oi * g.split_n;
  float* outp = g.out[oi];
  const int ldo = g.ldo[oi];
  float ssr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = row(r);
    const bool mok = m < Mlive, ok = nok && mok;
    const float v = epi_apply(g, acc[r], acc_scale, {e_ssq[r], e_rf[r], e_rh[r], e_rl[r]}, m, n, mok, ok, outp, ldo, oi, on);
    ssr[r] = ok ? v * v : 0.f;
  }
  if (g.ssq_out) {   // the 16 lanes of a row group hold this block's 16 columns of rows rsub .. rsub + 3
#pragma unroll
    for (int o = 8; o > 0; o >>= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r) ssr[r] += __shfl_xor(ssr[r], o, 64);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (bm + rsub + r < Mlive) atomicAdd(g.ssq_out + bm + rsub + r, ssq_to_fix(ssr[r], g.sat));
    }
  }
}

// ---- wave-split tiles for 33 to ~1500 rows (one to ~150 queries in flight) ---------------------------------------------------
// Such a launch is a weight stream: 2.4 MB of W for 10 live rows. The 128-row tile kernels give it N/64..N/32 blocks that
// each walk all of K through ONE LDS-DMA stream (~25 GB/s per CU): 18-29 us per launch, 2385 launches per search. Here a
// block is a (32 TM) x (32 TN) output tile whose four waves split K between them (wave w takes K-tiles w, w+4, ...), each
// with a private ST-stage LDS ring fed by its own LDS-DMA stream and no block barrier in the loop (a wave only reads what it
// loaded itself: s_waitcnt vmcnt is the whole synchronisation). The four partial accumulators are added in the fixed order
// 0..3 through LDS and the waves of quadrant (i, j) run the fused epilogue of their 32 x 32 part — deterministic, and the
// same arithmetic in the same order for every tile shape: bit-identical results.
// 32 x 32 tiles (TM = TN = 1, four 8-KB stages) serve up to 352 rows. Beyond that a launch is bound by what ONE CU can keep
// in flight between L2 and its LDS (ring bytes / memory latency ~ 60-85 GB/s per CU), and with 32 x 32 tiles every column
// tile re-streams its activation rows and every row tile the weights: a 280 x 3072 x 768 product moved 165 MB through
// LDS-DMA (24 us per launch, 121 launches = the tail pass of a single-query search), 640 rows went to 128 x 64 tiles with
// split-K over blocks plus a separate epilogue launch (17 + 6 us). 64 x 32 and 64 x 64 tiles move 1/2 .. 1/3 of the bytes
// with the same number of bytes in flight per CU: ST stages of 2 (BM + BN) rows x 64 B per wave = 144 KB (64 x 32, three
// stages) or 128 KB (64 x 64, two stages) per block.
// SPLIT (ksplit > 1): blockIdx.y = K range, raw partial sums to out[0] + y * part_stride, the caller runs
// splitk_epilogue*_kernel behind it. A compile-time flag: with the split decided at run time the 32 x 32 tile took ~3 % more
// time per decoder layer at 64 rows than the separate 32 x 32 kernel it replaced (tools/gemm_bench.py 64 160 320).
template <bool FULL, int TM, int TN, int ST, bool SPLIT>
__global__ __launch_bounds__(256, 1) void gemm_h2_wsplit_kernel(GemmH2Args g, int tiles_m, int tiles_n) {
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  constexpr int BM = 32 * TM, BN = 32 * TN, ROWS = 2 * (BM + BN), PIECES = ROWS / 16, NQ = TM * TN;
  static_assert(NQ <= 4, "one epilogue wave per 32 x 32 quadrant");
  static_assert((size_t)4 * NQ * 16 * 64 * sizeof(float) <= (size_t)4 * ST * ROWS * HBK * sizeof(__half), "the partial tiles fit the rings");
  __shared__ __attribute__((aligned(16))) __half smem[4 * ST * ROWS * HBK];
  const int tile = blockIdx.x, tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int bm = tm * BM, bn = tn * BN;
  const int Mlive = live_rows(g);
  if (bm >= Mlive) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  __half* wsm = smem + (size_t)wave * ST * ROWS * HBK;
  const int qi = wave / TN, qj = wave - qi * TN;            // the quadrant this wave finishes (waves >= NQ: none)
  // epilogue operands of the quadrant waves, requested before the K walk: lane = column n, rows rsub + (r & 3) + 8 (r >> 2)
  const int n = bn + 32 * qj + (lane & 31), rsub = bm + 32 * qi + 4 * (lane >> 5);
  const bool nok = FULL || n < g.N;
  const auto row = [&](int r) { return rsub + (r & 3) + 8 * (r >> 2); };
  unsigned long long e_ssq[16];
  float e_rf[16];
  unsigned int e_rh[16], e_rl[16];
  if (wave < NQ && !SPLIT) epi_fetch(g, e_ssq, e_rf, e_rh, e_rl, n, nok, Mlive, row);
  // K range of this block, then K-tiles wave, wave + 4, ... of it
  int nkt = g.K / HBK, kbeg = 0;
  if (SPLIT) {
    const int per = (nkt + g.ksplit - 1) / g.ksplit;
    kbeg = blockIdx.y * per;
    nkt = min(per, nkt - kbeg);
  }
  // LDS rows of a stage: [A hi: BM][A lo: BM][W hi: BN][W lo: BN]; piece j = rows 16 j .. 16 j + 15
  const __half* src[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) {
    const int lrow = 16 * j + (lane >> 2);
    const int seg = (lane & 3) ^ ((lrow >> 2) & 3);
    const __half* base;
    int trow, limit;
    size_t ld;
    if (lrow < BM) { base = g.A; trow = bm + lrow; limit = g.M; ld = g.lda; }
    else if (lrow < 2 * BM) { base = g.A + g.a_ps; trow = bm + lrow - BM; limit = g.M; ld = g.lda; }
    else if (lrow < 2 * BM + BN) { base = g.W; trow = bn + lrow - 2 * BM; limit = g.N; ld = g.ldw; }
    else { base = g.W + g.w_ps; trow = bn + lrow - 2 * BM - BN; limit = g.N; ld = g.ldw; }
    if (!FULL && trow >= limit) trow = limit - 1;
    src[j] = base + (size_t)trow * ld + seg * 8 + (size_t)kbeg * HBK;
  }
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + k0),
                                       (__attribute__((address_space(3))) void*)(wsm + (size_t)buf * ROWS * HBK + 16 * j * HBK),
                                       16, 0, 0);
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int frow = lane & 31, sw = (lane >> 2) & 3, hf = lane >> 5;
  auto compute = [&](int buf) {
    const __half* base = wsm + (size_t)buf * ROWS * HBK;
#pragma unroll
    for (int c = 0; c < HBK / 16; ++c) {
      const int so = ((2 * c + hf) ^ sw) * 8;
      f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[i] = *reinterpret_cast<const f16x8*>(base + (32 * i + frow) * HBK + so);
        al[i] = *reinterpret_cast<const f16x8*>(base + (BM + 32 * i + frow) * HBK + so);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[j] = *reinterpret_cast<const f16x8*>(base + (2 * BM + 32 * j + frow) * HBK + so);
        bl[j] = *reinterpret_cast<const f16x8*>(base + (2 * BM + BN + 32 * j + frow) * HBK + so);
      }
      // per accumulator the same order of the three terms for every tile shape (lo x hi, hi x lo, hi x hi)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
  };
  const int mine = wave < nkt ? (nkt - wave + 3) / 4 : 0;
  constexpr int KEEP = PIECES * (ST - 2);                         // pieces of the younger tiles that may be pending
  static_assert(KEEP <= 63, "vmcnt is a 6-bit counter");
  constexpr int WAIT_KEEP = (KEEP & 15) | ((KEEP >> 4) << 14) | 0x0f70, WAIT_NONE = 0x0f70;
#pragma unroll
  for (int t = 0; t < ST - 1; ++t)
    if (t < mine) stage(t, (wave + 4 * t) * HBK);
  for (int i = 0; i < mine; ++i) {
    if (i + ST - 2 < mine) __builtin_amdgcn_s_waitcnt(WAIT_KEEP); else __builtin_amdgcn_s_waitcnt(WAIT_NONE);
    __builtin_amdgcn_sched_barrier(0);
    if (i + ST - 1 < mine) stage((i + ST - 1) % ST, (wave + 4 * (i + ST - 1)) * HBK);   // buffer of tile i-1: its reads are done
    compute(i % ST);
    __builtin_amdgcn_sched_barrier(0);
  }
  // the four waves' partial tiles through LDS (the rings are idle now): quadrant-major, added in the fixed order 0..3
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(((i * TN + j) * 4 + wave) * 16 + r) * 64 + lane] = acc[i][j][r];
  __syncthreads();
  if (wave >= NQ) return;
  f32x16 sum;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* q = red + ((size_t)(wave * 4) * 16 + r) * 64 + lane;
    sum[r] = ((q[0] + q[16 * 64]) + q[2 * 16 * 64]) + q[3 * 16 * 64];
  }
  if (SPLIT) {   // raw partial sums
    float* outp = g.out[0] + (size_t)blockIdx.y * g.part_stride;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = row(r);
      if (nok && m < Mlive) outp[(size_t)m * g.ldo[0] + n] = sum[r];
    }
    return;
  }
  const int oi = nok ? n / g.split_n : 0, on = n - oi * g.split_n;
  float* outp = g.out[oi];
  const int ldo = g.ldo[oi];
  float ssr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = row(r);
    const bool mok = m < Mlive, ok = nok && mok;
    const float v = epi_apply(g, sum[r], acc_scale, {e_ssq[r], e_rf[r], e_rh[r], e_rl[r]}, m, n, mok, ok, outp, ldo, oi, on);
    ssr[r] = ok ? v * v : 0.f;
  }
  if (g.ssq_out) {   // wave-uniform branch. The 16 butterflies are independent: issued level by level they overlap
                     // (one chain after the other cost ~4 us per launch — 12 % of a single-query search)
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
      for (int r = 0; r < 16; ++r) ssr[r] += __shfl_xor(ssr[r], o, 64);
    if ((lane & 31) == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = row(r);
        if (m < Mlive) atomicAdd(g.ssq_out + m, ssq_to_fix(ssr[r], g.sat));
      }
    }
  }
}

// The launchers pick the instantiation that a step of the plan (gemm_route.h) names and launch it on the step's grid.
template <int TM, int TN, int ST>
static void launch_wsplit_cfg(const GemmStep& p, const GemmH2Args& k, hipStream_t s) {
  const dim3 grid(p.grid_x, p.grid_y);
  const bool split = p.ksplit > 1;
  if (split && p.full) hipLaunchKernelGGL((gemm_h2_wsplit_kernel<true, TM, TN, ST, true>), grid, dim3(256), 0, s, k, p.tiles_m, p.tiles_n);
  else if (split) hipLaunchKernelGGL((gemm_h2_wsplit_kernel<false, TM, TN, ST, true>), grid, dim3(256), 0, s, k, p.tiles_m, p.tiles_n);
  else if (p.full) hipLaunchKernelGGL((gemm_h2_wsplit_kernel<true, TM, TN, ST, false>), grid, dim3(256), 0, s, k, p.tiles_m, p.tiles_n);
  else hipLaunchKernelGGL((gemm_h2_wsplit_kernel<false, TM, TN, ST, false>), grid, dim3(256), 0, s, k, p.tiles_m, p.tiles_n);
}

template <int BN, bool BF16 = false>
static void launch_cfg(const GemmStep& p, const GemmH2Args& a, hipStream_t s) {
  const dim3 grid(p.grid_x, p.grid_y), blk(256);
  if (p.stages == 4 && p.full) hipLaunchKernelGGL((gemm_h2_dma_kernel<128, BN, 2, 2, true, 4, BF16>), grid, blk, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.stages == 4) hipLaunchKernelGGL((gemm_h2_dma_kernel<128, BN, 2, 2, false, 4, BF16>), grid, blk, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.full) hipLaunchKernelGGL((gemm_h2_dma_kernel<128, BN, 2, 2, true, 2, BF16>), grid, blk, 0, s, a, p.tiles_m, p.tiles_n);
  else hipLaunchKernelGGL((gemm_h2_dma_kernel<128, BN, 2, 2, false, 2, BF16>), grid, blk, 0, s, a, p.tiles_m, p.tiles_n);
}

static void launch_256(const GemmStep& p, const GemmH2Args& a, hipStream_t s) {
  const dim3 gr(p.grid_x, p.grid_y), bl(512);
  if (p.bf16 && p.full) hipLaunchKernelGGL((gemm_h2_pp_kernel<true, true>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.bf16) hipLaunchKernelGGL((gemm_h2_pp_kernel<false, true>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.m16 && p.full) hipLaunchKernelGGL((gemm_h2_pp_kernel<true, false, true>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.m16) hipLaunchKernelGGL((gemm_h2_pp_kernel<false, false, true>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
  else if (p.full) hipLaunchKernelGGL((gemm_h2_pp_kernel<true>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
  else hipLaunchKernelGGL((gemm_h2_pp_kernel<false>), gr, bl, 0, s, a, p.tiles_m, p.tiles_n);
}

hipError_t launch_gemm_h2_group(const GemmGroupArgs& p, void* scratch, hipStream_t s) {
  if (p.n <= 0) return hipSuccess;
  if (!scratch || p.n > GemmGroupArgs::MAXP || p.K <= 0 || (p.K & 63) || (p.lda & 7) || (p.ldw & 7)) return hipErrorInvalidValue;
  bool full = true;
  int total = 0;
  for (int i = 0; i < p.n; ++i) {
    if (!p.A[i] || !p.W[i] || !p.out[i] || p.M[i] <= 0 || p.N[i] <= 0 || (p.ldo[i] & 3) || (p.N[i] & 3)) return hipErrorInvalidValue;
    total += ((p.M[i] + 255) / 256) * ((p.N[i] + 255) / 256);
    full = full && (p.M[i] % 256 == 0) && (p.N[i] % 256 == 0);
  }
  if (total > GemmGroupArgs::MAX_TILES || total >= 65536) return hipErrorInvalidValue;
  const std::vector<int> order = group_tile_order(p.M, p.N, p.n);
  GroupAssign asg;
  asg.n = (int)order.size();
  if (asg.n > GemmGroupArgs::MAX_BLOCKS) return hipErrorInvalidValue;
  std::copy(order.begin(), order.end(), asg.v);
  GemmH2Args* table = reinterpret_cast<GemmH2Args*>(scratch);
  int* assign = reinterpret_cast<int*>(static_cast<char*>(scratch) + GemmGroupArgs::TABLE_BYTES);
  hipLaunchKernelGGL(gemm_group_table_kernel, dim3(1), dim3(256), 0, s, p, asg, table, assign);
  const dim3 gr(asg.n), bl(512);
  if (full) hipLaunchKernelGGL((gemm_h2_pp_group_kernel<true>), gr, bl, 0, s, table, assign);
  else hipLaunchKernelGGL((gemm_h2_pp_group_kernel<false>), gr, bl, 0, s, table, assign);
  return hipGetLastError();
}

// out[m][n] = (resid ? resid[m][n] : 0) + sum over the splits, in split order (bitwise reproducible); N % 4 == 0
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int ks, size_t stride, int M, int N,
                                                             float* __restrict__ out, int ldo, const float* __restrict__ resid, int ldr) {
  const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = N >> 2;
  if (i4 >= (size_t)M * n4) return;
  const int m = (int)(i4 / n4), n = (int)(i4 - (size_t)m * n4) * 4;
  float4 a = resid ? *reinterpret_cast<const float4*>(resid + (size_t)m * ldr + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < ks; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(part + (size_t)k * stride + (size_t)m * N + n);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  *reinterpret_cast<float4*>(out + (size_t)m * ldo + n) = a;
}

// Fused epilogue of a split-K launch whose consumer needs more than a sum (search path, a few hundred to a few thousand
// rows in flight): out = epilogue(sum over the splits, in split order). One thread per output element, a wave covers 64
// consecutive columns of one row (N % 64 == 0). The small-tile kernels' per-element epilogue (epi_apply: accumulator
// scale, fused-RMSNorm row scale, ReLU, residual (fp32 or planes), f16-plane or fp32 output, K/V-cache layout included),
// then fixed-point row sums of squares.
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(GemmH2Args g, const float* __restrict__ part, int ks, size_t stride) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)g.M * g.N) return;                  // N % 64 == 0: a wave is inside or outside as a whole
  const int m = (int)(idx / g.N), n = (int)(idx - (size_t)m * g.N);
  float acc = 0.f;
  for (int k = 0; k < ks; ++k) acc += part[(size_t)k * stride + idx];
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  const int oi = n / g.split_n, on = n - oi * g.split_n;
  const float v = epi_apply(g, acc, acc_scale, epi_load(g, m, n, true, true), m, n, true, true, g.out[oi], g.ldo[oi], oi, on);
  if (g.ssq_out) {   // grid-uniform branch: all 64 lanes of the wave hold columns of row m
    float ss = v * v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(g.ssq_out + m, ssq_to_fix(ss, g.sat));
  }
}

// The same epilogue with FOUR consecutive columns per thread (N % 256 == 0: a wave is 256 consecutive columns of one row):
// 16-byte loads of the partials, 8-byte plane stores / 16-byte fp32 stores instead of one element per thread (2-byte plane
// stores). Per element the same arithmetic in the same order; the row sums of squares add four columns before the wave's
// butterfly.
__global__ __launch_bounds__(256) void splitk_epilogue4_kernel(GemmH2Args g, const float* __restrict__ part, int ks, size_t stride) {
  const size_t idx4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = g.N >> 2;
  if (idx4 >= (size_t)g.M * n4) return;                  // N % 256 == 0: a wave is inside or outside as a whole
  const int m = (int)(idx4 / n4), n = (int)(idx4 - (size_t)m * n4) * 4;
  const size_t idx = (size_t)m * g.N + n;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < ks; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(part + (size_t)k * stride + idx);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  const float rsc = g.row_ssq ? ssq_rsqrt(g.row_ssq[m], g.inv_d_fix, g.eps) : 1.0f;
  float v[4] = {a.x * acc_scale, a.y * acc_scale, a.z * acc_scale, a.w * acc_scale};
  float r[4] = {0.f, 0.f, 0.f, 0.f};
  if (g.resid) { const float4 q = *reinterpret_cast<const float4*>(g.resid + (size_t)m * g.ldr + n); r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w; }
  if (g.resid_h) {
    const uint2 hh = *reinterpret_cast<const uint2*>(g.resid_h + (size_t)m * g.ldrh + n);
    const uint2 ll = *reinterpret_cast<const uint2*>(g.resid_h + g.r_ps + (size_t)m * g.ldrh + n);
    const __half* h = reinterpret_cast<const __half*>(&hh); const __half* l = reinterpret_cast<const __half*>(&ll);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = x_from_planes(h[e], l[e]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (g.row_ssq) v[e] *= rsc;
    if (g.relu) v[e] = fmaxf(v[e], 0.f);
    if (g.resid || g.resid_h) v[e] = r[e] + v[e];
  }
  if (g.out_h) {
    __half hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      split_f16(v[e] * g.plane_scale, hi[e], lo[e], g.sat);
      v[e] = (__half2float(hi[e]) + __half2float(lo[e])) / g.plane_scale;   // the value the planes carry (row sums below)
    }
    *reinterpret_cast<uint2*>(g.out_h + (size_t)m * g.ldoh + n) = *reinterpret_cast<uint2*>(hi);
    *reinterpret_cast<uint2*>(g.out_h + g.o_ps + (size_t)m * g.ldoh + n) = *reinterpret_cast<uint2*>(lo);
  } else {
    const int oi = n / g.split_n, on = n - oi * g.split_n;
    *reinterpret_cast<float4*>(g.out[oi] + out_off(g, oi, m, g.ldo[oi], on)) = make_float4(v[0], v[1], v[2], v[3]);
  }
  if (g.ssq_out) {   // grid-uniform branch: all 64 lanes of the wave hold columns of row m
    float ss = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(g.ssq_out + m, ssq_to_fix(ss, g.sat));
  }
}

// The route thresholds; in a development build with the switches of the environment (read once).
static const GemmTuning& gemm_tuning() {
  static const GemmTuning tuning = [] {
    GemmTuning t;
    const auto sw = [](const char* e, int& v) { if (e) v = atoi(e); };
    sw(dev_getenv("RPR_GEMM_TILE"), t.force_tile);
    sw(dev_getenv("RPR_GEMM_ROWSPLIT"), t.row_split);
    sw(dev_getenv("RPR_GEMM_ROWSPLIT_LOG"), t.row_split_log);
    sw(dev_getenv("RPR_GEMM_WSPLIT_MAX"), t.wsplit_max);
    sw(dev_getenv("RPR_WSPLIT_CFG"), t.wsplit_cfg);
    sw(dev_getenv("RPR_WSPLIT_KS"), t.wsplit_ks);
    sw(dev_getenv("RPR_PP_SUPERTILE"), t.supertile);
    return t;
  }();
  return tuning;
}

static GemmRouteIn route_inputs(const GemmH2Args& a) {
  GemmRouteIn r;
  r.M = a.M; r.N = a.N; r.K = a.K; r.cus = a.cus;
  r.split_n = a.split_n; r.rm_B = a.rm_B; r.ksplit = a.ksplit; r.small_live = a.small_live; r.live_lo = a.live_lo; r.live_hi = a.live_hi;
  r.part_cap = a.part_cap;
  r.part = a.part; r.mid_split = a.mid_split; r.m_dev = a.m_dev; r.bf16 = a.bf16; r.no_row_split = a.no_row_split;
  r.force_pp = a.force_pp; r.mfma16 = a.mfma16;
  r.out_h = a.out_h; r.row_ssq = a.row_ssq; r.ssq_out = a.ssq_out; r.resid = a.resid; r.resid_h = a.resid_h; r.relu = a.relu;
  r.out_b = a.out_b; r.out_bt = a.out_bt;
  r.ab_al8 = !(a.lda & 7) && !(a.ldw & 7);
  r.ldo0_al4 = !(a.ldo[0] & 3);
  r.ldr_al4 = !a.resid || !(a.ldr & 3);
  r.epi_al4 = !(a.ldo[0] & 3) && !(a.ldo[1] & 3) && !(a.ldo[2] & 3) && r.ldr_al4 && (!a.resid_h || !(a.ldrh & 3)) && (!a.out_h || !(a.ldoh & 3));
  r.outb_al = !(a.out_b && (a.ldob & 7)) && !(a.out_bt && ((a.ldobt & 7) || a.ldobt < a.M)) && !(a.mask_src && (a.ldmask & 3));
  return r;
}

// (The order in which the instantiations are first named here is their order in the code object.)
static hipError_t launch_step(const GemmStep& p, const GemmH2Args& a, hipStream_t s) {
  if (p.family == GEMM_SKINNY16) {
    const dim3 grid(p.grid_x, p.grid_y);
    if (p.full) hipLaunchKernelGGL((gemm_h2_skinny16_kernel<true>), grid, dim3(256), 0, s, a, p.tiles_n);
    else hipLaunchKernelGGL((gemm_h2_skinny16_kernel<false>), grid, dim3(256), 0, s, a, p.tiles_n);
  }
  else if (p.family == GEMM_PP) launch_256(p, a, s);
  else if (p.family == GEMM_WSPLIT && p.bm == 32) launch_wsplit_cfg<1, 1, 4>(p, a, s);
  else if (p.family == GEMM_DMA && p.bn == 64 && !p.bf16) launch_cfg<64>(p, a, s);
  else if (p.family == GEMM_DMA && p.bn == 64) launch_cfg<64, true>(p, a, s);
  else if (p.family == GEMM_DMA && p.bf16) launch_cfg<128, true>(p, a, s);
  else if (p.family == GEMM_DMA) launch_cfg<128>(p, a, s);
  else if (p.bn == 32) launch_wsplit_cfg<2, 1, 3>(p, a, s);
  else launch_wsplit_cfg<2, 2, 2>(p, a, s);
  return hipGetLastError();
}

// Split-K over blockIdx.y: the tile launch writes the fp32 partial sums of the ks K ranges to the caller's scratch a.part, then
// one launch combines them in split order (bitwise reproducible). REDUCE_SUM: splitk_reduce_kernel adds them to the fp32
// residual (a plain sum into out[0]); REDUCE_FUSED{,4}: splitk_epilogue{,4}_kernel applies a's whole epilogue to the sum, so
// the tile launch runs with every epilogue field cleared.
static GemmH2Args splitk_tile_args(const GemmH2Args& a, const GemmStep& st) {
  GemmH2Args p = a;
  p.ksplit = st.ksplit; p.part_stride = (size_t)a.M * a.N;
  p.out[0] = p.out[1] = p.out[2] = a.part; p.ldo[0] = p.ldo[1] = p.ldo[2] = a.N; p.split_n = a.N; p.resid = nullptr;
  if (st.reduce != REDUCE_SUM) {
    p.out_h = nullptr; p.resid_h = nullptr; p.relu = 0; p.row_ssq = nullptr; p.ssq_out = nullptr;
    p.rm_B = 0; p.acc_scale = 1.0f; p.dyn_a = p.dyn_b = nullptr;
  }
  return p;
}

static hipError_t launch_splitk_reduce(const GemmH2Args& a, const GemmStep& st, hipStream_t s) {
  const size_t n = (size_t)a.M * a.N, n4 = (size_t)a.M * (a.N >> 2);
  if (st.reduce == REDUCE_SUM)
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.part, st.ksplit, n, a.M, a.N,
                       a.out[0], a.ldo[0], a.resid, a.ldr);
  else if (st.reduce == REDUCE_FUSED4)
    hipLaunchKernelGGL(splitk_epilogue4_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, a, a.part, st.ksplit, n);
  else
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, a.part, st.ksplit, n);
  return hipGetLastError();
}

bool gemm_h2_pp_only(const GemmH2Args& a) { return plan_is_pp_only(plan_gemm_h2(route_inputs(a), gemm_tuning())); }

hipError_t launch_gemm_h2(GemmH2Args& a_in, hipStream_t s) {
  GemmH2Args a = a_in;
  if (a.acc_scale == 0.f) a.acc_scale = 1.f;      // zero-initialised args mean "no scaling"
  if (a.plane_scale == 0.f) a.plane_scale = 1.f;
  const GemmTuning& tune = gemm_tuning();
  const GemmPlan plan = plan_gemm_h2(route_inputs(a), tune);
  a_in.kernel_cls = plan.cls;
  if (plan.invalid) return hipErrorInvalidValue;
  for (int i = 0; i < plan.n; ++i) {
    const GemmStep& st = plan.step[i];
    GemmH2Args p = a;   // this step's rows of the product, its live window and tile order
    p.M = st.rows; p.live_lo = st.live_lo; p.live_hi = st.live_hi; p.tile_cw = st.tile_cw; p.tile_rb = st.tile_rb;
    if (st.m_base > 0) {   // the rows behind a row split
      const int r0 = st.m_base;
      if (tune.row_split_log) fprintf(stderr, "[rowsplit] M=%d N=%d K=%d: %d rows on 256x256 tiles, %d on 128x128\n", a.M, a.N, a.K, r0, st.rows);
      p.m_base = a.m_base + r0;
      p.A = a.A + (size_t)r0 * a.lda;
      for (int o = 0; o < 3; ++o) if (a.out[o]) p.out[o] = a.out[o] + (size_t)r0 * a.ldo[o];
      if (a.out_h) p.out_h = a.out_h + (size_t)r0 * a.ldoh;
      if (a.resid) p.resid = a.resid + (size_t)r0 * a.ldr;
      if (a.resid_h) p.resid_h = a.resid_h + (size_t)r0 * a.ldrh;
      if (a.row_ssq) p.row_ssq = a.row_ssq + r0;
      if (a.ssq_out) p.ssq_out = a.ssq_out + r0;
    }
    hipError_t e = launch_step(st, st.reduce == REDUCE_NONE ? p : splitk_tile_args(p, st), s);
    if (e == hipSuccess && st.reduce != REDUCE_NONE) e = launch_splitk_reduce(p, st, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// fp32 [rows, cols] -> two f16 planes [2][rows][cols] (weights at load time, generic activations)
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, __half* __restrict__ out,
                                                            size_t n, size_t plane_stride, float scale,
                                                            const float* __restrict__ colscale, int cols,
                                                            unsigned int* sat) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float4 v = *reinterpret_cast<const float4*>(x + i);
  if (colscale) {   // cols % 4 == 0: the four elements stay inside one row
    const float4 c = *reinterpret_cast<const float4*>(colscale + (i % (size_t)cols));
    v.x *= c.x; v.y *= c.y; v.z *= c.z; v.w *= c.w;
  }
  __half h[4], l[4];
  split_f16(v.x * scale, h[0], l[0], sat); split_f16(v.y * scale, h[1], l[1], sat);
  split_f16(v.z * scale, h[2], l[2], sat); split_f16(v.w * scale, h[3], l[3], sat);
  *reinterpret_cast<uint2*>(out + i) = *reinterpret_cast<uint2*>(h);
  *reinterpret_cast<uint2*>(out + plane_stride + i) = *reinterpret_cast<uint2*>(l);
}

hipError_t launch_split_planes(const float* x, __half* out, size_t n, size_t plane_stride, hipStream_t s, float scale,
                               const float* colscale, int cols, unsigned int* sat) {
  if (n == 0) return hipSuccess;
  if ((n & 3) || (colscale && (cols <= 0 || (cols & 3)))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, x, out, n, plane_stride,
                     scale, colscale, cols, sat);
  return hipGetLastError();
}

}  // namespace rpr
