// Body of the 256x256 ping-pong GEMM kernels (see gemm_h2.hip): textually included by gemm_h2_pp_kernel (one product, its
// arguments `g` by value) and gemm_h2_pp_group_kernel (`g` = an entry of a table in device memory), so that the single-product
// kernel of the search path compiles exactly as it did as a self-contained kernel (a shared device function taking the
// arguments by reference changed its register allocation). Expects: FULL, BF16, M16 (template parameters; the grouped kernel
// sets BF16 = true, M16 = false), g, tiles_m, tiles_n. M16: the K-loop of a search's tail passes on v_mfma_f32_16x16x32_f16 (below).
  // per-tensor dynamic plane scales (training): read from the device; g itself must stay untouched — a kernel that writes
  // to its by-value argument struct gets a private copy of all 320 bytes in scratch (measured: +20 % per launch)
  const float acc_scale = g.dyn_a ? 1.0f / (dyn_plane_scale(*g.dyn_a) * dyn_plane_scale(*g.dyn_b)) : g.acc_scale;
  constexpr int BM = 256, BN = 256, WM = 2, WN = 4, NW = 8, TM = 4, TN = 2;
  constexpr int ROWS = 2 * (BM + BN), PER_WAVE = ROWS / 16 / NW;   // 8 DMA pieces per wave and K-tile
  __shared__ __attribute__((aligned(16))) __half smem[2 * ROWS * HBK];
  __shared__ float rs_tile[BM];                      // fused RMSNorm: rsqrt(mean(x^2) + eps) of the tile's rows

  // PERSISTENT: the grid is (at most) one block per CU and a block walks the tiles of its XCD's chunk — the stores of a
  // tile's epilogue drain under the first K-tiles of the block's next tile instead of holding the CU until the block
  // retires.
  int nt = tiles_m * tiles_n;
  if (g.m_dev) {                                             // packed rows: only the tiles holding live rows
    if (g.live_hi > 0 && (*g.m_dev <= g.live_lo || *g.m_dev > g.live_hi)) return;   // the other kernel of the pair runs
    nt = ((min(*g.m_dev, g.M) + BM - 1) / BM) * tiles_n;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
#ifdef PP_GROUP_TILE
  // grouped launch: one tile per block, chosen by the caller's assignment table (whole super-tiles of a product per XCD)
  const int xk = 0, xstep = 1, chunk0 = (PP_GROUP_TILE), chunk_n = 1;
#else
  // tile order: XCD x = block & 7 owns a contiguous chunk of the live tiles; its blocks walk the chunk side by side
  // (blocks of XCD x: those with index = x mod 8, (gridDim.x - x + 7) / 8 of them — with one block per tile that is the
  // chunk size and every block handles exactly one tile)
  const int xq = nt >> 3, xr = nt & 7, xcd = blockIdx.x & 7, xk = blockIdx.x >> 3, xstep = ((int)gridDim.x - xcd + 7) >> 3;
  const int chunk0 = xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq, chunk_n = xcd < xr ? xq + 1 : xq;
#endif
  int round = 0;
  for (int ti = xk; ti < chunk_n; ti += xstep, ++round) {
  const int bid = chunk0 + ti;
  int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  if (g.tile_cw > 0) {
    // super-tile order (GemmH2Args::tile_cw): wide products in row-major order put 1-2 row panels and every column tile of
    // W under the blocks of an XCD at a time — the W panels, used by one or two blocks each, come back over the fabric every round
    const int band_sz = g.tile_rb * tiles_n, band = bid / band_sz, rem = bid - band * band_sz;
    const int rb = min(g.tile_rb, nt / tiles_n - band * g.tile_rb);       // row panels of this band (the last one is shorter)
    const int gsz = rb * g.tile_cw, gi = rem / gsz, r2 = rem - gi * gsz;
    const int c0 = gi * g.tile_cw, cwg = min(g.tile_cw, tiles_n - c0);     // (the last column group is narrower)
    const int pr = r2 / cwg;
    tm = band * g.tile_rb + pr; tn = c0 + (r2 - pr * cwg);
  }
  const int bm = tm * BM, bn = tn * BN;
  if (g.row_ssq && tid < BM) {   // one dependent load + rsqrt per row, hidden behind the first K-tile's DMA; the epilogue
    const int m = bm + tid;      // (after the K-loop's barriers) reads the scales from LDS instead of global memory
    rs_tile[tid] = (m < g.M) ? ssq_rsqrt(g.row_ssq[m], g.inv_d_fix, g.eps) : 1.f;
  }

  // split-K (weight gradients of the training step: few output tiles, K = thousands of rows): blockIdx.y walks its own
  // range of K-tiles and stores a partial result at out + blockIdx.y * part_stride (splitk_reduce_kernel adds them in order)
  constexpr int KSTEP = BF16 ? 2 * HBK : HBK;
  int nkt = g.K / KSTEP, kbeg = 0;
  if (g.ksplit > 1) {
    const int per = (nkt + g.ksplit - 1) / g.ksplit;
    kbeg = blockIdx.y * per;
    nkt = min(per, nkt - kbeg);
  }
  // (the lane index is laundered per tile: otherwise the compiler hoists the eight per-piece row / segment terms out of
  // the tile loop and the 256-register kernel spills)
  int lane_t = lane;
  asm volatile("" : "+v"(lane_t));
  const __half* src[PER_WAVE];
// (operand, plane, limit and leading dimension are chosen from the wave-uniform 16-row group with value selects: an if / else
// chain over the struct's fields made the compiler select field ADDRESSES and keep a private copy of the argument struct
// in scratch)
#define PP_SRC_SETUP(dst, lane_x, bm_x, bn_x)                                                                         \
  _Pragma("unroll") for (int j = 0; j < PER_WAVE; ++j) {                                                              \
    const int grow = 16 * (wave + NW * j);                      /* first LDS row of this piece: wave-uniform */       \
    const int lrow = grow + ((lane_x) >> 2);                                                                          \
    const int seg = ((lane_x) & 3) ^ ((lrow >> 2) & 3);                                                               \
    const bool is_a = grow < 2 * BM, second = is_a ? grow >= BM : grow >= 2 * BM + BN;                                \
    const __half* base = is_a ? g.A : g.W;                                                                            \
    const size_t plane = second ? (BF16 ? (size_t)HBK : (is_a ? g.a_ps : g.w_ps)) : 0;                                \
    const int limit = is_a ? g.M : g.N;                                                                               \
    const size_t ld = is_a ? (size_t)g.lda : (size_t)g.ldw;                                                           \
    int trow = (is_a ? (bm_x) + lrow - (second ? BM : 0) : (bn_x) + lrow - 2 * BM - (second ? BN : 0));               \
    if (M16 && !is_a) {   /* the output-column map of the register epilogue (acc16): LDS row 16 j + c of a wave's 64 = W tile j, lane c */ \
      const int wrow = trow - (bn_x), wc = wrow & 15, wj = (wrow >> 4) & 3;                                           \
      trow = (bn_x) + ((wrow & ~63) | (g.out_h ? 8 * (wc & 7) + 4 * (wc >> 3) + wj : 4 * wc + wj));                   \
    }                                                                                                                 \
    if (!FULL && trow >= limit) trow = limit - 1;                                                                     \
    dst[j] = base + plane + (size_t)trow * ld + seg * 8 + (size_t)kbeg * KSTEP;                                       \
  }
  PP_SRC_SETUP(src, lane_t, bm, bn)
#define PP_PIECE(buf, k0, j)                                                                                   \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + (k0)),             \
                                   (__attribute__((address_space(3))) void*)(smem + (size_t)(buf) * ROWS * HBK + \
                                                                             16 * (wave + NW * (j)) * HBK),     \
                                   16, 0, 0)

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, sw = (lane >> 2) & 3, hf = lane >> 5;
  const int a_row = wm * (BM / WM) + frow, w_row = 2 * BM + wn * (BN / WN) + frow;
  const int so0 = ((0 + hf) ^ sw) * 8, so1 = ((2 + hf) ^ sw) * 8;   // segment offsets of chunk 0 / 1

  f16x8 ah0, ah1, al0, al1, bh0, bh1, bl0, bl1;
  f16x8 ah2, ah3, al2, al3;   // two-phase schedule: all four 32-row fragments of the wave's A rows per k-chunk
  // M16 (tail-pass launches, GemmH2Args::mfma16): the wave's 128 x 64 outputs as 8 x 4 tiles of 16 x 16, the same 128 registers.
  // Lane (c, g) holds rows 4g .. 4g+3 of ONE column per tile, and which W row the DMA puts into LDS row 16 j + c of the wave's
  // 64 is free (PP_SRC_SETUP): fp32 outputs take column 4 c + j, so the lane's four tiles are four consecutive columns and
  // the 16 lanes of a group a row's 256 contiguous bytes; plane outputs take 8 (c & 7) + 4 (c >> 3) + j, so lanes c and c ^ 8
  // hold the halves of an 8-column piece. The epilogue stores 16-byte row pieces from the accumulators (h2_direct16_*,
  // gemm_h2.hip); the K-loop does not know the map.
  // Lane (c = lane & 15, g = lane >> 4) holds k = 8g .. 8g+7 of row base + c: ONE 16-byte segment of the row, at the
  // inverse of the DMA's swizzle (PP_SRC_SETUP: seg ^ ((row >> 2) & 3); tile bases are multiples of 16, so the term is the
  // lane's own) — the 16 lanes of a group read 16 different 16-byte slots of a 256-byte bank line.
  f32x4 acc16[8][4];
  f16x8 wh2, wh3, wl2, wl3;   // (with bh0, bh1, bl0, bl1: the four 16-row W fragments, kept over both phases of a K-tile)
  // (from the per-tile laundered lane index: recomputed per tile instead of living through the epilogue, which needs the registers)
  const int a_row16 = wm * (BM / WM) + (lane_t & 15), w_row16 = 2 * BM + wn * (BN / WN) + (lane_t & 15);
  const int so16 = ((lane_t >> 4) ^ ((lane_t >> 2) & 3)) * 8;
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#define PP_LOAD_W(buf, so)                                                                              \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK;                                            \
    bh0 = *reinterpret_cast<const f16x8*>(base_ + (w_row) * HBK + (so));                                \
    bh1 = *reinterpret_cast<const f16x8*>(base_ + (w_row + 32) * HBK + (so));                           \
    bl0 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row) * HBK + (so));                           \
    bl1 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row + 32) * HBK + (so));                      \
  }
#define PP_LOAD_A(buf, so, i0)                                                                          \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK;                                            \
    ah0 = *reinterpret_cast<const f16x8*>(base_ + (a_row + (i0) * 32) * HBK + (so));                    \
    ah1 = *reinterpret_cast<const f16x8*>(base_ + (a_row + (i0) * 32 + 32) * HBK + (so));               \
    al0 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row + (i0) * 32) * HBK + (so));               \
    al1 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row + (i0) * 32 + 32) * HBK + (so));          \
  }
#define PP_LOAD_A4(buf, so)                                                                             \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK;                                            \
    ah0 = *reinterpret_cast<const f16x8*>(base_ + (a_row) * HBK + (so));                                \
    ah1 = *reinterpret_cast<const f16x8*>(base_ + (a_row + 32) * HBK + (so));                           \
    ah2 = *reinterpret_cast<const f16x8*>(base_ + (a_row + 64) * HBK + (so));                           \
    ah3 = *reinterpret_cast<const f16x8*>(base_ + (a_row + 96) * HBK + (so));                           \
    al0 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row) * HBK + (so));                           \
    al1 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row + 32) * HBK + (so));                      \
    al2 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row + 64) * HBK + (so));                      \
    al3 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row + 96) * HBK + (so));                      \
  }
#define PP_MFMA(a, b, c)                                                                                 \
  do {                                                                                                   \
    if (BF16) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0); \
    else c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);                                   \
  } while (0)
// the 12 MFMAs of a phase in three groups of four (lo*hi, hi*lo, hi*hi); D1..D3 are statements issued in the
// MFMA shadows after the 2nd, 6th and 10th MFMA (LDS-DMA pieces of the next tile, or nothing)
#define PP_MMA(i0, D1, D2, D3)                                                                          \
  {                                                                                                     \
    if (BF16) {   /* slice 1 x slice 1 ("lo" rows), then slice 0 x slice 0 */                           \
      PP_MFMA(al0, bl0, acc[(i0)][0]); PP_MFMA(al0, bl1, acc[(i0)][1]);                                 \
      __builtin_amdgcn_sched_barrier(0); D1; __builtin_amdgcn_sched_barrier(0);                         \
      PP_MFMA(al1, bl0, acc[(i0) + 1][0]); PP_MFMA(al1, bl1, acc[(i0) + 1][1]);                         \
      __builtin_amdgcn_sched_barrier(0); D2; __builtin_amdgcn_sched_barrier(0);                         \
      PP_MFMA(ah0, bh0, acc[(i0)][0]); PP_MFMA(ah0, bh1, acc[(i0)][1]);                                 \
      __builtin_amdgcn_sched_barrier(0); D3; __builtin_amdgcn_sched_barrier(0);                         \
      PP_MFMA(ah1, bh0, acc[(i0) + 1][0]); PP_MFMA(ah1, bh1, acc[(i0) + 1][1]);                         \
    } else {                                                                                            \
    PP_MFMA(al0, bh0, acc[(i0)][0]); PP_MFMA(al0, bh1, acc[(i0)][1]);                                   \
    __builtin_amdgcn_sched_barrier(0); D1; __builtin_amdgcn_sched_barrier(0);                           \
    PP_MFMA(al1, bh0, acc[(i0) + 1][0]); PP_MFMA(al1, bh1, acc[(i0) + 1][1]);                           \
    PP_MFMA(ah0, bl0, acc[(i0)][0]); PP_MFMA(ah0, bl1, acc[(i0)][1]);                                   \
    __builtin_amdgcn_sched_barrier(0); D2; __builtin_amdgcn_sched_barrier(0);                           \
    PP_MFMA(ah1, bl0, acc[(i0) + 1][0]); PP_MFMA(ah1, bl1, acc[(i0) + 1][1]);                           \
    PP_MFMA(ah0, bh0, acc[(i0)][0]); PP_MFMA(ah0, bh1, acc[(i0)][1]);                                   \
    __builtin_amdgcn_sched_barrier(0); D3; __builtin_amdgcn_sched_barrier(0);                           \
    PP_MFMA(ah1, bh0, acc[(i0) + 1][0]); PP_MFMA(ah1, bh1, acc[(i0) + 1][1]);                           \
    }                                                                                                   \
  }
// the 24 MFMAs of a phase of the two-phase schedule: lo*hi, hi*lo, hi*hi over the wave's 4 x 2 output tiles (every
// accumulator is touched once per group of eight: no back-to-back dependence); D0..D7 = statements in the MFMA shadows.
// (The three products of an accumulator back to back, as the 16x16x32 body issues them below, did NOT pay on this shape:
// registers only, 1709 against 1718 TF/s, -0.5 % in every round, tools/mfma_chain_probe.hip — the order stays interleaved.)
#define PP_SB __builtin_amdgcn_sched_barrier(0)
#define PP_MMA8(A0, A1, A2, A3, B0, B1, Da, Db, Dc)                                                     \
    PP_MFMA(A0, B0, acc[0][0]); PP_MFMA(A0, B1, acc[0][1]); PP_MFMA(A1, B0, acc[1][0]);                 \
    PP_SB; Da; PP_SB;                                                                                   \
    PP_MFMA(A1, B1, acc[1][1]); PP_MFMA(A2, B0, acc[2][0]); PP_MFMA(A2, B1, acc[2][1]);                 \
    PP_SB; Db; PP_SB;                                                                                   \
    PP_MFMA(A3, B0, acc[3][0]); PP_MFMA(A3, B1, acc[3][1]);                                             \
    PP_SB; Dc; PP_SB;
#define PP_MMA24(D0, D1, D2, D3, D4, D5, D6, D7)                                                        \
  {                                                                                                     \
    if (BF16) {   /* slice 1 x slice 1 ("lo" rows), then slice 0 x slice 0 */                           \
      PP_MMA8(al0, al1, al2, al3, bl0, bl1, D0, D1, D2)                                                 \
      PP_SB; D3; D4; PP_SB;                                                                             \
      PP_MMA8(ah0, ah1, ah2, ah3, bh0, bh1, D5, D6, D7)                                                 \
    } else {                                                                                            \
      PP_MMA8(al0, al1, al2, al3, bh0, bh1, D0, D1, D2)                                                 \
      PP_MMA8(ah0, ah1, ah2, ah3, bl0, bl1, D3, D4, D5)                                                 \
      PP_MMA8(ah0, ah1, ah2, ah3, bh0, bh1, D6, D7, (void)0)                                            \
    }                                                                                                   \
  }
// the 8 LDS-DMA pieces of the next tile go into the MFMA shadows of M_0 / M_1 / M_2 (3 + 3 + 2); issuing them in
// the load segments instead (4+4 or 3+3+2), with or without s_setprio, measured the same within 0.5 % (DVFS)
#define PP_DMA(j) if (more) PP_PIECE(nxt, k1, j)
#define PP_DMA_M(j) PP_DMA(j)
// end of a load segment: retire this wave's ds_reads (and, with VM, its LDS-DMA), then the segment barrier
#define PP_L_END(waitimm, ph)                                                                           \
  __builtin_amdgcn_sched_barrier(0);                                                                    \
  __builtin_amdgcn_s_waitcnt(waitimm);                                                                  \
  __builtin_amdgcn_s_barrier();                                                                         \
  __builtin_amdgcn_sched_barrier(0);                                                                    \
  __builtin_amdgcn_s_setprio(1)
#define PP_M_END(ph)                                                                                    \
  __builtin_amdgcn_sched_barrier(0);                                                                    \
  __builtin_amdgcn_s_setprio(0);                                                                        \
  __builtin_amdgcn_s_barrier();                                                                         \
  __builtin_amdgcn_sched_barrier(0)
  constexpr int WAIT_LGKM = 0xc07f, WAIT_ALL = 0x0070;   // lgkmcnt(0) | vmcnt(0) lgkmcnt(0)
  constexpr int WAIT_VM4 = 0x0074;                       // vmcnt(4) lgkmcnt(0)
// ---- 16x16x32 body: one MFMA spans the K-tile's 32 columns, so the two phases of a K-tile split the wave's A rows (phase p:
// A tiles 4p .. 4p+3 against the four W tiles = 16 outputs x 3 products = 48 MFMAs of 16 cycles, the 768 matrix-pipe cycles
// of the 24 x 32 above). Every accumulator takes lo*hi, hi*lo, hi*hi in that order, BACK TO BACK (PP16_MMA3): the second and
// third MFMA of a triple take C from the result of the one before instead of from the register file, and a dependent MFMA on the
// same accumulator issues without a wait state. Sixteen triples per phase, A tile i outer, W tile j inner; the fences keep the
// compiler from interleaving two triples again. Per accumulator the products and their order are what they were with the three
// products 16 MFMAs apart: the same bits (tests/test_gpu_gemm_issue_order.py). Registers only, chained against interleaved:
// 2150 against 1958 TF/s, +10 %, at 2.12 against 1.94 GHz (tools/mfma_chain_probe.hip). The DMA pieces sit after every second
// triple (96 cycles, as after every 3rd MFMA above). 8 W + 8 A fragment reads in L_0, 8 A reads in L_1: 24 per K-tile.
#define PP16_LOAD_W(buf)                                                                                \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK + so16;                                     \
    bh0 = *reinterpret_cast<const f16x8*>(base_ + (w_row16) * HBK);                                     \
    bh1 = *reinterpret_cast<const f16x8*>(base_ + (w_row16 + 16) * HBK);                                \
    wh2 = *reinterpret_cast<const f16x8*>(base_ + (w_row16 + 32) * HBK);                                \
    wh3 = *reinterpret_cast<const f16x8*>(base_ + (w_row16 + 48) * HBK);                                \
    bl0 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row16) * HBK);                                \
    bl1 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row16 + 16) * HBK);                           \
    wl2 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row16 + 32) * HBK);                           \
    wl3 = *reinterpret_cast<const f16x8*>(base_ + (BN + w_row16 + 48) * HBK);                           \
  }
#define PP16_LOAD_A(buf, ph)                                                                            \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK + so16;                                     \
    ah0 = *reinterpret_cast<const f16x8*>(base_ + (a_row16 + (ph) * 64) * HBK);                         \
    ah1 = *reinterpret_cast<const f16x8*>(base_ + (a_row16 + (ph) * 64 + 16) * HBK);                    \
    ah2 = *reinterpret_cast<const f16x8*>(base_ + (a_row16 + (ph) * 64 + 32) * HBK);                    \
    ah3 = *reinterpret_cast<const f16x8*>(base_ + (a_row16 + (ph) * 64 + 48) * HBK);                    \
    al0 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row16 + (ph) * 64) * HBK);                    \
    al1 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row16 + (ph) * 64 + 16) * HBK);               \
    al2 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row16 + (ph) * 64 + 32) * HBK);               \
    al3 = *reinterpret_cast<const f16x8*>(base_ + (BM + a_row16 + (ph) * 64 + 48) * HBK);               \
  }
#define PP16_MFMA(a, b, c) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define PP16_MMA3(i, j, AL, AH, BH, BL)                                                                 \
    PP16_MFMA(AL, BH, acc16[i][j]); PP16_MFMA(AH, BL, acc16[i][j]); PP16_MFMA(AH, BH, acc16[i][j]);     \
    PP_SB;
#define PP16_ROW(i, AL, AH, Da, Db)   /* the four accumulators of A tile i: twelve MFMAs, two DMA slots */ \
    PP16_MMA3(i, 0, AL, AH, bh0, bl0) PP16_MMA3(i, 1, AL, AH, bh1, bl1)                                 \
    Da; PP_SB;                                                                                          \
    PP16_MMA3(i, 2, AL, AH, wh2, wl2) PP16_MMA3(i, 3, AL, AH, wh3, wl3)                                 \
    Db; PP_SB;
#define PP16_MMA48(i0, D0, D1, D2, D3, D4, D5, D6, D7)                                                  \
  {                                                                                                     \
    PP16_ROW((i0), al0, ah0, D0, D1)                                                                    \
    PP16_ROW((i0) + 1, al1, ah1, D2, D3)                                                                \
    PP16_ROW((i0) + 2, al2, ah2, D4, D5)                                                                \
    PP16_ROW((i0) + 3, al3, ah3, D6, D7)                                                                \
  }

#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) PP_PIECE(0, 0, j);
  if (BF16 && nkt > 1) {   // BF16 schedule (below): the first 32-column slice of tile 1 is already on its way
    PP_PIECE(1, KSTEP, 0); PP_PIECE(1, KSTEP, 1); PP_PIECE(1, KSTEP, 4); PP_PIECE(1, KSTEP, 5);
    __builtin_amdgcn_s_waitcnt(WAIT_VM4);
  } else {
    __builtin_amdgcn_s_waitcnt(WAIT_ALL);
  }
  __builtin_amdgcn_s_barrier();                      // tile 0 landed for everyone
  __builtin_amdgcn_sched_barrier(0);
  if (wm == 1) __builtin_amdgcn_s_barrier();         // group 1 runs one barrier behind
  __builtin_amdgcn_sched_barrier(0);
  if (BF16) {
    // One bf16 MFMA per product: a K-tile is 0.85 us of matrix-pipe time, and with the schedule of the split-precision
    // kernel (all 8 pieces of tile t+1 issued in M_0 of tile t, retired at the end of L_1 of tile t: half a K-tile of
    // cover) the loop ran at the memory latency instead: 2.0 us per K-tile alone on the chip (267 us for the 128 K-tiles of a
    // decoder layer's weight gradients). Here a phase consumes ONE 32-column slice (the "hi" rows = columns 0-31 in phase 0, the
    // "lo" rows = columns 32-63 in phase 1; the h registers hold its first 16-column chunk, the l registers the second), so a
    // slice's rows are free after their own phase and are refilled two phases later with the slice of the tile after next:
    //   M_0(t): slice 1 of tile t+1 -> the other buffer (last read in L_1(t-1));  M_1(t): slice 0 of tile t+2 -> this buffer
    //   (last read in L_0(t), by group 1 one barrier later — hence not before M_1). A slice is retired by vmcnt(4) — all but
    //   the four pieces of the slice issued after it — at the end of the load segment one phase before its first read (the
    //   staggered groups need that barrier): a whole K-tile between issue and wait instead of half of one.
    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1, nxt = cur ^ 1;
      const bool more1 = kt + 1 < nkt, more2 = kt + 2 < nkt;
      const int k1 = (kt + 1) * KSTEP, k2 = (kt + 2) * KSTEP;
#define PP_LOAD_SLICE(buf, sl)                                                                            \
  {                                                                                                     \
    const __half* base_ = smem + (size_t)(buf) * ROWS * HBK;                                            \
    bh0 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BN + w_row) * HBK + so0);                     \
    bh1 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BN + w_row + 32) * HBK + so0);                \
    bl0 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BN + w_row) * HBK + so1);                     \
    bl1 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BN + w_row + 32) * HBK + so1);                \
    ah0 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row) * HBK + so0);                     \
    ah1 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 32) * HBK + so0);                \
    ah2 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 64) * HBK + so0);                \
    ah3 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 96) * HBK + so0);                \
    al0 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row) * HBK + so1);                     \
    al1 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 32) * HBK + so1);                \
    al2 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 64) * HBK + so1);                \
    al3 = *reinterpret_cast<const f16x8*>(base_ + ((sl) * BM + a_row + 96) * HBK + so1);                \
  }
#define PP_DMA1(j) if (more1) PP_PIECE(nxt, k1, j)
#define PP_DMA2(j) if (more2) PP_PIECE(cur, k2, j)
      PP_LOAD_SLICE(cur, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more1) __builtin_amdgcn_s_waitcnt(WAIT_VM4); else __builtin_amdgcn_s_waitcnt(WAIT_ALL);   // slice 1 of this tile
      PP_L_END(WAIT_LGKM, 0);
      PP_MMA24(PP_DMA1(2), (void)0, PP_DMA1(3), (void)0, (void)0, PP_DMA1(6), (void)0, PP_DMA1(7));
      PP_M_END(0);
      PP_LOAD_SLICE(cur, 1);
      __builtin_amdgcn_sched_barrier(0);
      if (more1) __builtin_amdgcn_s_waitcnt(WAIT_VM4); else __builtin_amdgcn_s_waitcnt(WAIT_ALL);   // slice 0 of the next tile
      PP_L_END(WAIT_LGKM, 1);
      PP_MMA24(PP_DMA2(0), (void)0, PP_DMA2(1), (void)0, (void)0, PP_DMA2(4), (void)0, PP_DMA2(5));
      PP_M_END(1);
#undef PP_LOAD_SLICE
#undef PP_DMA1
#undef PP_DMA2
    }
  } else if constexpr (M16) {
    for (int kt = 0; kt < nkt; ++kt) {   // same segments, waits and barriers as the 32x32x16 loop below
      const int cur = kt & 1, nxt = cur ^ 1;
      const bool more = kt + 1 < nkt;
      const int k1 = (kt + 1) * KSTEP;
      PP16_LOAD_W(cur);
      PP16_LOAD_A(cur, 0);
      PP_L_END(WAIT_LGKM, 0);
      PP16_MMA48(0, PP_DMA_M(0), PP_DMA_M(1), PP_DMA_M(2), PP_DMA_M(3), PP_DMA_M(4), PP_DMA_M(5), PP_DMA_M(6), PP_DMA_M(7));
      PP_M_END(0);
      // phase 1: the other 64 A rows (the W fragments stay in registers); tile kt+1 must have landed before anyone's next L_0
      PP16_LOAD_A(cur, 1);
      PP_L_END(WAIT_ALL, 1);
      PP16_MMA48(4, (void)0, (void)0, (void)0, (void)0, (void)0, (void)0, (void)0, (void)0);
      PP_M_END(1);
    }
  } else
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1, nxt = cur ^ 1;
    const bool more = kt + 1 < nkt;
    const int k1 = (kt + 1) * KSTEP;
    // Two phases per K-tile (one per 16-column k-chunk), each = load segment (4 W + 8 A fragments) | barrier | MFMA segment
    // (24 MFMAs; the 8 LDS-DMA pieces of the next tile in the shadows of the FIRST one) | barrier. Four phases of 12 MFMAs
    // (a phase per k-chunk and half of the A rows) cost twice the barriers: per-segment stamps showed every one of the 8
    // barrier intervals of a K-tile at ~630 cycles for 384 of MFMA issue (M 460-550 with the DMA pieces and fixed costs,
    // ~100 of barrier latency): 5076 cycles per K-tile against 3072 of matrix-pipe time.
    PP_LOAD_W(cur, so0);
    PP_LOAD_A4(cur, so0);
    PP_L_END(WAIT_LGKM, 0);
    PP_MMA24(PP_DMA_M(0), PP_DMA_M(1), PP_DMA_M(2), PP_DMA_M(3), PP_DMA_M(4), PP_DMA_M(5), PP_DMA_M(6), PP_DMA_M(7));
    PP_M_END(0);
    // phase 1: chunk 1; tile kt+1 must have landed before anyone's next L_0
    PP_LOAD_W(cur, so1);
    PP_LOAD_A4(cur, so1);
    PP_L_END(WAIT_ALL, 1);
    PP_MMA24((void)0, (void)0, (void)0, (void)0, (void)0, (void)0, (void)0, (void)0);
    PP_M_END(1);
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();         // group 0 catches the extra barrier of group 1
  __builtin_amdgcn_sched_barrier(0);
#undef PP_LOAD_W
#undef PP_LOAD_A
#undef PP_MFMA
#undef PP_MMA
#undef PP_MMA8
#undef PP_MMA24
#undef PP16_LOAD_W
#undef PP16_LOAD_A
#undef PP16_MFMA
#undef PP16_MMA3
#undef PP16_ROW
#undef PP16_MMA48
#undef PP_SB
#undef PP_LOAD_A4
#undef PP_DMA
#undef PP_DMA_M
#undef PP_L_END
#undef PP_M_END

  int lane_e = lane;   // laundered like lane_t: the epilogue's per-lane offsets must not live through the K-loop
  asm volatile("" : "+v"(lane_e));
  if constexpr (M16) h2_epilogue_256<FULL, TM, TN, WM, WN, 256, 256, false, true>(g, acc16, smem, wave, lane_e, bm, bn, wm, wn, g.row_ssq ? rs_tile : nullptr, acc_scale);
  else
  h2_epilogue_256<FULL, TM, TN, WM, WN, 256, 256, BF16 && FULL>(g, acc, smem, wave, lane_e, bm, bn, wm, wn, g.row_ssq ? rs_tile : nullptr, acc_scale);
  // The staging strips (M16: only the K/V-scatter and fp32-residual variants have them) alias the operand buffers the next
  // tile's LDS-DMA writes, and rs_tile is rewritten: every wave's LDS
  // reads must have returned (lgkmcnt(0)) before anyone goes on. NOT __syncthreads(): its fence also waits for vmcnt(0),
  // i.e. for every global store of this tile to be acknowledged by the L2 (2-5 us under load) — the stores take their data
  // from registers and drain under the next tile's prologue instead.
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
#undef PP_PIECE
#undef PP_SRC_SETUP
  }
