// Route policy of the split-precision GEMM (gemm_h2.hip): which kernel family, tile shape, K split and reduction a launch
// of launch_gemm_h2 / launch_gemm_h2_group takes. Plain host arithmetic on the shape and a few flags — no HIP types, so
// tests/test_gemm_route.py compiles it with the host compiler and checks the shape -> route table without a GPU.
// gemm_h2.hip fills GemmRouteIn from GemmH2Args, asks plan_gemm_h2 and launches the steps of the plan in order.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#include "../../include/ripor_hip.h"

namespace rpr {

constexpr int HBK = 32;  // K-tile depth = halves per LDS row (64 B, unpadded)

// What the routes test of a GemmH2Args (common.h). The alignment bits are true when the launch qualifies.
struct GemmRouteIn {
  int M = 0, N = 0, K = 0, cus = 0;      // cus: CUs the launch may use (0 = the whole chip, 256)
  int split_n = 0, rm_B = 0, ksplit = 0, small_live = 0, live_lo = 0, live_hi = 0;
  size_t part_cap = 0;
  bool part = false, mid_split = false, m_dev = false, bf16 = false, no_row_split = false;
  bool force_pp = false;  // the caller pins this launch to the 256x256 ping-pong kernel, unsplit (GemmH2Args::force_pp)
  bool mfma16 = false;    // a tail pass's launch: its ping-pong step runs the 16x16x32 body (GemmH2Args::mfma16)
  bool out_h = false, row_ssq = false, ssq_out = false, resid = false, resid_h = false, relu = false, out_b = false, out_bt = false;
  bool ab_al8 = true;     // lda and ldw multiples of 8
  bool ldo0_al4 = true;   // ldo[0] a multiple of 4
  bool ldr_al4 = true;    // no fp32 residual, or ldr a multiple of 4
  bool epi_al4 = true;    // ldo[0..2] and the leading dimensions of resid / resid_h / out_h in use multiples of 4
  bool outb_al = true;    // out_b / out_bt / mask_src in use: ldob, ldobt multiples of 8, ldobt >= M, ldmask a multiple of 4
};

// Thresholds (with the measurements behind them) and the development switches that override them. The product library
// runs the defaults; the development build fills the switches from the environment once (gemm_h2.hip: gemm_tuning).
struct GemmTuning {
  int skinny = 352;         // max rows of the skinny routes (measured per search: 320 rows skinny 66.0 vs split-K route 68.5 ms, 400 rows 95.5 vs 71.8)
  int wsplit_max = 1400;    // max rows of a wave-split launch. RPR_GEMM_WSPLIT_MAX (0: the routes behind it)
  int splitk_target = 640;  // partial tiles per split-K launch that the 128 x 64 routes aim for
  int bf_pp = 200;          // bf16: min tiles of 256^2 for the ping-pong kernel (they fill the chip)
  int deep_max = 128;       // blocks up to which the 128-row tiles run 4 stages deep (fewer tiles than CUs: one block per CU, 3 K-tiles in flight)
  // 256x256 ping-pong: >= ~112 tiles (per 256 CUs) to beat the 128x128 kernel (measured), i.e. M = Q*B >= ~10k rows for N = 768.
  // 256-tile rounds on the 256 CUs: a launch just over a whole number of rounds (e.g. 288 tiles) leaves most of the chip idle
  // in its last round; the 128-tile kernels quantise finer (measured M = 8192, N = 2304: 135 vs 151 us)
  int pp_min_tiles = 112;
  double pp_round_eff = 0.6;
  // Row split of a ping-pong launch just over a whole number of rounds (beam 1000 with one query: 318 tiles of 256^2 for the
  // N = 768 products = 1.24 rounds, the second one with 62 of 256 CUs busy): the row tiles that fill whole rounds go to the
  // ping-pong kernel, the rows behind them to the 128 x 128 tile kernel (a quarter of the work per block, 1.22 x the time per
  // flop), as a second launch on the same stream. Taken when the estimate — whole rounds + rs_round128 per round of 128^2
  // tiles (measured: 5240 rows x 768 columns = 246 such tiles in 35.7 us against 87.1 us for the 255 tiles of 256^2 in front
  // of them, profiles/archive/r05x_rowsplit_gemm.txt) + ~rs_launch_us for the second launch (a 256^2 tile takes rs_tile_us at
  // K = 768) — is under rs_gain of the rounds the ping-pong kernel alone would need.
  double rs_round128 = 0.43, rs_launch_us = 6.0, rs_tile_us = 78.0, rs_gain = 0.9;
  int force_tile = 0;       // RPR_GEMM_TILE: 256 = ping-pong, 64 / other = 128x64 / 128x128 tiles, whatever the shape
  int row_split = 1;        // RPR_GEMM_ROWSPLIT: 0 = off; 2 (tests) = every ping-pong launch with two or more row tiles is split in the middle
  int row_split_log = 0;    // RPR_GEMM_ROWSPLIT_LOG: one stderr line per row split
  int wsplit_cfg = -1, wsplit_ks = 0;   // RPR_WSPLIT_CFG / RPR_WSPLIT_KS force the wave-split tile shape (0..2) / K split
  // RPR_PP_SUPERTILE: super-tile order of ping-pong products more than four column tiles wide (N = 2304, 3072): column groups of
  // 3 or 4 tiles (> 1: of that many), bands of as many row panels as the blocks of one XCD fill with such a group. 0: row-major
  int supertile = 1;
};

enum GemmFamily { GEMM_SKINNY16, GEMM_WSPLIT, GEMM_DMA, GEMM_PP };   // 16-row skinny, wave-split, 128-row LDS-DMA tiles, 256x256 ping-pong
// What follows a K split over blockIdx.y: splitk_reduce_kernel (sum + fp32 residual), or the whole epilogue on the sum,
// one (splitk_epilogue_kernel) or four (splitk_epilogue4_kernel) columns per thread
enum GemmReduce { REDUCE_NONE, REDUCE_SUM, REDUCE_FUSED, REDUCE_FUSED4 };

struct GemmStep {
  int family = GEMM_DMA, bm = 0, bn = 0, stages = 0;   // kernel family, tile shape, LDS ring depth (0: the ping-pong / skinny kernels have one)
  bool full = false, bf16 = false;                     // FULL instantiation (no ragged tiles, no device row count); bf16 operands
  bool m16 = false;                                    // ping-pong step of a tail-pass launch: the 16x16x32 body (never bf16, never a K split)
  int rows = 0, m_base = 0;                            // covers rows [m_base, m_base + rows) of the product
  int live_lo = 0, live_hi = 0;                        // live-count window (GemmH2Args::live_lo)
  int ksplit = 1, reduce = REDUCE_NONE;
  int tile_cw = 0, tile_rb = 0;                        // ping-pong tile order (GemmH2Args::tile_cw)
  int tiles_m = 0, tiles_n = 0, grid_x = 0, grid_y = 1, block = 256;
};

struct GemmPlan {
  bool invalid = false;            // the arguments are refused (hipErrorInvalidValue)
  int cls = RPR_K_GEMM_SMALL;      // profile class reported to the caller
  int n = 0;
  GemmStep step[4];                // (a compacted stage whose large-tile launch is row-split has four)
  void add(const GemmStep& s) { step[n++] = s; }
};

// Largest split count <= ks in which every split owns at least one of the nkt K-tiles.
inline long trim_ks(long ks, int nkt) {
  while (ks > 1 && (ks - 1) * ((nkt + ks - 1) / ks) >= nkt) --ks;
  return ks;
}

// Tile shape and K split of a wave-split launch. These launches are latency-bound by LDS capacity: a block keeps at most its
// rings in flight (64-96 KB) against a loaded L2 / Infinity-Cache latency of ~3 us, i.e. 40-50 GB/s per CU whatever the tile
// (tools/attic/fill_probe.hip: the LDS-DMA path itself sustains > 100 GB/s per CU from L2), one block per CU (128-144 KB of LDS).
// Model fitted to tools/wsplit_bench.sh on MI355X (profiles/archive/r05d_wsplit_gemm_bench.txt): launch = 5 us + rounds of blocks over
// the CUs x (3 us + KB per block / rate), + one reduction launch for a K split over blocks.
// cfg 0: 32 x 32 (four stages), 1: 64 x 32 (three), 2: 64 x 64 (two).
struct WsplitChoice { int cfg, ks; double us; long rounds; };
inline WsplitChoice choose_wsplit(int M, int N, int K, int cus, bool can_split, size_t part_cap) {
  constexpr double lat_us = 3.0, split_us = 4.5;   // per round of blocks; the reduction launch of a K split
  const int bm[3] = {32, 64, 64}, bn[3] = {32, 32, 64};
  const double rate_gbs[3] = {48.0, 48.0, 41.0};
  WsplitChoice best{0, 1, 1e30, 1};
  for (int c = 0; c < 3; ++c) {
    const long tiles = (long)((M + bm[c] - 1) / bm[c]) * ((N + bn[c] - 1) / bn[c]);
    for (int ks = 1; ks <= 4; ++ks) {
      if (ks > 1 && (!can_split || K / ks < 256 || (size_t)M * N * ks > part_cap)) break;
      const int nkt = K / HBK;
      if (ks > 1 && (ks - 1) * ((nkt + ks - 1) / ks) >= nkt) continue;
      const long blocks = tiles * ks, rounds = (blocks + cus - 1) / cus;
      const double kb = (double)(bm[c] + bn[c]) * ((double)K / ks) * 4.0 * 1e-3;
      const double us = 5.0 + rounds * (lat_us + kb / rate_gbs[c]) + (ks > 1 ? split_us : 0.0);
      if (us < best.us) best = {c, ks, us, rounds};
    }
  }
  return best;
}

inline long ceil_tiles(int M, int N, int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// K split of a 128 x 64 launch: enough splits for `want` blocks, at most ks_max, within the scratch, trimmed to the nkt K-tiles.
inline long splitk_128x64(const GemmRouteIn& a, long want, long ks_max, int nkt) {
  const long t = ceil_tiles(a.M, a.N, 128, 64);
  long ks = std::min<long>((want + t - 1) / t, ks_max);
  ks = std::min<long>(ks, (long)(a.part_cap / ((size_t)a.M * a.N)));
  return trim_ks(ks, nkt);
}

// splitk_epilogue4_kernel applies: N % 256 == 0 and every column split and leading dimension a multiple of 4.
inline int fused_reduce(const GemmRouteIn& a) { return (a.N & 255) == 0 && (a.split_n & 3) == 0 && a.epi_al4 ? REDUCE_FUSED4 : REDUCE_FUSED; }

inline GemmStep route_step(const GemmRouteIn& a, int family, int bm, int bn, int ks, int reduce) {
  GemmStep s;
  s.family = family; s.bm = bm; s.bn = bn; s.bf16 = a.bf16;
  s.rows = a.M; s.live_lo = a.live_lo; s.live_hi = a.live_hi;
  s.tiles_m = (a.M + bm - 1) / bm; s.tiles_n = (a.N + bn - 1) / bn;
  s.full = (a.M % bm == 0) && (a.N % bn == 0) && !a.m_dev;
  s.ksplit = ks > 1 ? ks : (a.ksplit > 1 ? a.ksplit : 1);   // (ks <= 1: a split the caller set up itself passes through)
  s.reduce = ks > 1 ? reduce : REDUCE_NONE;
  s.grid_x = s.tiles_m * s.tiles_n; s.grid_y = s.ksplit;
  return s;
}

// 128 x 64 / 128 x 128 LDS-DMA tiles
inline GemmStep dma_step(const GemmRouteIn& a, const GemmTuning& t, int bn, int ks = 1, int reduce = REDUCE_NONE) {
  GemmStep s = route_step(a, GEMM_DMA, 128, bn, ks, reduce);
  s.stages = (s.grid_x * s.ksplit <= t.deep_max && (!a.m_dev || a.live_hi > 0)) ? 4 : 2;
  return s;
}

// 256x256 tile, 8 waves (2x4) of 128x64, ping-pong schedule: half the staged bytes per MFMA of the 128x128 tile.
// Persistent blocks: one per CU of the stream (a whole number per XCD), fewer when the launch has fewer tiles; split-K
// launches are not persistent: one block per (tile, K range).
inline GemmStep pp_step(const GemmRouteIn& a, const GemmTuning& t, int ks = 1, int reduce = REDUCE_NONE) {
  GemmStep s = route_step(a, GEMM_PP, 256, 256, ks, reduce);
  const int cus = a.cus > 0 ? a.cus : 256, nt = s.grid_x, grid = nt > cus ? cus : nt;
  s.block = 512;
  s.m16 = a.mfma16 && !a.bf16 && s.ksplit == 1;
  if (s.ksplit == 1) s.grid_x = grid;
  if (t.supertile && s.ksplit == 1 && s.tiles_n > 4 && nt > grid) {
    s.tile_cw = t.supertile > 1 ? t.supertile : (s.tiles_n % 4 == 0 ? 4 : (s.tiles_n % 3 == 0 ? 3 : 4));
    s.tile_rb = std::max(1, (grid / 8) / s.tile_cw);
  }
  return s;
}

// cfg 0 .. 2 of choose_wsplit; a K split is followed by the fused epilogue
inline GemmStep wsplit_step(const GemmRouteIn& a, int cfg, int ks = 1) {
  const int bm[3] = {32, 64, 64}, bn[3] = {32, 32, 64}, st[3] = {4, 3, 2};
  GemmStep s = route_step(a, GEMM_WSPLIT, bm[cfg], bn[cfg], ks, fused_reduce(a));
  s.stages = st[cfg];
  return s;
}

// at most `skinny` rows: one query in flight (<= 32 rows) on 16 x 16 tiles, all of K = 768 in flight; otherwise 32 x 32
// wave-split tiles (with m_dev: row tiles past the live rows exit)
inline GemmStep skinny_step(const GemmRouteIn& a) {
  if (!(a.M <= 32 && (a.N & 15) == 0)) return wsplit_step(a, 0);
  GemmStep s = route_step(a, GEMM_SKINNY16, 16, 16, 1, REDUCE_NONE);
  s.full = !a.m_dev;
  s.ksplit = 1; s.grid_x = s.tiles_n; s.grid_y = s.tiles_m;
  return s;
}

// Split-K through the 256x256 ping-pong kernel (weight gradients of the training step: dW[N, K] = dY^T X reduces over the
// 8192 rows of the batch into 9 .. 36 output tiles): one round of (tile, K range) blocks on the chip, at least 4 K-tiles per
// block, partial tiles to the caller's scratch. False when the shape does not qualify (the caller goes on to the 128x64 split-K route).
inline bool pp_splitk(const GemmRouteIn& a, const GemmTuning& t, GemmPlan& pl) {
  const int kstep = a.bf16 ? 2 * HBK : HBK;
  if (!a.part || (a.M & 255) || (a.N & 255) || (a.K % kstep) || a.relu || a.out_h || a.row_ssq || a.ssq_out || a.resid_h ||
      a.m_dev || a.rm_B || a.split_n < a.N || !a.ldo0_al4 || !a.ldr_al4)
    return false;
  const long tiles = (long)(a.M / 256) * (a.N / 256);
  const int cus = a.cus > 0 ? a.cus : 256, nkt = a.K / kstep;
  long ks = std::min<long>(cus / tiles, nkt / 4);
  ks = std::min<long>(ks, (long)(a.part_cap / ((size_t)a.M * a.N)));
  ks = trim_ks(ks, nkt);
  if (tiles > 64 || ks < 2) return false;
  pl.cls = RPR_K_GEMM;
  pl.add(pp_step(a, t, (int)ks, REDUCE_SUM));
  return true;
}

// One bf16 plane per operand (training GEMMs, RPR_PREC_BF16): fp32 output, optional residual / ReLU, split-K for the long
// reductions into few tiles (weight gradients); K-tiles of 64 columns.
inline void route_bf16(const GemmRouteIn& a, const GemmTuning& t, GemmPlan& pl) {
  if (a.out_h || a.row_ssq || a.ssq_out || a.resid_h || a.m_dev || a.rm_B || (a.K & 63) || (a.N & 3) || !a.ldo0_al4 || !a.ldr_al4 ||
      a.split_n < a.N) {
    pl.invalid = true;                                   // (the bf16 kernels' epilogues store 16-byte pieces of ONE fp32 output)
    return;
  }
  if (a.out_b || a.out_bt) {
    // bf16 operands for the consumers straight from the epilogue (GemmH2Args::out_b): the 256 x 256 kernel's FULL instantiation only
    if ((a.M & 255) || (a.N & 255) || a.resid || a.ksplit > 1 || !a.outb_al) { pl.invalid = true; return; }
    pl.cls = RPR_K_GEMM;
    return pl.add(pp_step(a, t));
  }
  const long t128b = ceil_tiles(a.M, a.N, 128, 128);
  // (A kernel with 128x128 wave tiles — 256x256 block, four waves, one per SIMD, 512 registers: two thirds of the LDS reads
  // per MFMA — was built and measured: 31-34 us per 256x256x768 tile against 23 us for this shape on the 128-row kernel
  // and 60-65 us against 54-58 on the ping-pong kernel. With ONE wave per SIMD the 16 LDS-DMA pieces and 32 fragment reads
  // of a K-tile are issued by the wave that also issues the 64 MFMAs, in series: ~2.2 us per K-tile again. Source kept
  // as tools/attic/gemm_bf16_w128.hip.txt; HISTORY.md.)
  if (a.K >= 2048 && pp_splitk(a, t, pl)) return;
  if (a.part && a.K >= 2048 && t128b * 2 < t.splitk_target && !a.relu) {
    const long ks = splitk_128x64(a, t.splitk_target, a.K / 1024, a.K / (2 * HBK));
    if (ks > 1) return pl.add(dma_step(a, t, 64, (int)ks, REDUCE_SUM));
  }
  if (ceil_tiles(a.M, a.N, 256, 256) >= t.bf_pp) return pl.add(pp_step(a, t));
  pl.add(dma_step(a, t, t128b < 256 ? 64 : 128));
}

// Everything but the compacted triple: the steps of one product whose live window, if any, is a's.
inline void route_one(const GemmRouteIn& a, const GemmTuning& t, GemmPlan& pl) {
  if (a.bf16) return route_bf16(a, t, pl);
  const int force = a.force_pp ? 256 : t.force_tile;
  const long t256 = ceil_tiles(a.M, a.N, 256, 256);
  const int cus = a.cus > 0 ? a.cus : 256;         // a lane stream owns part of the chip: thresholds scale with it
  const double round_eff = (double)t256 / (double)(((t256 + cus - 1) / cus) * cus);
  if (force == 256 || (force == 0 && t256 >= (long)t.pp_min_tiles * cus / 256 && (round_eff >= t.pp_round_eff || a.out_h || a.row_ssq))) {
    pl.cls = RPR_K_GEMM;
    const bool split_all = t.row_split == 2 && a.M > 256 && !a.force_pp;
    if (t.row_split && (force == 0 || split_all) && !a.rm_B && a.ksplit <= 1 && a.small_live == 0 && (!a.no_row_split || split_all) &&
        (t256 > cus || split_all)) {
      const int tiles_n = (a.N + 255) / 256;
      const long rounds = t256 / cus;
      const int rows_main = split_all ? ((a.M + 255) / 256 / 2) * 256 : (int)((rounds * cus) / tiles_n) * 256, m_rest = a.M - rows_main;
      if ((t256 % cus != 0 || split_all) && rows_main > 0 && m_rest > 0) {
        const long t128r = ceil_tiles(m_rest, a.N, 128, 128);
        const double tile_us = t.rs_tile_us * a.K / 768.0;
        const double cost_split = (double)rounds + t.rs_round128 * (double)((t128r + cus - 1) / cus) + t.rs_launch_us / tile_us;
        if (split_all || cost_split < t.rs_gain * (double)(rounds + 1)) {
          GemmRouteIn main_p = a, rest = a;
          main_p.M = rows_main; rest.M = m_rest;
          pl.add(pp_step(main_p, t));
          pl.add(dma_step(rest, t, 128));
          pl.step[pl.n - 1].m_base = rows_main;
          return;
        }
      }
    }
    return pl.add(pp_step(a, t));
  }
  // a handful of rows (one to a few queries in flight): the launch is a weight stream; a 128-row tile would spend
  // most of the per-CU LDS-DMA rate (~25 GB/s) on padding rows, and 32-wide column tiles give 4x the blocks
  // 33 .. ~1500 rows (a handful to ~150 queries in flight, the tail pass of one query, beam 1000 at batch 1): wave-split tiles,
  // shape and K split from choose_wsplit
  if (force == 0 && a.M > 32 && a.M <= t.wsplit_max) {
    const bool can_split = a.part && a.mid_split && !a.m_dev && (a.N & 63) == 0;
    WsplitChoice ch = choose_wsplit(a.M, a.N, a.K, cus, can_split, a.part_cap);
    // beyond the 32 x 32 tile's old range the 128 x 64 split-K route is as fast once the best wave-split shape needs a second
    // round of blocks (measured at 640 rows: N = 2304 / 3072 27.8 / 28.9 us against 28.9 / 30.0): those launches stay where they were
    const bool take = a.M <= t.skinny || ch.rounds <= 1 || t.wsplit_cfg >= 0;
    if (t.wsplit_cfg >= 0 && t.wsplit_cfg <= 2) ch.cfg = t.wsplit_cfg;
    if (t.wsplit_ks > 0 && (t.wsplit_ks == 1 || (can_split && (size_t)a.M * a.N * t.wsplit_ks <= a.part_cap && a.K / t.wsplit_ks >= 64))) ch.ks = t.wsplit_ks;
    if (take) return pl.add(wsplit_step(a, ch.cfg, ch.ks));
  }
  if (force == 0 && a.M <= t.skinny) return pl.add(skinny_step(a));
  const long t128 = ceil_tiles(a.M, a.N, 128, 128);
  // A few hundred to a few thousand rows in flight (beam 1000 with one query, beam 100 with a dozen, beam 10 with
  // 40-400): the 128x64 launch has fewer blocks than CUs and each walks all of K alone (24-96 K-tiles at ~1 us).
  // Split K over blockIdx.y into the caller's scratch and run the fused epilogue as its own launch.
  if (force == 0 && a.part && a.mid_split && !a.m_dev && (a.N & 63) == 0 && a.K >= 512) {
    const long ks = splitk_128x64(a, 3L * cus / 2, std::min(4, a.K / 128), a.K / HBK);
    if (ks > 1 && ceil_tiles(a.M, a.N, 128, 64) < cus) return pl.add(dma_step(a, t, 64, (int)ks, fused_reduce(a)));
  }
  // split-K: the caller lent scratch for partial results and the launch is a long reduction into few tiles
  if (a.part && a.K >= 2048 && t128 * 2 < t.splitk_target) {
    if (!a.mid_split && pp_splitk(a, t, pl)) return;
    if (!a.out_h && !a.ssq_out && !a.row_ssq && !a.relu && !a.resid_h && !a.m_dev && a.split_n >= a.N && (a.N & 3) == 0 && a.ldo0_al4 && a.ldr_al4) {
      const long ks = splitk_128x64(a, t.splitk_target, a.K / 1024, a.K / HBK);
      if (ks > 1) return pl.add(dma_step(a, t, 64, (int)ks, REDUCE_SUM));
    }
  }
  const bool narrow = force ? (force == 64) : (t128 < 256);
  pl.add(dma_step(a, t, narrow ? 64 : 128));
}

// Every row of the product is computed by the ping-pong kernel walking all of K in one block: the launches whose rows a
// table made by that kernel (passes.hip: the layer-0 Q/K/V table) reproduces bit for bit.
inline bool plan_is_pp_only(const GemmPlan& pl) {
  if (pl.invalid || pl.n < 1) return false;
  for (int i = 0; i < pl.n; ++i)
    if (pl.step[i].family != GEMM_PP || pl.step[i].ksplit != 1) return false;
  return true;
}

// Size policy of that table (internal.h: rpr_model::l0_table): L * V + 1 rows of q | k | v = 3 * inner fp32 values. A model
// whose table would exceed the cap keeps its GEMM: the cap admits t5-base at 32 x 256 (75 MB) and at 16 x 1024 (151 MB) and
// t5-large at 32 x 256 (101 MB); t5-3b at 32 x 256 (403 MB) is over it.
constexpr size_t L0_TABLE_CAP = (size_t)160 << 20;
inline size_t l0_table_rows(int L, int V) { return (size_t)L * (size_t)V + 1; }
inline size_t l0_table_bytes(int L, int V, int inner) { return l0_table_rows(L, V) * 3 * (size_t)inner * sizeof(float); }
inline bool l0_table_fits(int L, int V, int inner) { return l0_table_bytes(L, V, inner) <= L0_TABLE_CAP; }

inline GemmPlan plan_gemm_h2(const GemmRouteIn& a, const GemmTuning& t = GemmTuning()) {
  GemmPlan pl;
  if (a.M <= 0 || a.N <= 0) return pl;
  if (a.K % HBK != 0 || a.K <= 0 || !a.ab_al8) { pl.invalid = true; return pl; }
  if (!(a.m_dev && a.small_live > 0 && a.M > a.small_live && !a.bf16)) { route_one(a, t, pl); return pl; }
  // a compacted stage: capacity M rows, usually a handful alive. The large-tile kernel would walk all of K with the
  // one or two blocks that hold live rows (60-250 us per launch). The launch is enqueued as a group of three, each
  // gated on the device-side live count (two of them exit at once): the large-tile kernel for more than small_live
  // rows, a 128x64 launch sized for small_live rows, and the skinny tiles for at most `skinny` rows (a few leftover
  // queries: 10 us instead of 17-20 for the 128x64 tile walking K alone).
  GemmRouteIn big = a, mid = a, sk = a;
  const int sk_rows = std::min(t.skinny, a.small_live);
  big.small_live = 0; big.live_lo = a.small_live; big.live_hi = INT_MAX;
  mid.small_live = 0; mid.live_lo = sk_rows; mid.live_hi = a.small_live; mid.M = a.small_live;
  sk.small_live = 0; sk.live_lo = -1; sk.live_hi = sk_rows; sk.M = (sk_rows + 31) / 32 * 32;
  route_one(big, t, pl);
  if (pl.invalid) return pl;
  if (sk_rows < a.small_live) pl.add(dma_step(mid, t, 64));
  pl.add(skinny_step(sk));
  return pl;
}

// Tile order of launch_gemm_h2_group for n products of M[i] x N[i]: every product is cut into super-tiles (nearly equal
// parts of at most 4 tile rows / columns); the tiles in super-tile order are cut into 8 equal runs: every XCD gets the same
// number of tiles (the main stream's kernels run beside this launch and are spread evenly over the XCDs: whole super-tiles
// per XCD, 21 blocks on one XCD and 12 on another, slowed those by 10 %), a run is one or two super-tiles plus parts of its
// neighbours. Block b runs on XCD b % 8, so run x fills the slots x, x + 8, ..: entry = (product << 16) | tile, -1 = unused.
inline std::vector<int> group_tile_order(const int* M, const int* N, int n) {
  std::vector<int> order;
  for (int i = 0; i < n; ++i) {
    const int tm = (M[i] + 255) / 256, tn = (N[i] + 255) / 256;
    const int pm = (tm + 3) / 4, pn = (tn + 3) / 4, sm = (tm + pm - 1) / pm, sn = (tn + pn - 1) / pn;
    for (int a0 = 0; a0 < tm; a0 += sm)
      for (int b0 = 0; b0 < tn; b0 += sn)
        for (int a = a0; a < std::min(a0 + sm, tm); ++a)
          for (int b = b0; b < std::min(b0 + sn, tn); ++b) order.push_back((i << 16) | (a * tn + b));
  }
  const size_t total = order.size(), slots = (total + 7) / 8;   // (the longest of the 8 runs)
  std::vector<int> asg(slots * 8, -1);
  for (size_t x = 0; x < 8; ++x)
    for (size_t k = x * total / 8; k < (x + 1) * total / 8; ++k) asg[x + 8 * (k - x * total / 8)] = order[k];
  return asg;
}

}  // namespace rpr
