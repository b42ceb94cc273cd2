// Route policy of the attention launches (t5_kernels.hip, attn_mfma.hip, train_kernels.hip): which kernel instantiation a
// shape takes, with which grid, block, dynamic LDS and scalar arguments. Plain host arithmetic — no HIP types, so the tests
// compile it with the host compiler and check the shape -> kernel table without a GPU (tests/test_attn_route.py the search
// sites, tests/test_attn_route_train.py the training step's). Every launch_* of an attention site fills the site's input struct,
// asks its planner and runs one switch over AttnLaunch::kernel:
//   search         launch_enc_attn, launch_dec_self_attn, launch_dec_cross_attn, launch_step_cross_attn, launch_tail_self_attn,
//                  launch_tail_cross_attn
//   training step  launch_enc_attn (mfma), launch_self_attn_bwd, launch_cross_attn_bwd, launch_self_attn_drop_fwd,
//                  launch_cross_attn_drop_fwd; train_setup admits a step by the same planners (train_attn_admitted)
#pragma once
#include <algorithm>
#include <cstddef>

namespace rpr {

constexpr int MAX_LQ = 256;          // encoder tokens per query supported by the attention kernels
constexpr int MAX_DEC_LEN = 64;      // decoder positions supported (reference uses 32 or 16)
constexpr int DKV = 64;              // head dim the fast attention kernels are written for (t5-base/large); d_kv = 128 (t5-3b) runs
                                     // on the generic kernels enc_attn_kernel<128> / dec_attn_kernel<., 128> without the forced tail,
                                     // its training attention on the <., 128> instantiations of train_kernels.hip
constexpr int SELF_MAXIT_MAX = 9;    // dec_self_attn_fast_kernel: 36 keys, covers L <= 35 (the reference uses L = 32 or 16)
constexpr int XK_LD = DKV + 4, QS_LD = DKV + 4;   // dec_cross_attn_block_kernel: K / q rows padded by 4 floats (68; 132 for 128-dim heads)
constexpr size_t LDS_MAX = 160 * 1024;            // LDS of a CU = the most a block may ask for
constexpr size_t LDS_CROSS128 = 96 * 1024;        // block cross-attention, 128-dim heads: beyond it the query's rows are chunked
constexpr size_t LDS_CROSS64 = 64 * 1024;         // ... 64-dim heads (two blocks per CU)
constexpr size_t LDS_TILE = 4 * (32 * 64) * sizeof(float);   // second-generation tiles: one 8-KB strip per wave

// Development switches (the product library runs the defaults; the development build fills them from the environment when
// it loads, attn_mfma.hip: g_attn_tuning).
struct AttnTuning {
  // RPR_TAIL_ATTN_GEN: generation of the fp32-MFMA tail attention. 1 = direct K / Q loads and V through LDS, 2 = scalar
  // bases, V straight into the P.V operand (bit-identical results); the encoder and step tiles exist in generation 2 only
  int gen = 2;
  int enc_mfma = 1;     // RPR_ENC_ATTN_MFMA: 0 = the search encoder stays on the VALU block kernel
  // RPR_STEP_CROSS_MFMA: 2 = the 16 x 16 tile kernel for at most 32 encoder positions, else the VALU block kernel; 1 = the
  // 32-row tile kernel of the tail (measured neutral at beam 10: 4969-4974 vs 4983 queries/s same-box, 10 of a tile's 32
  // rows are live); 0 = always the block kernel
  int step_cross = 2;
};

#define RPR_ATTN_KERNELS(X)                                                                                              \
  X(NONE)                                                                                                                \
  /* encoder / training self-attention forward */                                                                       \
  X(ENC_V2) X(ENC_VALU64) X(ENC_VALU128) X(ENC_VALU128_VG) X(TRAIN_SELF_MFMA)                                            \
  /* step self-attention: dec_self_attn_fast_kernel<n>, <n, 128>, dec_attn_kernel<true>, <true, 128> */                 \
  X(SELF_FAST2) X(SELF_FAST4) X(SELF_FAST6) X(SELF_FAST8) X(SELF_FAST9)                                                  \
  X(SELF_FAST4_D128) X(SELF_FAST8_D128) X(SELF_FAST12_D128) X(SELF_FAST18_D128) X(SELF_GENERIC) X(SELF_GENERIC_D128)     \
  /* block cross-attention: dec_cross_attn_block_kernel<64 / 128>, dec_attn_kernel<false, 128> */                       \
  X(CROSS_BLOCK64) X(CROSS_BLOCK128) X(CROSS_WAVE128)                                                                    \
  /* tail self-attention: v2<4>, first generation <1> / <2>, tail_self_attn_kernel<128> */                              \
  X(TAIL_SELF_V2) X(TAIL_SELF_G1_NKT1) X(TAIL_SELF_G1_NKT2) X(TAIL_SELF_VALU128)                                         \
  /* tail cross-attention: v2<9, 3, false> / <1, 4>, first generation <1> / <2> */                                      \
  X(TAIL_CROSS_V2_TPW9) X(TAIL_CROSS_V2_TPW1) X(TAIL_CROSS_G1_NKT1) X(TAIL_CROSS_G1_NKT2)                                \
  /* step cross-attention: step_cross_attn_mfma16_kernel<false> / <true> */                                             \
  X(STEP_CROSS16_ONE) X(STEP_CROSS16_MULTI)                                                                              \
  /* training self-attention backward: the fp32-MFMA tile, self_attn_bwd_kernel<., 64>, <., 128> */                     \
  X(TRAIN_BWD_MFMA) X(TRAIN_BWD_VALU) X(TRAIN_BWD_VALU128)                                                              \
  /* training attention beyond the one-head LDS carve: attn_bwd_tiled_kernel<bias>, attn_drop_fwd_tiled_kernel<bias> */ \
  X(TRAIN_SELF_BWD_TILED) X(TRAIN_CROSS_BWD_TILED) X(TRAIN_SELF_DROP_FWD_TILED) X(TRAIN_CROSS_DROP_FWD_TILED)           \
  /* training attention that holds a head in LDS: cross_attn_bwd_kernel<., 64>, <., 128>, self_attn_drop_fwd_kernel<64>, <128>, */ \
  /* cross_attn_drop_fwd_kernel<64>, <128> (appended: the ids above keep their values) */                               \
  X(TRAIN_CROSS_BWD) X(TRAIN_CROSS_BWD128) X(TRAIN_SELF_DROP_FWD) X(TRAIN_SELF_DROP_FWD128)                              \
  X(TRAIN_CROSS_DROP_FWD) X(TRAIN_CROSS_DROP_FWD128)

enum AttnKernel {
#define X(n) ATTN_##n,
  RPR_ATTN_KERNELS(X)
#undef X
};
#define X(n) +1
constexpr int ATTN_KERNEL_COUNT = 0 RPR_ATTN_KERNELS(X);
#undef X
inline const char* attn_kernel_name(int k) {
  static const char* const names[] = {
#define X(n) #n,
      RPR_ATTN_KERNELS(X)
#undef X
  };
  return names[k];
}

struct AttnLaunch {
  int kernel = ATTN_NONE;
  bool invalid = false;                 // the arguments are refused (hipErrorInvalidValue)
  unsigned grid_x = 0, grid_y = 1;
  int block = 256;
  size_t smem = 0;                      // dynamic LDS bytes
  int HB = 0;                           // blocks of four heads per (sequence / query / group)
  int groups = 0, tpw = 0, tiles = 0;   // row tiles of a query, tiles per wave, groups of tpw tiles
  int bchunk = 0;                       // block cross-attention: rows per block when a query's rows are split over blockIdx.y
};

inline AttnLaunch attn_invalid() { AttnLaunch p; p.invalid = true; return p; }
inline AttnLaunch attn_launch(int kernel, long grid_x, size_t smem) {
  AttnLaunch p;
  p.kernel = kernel; p.grid_x = (unsigned)grid_x; p.smem = smem;
  return p;
}

// udiv_magic (kernel_utils.h) divides x by d exactly for x < 2^32 / d: true when every x < n is in that range. The divisions of
// blockIdx.x by HB are held to 2^31.
inline bool magic_ok(long n, int d, int bits = 32) { return n < (1l << bits) / d; }
// the second-generation tiles address the rows of one query with 32-bit float offsets: rows x H x DKV stays under 2^29
inline bool offs32_ok(int rows, int H) { return (long)rows * H * DKV < (1l << 29); }
inline int head_blocks(int H) { return (H + 3) / 4; }

// ---- encoder / training self-attention forward (launch_enc_attn) ------------------------------------------------------------
struct EncAttnIn {
  int Q = 0, Lq = 0, H = 0, buckets = 0, dkv = 0;
  bool causal = false, mask = false, offs = false, out_h = false;   // mask / offs / out_h: the pointer is set
  bool mfma = false;                                                // EncAttnArgs::mfma (training forward)
};
inline size_t enc_attn_smem(int Lq, int D, bool stage_v = true) {
  return ((size_t)Lq * (D + 1) + (stage_v ? (size_t)Lq * D : 0) + 4 * (size_t)Lq + 2 * (size_t)Lq + 4 * 8 * (size_t)D + (size_t)Lq) * sizeof(float);
}
inline AttnLaunch plan_enc_attn(const EncAttnIn& a, const AttnTuning& t = AttnTuning()) {
  if (a.Lq > MAX_LQ || a.buckets > 64) return attn_invalid();
  const long blocks = (long)a.Q * a.H;   // the VALU kernel: one block per (query, head)
  if (a.dkv == 128) {   // t5-3b heads: the generic kernel only
    const size_t smem = enc_attn_smem(a.Lq, 128);
    if (smem <= LDS_MAX) return attn_launch(ATTN_ENC_VALU128, blocks, smem);   // Lq <= ~150: K and V of a head in LDS
    const size_t smem_k = enc_attn_smem(a.Lq, 128, false);   // up to MAX_LQ = 256 tokens: K in LDS (155 KB), V from global memory
    return smem_k > LDS_MAX ? attn_invalid() : attn_launch(ATTN_ENC_VALU128_VG, blocks, smem_k);
  }
  // training forward, at most 32 padded positions, fp32 output: one wave per (sequence, head), all keys in one tile
  if (a.mfma && a.Lq <= 32 && !a.offs && !a.out_h)
    return a.Lq < 1 ? attn_invalid() : attn_launch(ATTN_TRAIN_SELF_MFMA, (blocks + 3) / 4, 4 * (32 * 64 + 64) * sizeof(float));
  // the search encoder (bidirectional, key mask, packed or padded rows) at <= 32 positions: one wave per (query, head)
  const int HB = head_blocks(a.H);
  if (!a.mfma && t.enc_mfma && t.gen == 2 && !a.causal && a.mask && a.Lq <= 32 && magic_ok((long)a.Q * HB, HB, 31)) {
    AttnLaunch p = attn_launch(ATTN_ENC_V2, (long)a.Q * HB, LDS_TILE);
    p.HB = HB;
    return p;
  }
  return attn_launch(ATTN_ENC_VALU64, blocks, enc_attn_smem(a.Lq, 64));
}

// ---- self-attention of a sequential step (launch_dec_self_attn) -------------------------------------------------------------
// One wave per (beam, head); the fast kernel holds the t + 1 keys in SELF_MAXIT register groups of four keys (128-dim heads:
// of two). Early steps take the small instantiations: fewer VGPRs, 8 waves per SIMD instead of 4.
struct DecSelfAttnIn { int Q = 0, B = 0, H = 0, t = 0, dkv = 0; };
inline AttnLaunch plan_dec_self_attn(const DecSelfAttnIn& a) {
  const long items = (long)a.Q * a.B * a.H;
  if (!magic_ok(items, std::max(a.B, a.H))) return attn_invalid();
  const int nk = a.t + 1;
  int k;
  if (a.dkv == 128) {   // t5-3b heads; beyond 36 keys the generic one-wave-per-(beam, head) kernel
    if (nk > MAX_LQ) return attn_invalid();
    k = nk <= 8 ? ATTN_SELF_FAST4_D128 : nk <= 16 ? ATTN_SELF_FAST8_D128 : nk <= 24 ? ATTN_SELF_FAST12_D128 : nk <= 36 ? ATTN_SELF_FAST18_D128
                                                                                                                     : ATTN_SELF_GENERIC_D128;
  } else {
    k = nk <= 8 ? ATTN_SELF_FAST2 : nk <= 16 ? ATTN_SELF_FAST4 : nk <= 24 ? ATTN_SELF_FAST6 : nk <= 32 ? ATTN_SELF_FAST8
        : nk <= 4 * SELF_MAXIT_MAX ? ATTN_SELF_FAST9 : ATTN_SELF_GENERIC;
  }
  return attn_launch(k, (items + 3) / 4, 0);
}

// ---- cross-attention: the three sites share their shape ---------------------------------------------------------------------
struct CrossAttnIn { int Q = 0, B = 0, H = 0, Lq = 0, dkv = 0; };   // B = rows of a query: beams (step), beams x tail positions (tail)

// The block kernel (launch_dec_cross_attn): one block per (query, head) stages the head's K / V rows and the query's rows in
// LDS. When the rows of a query (a large beam; the tail pass: beams x remaining positions) pass the bar of the head dim,
// chunks of 64 rows or the largest smaller power of two under the bar go over blockIdx.y (K / V re-staged per chunk). When
// even the smallest chunk passes the LDS of a CU: 128-dim heads take one wave per (row, head) over the query's encoder rows,
// 64-dim heads are refused.
inline size_t cross_block_smem(int Lq, int D, int rows) {
  return ((size_t)Lq * ((D + 4) + D) + (size_t)rows * ((D + 4) + 2 * (Lq + 1)) + 4) * sizeof(float);
}
inline AttnLaunch plan_cross_block(const CrossAttnIn& a) {
  if (a.Lq > MAX_LQ) return attn_invalid();
  const int D = a.dkv == 128 ? 128 : DKV;
  const size_t bar = D == 128 ? LDS_CROSS128 : LDS_CROSS64;
  int bchunk = 0, chunks = 1;
  if (cross_block_smem(a.Lq, D, a.B) > bar) {
    bchunk = 64;
    while (bchunk > 1 && cross_block_smem(a.Lq, D, bchunk) > bar) bchunk >>= 1;
    chunks = (a.B + bchunk - 1) / bchunk;
  }
  const size_t smem = cross_block_smem(a.Lq, D, bchunk ? bchunk : a.B);
  if (smem > LDS_MAX) return D == 128 ? attn_launch(ATTN_CROSS_WAVE128, ((long)a.Q * a.B * a.H + 3) / 4, 0) : attn_invalid();
  AttnLaunch p = attn_launch(D == 128 ? ATTN_CROSS_BLOCK128 : ATTN_CROSS_BLOCK64, (long)a.Q * a.H, smem);
  p.grid_y = (unsigned)chunks; p.bchunk = bchunk;
  return p;
}

// Cross-attention of the tail rows (launch_tail_cross_attn): fp32-MFMA tiles of 32 rows for at most 64 encoder positions
// and 64-dim heads, else the block kernel (any Lq <= 256).
inline AttnLaunch plan_tail_cross_attn(const CrossAttnIn& a, const AttnTuning& t = AttnTuning()) {
  if (a.Lq > 64 || a.dkv == 128) return plan_cross_block(a);
  const int tiles = (a.B + 31) / 32;
  const long waves = (long)a.Q * a.H * tiles;
  if (t.gen == 2 && a.Lq <= 32) {
    // tiles per wave: many tiles (32768 waves of one) -> a wave keeps K / V for nine of them (fewer, longer waves: better on a
    // lane's half of the chip); few -> one tile per wave (more waves to fill the chip)
    const int tpw = waves >= 32768 ? 9 : 1;
    const int groups = (tiles + tpw - 1) / tpw, HB = head_blocks(a.H);
    const long blocks = (long)a.Q * groups * HB;
    if (magic_ok(blocks, HB, 31) && magic_ok((long)a.Q * groups, groups) && offs32_ok(a.B, a.H)) {
      // nine tiles per wave: three waves per SIMD, no second Q register set (658 vs 673 us per lane launch)
      AttnLaunch p = attn_launch(tpw == 9 ? ATTN_TAIL_CROSS_V2_TPW9 : ATTN_TAIL_CROSS_V2_TPW1, blocks, LDS_TILE);
      p.HB = HB; p.groups = groups; p.tpw = tpw; p.tiles = tiles;
      return p;
    }
  }
  // first generation: one wave per (query, head, tile), V rows of NKT key tiles in LDS
  AttnLaunch p = a.Lq <= 32 ? attn_launch(ATTN_TAIL_CROSS_G1_NKT1, (waves + 3) / 4, 4 * 32 * 64 * sizeof(float))
                            : attn_launch(ATTN_TAIL_CROSS_G1_NKT2, (waves + 3) / 4, 4 * 64 * 64 * sizeof(float));
  p.tiles = tiles;
  return p;
}

// Cross-attention of a sequential step (launch_step_cross_attn), a.B = the beams of a query.
inline AttnLaunch plan_step_cross_attn(const CrossAttnIn& a, const AttnTuning& t = AttnTuning()) {
  if (a.dkv == 128) return plan_cross_block(a);   // t5-3b heads: the generic kernel
  if (t.step_cross == 2 && t.gen == 2 && a.Lq <= 32 && offs32_ok(a.B, a.H)) {
    // 16-row tiles per wave: one while that gives the chip enough waves, else up to eight (K / V / mask loaded once per wave)
    const int tiles = (a.B + 15) / 16, HB = head_blocks(a.H);
    const int tpw = (long)a.Q * a.H * tiles >= 32768 ? std::min(tiles, 8) : 1;
    const int groups = (tiles + tpw - 1) / tpw;
    const long blocks = (long)a.Q * groups * HB;
    if (magic_ok(blocks, HB, 31) && magic_ok((long)a.Q * groups, groups)) {
      // at most 16 beams: one tile, no tile loop (35.0 against 37.5 us per lane launch at beam 10)
      AttnLaunch p = attn_launch(tiles == 1 ? ATTN_STEP_CROSS16_ONE : ATTN_STEP_CROSS16_MULTI, blocks, 4 * (16 * 68) * sizeof(float));
      p.HB = HB; p.groups = groups; p.tpw = tpw; p.tiles = tiles;
      return p;
    }
  }
  if (t.step_cross == 1 && t.gen == 2 && a.Lq <= 32) return plan_tail_cross_attn(a, t);
  return plan_cross_block(a);
}

// ---- self-attention of the tail pass (launch_tail_self_attn) ----------------------------------------------------------------
struct TailSelfAttnIn { int nseq_cap = 0, B = 0, H = 0, T = 0, L = 0, dkv = 0; };
inline size_t tail_self_attn_smem(int L, int D) { return ((size_t)L * (D + 1) + (size_t)L * D + 4 * 64 + 64) * sizeof(float); }
inline AttnLaunch plan_tail_self_attn(const TailSelfAttnIn& a, const AttnTuning& t = AttnTuning()) {
  if (a.L > MAX_DEC_LEN || a.T < 1 || a.T >= a.L) return attn_invalid();
  // t5-3b heads: the VALU kernel, one block per (sequence, head) (the MFMA tiles are written for 64-dim heads)
  if (a.dkv == 128) return attn_launch(ATTN_TAIL_SELF_VALU128, (long)a.nseq_cap * a.H, tail_self_attn_smem(a.L, 128));
  if (t.gen == 2 && a.L <= 32 && a.T <= 8) {   // every search of the bench's kind: a block = four heads of one sequence
    const int HB = head_blocks(a.H);
    const long blocks = (long)a.nseq_cap * HB;
    if (magic_ok(blocks, HB, 31) && magic_ok(a.nseq_cap, a.B)) {
      AttnLaunch p = attn_launch(ATTN_TAIL_SELF_V2, blocks, LDS_TILE);
      p.HB = HB;
      return p;
    }
  }
  // first generation: one wave per (sequence, head); per wave the V rows of ceil(L / 32) key tiles, the bias table and, with
  // two key tiles (a sequence may have more than one tile of 32 tail rows), a separate 32 x 64 output strip
  const long grid = ((long)a.nseq_cap * a.H + 3) / 4;
  return a.L <= 32 ? attn_launch(ATTN_TAIL_SELF_G1_NKT1, grid, 4 * (32 * 64 + 64) * sizeof(float))
                   : attn_launch(ATTN_TAIL_SELF_G1_NKT2, grid, 4 * (64 * 64 + 64 + 32 * 64) * sizeof(float));
}

// ---- the attention of the training step: the pieces (the planners of its four sites follow) ---------------------------------
// the resident plan of the self-attention backward without dropout
struct SelfAttnBwdIn { int S = 0, Ls = 0, H = 0, buckets = 0, dkv = DKV; };
// LDS of the VALU kernel (self_attn_bwd_kernel: rows padded to DKV + 1 floats); the training step is admitted by it whatever
// the kernel (train_api.hip). buckets <= 64: fixed slot. 128-dim heads (t5-3b) go through the same carve 64 columns at a time
// (129-float rows would need 4 * 64 * 129 + 2 * 64 * 65 + 5 * 64 + 64 = 41 728 floats at Ls = 64 against the 40 960 of a CU), so
// the lengths admitted do not depend on the head dim
inline size_t self_attn_bwd_smem(int Ls, int /*buckets*/) {
  return ((size_t)4 * Ls * (DKV + 1) + 2 * (size_t)Ls * (Ls + 1) + 64 + 5 * (size_t)Ls) * sizeof(float);
}
inline AttnLaunch plan_self_attn_bwd(const SelfAttnBwdIn& a) {
  const size_t smem = self_attn_bwd_smem(a.Ls, a.buckets);
  if (smem > LDS_MAX || a.buckets > 64 || a.Ls < 1 || (a.dkv != DKV && a.dkv != 128)) return attn_invalid();
  if (a.dkv == 128) return attn_launch(ATTN_TRAIN_BWD_VALU128, (long)a.S * a.H, smem);   // the MFMA plan is a 64-dim tile
  if (a.Ls <= 32) {   // one wave per (sequence, head) on the fp32 matrix cores, two waves per block
    AttnLaunch p = attn_launch(ATTN_TRAIN_BWD_MFMA, ((long)a.S * a.H + 1) / 2, 2 * (3 * 32 * 64 + 64 + 96 + 64 + 64) * sizeof(float));
    p.block = 128;
    return p;
  }
  return attn_launch(ATTN_TRAIN_BWD_VALU, (long)a.S * a.H, smem);
}

// ---- training attention beyond the one-head carve (attn_mfma.hip: attn_bwd_tiled_kernel, attn_drop_fwd_tiled_kernel) ---------
// 64-dim heads, up to MAX_LQ query rows and MAX_LQ keys per (sequence, head), bidirectional; the planners of the sites come here
// only when the plan above (self-attention) or the resident carve below (cross-attention) refuses the shape.
// One block of four waves per (sequence, head); queries and keys in 32-row tiles, nothing of the head resident:
//   per wave    two 32 x 64 strips (the tile pair of the moment: K | V, then Q | dO)       4096 floats
//               backward with a relative bias: its query tile's 2 MAX_LQ diagonals of dS     512
//   per block   row maximum, 1 / row sum, rowsum(dP P) of MAX_LQ queries                      768
//               key mask [MAX_LQ]                                                              256
//               with a relative bias: bias per diagonal and the diagonal sums, 2 x 512       1024
// self backward 4 (4096 + 512) + 768 + 256 + 1024 = 20 480 floats = 81 920 B (two blocks per CU); cross backward
// 4 x 4096 + 768 + 256 = 17 408 floats = 69 632 B; the forward needs no statistics: 4 x 4096 + 256 (+ 512) floats.
constexpr int TILED_WAVES = 4, TILED_STRIPS = 2 * 32 * DKV, TILED_DIAGS = 2 * MAX_LQ;
inline size_t attn_tiled_smem(bool bias, bool bwd) {
  return ((size_t)TILED_WAVES * (TILED_STRIPS + (bias && bwd ? TILED_DIAGS : 0)) + (bwd ? 3 * MAX_LQ : 0) + MAX_LQ +
          (bias ? (bwd ? 2 : 1) * TILED_DIAGS : 0)) * sizeof(float);
}
inline AttnLaunch plan_attn_tiled(int kernel, long S, int nq, int nk, int H, int buckets, int dkv, bool bias, bool bwd) {
  if (dkv != DKV || nq < 1 || nk < 1 || nq > MAX_LQ || nk > MAX_LQ || buckets > 64 || S < 1 || H < 1) return attn_invalid();
  return attn_launch(kernel, S * H, attn_tiled_smem(bias, bwd));   // block = 256 (AttnLaunch's default)
}
inline AttnLaunch plan_self_attn_bwd_tiled(const SelfAttnBwdIn& a) {
  return plan_attn_tiled(ATTN_TRAIN_SELF_BWD_TILED, a.S, a.Ls, a.Ls, a.H, a.buckets, a.dkv, true, true);
}
inline AttnLaunch plan_self_attn_drop_fwd_tiled(const SelfAttnBwdIn& a) {
  return plan_attn_tiled(ATTN_TRAIN_SELF_DROP_FWD_TILED, a.S, a.Ls, a.Ls, a.H, a.buckets, a.dkv, true, false);
}
// cross-attention of the training step: n = docs x L decoder rows of a query against its Lq encoder keys
struct CrossAttnBwdIn { int bz = 0, n = 0, Lq = 0, H = 0, dkv = DKV; };
// the carve of cross_attn_bwd_kernel / cross_attn_drop_fwd_kernel: q, dO [n][65], K, V [Lq][65], P, dS [n][Lq + 1], key mask [Lq]
inline size_t cross_attn_bwd_carve(int n, int Lq) {
  return ((size_t)2 * n * (DKV + 1) + 2 * (size_t)Lq * (DKV + 1) + 2 * (size_t)n * (Lq + 1) + (size_t)Lq) * sizeof(float);
}
inline bool cross_attn_bwd_resident(int n, int Lq) { return cross_attn_bwd_carve(n, Lq) <= LDS_MAX; }
inline AttnLaunch plan_cross_attn_bwd_tiled(const CrossAttnBwdIn& a) {
  return plan_attn_tiled(ATTN_TRAIN_CROSS_BWD_TILED, a.bz, a.n, a.Lq, a.H, 0, a.dkv, false, true);
}
inline AttnLaunch plan_cross_attn_drop_fwd_tiled(const CrossAttnBwdIn& a) {
  return plan_attn_tiled(ATTN_TRAIN_CROSS_DROP_FWD_TILED, a.bz, a.n, a.Lq, a.H, 0, a.dkv, false, false);
}


// ---- the four attention sites of the training step (train_kernels.hip) -------------------------------------------------------
// The self- and the cross-attention backward (launch_self_attn_bwd, launch_cross_attn_bwd) and, with dropout, the forward of both
// (launch_self_attn_drop_fwd, launch_cross_attn_drop_fwd; without dropout the forward is launch_enc_attn / launch_dec_cross_attn
// above). Each has a resident route, one block per (sequence or query, head) that holds the whole head in LDS, and beyond that
// carve, for 64-dim heads, the 32-row tiles. The template booleans of a kernel (DROP, CAUSAL, BIAS) are read from the input struct
// by the launcher's switch and have no names here.
struct TrainSelfAttnIn {
  int S = 0, Ls = 0, H = 0, buckets = 0, dkv = DKV;
  bool causal = false, mask = false;   // mask: the key-mask pointer is set
  bool drop = false;                   // backward: the probabilities were dropped out (the drop-forward always drops)
  int drop_L = 0;                      // DropAttn::L, positions per sequence of the mask's coordinates
};
struct TrainCrossAttnIn {
  int bz = 0, n = 0, Lq = 0, H = 0, dkv = DKV;
  bool mask = false, drop = false;
  int drop_L = 0;
};
inline SelfAttnBwdIn self_shape(const TrainSelfAttnIn& a) { return SelfAttnBwdIn{a.S, a.Ls, a.H, a.buckets, a.dkv}; }
inline CrossAttnBwdIn cross_shape(const TrainCrossAttnIn& a) { return CrossAttnBwdIn{a.bz, a.n, a.Lq, a.H, a.dkv}; }
inline bool train_dkv_ok(int dkv) { return dkv == DKV || dkv == 128; }
// what the tiles ask beyond their shape: a key mask and, with dropout, query rows that are whole sequences of drop_L positions (the
// coordinates the mask is drawn by)
inline AttnLaunch tiled_if(const AttnLaunch& p, bool mask, bool drop, int drop_L, int nq) {
  return !mask || (drop && (drop_L < 1 || nq % drop_L)) ? attn_invalid() : p;
}

// Self-attention backward: the resident plan; with dropped-out probabilities the VALU kernel in place of the MFMA tile, which knows
// no mask; where the carve refuses a bidirectional launch (Ls > 91), the tiles.
inline AttnLaunch plan_train_self_attn_bwd(const TrainSelfAttnIn& a) {
  const AttnLaunch p = plan_self_attn_bwd(self_shape(a));
  const size_t smem = self_attn_bwd_smem(a.Ls, a.buckets);
  if (p.invalid) return a.causal || smem <= LDS_MAX ? p : tiled_if(plan_self_attn_bwd_tiled(self_shape(a)), a.mask, a.drop, a.drop_L, a.Ls);
  return a.drop && p.kernel == ATTN_TRAIN_BWD_MFMA ? attn_launch(ATTN_TRAIN_BWD_VALU, (long)a.S * a.H, smem) : p;
}

// Self-attention forward with dropped-out probabilities. The resident kernel asks for the backward's carve (the step was admitted
// by it, and the request sets how many blocks share a CU) and draws its mask whatever drop_L is.
inline AttnLaunch plan_train_self_attn_drop_fwd(const TrainSelfAttnIn& a) {
  const size_t smem = self_attn_bwd_smem(a.Ls, a.buckets);
  if (smem > LDS_MAX && a.dkv == DKV && !a.causal && a.mask) return tiled_if(plan_self_attn_drop_fwd_tiled(self_shape(a)), a.mask, true, a.drop_L, a.Ls);
  if (smem > LDS_MAX || a.buckets > 64 || a.Ls < 1 || a.Ls > MAX_LQ || (!a.causal && !a.mask) || !train_dkv_ok(a.dkv)) return attn_invalid();
  return attn_launch(a.dkv == 128 ? ATTN_TRAIN_SELF_DROP_FWD128 : ATTN_TRAIN_SELF_DROP_FWD, (long)a.S * a.H, smem);
}

// Cross-attention, backward (fwd = false) or forward with dropped-out probabilities. Row r of a query is position r % drop_L of its
// decoder sequence r / drop_L; the resident backward's lanes carry the keep bits of 32 keys each, of MAX_LQ keys at most.
inline AttnLaunch plan_train_cross_attn(const TrainCrossAttnIn& a, bool fwd) {
  const size_t smem = cross_attn_bwd_carve(a.n, a.Lq);
  const bool drop = fwd || a.drop;
  if (smem > LDS_MAX)
    return a.dkv != DKV ? attn_invalid()
                        : tiled_if(fwd ? plan_cross_attn_drop_fwd_tiled(cross_shape(a)) : plan_cross_attn_bwd_tiled(cross_shape(a)), a.mask, drop,
                                   a.drop_L, a.n);
  if (!train_dkv_ok(a.dkv) || (drop && (a.drop_L < 1 || a.n % a.drop_L)) || (!fwd && drop && a.Lq > MAX_LQ)) return attn_invalid();
  const int k = fwd ? (a.dkv == 128 ? ATTN_TRAIN_CROSS_DROP_FWD128 : ATTN_TRAIN_CROSS_DROP_FWD)
                    : (a.dkv == 128 ? ATTN_TRAIN_CROSS_BWD128 : ATTN_TRAIN_CROSS_BWD);
  return attn_launch(k, (long)a.bz * a.H, smem);
}
inline AttnLaunch plan_train_cross_attn_bwd(const TrainCrossAttnIn& a) { return plan_train_cross_attn(a, false); }
inline AttnLaunch plan_train_cross_attn_drop_fwd(const TrainCrossAttnIn& a) { return plan_train_cross_attn(a, true); }

// A training step (train_api.hip: train_setup) is admitted when every attention launch it will make has a plan, with and without
// dropout: the encoder's self-attention over bz queries of Lq tokens (bidirectional, key mask), the decoder's over bz x docs
// sequences of L codes (causal) and the cross-attention of a query's docs x L rows against its Lq keys.
inline bool train_attn_admitted(int bz, int Lq, int L, int docs, int H, int buckets, int dkv) {
  for (const bool drop : {false, true}) {
    const TrainSelfAttnIn enc{bz, Lq, H, buckets, dkv, false, true, drop, Lq}, dec{bz * docs, L, H, buckets, dkv, true, false, drop, L};
    const TrainCrossAttnIn cross{bz, docs * L, Lq, H, dkv, true, drop, L};
    if (plan_train_self_attn_bwd(enc).invalid || plan_train_self_attn_bwd(dec).invalid || plan_train_cross_attn_bwd(cross).invalid) return false;
    if (drop && (plan_train_self_attn_drop_fwd(enc).invalid || plan_train_self_attn_drop_fwd(dec).invalid ||
                 plan_train_cross_attn_drop_fwd(cross).invalid))
      return false;
  }
  return true;
}

}  // namespace rpr
