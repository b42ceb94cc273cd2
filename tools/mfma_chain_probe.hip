// Diagnostic (GPU box): does it pay to issue the three products of one accumulator (lo*hi, hi*lo, hi*hi) back to back, so
// that two of three C operands come from the matrix pipe's result forward instead of the register file? Registers only (no
// LDS, no memory traffic in the loop), random f16 operands, the register budget of the ping-pong GEMM's K-loop
// (ripor_amd/csrc/gemm_h2_pp_body.inc): 16 operand fragments of 8 halves and 128 accumulator registers per lane. One loop
// iteration = the two phases of a K-tile:
//   shape 16  v_mfma_f32_16x16x32_f16, 2 x 48 MFMAs: phase p = A tiles 4p .. 4p+3 against the four W tiles
//   shape 32  v_mfma_f32_32x32x16_f16, 2 x 24 MFMAs over the wave's 4 x 2 accumulators (12 of the 16 fragments)
// each in two orders:
//   (a) interleaved, the K-loop's order before this probe: all lo*hi, then all hi*lo, then all hi*hi of the phase; an
//       accumulator's three products are 16 (shape 16) / 8 (shape 32) MFMAs apart
//   (b) chained: per accumulator (i outer, j inner) lo*hi, hi*lo, hi*hi consecutively
// Both orders add the same products in the same order per accumulator: the checksums must agree bit for bit (printed).
// Every arm: >= 2 s of back-to-back launches of itself, then timed launches; TF/s from hipEvents and the in-kernel clock
// = delta s_memtime / delta s_memrealtime x 100 MHz (median over the waves; the stamps go to a buffer of their own).
// (a) and (b) alternate in one process, three rounds. Build and run: tools/mfma_chain_probe.sh
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CHECK(x)                                                                                         \
  do {                                                                                                   \
    hipError_t e_ = (x);                                                                                 \
    if (e_ != hipSuccess) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } \
  } while (0)

#define SB __builtin_amdgcn_sched_barrier(0)
#define MF16(a, b, c) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define MF32(a, b, c) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
// (a), shape 16: PP16_MMA16 / PP16_MMA48 of the K-loop, the fences where its DMA slots are
#define ROW16(A, i) MF16(A, wB0, acc16[i][0]); MF16(A, wB1, acc16[i][1]); MF16(A, wB2, acc16[i][2]); MF16(A, wB3, acc16[i][3]);
#define MMA16_A(i0, A0, A1, A2, A3, B0, B1, B2, B3)                                                      \
  {                                                                                                      \
    const f16x8 wB0 = B0, wB1 = B1, wB2 = B2, wB3 = B3;                                                  \
    ROW16(A0, (i0))                                                                                      \
    MF16(A1, wB0, acc16[(i0) + 1][0]); MF16(A1, wB1, acc16[(i0) + 1][1]);                                \
    SB;                                                                                                  \
    MF16(A1, wB2, acc16[(i0) + 1][2]); MF16(A1, wB3, acc16[(i0) + 1][3]);                                \
    ROW16(A2, (i0) + 2)                                                                                  \
    SB;                                                                                                  \
    ROW16(A3, (i0) + 3)                                                                                  \
    SB;                                                                                                  \
  }
#define MMA48_A(i0)                                                                                      \
  MMA16_A(i0, al[0], al[1], al[2], al[3], wh[0], wh[1], wh[2], wh[3])                                    \
  MMA16_A(i0, ah[0], ah[1], ah[2], ah[3], wl[0], wl[1], wl[2], wl[3])                                    \
  MMA16_A(i0, ah[0], ah[1], ah[2], ah[3], wh[0], wh[1], wh[2], wh[3])
// (b): one accumulator's three products, fenced so that the compiler keeps them together
#define TRIPLE16(i, ia, j) MF16(al[ia], wh[j], acc16[i][j]); MF16(ah[ia], wl[j], acc16[i][j]); MF16(ah[ia], wh[j], acc16[i][j]); SB;
#define ROW16_B(i, ia) TRIPLE16(i, ia, 0) TRIPLE16(i, ia, 1) TRIPLE16(i, ia, 2) TRIPLE16(i, ia, 3)
#define MMA48_B(i0) ROW16_B((i0), 0) ROW16_B((i0) + 1, 1) ROW16_B((i0) + 2, 2) ROW16_B((i0) + 3, 3)
// (a), shape 32: PP_MMA8 / PP_MMA24
#define MMA8_A(A, B0, B1)                                                                                \
  MF32(A[0], B0, acc32[0][0]); MF32(A[0], B1, acc32[0][1]); MF32(A[1], B0, acc32[1][0]);                 \
  SB;                                                                                                    \
  MF32(A[1], B1, acc32[1][1]); MF32(A[2], B0, acc32[2][0]); MF32(A[2], B1, acc32[2][1]);                 \
  SB;                                                                                                    \
  MF32(A[3], B0, acc32[3][0]); MF32(A[3], B1, acc32[3][1]);                                              \
  SB;
#define MMA24_A MMA8_A(al, wh[0], wh[1]) MMA8_A(ah, wl[0], wl[1]) MMA8_A(ah, wh[0], wh[1])
#define TRIPLE32(i, j) MF32(al[i], wh[j], acc32[i][j]); MF32(ah[i], wl[j], acc32[i][j]); MF32(ah[i], wh[j], acc32[i][j]); SB;
#define MMA24_B TRIPLE32(0, 0) TRIPLE32(0, 1) TRIPLE32(1, 0) TRIPLE32(1, 1) TRIPLE32(2, 0) TRIPLE32(2, 1) TRIPLE32(3, 0) TRIPLE32(3, 1)

// src: per thread 16 fragments of 8 halves (ah 0-3, al 0-3, wh 0-3, wl 0-3); stamps: per wave {memtime, memrealtime} before and
// after the loop; out: one checksum per thread
template <bool SHAPE16, bool CHAIN>
__global__ __launch_bounds__(512, 2) void chain_kernel(const _Float16* __restrict__ src, float* __restrict__ out,
                                                       unsigned long long* __restrict__ stamps, int iters) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  f16x8 ah[4], al[4], wh[4], wl[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ah[i] = *reinterpret_cast<const f16x8*>(src + ((size_t)tid * 16 + i) * 8);
    al[i] = *reinterpret_cast<const f16x8*>(src + ((size_t)tid * 16 + 4 + i) * 8);
    wh[i] = *reinterpret_cast<const f16x8*>(src + ((size_t)tid * 16 + 8 + i) * 8);
    wl[i] = *reinterpret_cast<const f16x8*>(src + ((size_t)tid * 16 + 12 + i) * 8);
    asm volatile("" : "+v"(ah[i]), "+v"(al[i]), "+v"(wh[i]), "+v"(wl[i]));   // in registers before the first stamp
  }
  f32x4 acc16[8][4];
  f32x16 acc32[4][2];
  if (SHAPE16) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc32[i][j][r] = 0.f;
  }
  SB;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): the fragments and the stamps are in
  SB;
  for (int it = 0; it < iters; ++it) {
    if (SHAPE16) {
      if (CHAIN) { MMA48_B(0) MMA48_B(4) } else { MMA48_A(0) MMA48_A(4) }
    } else {
      if (CHAIN) { MMA24_B MMA24_B } else { MMA24_A MMA24_A }
    }
    SB;
  }
  SB;
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  SB;
  float s = 0.f;
  if (SHAPE16) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) s += acc16[i][j][0] + acc16[i][j][1] + acc16[i][j][2] + acc16[i][j][3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc32[i][j][r];
  }
  out[tid] = s;
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* p = stamps + (size_t)(tid >> 6) * 4;
    p[0] = c0; p[1] = r0; p[2] = c1; p[3] = r1;
  }
}

typedef void (*kernel_t)(const _Float16*, float*, unsigned long long*, int);
static const int BLOCKS = 256;   // one block per CU

struct Arm { double tfs, ghz; unsigned checksum; };

static Arm run_arm(kernel_t k, bool shape16, int threads, int iters, const _Float16* d, float* o, unsigned long long* st) {
  const int waves = BLOCKS * threads / 64;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  // warm-up: back-to-back launches of this arm for >= 2 s (the queue is never empty: the next batch is enqueued before the
  // previous one is waited for), then the timed launches follow without a gap
  const auto t0 = std::chrono::steady_clock::now();
  hipEvent_t prev = nullptr;
  for (;;) {
    hipEvent_t ev; CHECK(hipEventCreate(&ev));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(k, dim3(BLOCKS), dim3(threads), 0, 0, d, o, st, iters / 4);
    CHECK(hipEventRecord(ev));
    if (prev) { CHECK(hipEventSynchronize(prev)); CHECK(hipEventDestroy(prev)); }
    prev = ev;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.2) break;
  }
  const int reps = 2;
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k, dim3(BLOCKS), dim3(threads), 0, 0, d, o, st, iters);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  CHECK(hipEventDestroy(prev));
  float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> hs((size_t)waves * 4);
  CHECK(hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> clk(waves);
  for (int w = 0; w < waves; ++w) clk[w] = (double)(hs[w * 4 + 2] - hs[w * 4 + 0]) / (double)(hs[w * 4 + 3] - hs[w * 4 + 1]) * 0.1;
  std::sort(clk.begin(), clk.end());
  std::vector<float> ho((size_t)BLOCKS * threads);
  CHECK(hipMemcpy(ho.data(), o, ho.size() * 4, hipMemcpyDeviceToHost));
  unsigned cs = 0;
  for (float v : ho) { unsigned b; memcpy(&b, &v, 4); cs = cs * 31u + b; }
  const double flop_per_iter = shape16 ? 96 * 2.0 * 16 * 16 * 32 : 48 * 2.0 * 32 * 32 * 16;
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  return {(double)waves * iters * reps * flop_per_iter / (ms * 1e-3) / 1e12, clk[waves / 2], cs};
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 160000;   // 1536 matrix-pipe cycles each: ~0.15 s (1 wave / SIMD) at 1.6 GHz
  const size_t n = (size_t)BLOCKS * 512 * 16 * 8;
  std::vector<_Float16> h(n);
  srand(1);
  for (size_t i = 0; i < n; ++i) {
    const float u = (float)rand() / RAND_MAX * 2.f - 1.f;
    const bool lo = ((i / 8) % 8) >= 4;                    // fragments 4-7 and 12-15 of a thread: the lo planes, 2^-11 of the hi ones
    h[i] = (_Float16)(lo ? u * 4.8828125e-4f : u);
  }
  _Float16* d; float* o; unsigned long long* st;
  CHECK(hipMalloc(&d, n * 2)); CHECK(hipMalloc(&o, (size_t)BLOCKS * 512 * 4)); CHECK(hipMalloc(&st, (size_t)BLOCKS * 8 * 4 * 8));
  CHECK(hipMemcpy(d, h.data(), n * 2, hipMemcpyHostToDevice));
  const kernel_t kern[2][2] = {{chain_kernel<false, false>, chain_kernel<false, true>}, {chain_kernel<true, false>, chain_kernel<true, true>}};
  printf("iterations %d per launch; TF/s = 2MNK of the MFMAs issued; clock = median over waves of d(s_memtime) / d(s_memrealtime) x 100 MHz\n", iters);
  printf("%-9s %-11s %5s | %-28s | %-28s | %s\n", "shape", "waves/SIMD", "round", "(a) interleaved  TF/s   GHz", "(b) chained      TF/s   GHz", "b/a    checksums");
  for (int s16 = 1; s16 >= 0; --s16)
    for (int threads = 256; threads <= 512; threads += 256) {
      double a_min = 1e30, a_max = 0, gain_min = 1e30;
      for (int round = 0; round < 3; ++round) {
        const Arm a = run_arm(kern[s16][0], s16, threads, iters, d, o, st);
        const Arm b = run_arm(kern[s16][1], s16, threads, iters, d, o, st);
        a_min = std::min(a_min, a.tfs); a_max = std::max(a_max, a.tfs); gain_min = std::min(gain_min, b.tfs - a.tfs);
        printf("%-9s %-11d %5d | %21.1f %6.3f | %21.1f %6.3f | %.4f %s\n", s16 ? "16x16x32" : "32x32x16", threads / 256, round, a.tfs, a.ghz,
               b.tfs, b.ghz, b.tfs / a.tfs, a.checksum == b.checksum ? "equal" : "DIFFERENT");
        fflush(stdout);
      }
      // the gate of the order change: (b) above (a) in every round by more than (a)'s own spread across the rounds
      printf("%-9s %-11d  gate | spread of (a) %.1f TF/s (%.2f %%); smallest (b) - (a) of a round %.1f TF/s -> %s\n", s16 ? "16x16x32" : "32x32x16",
             threads / 256, a_max - a_min, (a_max - a_min) / a_min * 100, gain_min, gain_min > a_max - a_min ? "PASS" : "fail");
    }
  return 0;
}
