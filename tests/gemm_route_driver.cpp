// Prints the route plan of the split-precision GEMM (ripor_amd/csrc/gemm_route.h) for tests/test_gemm_route.py.
//   plan  key=value ...          one JSON object: the plan for these inputs / tuning overrides
//   sweep key=value ...          for N in {256, 768, 2304, 3072}, K in {768, 3072}, M in 1..60000 one line
//                                "M N K invalid n" + per step "rows m_base live_lo live_hi ksplit"
//   group M:N ...                the assignment vector of launch_gemm_h2_group, one line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ripor_amd/csrc/gemm_route.h"

using namespace rpr;

static bool set_field(GemmRouteIn& a, GemmTuning& t, const std::string& k, long long v) {
#define F(obj, name) if (k == #name) { obj.name = static_cast<decltype(obj.name)>(v); return true; }
  F(a, M) F(a, N) F(a, K) F(a, cus) F(a, split_n) F(a, rm_B) F(a, ksplit) F(a, small_live) F(a, live_lo) F(a, live_hi) F(a, part_cap)
  F(a, part) F(a, mid_split) F(a, m_dev) F(a, bf16) F(a, no_row_split) F(a, out_h) F(a, row_ssq) F(a, ssq_out) F(a, resid) F(a, resid_h)
  F(a, relu) F(a, out_b) F(a, out_bt) F(a, ab_al8) F(a, ldo0_al4) F(a, ldr_al4) F(a, epi_al4) F(a, outb_al)
  F(t, force_tile) F(t, row_split) F(t, row_split_log) F(t, wsplit_max) F(t, wsplit_cfg) F(t, wsplit_ks) F(t, supertile)
#undef F
  return false;
}

static int parse(int argc, char** argv, GemmRouteIn& a, GemmTuning& t) {
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq || !set_field(a, t, std::string(argv[i], eq - argv[i]), atoll(eq + 1))) { fprintf(stderr, "bad argument %s\n", argv[i]); return 1; }
  }
  if (a.split_n == 0) a.split_n = a.N;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  GemmRouteIn a;
  GemmTuning t;
  if (mode == "group") {
    int M[64], N[64], n = 0;
    for (int i = 2; i < argc && n < 64; ++i, ++n)
      if (sscanf(argv[i], "%d:%d", &M[n], &N[n]) != 2) return 2;
    for (int v : group_tile_order(M, N, n)) printf("%d ", v);
    printf("\n");
    return 0;
  }
  if (parse(argc, argv, a, t)) return 2;
  if (mode == "plan") {
    static const char* fam[] = {"skinny16", "wsplit", "dma", "pp"};
    static const char* red[] = {"none", "sum", "fused", "fused4"};
    const GemmPlan p = plan_gemm_h2(a, t);
    printf("{\"invalid\": %d, \"cls\": \"%s\", \"steps\": [", (int)p.invalid, p.cls == RPR_K_GEMM ? "gemm" : "gemm_small");
    for (int i = 0; i < p.n; ++i) {
      const GemmStep& s = p.step[i];
      printf("%s{\"family\": \"%s\", \"bm\": %d, \"bn\": %d, \"stages\": %d, \"full\": %d, \"bf16\": %d, \"rows\": %d, \"m_base\": %d, "
             "\"live_lo\": %d, \"live_hi\": %d, \"ksplit\": %d, \"reduce\": \"%s\", \"tile_cw\": %d, \"tile_rb\": %d, \"tiles_m\": %d, "
             "\"tiles_n\": %d, \"grid\": [%d, %d], \"block\": %d}",
             i ? ", " : "", fam[s.family], s.bm, s.bn, s.stages, (int)s.full, (int)s.bf16, s.rows, s.m_base, s.live_lo, s.live_hi, s.ksplit,
             red[s.reduce], s.tile_cw, s.tile_rb, s.tiles_m, s.tiles_n, s.grid_x, s.grid_y, s.block);
    }
    printf("]}\n");
    return 0;
  }
  if (mode == "sweep") {
    const int Ns[] = {256, 768, 2304, 3072}, Ks[] = {768, 3072};
    for (int N : Ns)
      for (int K : Ks)
        for (int M = 1; M <= 60000; ++M) {
          a.M = M; a.N = N; a.K = K; a.split_n = N;
          const GemmPlan p = plan_gemm_h2(a, t);
          printf("%d %d %d %d %d", M, N, K, (int)p.invalid, p.n);
          for (int i = 0; i < p.n; ++i)
            printf(" %d %d %d %d %d", p.step[i].rows, p.step[i].m_base, p.step[i].live_lo, p.step[i].live_hi, p.step[i].ksplit);
          printf("\n");
        }
    return 0;
  }
  return 2;
}
