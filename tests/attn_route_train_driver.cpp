// Prints the plans of the training step's four attention sites (ripor_amd/csrc/attn_route.h: plan_train_*, train_attn_admitted)
// for tests/test_attn_route_train.py, a whole grid in one process.
//   sweep self | cross | admit      one line per shape:
//          self   site Ls dkv causal mask drop drop_L buckets | kernel invalid grid block smem      (S 2, H 12)
//          cross  site n Lq dkv mask drop drop_L | kernel invalid grid block smem                   (bz 2, H 12)
//          admit  dkv docs L Lq buckets | admitted                                                  (bz 2, H 12)
#include <cstdio>
#include <string>

#include "../ripor_amd/csrc/attn_route.h"

using namespace rpr;

static void row(const AttnLaunch& p) {
  printf("%s %d %u %d %zu\n", attn_kernel_name(p.kernel), (int)p.invalid, p.grid_x, p.block, p.smem);
}

static int sweep(const std::string& what) {
  const int dkvs[] = {32, 64, 128};
  if (what == "self") {
    const int buckets[] = {32, 64, 65};
    for (int Ls = 0; Ls <= 258; ++Ls)
      for (int dkv : dkvs)
        for (int causal = 0; causal < 2; ++causal)
          for (int mask = 0; mask < 2; ++mask)
            for (int drop = 0; drop < 2; ++drop)
              for (int drop_L : {0, Ls, 7})
                for (int b : buckets) {
                  const TrainSelfAttnIn a{2, Ls, 12, b, dkv, causal != 0, mask != 0, drop != 0, drop_L};
                  printf("self_bwd %d %d %d %d %d %d %d | ", Ls, dkv, causal, mask, drop, drop_L, b);
                  row(plan_train_self_attn_bwd(a));
                  printf("self_drop_fwd %d %d %d %d %d %d %d | ", Ls, dkv, causal, mask, drop, drop_L, b);
                  row(plan_train_self_attn_drop_fwd(a));
                }
    return 0;
  }
  if (what == "cross") {
    for (int n : {1, 8, 16, 32, 64, 128, 256, 257})
      for (int Lq = 1; Lq <= 258; ++Lq)
        for (int dkv : dkvs)
          for (int mask = 0; mask < 2; ++mask)
            for (int drop = 0; drop < 2; ++drop)
              for (int drop_L : {0, 8, 7}) {
                const TrainCrossAttnIn a{2, n, Lq, 12, dkv, mask != 0, drop != 0, drop_L};
                printf("cross_bwd %d %d %d %d %d %d | ", n, Lq, dkv, mask, drop, drop_L);
                row(plan_train_cross_attn_bwd(a));
                printf("cross_drop_fwd %d %d %d %d %d %d | ", n, Lq, dkv, mask, drop, drop_L);
                row(plan_train_cross_attn_drop_fwd(a));
              }
    return 0;
  }
  if (what == "admit") {
    for (int dkv : {64, 128})
      for (int docs : {1, 2, 4, 8})
        for (int L : {1, 8, 32, 64})
          for (int Lq = 1; Lq <= 256; ++Lq)
            for (int b : {2, 32, 64})
              printf("%d %d %d %d %d | %d\n", dkv, docs, L, Lq, b, (int)train_attn_admitted(2, Lq, L, docs, 12, b, dkv));
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) { return argc == 3 && std::string(argv[1]) == "sweep" ? sweep(argv[2]) : 2; }
