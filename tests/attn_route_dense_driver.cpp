// Prints the plan of every attention launch of the dense first-stage step (train_api.hip: dense_run = one teacher-forced pass over
// S = 3 bz sequences of Lt tokens with one decoder sequence of ONE position each) for tests/test_attn_route_dense.py:
//   plan <dkv> <Lt>      one line per launch: site | kernel invalid grid block smem, then "admitted <0|1>"     (bz 2 -> S 6, H 12)
// Sites: the forward without dropout (launch_enc_attn for both stacks, launch_tail_cross_attn), the backward with and without
// dropped-out probabilities, and the forward with dropout; the shapes are the ones forward() / backward() build.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../ripor_amd/csrc/attn_route.h"

using namespace rpr;

static void row(const char* site, const AttnLaunch& p) {
  printf("%s | %s %d %u %d %zu\n", site, attn_kernel_name(p.kernel), (int)p.invalid, p.grid_x, p.block, p.smem);
}

int main(int argc, char** argv) {
  if (argc != 4 || std::string(argv[1]) != "plan") return 2;
  const int dkv = atoi(argv[2]), Lt = atoi(argv[3]);
  const int S = 6, H = 12, buckets = 32, L = 1, docs = 1;
  EncAttnIn enc_fwd, dec_fwd;
  enc_fwd.Q = S; enc_fwd.Lq = Lt; enc_fwd.H = H; enc_fwd.buckets = buckets; enc_fwd.dkv = dkv; enc_fwd.mask = true; enc_fwd.mfma = true;
  dec_fwd.Q = S * docs; dec_fwd.Lq = L; dec_fwd.H = H; dec_fwd.buckets = buckets; dec_fwd.dkv = dkv; dec_fwd.causal = true; dec_fwd.mfma = true;
  row("enc_self_fwd", plan_enc_attn(enc_fwd));
  row("dec_self_fwd", plan_enc_attn(dec_fwd));
  row("cross_fwd", plan_tail_cross_attn(CrossAttnIn{S, docs * L, H, Lt, dkv}));
  for (const bool drop : {false, true}) {
    const TrainSelfAttnIn enc{S, Lt, H, buckets, dkv, false, true, drop, Lt}, dec{S * docs, L, H, buckets, dkv, true, false, drop, L};
    const TrainCrossAttnIn cross{S, docs * L, Lt, H, dkv, true, drop, L};
    row(drop ? "enc_self_bwd_drop" : "enc_self_bwd", plan_train_self_attn_bwd(enc));
    row(drop ? "dec_self_bwd_drop" : "dec_self_bwd", plan_train_self_attn_bwd(dec));
    row(drop ? "cross_bwd_drop" : "cross_bwd", plan_train_cross_attn_bwd(cross));
    if (drop) {
      row("enc_self_drop_fwd", plan_train_self_attn_drop_fwd(enc));
      row("dec_self_drop_fwd", plan_train_self_attn_drop_fwd(dec));
      row("cross_drop_fwd", plan_train_cross_attn_drop_fwd(cross));
    }
  }
  printf("admitted %d\n", (int)train_attn_admitted(S, Lt, L, docs, H, buckets, dkv));
  return 0;
}
