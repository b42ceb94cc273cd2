// Prints the launch plan of an attention site (ripor_amd/csrc/attn_route.h) for tests/test_attn_route.py.
//   site key=value ...      one JSON object: the plan for these inputs / tuning overrides (gen, enc_mfma, step_cross)
//   sites: enc, dec_self, cross_block, tail_self, tail_cross, step_cross, bwd, and the four of the training step:
//          train_self_bwd, train_self_drop_fwd, train_cross_bwd, train_cross_drop_fwd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ripor_amd/csrc/attn_route.h"

using namespace rpr;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string site = argv[1];
  EncAttnIn e;
  DecSelfAttnIn ds;
  CrossAttnIn c;
  TailSelfAttnIn ts;
  SelfAttnBwdIn b;
  TrainSelfAttnIn tsf;
  TrainCrossAttnIn tc;
  AttnTuning t;
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    const std::string k(argv[i], eq - argv[i]);
    const long long v = atoll(eq + 1);
    bool ok = false;
#define F(obj, name) if (k == #name) { obj.name = static_cast<decltype(obj.name)>(v); ok = true; }
    F(t, gen) F(t, enc_mfma) F(t, step_cross)
    if (site == "enc") { F(e, Q) F(e, Lq) F(e, H) F(e, buckets) F(e, dkv) F(e, causal) F(e, mask) F(e, offs) F(e, out_h) F(e, mfma) }
    if (site == "dec_self") { F(ds, Q) F(ds, B) F(ds, H) F(ds, t) F(ds, dkv) }
    if (site == "cross_block" || site == "tail_cross" || site == "step_cross") { F(c, Q) F(c, B) F(c, H) F(c, Lq) F(c, dkv) }
    if (site == "tail_self") { F(ts, nseq_cap) F(ts, B) F(ts, H) F(ts, T) F(ts, L) F(ts, dkv) }
    if (site == "bwd") { F(b, S) F(b, Ls) F(b, H) F(b, buckets) }
    if (site == "train_self_bwd" || site == "train_self_drop_fwd") {
      F(tsf, S) F(tsf, Ls) F(tsf, H) F(tsf, buckets) F(tsf, dkv) F(tsf, causal) F(tsf, mask) F(tsf, drop) F(tsf, drop_L)
    }
    if (site == "train_cross_bwd" || site == "train_cross_drop_fwd") {
      F(tc, bz) F(tc, n) F(tc, Lq) F(tc, H) F(tc, dkv) F(tc, mask) F(tc, drop) F(tc, drop_L)
    }
#undef F
    if (!ok) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
  }
  AttnLaunch p;
  if (site == "enc") p = plan_enc_attn(e, t);
  else if (site == "dec_self") p = plan_dec_self_attn(ds);
  else if (site == "cross_block") p = plan_cross_block(c);
  else if (site == "tail_cross") p = plan_tail_cross_attn(c, t);
  else if (site == "step_cross") p = plan_step_cross_attn(c, t);
  else if (site == "tail_self") p = plan_tail_self_attn(ts, t);
  else if (site == "bwd") p = plan_self_attn_bwd(b);
  else if (site == "train_self_bwd") p = plan_train_self_attn_bwd(tsf);
  else if (site == "train_self_drop_fwd") p = plan_train_self_attn_drop_fwd(tsf);
  else if (site == "train_cross_bwd") p = plan_train_cross_attn_bwd(tc);
  else if (site == "train_cross_drop_fwd") p = plan_train_cross_attn_drop_fwd(tc);
  else return 2;
  printf("{\"kernel\": \"%s\", \"invalid\": %d, \"grid\": [%u, %u], \"block\": %d, \"smem\": %zu, \"HB\": %d, \"groups\": %d, \"tpw\": %d, "
         "\"tiles\": %d, \"bchunk\": %d}\n",
         attn_kernel_name(p.kernel), (int)p.invalid, p.grid_x, p.grid_y, p.block, p.smem, p.HB, p.groups, p.tpw, p.tiles, p.bchunk);
  return 0;
}
