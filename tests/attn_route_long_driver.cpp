// Prints the plans of the training attention beyond the one-head LDS carve (ripor_amd/csrc/attn_route.h) for
// tests/test_attn_route_long.py.
//   site key=value ...      one JSON object
//   sites: self_bwd (plan_self_attn_bwd, the resident plan), self_bwd_tiled, self_fwd_tiled (S Ls H buckets dkv),
//          cross_bwd_tiled, cross_fwd_tiled (bz n Lq H dkv; "resident": the carve of cross_attn_bwd_kernel fits a CU)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ripor_amd/csrc/attn_route.h"

using namespace rpr;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string site = argv[1];
  const bool self = site.rfind("self", 0) == 0;
  SelfAttnBwdIn b;
  CrossAttnBwdIn c;
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    const std::string k(argv[i], eq - argv[i]);
    const long long v = atoll(eq + 1);
    bool ok = false;
#define F(obj, name) if (k == #name) { obj.name = static_cast<decltype(obj.name)>(v); ok = true; }
    if (self) { F(b, S) F(b, Ls) F(b, H) F(b, buckets) F(b, dkv) }
    else { F(c, bz) F(c, n) F(c, Lq) F(c, H) F(c, dkv) }
#undef F
    if (!ok) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
  }
  AttnLaunch p;
  if (site == "self_bwd") p = plan_self_attn_bwd(b);
  else if (site == "self_bwd_tiled") p = plan_self_attn_bwd_tiled(b);
  else if (site == "self_fwd_tiled") p = plan_self_attn_drop_fwd_tiled(b);
  else if (site == "cross_bwd_tiled") p = plan_cross_attn_bwd_tiled(c);
  else if (site == "cross_fwd_tiled") p = plan_cross_attn_drop_fwd_tiled(c);
  else return 2;
  printf("{\"kernel\": \"%s\", \"invalid\": %d, \"grid\": [%u, %u], \"block\": %d, \"smem\": %zu, \"resident\": %d, \"carve\": %zu}\n",
         attn_kernel_name(p.kernel), (int)p.invalid, p.grid_x, p.grid_y, p.block, p.smem,
         self ? (int)(self_attn_bwd_smem(b.Ls, b.buckets) <= LDS_MAX) : (int)cross_attn_bwd_resident(c.n, c.Lq),
         self ? self_attn_bwd_smem(b.Ls, b.buckets) : cross_attn_bwd_carve(c.n, c.Lq));
  return 0;
}
