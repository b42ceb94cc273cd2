// Prints what ripor_amd/csrc/search_plan.h decides about a search that reports prefix lengths (rpr_search_prefixes), for
// tests/test_prefix_depths_host.py.
//   plan key=value ...    one JSON object: every field of the plan of plan_search; depths=4,8 are the call's prefix lengths,
//                         f=a,b,.. and mu=a,b,.. the trie statistics per depth
//   key                   one base plan with prefix lengths and its copies changed in ONE named field each: their names and
//                         the == and < of every pair, as JSON
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ripor_amd/csrc/search_plan.h"

using namespace rpr;

static std::vector<double> list_of(const char* s) {
  std::vector<double> v;
  for (char* end = nullptr; *s; s = *end ? end + 1 : end) v.push_back(strtod(s, &end));
  return v;
}

static int plan_mode(int argc, char** argv) {
  SearchSettings s;
  SearchModel m;
  SearchCall a;
  m.logit_bound = 1.0f; m.V = 256;
  std::vector<double> f, mu;
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return 2;
    const std::string k(argv[i], eq - argv[i]);
    const char* val = eq + 1;
    const long long v = atoll(val);
    if (k == "f") { f = list_of(val); continue; }
    if (k == "mu") { mu = list_of(val); continue; }
    if (k == "fork0") { s.fork_override[0] = (int)v; continue; }
    if (k == "fork1") { s.fork_override[1] = (int)v; continue; }
    if (k == "depths") {
      const std::vector<double> d = list_of(val);
      if (d.size() > (size_t)MAX_DEPTHS) return 2;
      a.n_depths = (int)d.size();
      for (size_t j = 0; j < d.size(); ++j) a.depths[j] = (int)d[j];
      continue;
    }
#define F(obj, name) if (k == #name) { obj.name = static_cast<decltype(obj.name)>(v); continue; }
    F(s, precision) F(s, forced_tail) F(s, n_fork_override) F(s, tail_extras) F(s, l0_mode) F(s, lane_cus) F(s, gemm_mfma16)
    F(m, V) F(m, f32_only) F(m, l0_current)
    F(a, Q) F(a, Lq) F(a, B) F(a, L) F(a, flags) F(a, taps) F(a, margins) F(a, lane) F(a, tail_rank_replay) F(a, select_radix)
#undef F
    fprintf(stderr, "bad argument %s\n", argv[i]);
    return 2;
  }
  const SearchPlan p = plan_search(s, m, a, [&] { return TrieStats{f.data(), mu.data()}; });
  printf("{\"Q\": %d, \"Lq\": %d, \"B\": %d, \"L\": %d, \"flags\": %u, \"lane\": %d, \"cus\": %d, \"prec\": %d, \"margins\": %d, \"l0\": %d, "
         "\"mfma16\": %d, \"extras\": %d, \"pool\": %d, \"forks\": [",
         p.Q, p.Lq, p.B, p.L, p.flags, p.lane, p.cus, p.prec, (int)p.margins, p.l0, p.mfma16, p.extras, p.pool);
  for (int i = 0; i < p.n_forks; ++i) printf("%s%d", i ? ", " : "", p.forks[i]);
  printf("], \"drop_last\": %d, \"tail_rank_replay\": %d, \"select_radix\": %d, \"depths\": [", (int)p.drop_last, p.tail_rank_replay,
         p.select_radix);
  for (int i = 0; i < p.n_depths; ++i) printf("%s%d", i ? ", " : "", p.depths[i]);
  printf("], \"n_depths\": %d}\n", p.n_depths);
  return 0;
}

static int key_mode() {
  SearchPlan base = plain_plan(100, 16, 10, 16);
  base.depths[0] = 4; base.depths[1] = 8; base.n_depths = 2;
  std::vector<std::string> names{"base", "copy"};
  std::vector<SearchPlan> plans{base, base};
  auto add = [&](const char* name, auto&& change) { SearchPlan p = base; change(p); names.push_back(name); plans.push_back(p); };
  add("no depths", [](SearchPlan& p) { p.depths[0] = p.depths[1] = 0; p.n_depths = 0; });
  add("depth0", [](SearchPlan& p) { p.depths[0] = 3; });
  add("depth1", [](SearchPlan& p) { p.depths[1] = 9; });
  add("depth2", [](SearchPlan& p) { p.depths[2] = 12; });
  add("n_depths", [](SearchPlan& p) { p.n_depths = 1; });
  printf("{\"names\": [");
  for (size_t i = 0; i < names.size(); ++i) printf("%s\"%s\"", i ? ", " : "", names[i].c_str());
  printf("], \"eq\": [");
  for (size_t i = 0; i < plans.size(); ++i) {
    printf("%s[", i ? ", " : "");
    for (size_t j = 0; j < plans.size(); ++j) printf("%s%d", j ? ", " : "", (int)(plans[i] == plans[j]));
    printf("]");
  }
  printf("], \"lt\": [");
  for (size_t i = 0; i < plans.size(); ++i) {
    printf("%s[", i ? ", " : "");
    for (size_t j = 0; j < plans.size(); ++j) printf("%s%d", j ? ", " : "", (int)(plans[i] < plans[j]));
    printf("]");
  }
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "plan")) return plan_mode(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "key")) return key_mode();
  return 2;
}
