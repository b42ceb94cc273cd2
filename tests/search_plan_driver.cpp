// Prints what ripor_amd/csrc/search_plan.h decides, for tests/test_search_plan.py.
//   budget mode Q B margins      tail_extras_budget
//   pool Q                       tail_extras_pool
//   plan key=value ...           one JSON object: the plan of plan_search for these settings / model facts / call;
//                                f=a,b,.. and mu=a,b,.. are the trie statistics per depth, "stats_calls" how often they were asked for
//   key                          one base plan and its copies changed in ONE named field each: their names and the == and <
//                                of every pair, as JSON
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
    if (k == "logit_bound") { m.logit_bound = (float)strtod(val, nullptr); continue; }
    if (k == "fork0") { s.fork_override[0] = (int)v; continue; }
    if (k == "fork1") { s.fork_override[1] = (int)v; continue; }
#define F(obj, name) if (k == #name) { obj.name = static_cast<decltype(obj.name)>(v); continue; }
    F(s, precision) F(s, forced_tail) F(s, n_fork_override) F(s, tail_extras) F(s, l0_mode) F(s, lane_cus)
    F(m, V) F(m, f32_only) F(m, l0_current)
    F(a, Q) F(a, Lq) F(a, B) F(a, L) F(a, flags) F(a, taps) F(a, margins) F(a, lane) F(a, tail_rank_replay) F(a, select_radix)
#undef F
    fprintf(stderr, "bad argument %s\n", argv[i]);
    return 2;
  }
  int calls = 0;
  const SearchPlan p = plan_search(s, m, a, [&] { ++calls; return TrieStats{f.data(), mu.data()}; });
  printf("{\"Q\": %d, \"Lq\": %d, \"B\": %d, \"L\": %d, \"flags\": %u, \"lane\": %d, \"cus\": %d, \"prec\": %d, \"margins\": %d, \"l0\": %d, "
         "\"extras\": %d, \"pool\": %d, \"forks\": [",
         p.Q, p.Lq, p.B, p.L, p.flags, p.lane, p.cus, p.prec, (int)p.margins, p.l0, p.extras, p.pool);
  for (int i = 0; i < p.n_forks; ++i) printf("%s%d", i ? ", " : "", p.forks[i]);
  printf("], \"drop_last\": %d, \"tail_rank_replay\": %d, \"select_radix\": %d, \"stats_calls\": %d}\n", (int)p.drop_last, p.tail_rank_replay,
         p.select_radix, calls);
  return 0;
}

static int key_mode() {
  SearchPlan base = plain_plan(100, 16, 10, 8);
  base.prec = RPR_PREC_F16X2; base.l0 = 1; base.extras = 2; base.pool = 4; base.forks[0] = 3; base.forks[1] = 5; base.n_forks = 2;
  std::vector<std::string> names{"base", "copy"};
  std::vector<SearchPlan> plans{base, base};
  auto add = [&](const char* name, auto&& change) { SearchPlan p = base; change(p); names.push_back(name); plans.push_back(p); };
  add("Q", [](SearchPlan& p) { p.Q = 101; });
  add("Lq", [](SearchPlan& p) { p.Lq = 24; });
  add("B", [](SearchPlan& p) { p.B = 11; });
  add("L", [](SearchPlan& p) { p.L = 9; });
  add("flag log_softmax", [](SearchPlan& p) { p.flags ^= RPR_FLAG_LOG_SOFTMAX; });
  add("flag no_graph", [](SearchPlan& p) { p.flags ^= RPR_FLAG_NO_GRAPH; });
  add("lane", [](SearchPlan& p) { p.lane = 1; });
  add("cus", [](SearchPlan& p) { p.cus = 128; });
  add("prec", [](SearchPlan& p) { p.prec = RPR_PREC_F32; });
  add("margins", [](SearchPlan& p) { p.margins = true; });
  add("l0", [](SearchPlan& p) { p.l0 = 2; });
  add("extras", [](SearchPlan& p) { p.extras = 3; });
  add("pool", [](SearchPlan& p) { p.pool = 5; });
  add("fork0", [](SearchPlan& p) { p.forks[0] = 2; });
  add("fork1", [](SearchPlan& p) { p.forks[1] = 6; });
  add("n_forks", [](SearchPlan& p) { p.n_forks = 1; });
  add("drop_last", [](SearchPlan& p) { p.drop_last = true; });
  add("tail_rank_replay", [](SearchPlan& p) { p.tail_rank_replay = 1; });
  add("select_radix", [](SearchPlan& p) { p.select_radix = 0; });
  const size_t n = plans.size();
  printf("{\"names\": [");
  for (size_t i = 0; i < n; ++i) printf("%s\"%s\"", i ? ", " : "", names[i].c_str());
  for (int lt = 0; lt < 2; ++lt) {
    printf("], \"%s\": [", lt ? "lt" : "eq");
    for (size_t i = 0; i < n; ++i) {
      printf("%s[", i ? ", " : "");
      for (size_t j = 0; j < n; ++j) printf("%s%d", j ? ", " : "", (int)(lt ? plans[i] < plans[j] : plans[i] == plans[j]));
      printf("]");
    }
  }
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "budget" && argc == 6) { printf("%d\n", tail_extras_budget(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0)); return 0; }
  if (mode == "pool" && argc == 3) { printf("%d\n", tail_extras_pool(atoi(argv[2]))); return 0; }
  if (mode == "plan") return plan_mode(argc, argv);
  if (mode == "key") return key_mode();
  return 2;
}
