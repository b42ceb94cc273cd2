// Plan of one constrained beam search on one workspace: everything that is decided about it before anything is sized,
// enqueued or looked up in the graph cache — effective precision, margins, the layer-0 table, the forced-tail forks and the
// extras they take along. api.hip fills the inputs from the ctx, the model and the call and asks plan_search once per
// workspace; alloc_workspace and enqueue_search (passes.hip) read the plan, and the plan itself is the graph key. Plain host
// arithmetic, no HIP types: tests/test_search_plan.py compiles it with the host compiler and checks it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <tuple>

#include "../../include/ripor_hip.h"

namespace rpr {

constexpr int MAX_FORKS = 2;
constexpr int MAX_DEPTHS = 3;   // prefix lengths one search may report besides its own (rpr_search_prefixes)

struct SearchPlan {
  int Q = 0, Lq = 0, B = 0, L = 0;
  unsigned flags = 0;            // the caller's RPR_FLAG_*
  int lane = -1, cus = 0;        // lane: -1 = the ctx workspace; cus: CUs of the stream it runs on (0 = the whole chip)
  int prec = RPR_PREC_F16X2;     // effective_precision of the call
  bool margins = false;          // rpr_search_margins: every selection step is followed by the pruning-margin kernel
  int l0 = 0;                    // the layer-0 Q/K/V table: 0 = not read, 1 / 2 = read in that rpr_set_l0_table mode
  int mfma16 = 0;                // 1: the 256x256 ping-pong GEMM launches of this search's tail passes run the 16x16x32 body (rpr_set_gemm_mfma16)
  int extras = 0, pool = 0;      // forced with extras: budget per forced query, spare tail entries per fork (both 0 without forks)
  int forks[MAX_FORKS] = {0, 0}; // depths at which forced queries leave the sequential steps (ascending, each in [1, L-1])
  int n_forks = 0;               //   0 = plain search
  bool drop_last = false;        // no stage after the last fork (optimistic mode, see plan_forks): its caches are not needed
  int tail_rank_replay = 0, select_radix = -1;   // per-call test selectors of the ranking / selection launchers (tests flip them between calls)
  int depths[MAX_DEPTHS] = {0, 0, 0};   // rpr_search_prefixes: prefix lengths whose beams are reported too (ascending, each in [1, L-1])
  int n_depths = 0;                     //   0 = none: the plan, the launches and the key of a plain search
  bool log_softmax() const { return (flags & RPR_FLAG_LOG_SOFTMAX) != 0; }
  auto key() const {
    return std::tie(Q, Lq, B, L, flags, lane, cus, prec, margins, l0, mfma16, extras, pool, forks[0], forks[1], n_forks, drop_last,
                    tail_rank_replay, select_radix, depths[0], depths[1], depths[2], n_depths);
  }
  bool operator<(const SearchPlan& o) const { return key() < o.key(); }
  bool operator==(const SearchPlan& o) const { return key() == o.key(); }
};
static_assert(MAX_FORKS == 2, "SearchPlan::key names every fork depth");
static_assert(MAX_DEPTHS == 3, "SearchPlan::key names every prefix length");

// the plan of a call that only sizes the shared buffers (rpr_encode, the training step): no forks, no margins
inline SearchPlan plain_plan(int Q, int Lq, int B, int L) {
  SearchPlan p;
  p.Q = Q; p.Lq = Lq; p.B = B; p.L = L;
  return p;
}

// Precision of what one call enqueues: bf16 is a training-GEMM mode (scores need fp32-equivalent arithmetic), and a model
// whose weights do not fit the f16 planes runs on the exact-fp32 kernels whatever the ctx setting
inline int effective_precision(int ctx_precision, bool f32_only) {
  return f32_only ? RPR_PREC_F32 : (ctx_precision == RPR_PREC_BF16 ? RPR_PREC_F16X2 : ctx_precision);
}

// Forced with extras (common.h: ForkArgs::E): how many extra sequences a forced query may carry into the tail pass, and how
// many spare tail entries a stage keeps for such queries. Automatic mode: stages with more than 4096 decoder rows (the
// threshold of plan_forks for "steps bound by the matrix pipes": there a leftover stage costs two partly filled launches
// per GEMM) and fewer than 32 beams (the one-block selection; with more beams extras are the rule and a spare entry of B
// slots per query is the wrong layout). Never with the pruning margins: a query with extras is still pruned inside the tail.
constexpr int TAIL_EXTRAS_AUTO = 4;
inline int tail_extras_budget(int mode, int Q, int B, bool margins) {
  if (mode == 0 || B >= 32 || margins) return 0;
  if (mode > 0) return mode < B ? mode : B;
  return (int64_t)Q * B > 4096 ? (TAIL_EXTRAS_AUTO < B ? TAIL_EXTRAS_AUTO : B) : 0;
}
inline int tail_extras_pool(int Q) { return Q / 32 < 4 ? 4 : (Q / 32 > 64 ? 64 : Q / 32); }

// P(X > k) and E[max(0, X - k)] of X ~ Poisson(lam), summed term by term (the terms of interest are far below 1 - sum)
inline double poisson_pmf(double lam, int i) { return lam > 0 ? std::exp(-lam + i * std::log(lam) - std::lgamma((double)i + 1.0)) : (i == 0 ? 1.0 : 0.0); }
inline double poisson_tail(double lam, int k) {
  if (lam <= 0) return 0.0;
  if (lam > 4.0 * k + 50.0) return 1.0;
  double s = 0;
  const int n = k + 60 + (int)(lam + 12.0 * std::sqrt(lam));
  for (int i = k + 1; i <= n; ++i) s += poisson_pmf(lam, i);
  return s < 1.0 ? s : 1.0;
}
inline double poisson_excess(double lam, int k) {
  if (lam <= 0) return 0.0;
  if (lam > 4.0 * k + 50.0) return lam;            // (an upper bound: E[(X - k)+] <= E[X])
  double s = 0;
  const int n = k + 60 + (int)(lam + 12.0 * std::sqrt(lam));
  for (int i = k + 1; i <= n; ++i) s += (double)(i - k) * poisson_pmf(lam, i);
  return s;
}

// Fork depths from the trie statistics, into forks[MAX_FORKS]; returns their number (rpr_plan_forks exposes it to the host
// tests). f[t] = the share of the depth-t nodes under which one distinct sequence remains (trie_single_frac): a query whose
// B beams sit on random depth-t nodes is forced with probability ~ f[t]^B. First fork: the first depth where that reaches
// one half. Second fork: the first depth after it where fewer than 0.05 queries of the call are expected to stay unforced,
// so that the last stage is almost always empty (a stage with a handful of live rows still pays ~100 launches per step).
// Expected number of queries a fork at depth t leaves behind, left(t):
//   E = 0 (no extras):  Q * (1 - f[t]^B).
//   E > 0 (the fork also takes queries with up to E extra sequences, each in one of `pool` spare tail entries): with
//   mu[t] = the mean of (distinct sequences - 1) over the depth-t nodes (trie_single_frac's extra_mean), the extras of a
//   query are taken as Poisson with mean lam = B * mu[t]; a query stays behind when it has more than E of them, or when it
//   has some and the pool is empty — the queries that want a spare entry are Poisson with mean Q * (1 - exp(-lam)):
//     left(t) = Q * P[Poisson(lam) > E] + E[max(0, Poisson(Q * (1 - exp(-lam))) - pool)].
//   (1 - f <= mu, so the share without extras, exp(-lam), is never above f^B: the estimate of the queries that need a spare
//   entry is on the high side. Nodes with very many sequences make the true tail heavier than Poisson's; the optimistic
//   mode's leftover flag and the caller's back-off cover that.)
inline int plan_forks(const double* f, const double* mu, int Q, int B, int L, int forced_tail, int E, int pool, int* forks, bool* drop_last) {
  int n = 0;
  *drop_last = false;
  auto p_forced = [&](int t) { return std::pow(f[t], (double)B); };
  auto left = [&](int t) {
    if (E <= 0) return (double)Q * (1.0 - p_forced(t));
    const double lam = (double)B * mu[t];
    return (double)Q * poisson_tail(lam, E) + poisson_excess((double)Q * (1.0 - std::exp(-lam)), pool);
  };
  int t0 = 0;
  for (int t = 1; t <= L - 2 && !t0; ++t) if (p_forced(t) >= 0.5) t0 = t;
  // a tail pass costs what its positions cost step by step minus the K/V gathering, plus a fork (~100 launches, two
  // partly filled launches for the leftovers): with thousands of decoder rows in flight — steps bound by the matrix
  // pipes — the plain loop is as fast below 8 remaining positions (measured at beam 100, len 8, 214 queries: 1890
  // queries/s without forks, 1510 with). A few hundred rows (the reference's rank-data flags: beam 100, batch 4, len 8)
  // are bound by the launch chain instead: a step of 12 layers costs 1.6 ms whatever it computes, the four remaining
  // positions as ONE pass of 1600 rows cost as much as one and a half steps (round 6: 306 -> 378 queries/s)
  const int min_tail = (int64_t)Q * B <= 4096 ? 2 : 8;
  if (!t0 || L - t0 < min_tail) return n;
  forks[n++] = t0;
  // Optimistic mode (rpr_set_forced_tail(ctx, 2)): when the statistics promise an (almost always) empty last stage, that
  // stage is not enqueued at all — ~100 launches per step for nobody — and a query that is still unforced at the last
  // fork raises RPR_STATUS_TAIL_LEFTOVER instead; the caller then repeats the batch in the exact mode (1).
  // A handful of queries in flight, or a fork that takes the few queries with extras along: the first fork already leaves
  // fewer than 0.05 queries behind in expectation, so the second fork (a compacted stage, its steps and a second tail pass:
  // ~300 launches that almost always work on nothing, 2 of the 9.8 ms of a single-query search) is not enqueued either.
  if (forced_tail == 2 && left(t0) <= 0.05) { *drop_last = true; return n; }
  for (int t = t0 + 1; t <= L - 2 && t <= t0 + 12; ++t)
    if (left(t) <= 0.05) { forks[n++] = t; break; }
  *drop_last = forced_tail == 2 && n == 2;
  return n;
}

// ---- the inputs of plan_search: what it needs of the ctx, of the model and of the call ----------------------------------
struct SearchSettings {          // the base of rpr_ctx (internal.h)
  int precision = RPR_PREC_F16X2;
  int forced_tail = 1;           // 0 = every query runs all L steps sequentially, 1 = exact forced tail, 2 = optimistic (see plan_forks)
  int fork_override[MAX_FORKS] = {0, 0};   // explicit fork depths (rpr_set_fork_depths / RPR_FORK_DEPTHS)
  int n_fork_override = -1;      // -1 = automatic: from the trie statistics
  int tail_extras = -1;          // rpr_set_tail_extras: -1 = automatic (tail_extras_budget), 0 = off, n > 0 = always, up to n extra sequences per query
  int l0_mode = 1;               // rpr_set_l0_table: 0 = the table is never made nor read, 1 = it replaces the launches the route planner
                                 //   sends to the ping-pong kernel, 2 = every layer-0 Q/K/V launch of a search (tests)
  int gemm_mfma16 = 1;           // rpr_set_gemm_mfma16: MFMA shape of the 256x256 ping-pong GEMM, 0 = 32x32x16 everywhere,
                                 //   1 = 16x16x32 in the tail passes of a search (forced sequences: scores only, no pruning decision)
  int lane_cus = 0;              // CUs per lane
};
struct SearchModel {             // rpr_model
  float logit_bound = INFINITY;
  int V = 0;
  bool f32_only = false;
  bool l0_current = false;       // the layer-0 table is made and current for the ctx state
};
struct SearchCall {
  int Q = 0, Lq = 0, B = 0, L = 0;
  unsigned flags = 0;
  bool taps = false, margins = false;
  int lane = -1;
  int tail_rank_replay = 0, select_radix = -1;   // RPR_TAIL_RANK_REPLAY / RPR_SELECT_RADIX as the launchers will read them
  int depths[MAX_DEPTHS] = {0, 0, 0};            // rpr_search_prefixes: the prefix lengths asked for (checked by the caller)
  int n_depths = 0;
};
struct TrieStats { const double* single_frac; const double* extra_mean; };   // per depth 0..L (trie_single_frac)

// stats(): the TrieStats of the call's trie and L; asked for only when the automatic fork planner needs them (gates passed,
// no explicit depths). Explicit depths (rpr_set_fork_depths / RPR_FORK_DEPTHS) win; otherwise they come from plan_forks.
template <class Stats>
SearchPlan plan_search(const SearchSettings& s, const SearchModel& m, const SearchCall& a, Stats&& stats) {
  SearchPlan p;
  p.Q = a.Q; p.Lq = a.Lq; p.B = a.B; p.L = a.L; p.flags = a.flags;
  p.lane = a.lane; p.cus = a.lane >= 0 ? s.lane_cus : 0;
  p.prec = effective_precision(s.precision, m.f32_only);
  p.margins = a.margins;
  p.l0 = s.l0_mode > 0 && m.l0_current && p.prec == RPR_PREC_F16X2 ? s.l0_mode : 0;
  p.mfma16 = s.gemm_mfma16 && p.prec == RPR_PREC_F16X2 ? 1 : 0;
  p.tail_rank_replay = a.tail_rank_replay ? 1 : 0; p.select_radix = a.select_radix;
  p.n_depths = a.n_depths < MAX_DEPTHS ? a.n_depths : MAX_DEPTHS;
  for (int i = 0; i < p.n_depths; ++i) p.depths[i] = a.depths[i];
  if (!s.forced_tail || a.taps || a.L < 3 || !std::isfinite(m.logit_bound)) return p;
  const double per_step = 2.0 * (double)m.logit_bound + (p.log_softmax() ? std::log((double)m.V) : 0.0);
  if (1e8 - a.L * per_step <= 1e7) return p;   // logits too large for the masked-candidate proof (passes.hip: enqueue_fork)
  const int E = tail_extras_budget(s.tail_extras, a.Q, a.B, a.margins), pool = E > 0 ? tail_extras_pool(a.Q) : 0;
  if (s.n_fork_override >= 0) {
    int prev = 0;
    for (int i = 0; i < s.n_fork_override && i < MAX_FORKS; ++i) {
      const int t = s.fork_override[i];
      if (t > prev && t <= a.L - 1) { p.forks[p.n_forks++] = t; prev = t; }
    }
    p.drop_last = s.forced_tail == 2 && p.n_forks > 0;
  } else {
    const TrieStats ts = stats();
    p.n_forks = plan_forks(ts.single_frac, ts.extra_mean, a.Q, a.B, a.L, s.forced_tail, E, pool, p.forks, &p.drop_last);
  }
  // Prefix lengths: the forks stay where the same (Q, B, L) has them without (planned above with that call's extras), but
  // no query is forced with extras — it would be pruned inside the tail, where its intermediate beam sets do not exist.
  // In optimistic mode such a query raises the leftover flag instead.
  if (p.n_forks > 0 && p.n_depths == 0) { p.extras = E; p.pool = pool; }
  return p;
}

}  // namespace rpr
