"""not-gpu: the host side of the forced-with-extras fork (rpr_set_tail_extras): the trie statistic trie_extra_mean
(rpr_trie_extra_mean) against a numpy count, and the fork planner (rpr_plan_forks) on the statistics of synthetic tries."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import engine
    return engine


def _brute_extra_mean(codes, L):
    """mean over the distinct t-prefixes of (distinct L-token sequences under the prefix - 1), t = 0..L"""
    seqs = np.unique(np.asarray(codes)[:, :L], axis=0)
    out = []
    for t in range(L + 1):
        nodes = len(np.unique(seqs[:, :t], axis=0)) if t else 1
        out.append((len(seqs) - nodes) / nodes)
    return np.array(out)


def test_extra_mean_matches_numpy_count_on_random_tables(E):
    from ripor_amd.utils import synth
    for N, L, V, seed in ((500, 6, 4, 1), (3000, 5, 16, 2), (64, 3, 2, 3), (1, 4, 256, 4)):
        codes = synth.make_codes(N, L, V, seed=seed)
        np.testing.assert_allclose(E.trie_extra_mean(codes), _brute_extra_mean(codes, L), rtol=0, atol=1e-12)


def test_extra_mean_hand_made_table_duplicates_and_prefix_search(E):
    # node (1,) holds three sequences, node (2,) one sequence in four rows (a duplicated smtid), node (3,) two
    codes = np.array([[1, 0, 0, 0], [1, 0, 0, 1], [1, 5, 0, 0],
                      [2, 2, 2, 2], [2, 2, 2, 2], [2, 2, 2, 2], [2, 2, 2, 2],
                      [3, 1, 0, 7], [3, 1, 9, 7]], dtype=np.uint16)
    mu = E.trie_extra_mean(codes[::-1])   # any row order
    # 6 distinct sequences; nodes per depth 1, 3, 4, 5, 6
    np.testing.assert_allclose(mu, [5.0, 3 / 3, 2 / 4, 1 / 5, 0.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(mu, _brute_extra_mean(codes, 4), rtol=0, atol=1e-15)
    # duplicated rows count once: the same table with every row repeated gives the same statistic
    np.testing.assert_allclose(E.trie_extra_mean(np.repeat(codes, 3, axis=0)), mu, rtol=0, atol=1e-15)
    # prefix search L < Lc: sequences are the distinct L-prefixes ((1,0,0,0) and (1,0,0,1) merge at L = 3)
    for L in (1, 2, 3):
        np.testing.assert_allclose(E.trie_extra_mean(codes, L), _brute_extra_mean(codes, L), rtol=0, atol=1e-15)
    np.testing.assert_allclose(E.trie_extra_mean(codes, 3), [4.0, 2 / 3, 1 / 4, 0.0], rtol=0, atol=1e-15)
    # the older statistic comes from the same pass and is unchanged by it
    f = E.trie_single_frac(codes)
    np.testing.assert_allclose(f, [0.0, 1 / 3, 2 / 4, 4 / 5, 1.0], rtol=0, atol=1e-15)


def test_planner_single_fork_and_drop_last_where_extras_apply(E):
    """A uniform trie of 40k docs, V = 256: depth 3 has 16.7M prefixes, so nearly every depth-3 node is single and the
    few collisions hold two sequences — about 13 of 1075 queries are expected to stand on one, within the 33 spare entries
    of such a stage (a few hundred thousand docs would want more than the pool holds): with more than 4096 decoder rows in
    flight the automatic mode takes them along, the first fork leaves (almost) nobody behind and in the optimistic mode
    nothing is enqueued after it. At 4096 rows or fewer, and with the feature off, the depths are the old ones."""
    from ripor_amd.utils import synth
    N, L, V, B = 40_000, 16, 256, 10
    codes = synth.make_codes_fast(N, L, V, seed=5)
    f, mu = E.trie_single_frac(codes), E.trie_extra_mean(codes)
    assert 0 < mu[3] < 0.02 and f[3] ** B >= 0.5 > f[2] ** B, (f[:5], mu[:5])

    def old_rule(Q, mode):
        """the planner before the feature (choose_forks: first fork at f^B >= 1/2, second where Q (1 - f^B) <= 0.05)"""
        t0 = next(t for t in range(1, L - 1) if f[t] ** B >= 0.5)
        if L - t0 < (2 if Q * B <= 4096 else 8):
            return [], False
        if mode == 2 and Q * (1 - f[t0] ** B) <= 0.05:
            return [t0], True
        second = [t for t in range(t0 + 1, min(L - 2, t0 + 12) + 1) if Q * (1 - f[t] ** B) <= 0.05][:1]
        return [t0] + second, mode == 2 and len(second) == 1

    Q = 1075                                                  # Q * B > 4096: the feature applies in the automatic mode
    assert Q * (1 - f[3] ** B) > 0.05, "the trie is too sparse for the test: the old rule already drops the stage"
    assert E.plan_forks(f, mu, Q, B, L, forced_tail=2, tail_extras=-1) == ([3], True)
    assert E.plan_forks(f, mu, Q, B, L, forced_tail=2, tail_extras=4) == ([3], True)
    depths, drop = E.plan_forks(f, mu, Q, B, L, forced_tail=1, tail_extras=-1)
    assert depths[0] == 3 and not drop                       # exact mode: the first fork stays, a stage follows the last one
    # feature off: the old depths, in both modes
    for mode in (1, 2):
        assert E.plan_forks(f, mu, Q, B, L, forced_tail=mode, tail_extras=0) == old_rule(Q, mode)
    assert len(old_rule(Q, 2)[0]) == 2
    # Q * B <= 4096: the automatic mode is off, the depths are the old ones
    for Qs in (1, 48, 409):
        for mode in (1, 2):
            assert E.plan_forks(f, mu, Qs, B, L, forced_tail=mode, tail_extras=-1) == old_rule(Qs, mode), (Qs, mode)
    # 32 beams or more: never
    assert E.plan_forks(f, mu, 1000, 32, L, forced_tail=2, tail_extras=8) == E.plan_forks(f, mu, 1000, 32, L, forced_tail=2, tail_extras=0)


def test_planner_keeps_the_stage_when_the_pool_or_the_budget_would_not_do(E):
    """A denser trie: many queries would want a spare entry (more than the pool holds) — the expected leftovers stay above
    0.05 and the optimistic mode keeps its second fork."""
    from ripor_amd.utils import synth
    N, L, V, B = 800_000, 16, 256, 10
    codes = synth.make_codes_fast(N, L, V, seed=6)[:, :L]
    f, mu = E.trie_single_frac(codes), E.trie_extra_mean(codes)
    Q = 2000
    lam = B * mu[3]
    assert f[3] ** B >= 0.5 and Q * (1 - np.exp(-lam)) > 3 * 64, (f[3], mu[3])   # far more takers than the largest pool
    depths, drop = E.plan_forks(f, mu, Q, B, L, forced_tail=2, tail_extras=-1)
    assert depths[0] == 3 and len(depths) == 2 and drop
