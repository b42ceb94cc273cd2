"""-m gpu: the fork that takes queries with a few extra sequences along (rpr_set_tail_extras; tail_kernels.hip:
fork_classify_kernel, fork_scan_kernel, fork_extras_kernel, tail_rank_extras) against the plain step-by-step loop and the CPU
oracle.

The code tables are built by hand. The beams of a query after T steps depend on the set of T-prefixes only, so a table is
made in two passes: a base table with ONE sequence under every T-prefix, on which a plain prefix search of length T gives
every query's beams; then the tails of chosen nodes — nodes under one query's beams only — are replaced by several
sequences (diverging at the first or at the last tail position, duplicated rows, more than the budget). What each query
then holds is counted on the CPU from the table and the beams, and every case a test is about is asserted to occur."""
import numpy as np
import pytest
import torch

from conftest import ORDER_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu

POOL = 4          # spare tail entries of a stage of fewer than 160 queries (csrc/search_plan.h: tail_extras_pool)


@pytest.fixture(scope="module")
def E():
    from ripor_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


@pytest.fixture(autouse=True)
def _restore(E):
    ctx = E.Context.get(0)
    yield
    ctx.set_tail_extras(-1)
    ctx.set_fork_depths(None)
    ctx.set_forced_tail(True)


class World:
    """model, queries and the base table of one configuration; `beams` = every query's T-prefixes after T plain steps"""

    def __init__(self, E, L, V, B, Q, T, n_prefix, seed, sd_edit=None):
        from ripor_amd.utils import synth
        self.E, self.L, self.V, self.B, self.Q, self.T, self.seed = E, L, V, B, Q, T, seed
        self.dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
        self.sd = synth.make_state_dict(self.dims, seed=seed)
        if sd_edit:
            sd_edit(self.sd)
        self.ids, self.mask = synth.make_queries(Q, vocab_size=self.dims.vocab_size, seed=seed, max_len=14)
        self.ti, self.tm = torch.from_numpy(self.ids), torch.from_numpy(self.mask)
        self.ctx = E.Context.get(0)
        self.model = E.DeviceModel(self.ctx, self.sd, self.dims)
        self.rng = np.random.default_rng(seed)
        self.pref = np.unique(synth.make_codes(n_prefix, T, V, seed=seed), axis=0)
        tails = self.rng.integers(0, V, size=(len(self.pref), L - T))
        # node -> list of (tail, rows); the base table: one sequence, one row
        self.plan = {tuple(int(x) for x in p): [(tuple(int(x) for x in t), 1)] for p, t in zip(self.pref, tails)}
        self.ctx.set_forced_tail(False)
        r = E.search(self.model, self.trie(), self.ti, self.tm, B, T)
        torch.cuda.synchronize()
        self.ctx.set_forced_tail(True)
        self.beams = r.tokens.cpu().numpy()                                  # [Q, B, T]
        self.live = (r.row_hi > r.row_lo).cpu().numpy()
        assert self.live.all(), "a dead beam at the fork depth: enlarge the prefix set"
        owners = {}
        for q in range(Q):
            for b in range(B):
                owners.setdefault(tuple(int(x) for x in self.beams[q, b]), set()).add(q)
        self.owners = owners
        self.private = [[n for n in (tuple(int(x) for x in self.beams[q, b]) for b in range(B)) if owners[n] == {q}] for q in range(Q)]

    def codes(self):
        rows = []
        for node, seqs in self.plan.items():
            for tail, rep in seqs:
                rows += [node + tail] * rep
        rows = np.array(rows, dtype=np.uint16)
        return rows[np.random.default_rng(self.seed + 1).permutation(len(rows))]

    def trie(self):
        return self.E.DeviceTrie.from_codes(self.ctx, self.codes(), self.V)

    def split(self, node, n, at=None, reps=None):
        """n distinct sequences under `node`: copies of its tail changed at tail position `at` (default: a random one)"""
        base = list(self.plan[node][0][0])
        seqs, seen = [], set()
        while len(seqs) < n:
            t = list(base)
            if seqs:
                p = at if at is not None else int(self.rng.integers(0, self.L - self.T))
                t[p] = int((t[p] + 1 + self.rng.integers(0, self.V - 1)) % self.V)
                if at is None:       # everything behind the divergence is the sequence's own
                    t[p + 1:] = [int(x) for x in self.rng.integers(0, self.V, size=self.L - self.T - p - 1)]
            if tuple(t) not in seen:
                seen.add(tuple(t))
                seqs.append(tuple(t))
        self.plan[node] = [(s, (reps[i] if reps else 1)) for i, s in enumerate(seqs)]

    def targets(self, need, among=None):
        """distinct queries with at least need[i] private nodes (the beams of these small models overlap heavily: a
        query has zero to a few nodes of its own), the most demanding entry served first; one query per entry of `need`"""
        out, used = [None] * len(need), set()
        for i in sorted(range(len(need)), key=lambda i: -need[i]):
            q = next((q for q in (among if among is not None else range(self.Q)) if q not in used and len(self.private[q]) >= need[i]), None)
            assert q is not None, ("not enough queries with private nodes", [len(p) for p in self.private])
            out[i] = q
            used.add(q)
        return out

    def least_shared(self, n):
        """n nodes under the beams, those under the fewest queries first"""
        return sorted(self.owners, key=lambda node: (len(self.owners[node]), node))[:n]

    def extras(self, beams=None):
        """per query: sum over its beams of (distinct sequences under the beam's node - 1), counted from the table"""
        beams = self.beams if beams is None else beams
        return np.array([sum(len(self.plan[tuple(int(x) for x in beams[q, b])]) - 1 for b in range(self.B)) for q in range(self.Q)])

    def predicted_forced(self, budget, halves=False, beams=None):
        """which queries the fork at depth T takes: no extras, or 1..budget extras and a spare entry left (handed out in
        query order, per lane when the batch is split)"""
        ex = self.extras(beams)
        forced = np.zeros(self.Q, dtype=bool)
        h = (self.Q + 1) // 2
        for lo, hi in (((0, h), (h, self.Q)) if halves else ((0, self.Q),)):
            used = 0
            for q in range(lo, hi):
                if ex[q] == 0:
                    forced[q] = True
                elif ex[q] <= budget and used < POOL:
                    forced[q] = True
                    used += 1
        return forced, ex


def _compare(res, plain, label):
    """the criterion of test_gpu_forced_tail._same_as_plain: identical sequences and row ranges at every rank outside score
    near-ties, scores within 0.3 of the parity tolerance"""
    same = (res.tokens == plain.tokens).all(dim=2)
    close = (res.scores - plain.scores).abs() <= ORDER_TOL
    live = plain.scores > -1e6
    assert bool((same | close | ~live).all()), f"{label}: sequences differ from the step-by-step loop"
    err = float(((res.scores - plain.scores).abs() * live).max())
    print(f"[tail extras] {label}: max score diff {err:.2e}, {int(same.sum())}/{same.numel()} ranks identical")
    assert err <= 0.3 * SCORE_TOL, (label, err)
    both = same & live
    assert torch.equal(res.row_lo[both], plain.row_lo[both]) and torch.equal(res.row_hi[both], plain.row_hi[both]), label
    return same


def _run(w, trie, budget, mode=1, log_softmax=False, halves=False, label=""):
    ctx, E = w.ctx, w.E
    ctx.set_forced_tail(False)
    plain = E.search(w.model, trie, w.ti, w.tm, w.B, w.L, apply_log_softmax_for_scores=log_softmax)
    # the beams at the fork under THIS scoring and precision (log-softmax scores and exact fp32 may select other prefixes
    # than the ones the table was made for): a plain prefix search of length T on the same trie
    at_fork = E.search(w.model, trie, w.ti, w.tm, w.B, w.T, apply_log_softmax_for_scores=log_softmax)
    beams = at_fork.tokens.cpu().numpy()
    assert bool((at_fork.row_hi > at_fork.row_lo).all())
    ctx.set_forced_tail(mode)
    ctx.set_fork_depths([w.T])
    ctx.set_tail_extras(budget)
    ctx.status(clear=True)
    res = E.search(w.model, trie, w.ti, w.tm, w.B, w.L, apply_log_softmax_for_scores=log_softmax)
    torch.cuda.synchronize()
    stats = ctx.last_fork_stats()
    status = ctx.status(clear=True)
    forced, ex = w.predicted_forced(budget, halves, beams)
    print(f"[tail extras] {label}: forks {stats}, extras of the queries {ex.tolist()}")
    assert stats[0]["depth"] == w.T and stats[0]["forced"] == int(forced.sum()) and stats[0]["left"] == w.Q - int(forced.sum()), (stats, forced)
    return res, plain, forced, ex, status


def _check_ranges_and_survivors(w, codes, plain, forced, ex):
    """Of the queries forced with extras: the returned range of every sequence covers exactly its duplicated rows; and how
    many extra sequences (not the first of their node) survived / were pruned, and how many first sequences lost their slot."""
    T, L = w.T, w.L
    survived = pruned = first_lost = 0
    tok = plain.tokens.cpu().numpy()
    width = (plain.row_hi - plain.row_lo).cpu().numpy()
    for q in np.flatnonzero(forced & (ex > 0)):
        got = {tuple(int(x) for x in tok[q, r]): int(width[q, r]) for r in range(w.B)}
        for b in range(w.B):
            node = tuple(int(x) for x in w.beams[q, b])
            seqs = sorted(w.plan[node])                    # the trie's order: the first sequence is the smallest tail
            for i, (tail, rep) in enumerate(seqs):
                full = node + tail
                if full in got:
                    assert got[full] == rep == int((codes == np.array(full, dtype=np.uint16)).all(axis=1).sum()), (q, full)
                    survived += i > 0
                else:
                    pruned += i > 0
                    first_lost += i == 0
    return survived, pruned, first_lost


CONFIGS = {"b4": dict(L=8, V=16, B=4, Q=16, T=3, n_prefix=2500, budget=3),
           "b10": dict(L=12, V=256, B=10, Q=48, T=2, n_prefix=30000, budget=4)}


def _world(E, name, seed, **kw):
    c = dict(CONFIGS[name])
    budget = c.pop("budget")
    return World(E, seed=seed, **c, **kw), budget


@pytest.mark.parametrize("name", ["b4", "b10"])
def test_extras_by_construction_equal_the_plain_loop(E, name):
    """Cases 1-5 of the fork: two sequences diverging at the first / at the last tail position, extras spread over several
    beams up to exactly the budget, budget + 1 extras (not forced, same result through the next stage), duplicated rows
    next to a real extra; over three tables, extra sequences both survive and are pruned, and first sequences lose slots."""
    tot = np.zeros(3, dtype=int)
    for seed in (4, 6, 9):
        w, budget = _world(E, name, seed)
        Lt = w.L - w.T
        qa, qb, qc, qd, qe = w.targets([1, 1, 2, 1, 2])
        w.split(w.private[qa][0], 2, at=0)
        w.split(w.private[qb][0], 2, at=Lt - 1)
        nodes = w.private[qc][:budget]                       # exactly `budget` extras over two or more beams
        for i, n in enumerate(nodes):
            w.split(n, 1 + budget // len(nodes) + (i < budget % len(nodes)))
        w.split(w.private[qd][0], budget + 2)
        w.split(w.private[qe][0], 2, reps=[3, 2])
        w.split(w.private[qe][1], 1, reps=[4])
        codes = w.codes()
        trie = w.E.DeviceTrie.from_codes(w.ctx, codes, w.V)
        res, plain, forced, ex, _ = _run(w, trie, budget, label=f"{name} seed {seed}")
        assert ex[qa] == 1 and ex[qb] == 1 and ex[qc] == budget and ex[qd] == budget + 1 and ex[qe] == 1, ex
        assert forced[[qa, qb, qc, qe]].all() and not forced[qd]
        assert int((ex > 0).sum()) == 5 and int((forced & (ex > 0)).sum()) == POOL
        _compare(res, plain, f"{name} seed {seed}")
        tot += _check_ranges_and_survivors(w, codes, plain, forced, ex)
        if seed == 4:      # a handful of queries against the CPU oracle, the expanded ones among them
            from oracle import beam_ref, t5_ref
            from ripor_amd.utils import synth
            sel = sorted({qa, qc, qd, qe})
            pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(codes)), w.V)
            seqs, sc = beam_ref.beam_search_ref(t5_ref.T5RefCached(w.sd, w.dims), pm, w.ids[sel], w.mask[sel], w.B, w.L, use_kv_cache=True)
            ref_tok = seqs.numpy().reshape(len(sel), w.B, w.L + 1)[:, :, 1:]
            ref_sc = sc.numpy().reshape(len(sel), w.B)
            got_tok, got_sc = res.tokens[sel].cpu().numpy(), res.scores[sel].cpu().numpy()
            near = np.zeros((len(sel), w.B), dtype=bool)
            near[:, 1:] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
            near[:, :-1] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
            assert ((got_tok == ref_tok).all(axis=2) | near).all(), "sequences differ from the oracle"
            np.testing.assert_allclose(got_sc, ref_sc, atol=SCORE_TOL, rtol=0)
    print(f"[tail extras] {name}: extra sequences survived {tot[0]}, pruned {tot[1]}, first sequences that lost their slot {tot[2]}")
    assert tot[0] > 0 and tot[1] > 0 and tot[2] > 0, tot


def test_pool_exhausted_overflow_walks_on(E):
    """More expanded queries than spare entries: the first POOL in query order are forced, the others take the next stage."""
    w, budget = _world(E, "b4", 6)
    qs = sorted(w.targets([1] * (POOL + 2)))
    for q in qs:
        w.split(w.private[q][0], 2)
    res, plain, forced, ex, _ = _run(w, w.trie(), budget, label="pool exhausted")
    assert forced[qs[:POOL]].all() and not forced[qs[POOL:]].any() and (ex[qs] == 1).all() and int((ex > 0).sum()) == POOL + 2
    _compare(res, plain, "pool exhausted")


def test_modes_optimistic_lanes_fp32_log_softmax(E):
    """The same table (four expanded queries, nobody over the budget) in the optimistic mode with one fork (no leftover
    flag), split over the two lanes at 64 decoder rows, in exact fp32 and with log-softmax scores."""
    w, budget = _world(E, "b4", 9)
    h = (w.Q + 1) // 2
    # two expanded queries in each half of the batch
    lo_half = w.targets([1, 1], among=range(h))
    hi_half = w.targets([1, 2], among=range(h, w.Q))
    w.split(w.private[lo_half[0]][0], 2, at=0)
    w.split(w.private[lo_half[1]][0], 3)
    w.split(w.private[hi_half[0]][0], 2, at=w.L - w.T - 1)
    w.split(w.private[hi_half[1]][0], 2)
    w.split(w.private[hi_half[1]][1], 2)
    trie = w.trie()
    ctx = w.ctx
    res, plain, forced, ex, status = _run(w, trie, budget, mode=2, label="optimistic, one fork")
    assert forced.all() and int((ex > 0).sum()) == 4
    assert not (status & E._lib.STATUS_TAIL_LEFTOVER), "every query was forced: the optimistic mode must raise no flag"
    _compare(res, plain, "optimistic, one fork")
    res, plain, forced, ex, _ = _run(w, trie, budget, log_softmax=True, label="log-softmax")
    assert int((forced & (ex > 0)).sum()) >= 1, "log-softmax: no query was forced with extras"
    _compare(res, plain, "log-softmax")
    saved = ctx.lane_split()
    try:
        ctx.set_lane_split(64)
        if ctx.lane_split() == 64:
            assert w.Q * w.B >= 64
            res, plain, forced, ex, _ = _run(w, trie, budget, halves=True, label="two lanes")
            assert forced.all() and int((ex[:h] > 0).sum()) == 2 and int((ex[h:] > 0).sum()) == 2
            _compare(res, plain, "two lanes")
    finally:
        ctx.set_lane_split(saved if saved else 10240)
    try:
        ctx.set_precision("f32")
        res, plain, forced, ex, _ = _run(w, trie, budget, label="exact fp32")
        assert int((forced & (ex > 0)).sum()) >= 1, "exact fp32: no query was forced with extras"
        _compare(res, plain, "exact fp32")
    finally:
        ctx.set_precision("f16x2")


def test_exact_score_ties_with_extras(E, monkeypatch):
    """Output codebooks that are all zero from position 1 on (the construction of
    test_exact_score_ties_resolve_identically_on_every_path): every candidate under one first token ties exactly, at every
    step and in the final ranking, so the replay's tie rules (ascending slot * V + token inside the steps, reverse slot
    order at the end) decide who is pruned. With every tail logit exactly 0 on both sides the result must equal the plain
    loop's bit for bit, with RPR_TAIL_RANK_REPLAY on and off."""
    def zero_codebooks(sd):
        for p in range(1, CONFIGS["b4"]["L"]):
            sd[f"list_output_embeds.{p}.weight"][...] = 0.0

    w, budget = _world(E, "b4", 8, sd_edit=zero_codebooks)
    # (with tied scores the queries that share a best first token share all their beams: the nodes under the fewest queries)
    n0, n1, n2 = w.least_shared(3)
    w.split(n0, 2, at=0)
    w.split(n1, 2)
    w.split(n2, 2, at=w.L - w.T - 1)
    trie = w.trie()
    for replay in ("0", "1"):
        monkeypatch.setenv("RPR_TAIL_RANK_REPLAY", replay)
        res, plain, forced, ex, _ = _run(w, trie, budget, label=f"zero codebooks, replay {replay}")
        assert int((forced & (ex > 0)).sum()) >= 1, "no query was forced with extras"
        live = plain.scores > -1e6
        tied = int(((plain.scores[:, 1:] == plain.scores[:, :-1]) & live[:, 1:]).sum())
        assert tied > 0, "no exact ties among the returned scores"
        assert torch.equal(res.tokens[live], plain.tokens[live]) and torch.equal(res.scores[live], plain.scores[live])
        assert torch.equal(res.row_lo[live], plain.row_lo[live]) and torch.equal(res.row_hi[live], plain.row_hi[live])


def test_feature_on_without_extras_is_bit_identical_to_off(E):
    """A batch in which no query has extras: the search with the feature on returns the bits of the search with it off."""
    w, budget = _world(E, "b10", 9)
    trie = w.trie()
    assert (w.extras() == 0).all()
    w.ctx.set_forced_tail(True)
    w.ctx.set_fork_depths([w.T])
    out = {}
    for mode in (0, budget):
        w.ctx.set_tail_extras(mode)
        out[mode] = E.search(w.model, trie, w.ti, w.tm, w.B, w.L)
        torch.cuda.synchronize()
        st = w.ctx.last_fork_stats()
        assert st[0]["forced"] == w.Q and st[0]["left"] == 0, st
    a, b = out[0], out[budget]
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores)
    assert torch.equal(a.row_lo, b.row_lo) and torch.equal(a.row_hi, b.row_hi)
