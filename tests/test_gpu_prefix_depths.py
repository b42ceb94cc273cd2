"""-m gpu: one constrained search that also returns its beams at shorter prefix lengths (rpr_search_prefixes,
E.search(..., prefix_lengths=...)) against separate searches of those lengths on the same model and trie.

Beam search decides step by step: the beams of a search of length p are what a longer search holds after its p-th
selection step. Queries walking step by step at depth p are ranked there by the finalize kernel (same launches on the same
rows as the separate search: equal bits without forks); queries that left at a fork T < p are ranked by the tail pass's rule
stopped at p (a partial sum of the same gold scores: the forced-tail rule of test_gpu_forced_tail.py, restated here).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ORDER_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from ripor_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _setup(E, codes, L_model, V, seed=3, Q=24):
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=L_model, V=V, enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=seed)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=seed, max_len=14)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, sd, dims)
    trie = E.DeviceTrie.from_codes(ctx, codes, V)
    return ctx, model, trie, sd, dims, torch.from_numpy(ids), torch.from_numpy(mask)


def _bits_equal(a, b):
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores) and torch.equal(a.row_lo, b.row_lo)
            and torch.equal(a.row_hi, b.row_hi))


def _plain_loops(E, ctx, model, trie, ti, tm, B, lengths, **kw):
    """the step-by-step search (no forks) of every length: the reference of every comparison below"""
    saved = ctx.forced_tail()
    ctx.set_forced_tail(0)
    try:
        out = {p: E.search(model, trie, ti, tm, B, p, **kw) for p in lengths}
        torch.cuda.synchronize()
    finally:
        ctx.set_forced_tail(saved)
    return out


def _same_as_plain(res, plain, label):
    """test_gpu_forced_tail.py's rule: at every live rank tokens equal or scores within ORDER_TOL; max score difference
    <= 0.3 * SCORE_TOL; ranges equal wherever tokens are equal and live. No rank is left out."""
    assert res.tokens.shape == plain.tokens.shape, (label, res.tokens.shape, plain.tokens.shape)
    same = (res.tokens == plain.tokens).all(dim=2)
    close = (res.scores - plain.scores).abs() <= ORDER_TOL
    live = plain.scores > -1e6                   # dead beams (-1e9) carry arbitrary masked tokens in both paths
    err = float(((res.scores - plain.scores).abs() * live).max())
    print(f"[prefix depths] {label}: max score diff {err:.2e}, {int((same & live).sum())}/{int(live.sum())} live ranks identical")
    assert bool((same | close | ~live).all()), f"{label}: sequences differ from the step-by-step loop"
    assert err <= 0.3 * SCORE_TOL, (label, err)
    both = same & live
    assert torch.equal(res.row_lo[both], plain.row_lo[both]) and torch.equal(res.row_hi[both], plain.row_hi[both]), label


def _check_all(res, plain, L, depths, label):
    assert sorted(res.prefixes) == list(depths)
    for p in depths:
        _same_as_plain(res.prefixes[p], plain[p], f"{label}, depth {p}")
    _same_as_plain(res, plain[L], f"{label}, final")


def test_no_forks_equal_bits_and_graph_replay(E):
    """Case 1: forced tail off, trie deeper than the search. The first p steps of the search are the launches of the separate
    search of length p on the same rows: every output must carry the same bits; so must a graph replay, and the plain search
    of the full length before and after."""
    from ripor_amd.utils import synth
    Lc, L, V, B, N, depths = 8, 8, 256, 10, 30_000, (2, 5)
    codes = synth.make_codes(N, Lc, V, seed=31)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, Lc, V, Q=24)
    ctx.set_forced_tail(0)
    try:
        before = E.search(model, trie, ti, tm, B, L)
        sep = {p: E.search(model, trie, ti, tm, B, p) for p in depths}
        a = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        b = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        after = E.search(model, trie, ti, tm, B, L)
        torch.cuda.synchronize()
        assert ctx.last_fork_stats() == []
    finally:
        ctx.set_forced_tail(1)
    assert _bits_equal(before, after)
    assert _bits_equal(a, before) and _bits_equal(b, before)
    for p in depths:
        assert a.prefixes[p].tokens.shape == (24, B, p)
        assert _bits_equal(a.prefixes[p], sep[p]), f"depth {p} differs from the separate search"
        assert _bits_equal(b.prefixes[p], sep[p]), f"depth {p}: graph replay differs"


def test_forks_before_the_depths(E):
    """Case 2: the dense trie on which the fork at 2 takes a share of the queries and the fork at 3 most of the rest. Depth 3
    comes from the first tail pass for the queries forced at 2 and from the stage's finalize (before the second fork
    classifies) for the others; depths 4 and 8 from both tail passes and the last stage. Then the automatic forks, and
    the CPU oracle on six queries."""
    from oracle import beam_ref, t5_ref
    from ripor_amd.utils import synth
    L, V, B, N, depths = 12, 256, 10, 60_000, (3, 4, 8)
    codes = synth.make_codes(N, L, V, seed=11)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, L, V, Q=48)
    plain = _plain_loops(E, ctx, model, trie, ti, tm, B, depths + (L,))
    ctx.set_forced_tail(1)
    ctx.set_fork_depths([2, 3])
    try:
        res = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        torch.cuda.synchronize()
        st = ctx.last_fork_stats()
    finally:
        ctx.set_fork_depths(None)
    # (measured: the fork at 2 forces none of the 48 queries of this trie — 0.92 documents per depth-2 prefix, ten beams all on
    # single-sequence nodes is a 1 % event — so here depth 3 comes from the stage's finalize for every query; the sparser trie
    # of test_queries_forced_before_a_depth_are_ranked_by_the_tail has queries leave at both forks)
    assert [f["depth"] for f in st] == [2, 3] and st[1]["forced"] > 0 and st[0]["left"] > 0, st
    _check_all(res, plain, L, depths, "dense 60k forks [2, 3]")
    auto = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
    torch.cuda.synchronize()
    st = ctx.last_fork_stats()
    assert [f["depth"] for f in st] == ctx.fork_depths(model, trie, 48, B, L) and st[0]["forced"] > 0, st
    _check_all(auto, plain, L, depths, f"dense 60k automatic forks {[f['depth'] for f in st]}")
    # the oracle (the KV-cached CPU restatement of the reference loop) at every depth on a few queries
    nq = 6
    pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(codes)), V)
    ref_model = t5_ref.T5RefCached(sd, dims)
    for p in depths:
        seqs, sc = beam_ref.beam_search_ref(ref_model, pm, ti[:nq].numpy(), tm[:nq].numpy(), B, p, use_kv_cache=True)
        ref_tok, ref_sc = seqs.numpy().reshape(nq, B, p + 1)[:, :, 1:], sc.numpy().reshape(nq, B)
        near = np.zeros((nq, B), dtype=bool)
        near[:, 1:] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
        near[:, :-1] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
        for r in (res, auto):
            got_tok, got_sc = r.prefixes[p].tokens[:nq].cpu().numpy(), r.prefixes[p].scores[:nq].cpu().numpy()
            assert ((got_tok == ref_tok).all(axis=2) | near).all(), f"depth {p}: sequences differ from the oracle"
            np.testing.assert_allclose(got_sc, ref_sc, atol=SCORE_TOL, rtol=0)


def test_queries_forced_before_a_depth_are_ranked_by_the_tail(E):
    """Case 2 on a trie where the fork at 2 does take queries (20 000 documents under 65 536 depth-2 prefixes: a beam's node
    holds one sequence with probability ~0.85, all ten with ~0.2): forced > 0 at both forks and left > 0 at the first, so
    depth 3 comes from the first tail pass for the queries forced at 2 and from the stage's finalize, before the second
    fork classifies, for the rest."""
    from ripor_amd.utils import synth
    L, V, B, N, depths = 12, 256, 10, 20_000, (3, 4, 8)
    codes = synth.make_codes(N, L, V, seed=11)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, L, V, Q=48)
    plain = _plain_loops(E, ctx, model, trie, ti, tm, B, depths + (L,))
    ctx.set_forced_tail(1)
    ctx.set_fork_depths([2, 3])
    try:
        res = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        torch.cuda.synchronize()
        st = ctx.last_fork_stats()
    finally:
        ctx.set_fork_depths(None)
    assert [f["depth"] for f in st] == [2, 3] and st[0]["forced"] > 0 and st[1]["forced"] > 0 and st[0]["left"] > 0, st
    _check_all(res, plain, L, depths, f"20k forks [2, 3] {st}")


def test_exact_ties_at_the_depths(E, monkeypatch):
    """Case 3: codebooks with pairwise identical rows / all-zero codebooks from position 1 on tie candidates exactly, inside
    the steps and up to the ranking of every depth. The tail ranking stopped at p must detect the ties and replay p - T
    steps: the same bits as with the replay forced, and the plain loop's tokens."""
    from ripor_amd.utils import synth
    L, V, N, B, depths = 12, 256, 40_000, 12, (3, 4, 8)
    codes = synth.make_codes(N, L, V, seed=21)
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    ids, mask = synth.make_queries(6, vocab_size=dims.vocab_size, seed=4, max_len=14)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    ctx = E.Context.get(0)
    trie = E.DeviceTrie.from_codes(ctx, codes, V)
    for variant in ("paired rows", "zero codebooks"):
        sd = synth.make_state_dict(dims, seed=6)
        for p in range(L):
            w = sd[f"list_output_embeds.{p}.weight"]
            if variant == "paired rows":
                w[1::2] = w[0::2]
            elif p >= 1:
                w[...] = 0.0
        model = E.DeviceModel(ctx, sd, dims)
        monkeypatch.delenv("RPR_TAIL_RANK_REPLAY", raising=False)
        plain = _plain_loops(E, ctx, model, trie, ti, tm, B, depths)
        ctx.set_forced_tail(1)
        a = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        torch.cuda.synchronize()
        st = ctx.last_fork_stats()
        assert st and st[0]["forced"] > 0 and st[0]["depth"] < depths[-1], (variant, st)
        monkeypatch.setenv("RPR_TAIL_RANK_REPLAY", "1")
        b = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths)
        torch.cuda.synchronize()
        monkeypatch.delenv("RPR_TAIL_RANK_REPLAY")
        assert _bits_equal(a, b), variant
        for p in depths:
            assert _bits_equal(a.prefixes[p], b.prefixes[p]), (variant, p)
            live = plain[p].scores > -1e6
            assert torch.equal(a.prefixes[p].tokens[live], plain[p].tokens[live]), (variant, p)


@pytest.mark.parametrize("shape", ["log_softmax", "beam1", "beam100", "lane_split"])
def test_other_shapes(E, shape):
    """Case 4: log-softmax scores with a fork at 2; one beam; beam 100 with 4 queries (the radix selection, the rank-data
    pass's flags) at L = 8, depth 4, automatic forks; a lane-split threshold the batch exceeds (the call runs unsplit)."""
    from ripor_amd.utils import synth
    V = 256
    kw, seed = {}, 51
    if shape == "beam100":
        L, B, Q, N, depths, forks = 8, 100, 4, 50_000, (4,), None
    elif shape == "beam1":
        L, B, Q, N, depths, forks = 8, 1, 24, 40_000, (3, 5), [2, 4]
    elif shape == "log_softmax":
        L, B, Q, N, depths, forks, seed = 12, 4, 16, 20_000, (3, 6), [2], 11
        kw = dict(apply_log_softmax_for_scores=True)
    else:
        L, B, Q, N, depths, forks = 8, 10, 40, 50_000, (4, 6), [3, 4]
    codes = synth.make_codes(N, L, V, seed=seed)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, L, V, Q=Q)
    plain = _plain_loops(E, ctx, model, trie, ti, tm, B, depths + (L,), **kw)
    saved = ctx.lane_split()
    ctx.set_forced_tail(1)
    ctx.set_fork_depths(forks)
    if shape == "lane_split":
        ctx.set_lane_split(64)               # 40 queries x 10 beams >= 64 rows: a plain call would run as two lanes
    try:
        res = E.search(model, trie, ti, tm, B, L, prefix_lengths=depths, **kw)
        torch.cuda.synchronize()
        st = ctx.last_fork_stats()
    finally:
        ctx.set_fork_depths(None)
        ctx.set_lane_split(saved)
    if shape == "lane_split":
        assert st[0]["forced"] + st[0]["left"] == Q, st    # one workspace saw every query
    if forks is not None:
        assert [f["depth"] for f in st] == forks, st
    assert sum(f["forced"] for f in st) > 0, st           # some query's depths come from a tail pass
    _check_all(res, plain, L, depths, f"{shape} forks {[f['depth'] for f in st]}")


def test_optimistic_mode_leftover_is_repeated_with_the_same_depths(E):
    """Case 5: forks [1, 2] on the dense trie leave queries unforced at the last fork: the optimistic call raises the
    leftover flag, search_guarded repeats the batch in the exact mode with the same prefix lengths."""
    from ripor_amd.utils import synth
    L, V, B, depths = 8, 256, 10, (3, 5)
    codes = synth.make_codes(60_000, L, V, seed=11)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, L, V, Q=48)
    plain = _plain_loops(E, ctx, model, trie, ti, tm, B, depths + (L,))
    ctx.set_forced_tail(1)
    ctx._leftover_streak, ctx._exact_calls_left = 0, 0
    ctx.set_fork_depths([1, 2])
    try:
        g = E.search_guarded(model, trie, ti, tm, B, L, optimistic=True, prefix_lengths=depths)
        r = g.result()
        assert g.repeated and ctx.forced_tail() == 1
        with pytest.raises(ValueError):
            E.search_guarded(model, trie, ti, tm, B, L, margin_guard=1e-3, prefix_lengths=depths)
    finally:
        ctx.set_fork_depths(None)
        ctx._leftover_streak, ctx._exact_calls_left = 0, 0
    _check_all(r, plain, L, depths, "guard's exact repeat, forks [1, 2]")


def test_refusals_leave_the_outputs_untouched(E):
    """Case 6: unsorted, repeated, out-of-range and too many prefix lengths are refused with status -1 before anything is
    written."""
    from ripor_amd.utils import synth
    L, V, B, Q = 8, 256, 4, 3
    codes = synth.make_codes(5_000, L, V, seed=7)
    ctx, model, trie, sd, dims, ti, tm = _setup(E, codes, L, V, Q=Q)
    dev = ctx.device
    ids = ti.to(device=dev, dtype=torch.int32).contiguous()
    mask = tm.to(device=dev, dtype=torch.int32).contiguous()
    Lq = ids.shape[1]

    def call(depths, null_at=None):
        n = len(depths)
        tok = torch.full((Q, B, L), -7, dtype=torch.int32, device=dev)
        sc = torch.full((Q, B), -7.0, dtype=torch.float32, device=dev)
        lo = torch.full((Q, B), -7, dtype=torch.int64, device=dev)
        hi = torch.full((Q, B), -7, dtype=torch.int64, device=dev)
        d = [(torch.full((Q, B, L), -7, dtype=torch.int32, device=dev), torch.full((Q, B), -7.0, dtype=torch.float32, device=dev),
              torch.full((Q, B), -7, dtype=torch.int64, device=dev), torch.full((Q, B), -7, dtype=torch.int64, device=dev))
             for _ in range(n)]
        arr = lambda j: (C.c_void_p * n)(*[None if null_at == (k, j) else d[k][j].data_ptr() for k in range(n)])
        status = ctx.lib.rpr_search_prefixes(ctx.handle, model.handle, trie.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq, B, L, 0,
                                             tok.data_ptr(), sc.data_ptr(), lo.data_ptr(), hi.data_ptr(), n,
                                             (C.c_int32 * n)(*depths), arr(0), arr(1), arr(2), arr(3), None)
        torch.cuda.synchronize()
        flat = [tok, sc, lo, hi] + [t for k in d for t in k]
        return status, all(bool((t == -7).all()) for t in flat)

    for depths in ((4, 4), (5, 3), (0,), (L,), (1, 2, 3, 4)):
        status, untouched = call(depths)
        assert status == -1 and untouched, (depths, status, untouched)
    status, untouched = call((2, 4), null_at=(1, 2))
    assert status == -1 and untouched
    status, untouched = call((2, 4))
    assert status == 0 and not untouched
    with pytest.raises(ValueError):
        E.search(model, trie, ti, tm, B, L, prefix_lengths=(2,), margins=True)


def test_rankdata_files_of_one_search_equal_those_of_separate_runs(E, tmp_path):
    """Case 7: constrained_decode_smtid on an in-memory model, forced tail off. max_new_token = 8 with {4: dir} writes into
    dir what a separate max_new_token = 4 run writes, and into the main directory what a plain run writes."""
    import json
    import os
    from ripor_amd import evaluate
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder
    from ripor_amd.tasks.generation import PrefixConstrainLogitProcessorFastSparse
    from ripor_amd.utils import synth
    L, V, N, B = 8, 256, 600, 5
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    model = T5SeqAQEncoder.from_synthetic(dims, seed=77).to(0)
    model.eval()
    model.base_model.config.decoding = True
    codes = synth.make_codes(N, L, V, seed=77)
    proc = PrefixConstrainLogitProcessorFastSparse.from_codes(codes, V)
    table = evaluate.DocidTable([str(100 + i) for i in range(N)])
    ids, mask = synth.make_queries(7, vocab_size=dims.vocab_size, seed=5, max_len=14)
    loader = [{"id": torch.arange(900 + i, 900 + min(i + 4, 7)), "input_ids": torch.from_numpy(ids[i:i + 4]),
               "attention_mask": torch.from_numpy(mask[i:i + 4])} for i in (0, 4)]
    dirs = {k: str(tmp_path / k) for k in ("one", "one4", "plain8", "plain4")}
    for d in ("one", "plain8", "plain4"):
        os.makedirs(dirs[d])
    ctx = E.Context.get(0)
    ctx.set_forced_tail(0)
    try:
        evaluate.constrained_decode_smtid(model.base_model, loader, proc, table, 8, 0, dirs["one"], 0, topk=B,
                                          prefix_out_dirs={4: dirs["one4"]})
        evaluate.constrained_decode_smtid(model.base_model, loader, proc, table, 8, 0, dirs["plain8"], 0, topk=B)
        evaluate.constrained_decode_smtid(model.base_model, loader, proc, table, 4, 0, dirs["plain4"], 0, topk=B)
    finally:
        ctx.set_forced_tail(1)
    load = lambda d: json.load(open(os.path.join(dirs[d], "qid_smtid_rankdata_0.json")))
    one4, plain4 = load("one4"), load("plain4")
    assert set(one4) == {str(900 + i) for i in range(7)}
    assert all(len(s.split("_")) == 4 for q in one4.values() for s in q) and all(len(q) == B for q in one4.values())
    assert one4 == plain4
    assert load("one") == load("plain8")
