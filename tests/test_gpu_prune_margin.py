"""-m gpu: per-query pruning margins (rpr_search_margins, ripor_amd/csrc/prune_margin.hip) and the near-tie guard built on
them (ripor_amd/engine.py: search_guarded(margin_guard=...), evaluate.py --near_tie_guard).

The margin of a query is the smallest gap, over the decode steps, between the last kept candidate (rank B-1) and the first
dropped live one (rank B): conftest.prune_margins on the reference's goldens, tests/prune_margin_ref.py on a search's own taps.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PRUNE_TOL, prune_margins
from prune_margin_ref import prune_margin_ref, unpack_valid

pytestmark = pytest.mark.gpu

# small beams (single-block selection), a vocabulary of 1024, padded vocabulary columns (V = 100), log-softmax scores, shared
# in/out codebooks, 32 steps, and 100 beams (the radix selection)
GOLDENS = ["g1_mini_b4_l8", "g1_mini_b2_l4_v1024", "g1_mini_b4_l8_v100", "g1_mini_b4_l8_logsoftmax", "g1_mini_b4_l8_shared",
           "g1_mini_b10_l32", "g6_base_v1024_b100_l16"]
TAPPED = [n for n in GOLDENS if "logsoftmax" not in n and "_v100" not in n]   # (the taps need V % 64 == 0)


@pytest.fixture(scope="module")
def E():
    from ripor_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def built(E, golden_cache):
    """golden name -> (golden, ctx, model, trie), built once per module"""
    cache = {}

    def get(name):
        if name not in cache:
            g = golden_cache(name)
            ctx = E.Context.get(0)
            cache[name] = (g, ctx, E.DeviceModel(ctx, g.state_dict, g.dims), E.DeviceTrie.from_codes(ctx, g.codes, g.V))
        return cache[name]

    return get


def _run(E, g, model, trie, **kw):
    res = E.search(model, trie, torch.from_numpy(g.input_ids), torch.from_numpy(g.attention_mask), g.B, g.L,
                   apply_log_softmax_for_scores=g.log_softmax, **kw)
    torch.cuda.synchronize()
    return res


def _margins(E, g, model, trie, **kw):
    return _run(E, g, model, trie, margins=True, **kw).margins.cpu().numpy()


def _within_bound(got, want, label):
    """inf where the other has inf, otherwise within PRUNE_TOL; returns the worst difference"""
    assert got.dtype == np.float64 and not np.isnan(got).any(), (label, got)
    assert (np.isinf(got) == np.isinf(want)).all(), (label, got, want)
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"[margin] {label}: {int(fin.sum())}/{len(want)} finite, worst difference {err:.3g}")
    assert err <= PRUNE_TOL, (label, err)
    return err


def _same_result(a, b):
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores) and torch.equal(a.row_lo, b.row_lo)
            and torch.equal(a.row_hi, b.row_hi))


# ---- 1. against the reference goldens ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x2", "f32"])
@pytest.mark.parametrize("name", GOLDENS)
def test_margins_match_the_reference_goldens(E, built, name, prec):
    """|margin - prune_margins(golden)| <= PRUNE_TOL, inf where the reference has inf: an error beyond the guard's own
    threshold would make the guard meaningless. Measured on MI355X: see DESIGN.md 5f."""
    g, ctx, model, trie = built(name)
    ctx.set_precision(prec)
    try:
        got = _margins(E, g, model, trie)
    finally:
        ctx.set_precision("f16x2")
    _within_bound(got, prune_margins(g)[0], f"{name} {prec}")


# ---- 2. bit-exact against the device's own taps ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TAPPED)
def test_margins_equal_the_restatement_on_the_runs_own_taps(E, built, name):
    """The same float64 adds on the same float32 logits, bitmap and beam scores: equal with == (tapped runs are eager, unforked,
    unshared step 0: single-block selection below 32 beams, the five-launch radix selection from 32 on)."""
    g, ctx, model, trie = built(name)
    res = _run(E, g, model, trie, taps=True, margins=True)
    t = res.taps
    want = prune_margin_ref(t["step_logits"].cpu().numpy(), unpack_valid(t["step_valid"].cpu().numpy(), g.B, g.V),
                            t["step_scores"].cpu().numpy(), g.B)
    got = res.margins.cpu().numpy()
    assert (got == want).all(), (name, got, want)
    # the untapped search of the same batch computes step 0 once per query and forks (tail passes, compacted stages): other
    # GEMM shapes, so the bound of the golden test, not ==
    _within_bound(_margins(E, g, model, trie), got, f"{name} untapped vs tapped")


# ---- 3. route independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1_mini_b4_l8", "g1_mini_b4_l8_logsoftmax", "g6_base_v1024_b100_l16"])
def test_graph_replay_and_eager_launches_agree(E, built, name):
    g, ctx, model, trie = built(name)
    first = _margins(E, g, model, trie)            # captures (or replays) the margin-mode graph
    assert (_margins(E, g, model, trie) == first).all()                       # replay
    assert (_margins(E, g, model, trie, use_graph=False) == first).all()      # RPR_FLAG_NO_GRAPH


@pytest.mark.parametrize("name", ["g1_mini_b4_l8", "g1_mini_b4_l8_v100", "g1_mini_b4_l8_logsoftmax", "g1_mini_b10_l32",
                                  "g6_base_v1024_b100_l16"])
def test_radix_and_single_block_selection_agree(E, built, name, monkeypatch):
    """RPR_SELECT_RADIX=0 / 1 as tests/test_gpu_select_radix.py switches them: the margin kernel reads the bitmap either path
    exports and derives the shared step 0 itself."""
    g, ctx, model, trie = built(name)
    monkeypatch.setenv("RPR_SELECT_RADIX", "0")
    single = _run(E, g, model, trie, margins=True)
    monkeypatch.setenv("RPR_SELECT_RADIX", "1")
    radix = _run(E, g, model, trie, margins=True)
    assert _same_result(single, radix)
    assert torch.equal(single.margins, radix.margins), (single.margins, radix.margins)


@pytest.fixture(scope="module")
def dense(E):
    """60k docs under 65k depth-2 prefixes (tests/test_gpu_forced_tail.py): at beam 10 no query is forced at depth 2, nearly all
    are at depth 3 and the rest walks on through a compacted stage; nearly every query has a finite margin."""
    from ripor_amd.utils import synth
    L, V, B, N, Q = 12, 256, 10, 60_000, 48
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=3)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=3, max_len=14)
    ctx = E.Context.get(0)
    return dict(ctx=ctx, model=E.DeviceModel(ctx, sd, dims), trie=E.DeviceTrie.from_codes(ctx, synth.make_codes(N, L, V, seed=11), V),
                ids=torch.from_numpy(ids), mask=torch.from_numpy(mask), B=B, L=L, Q=Q)


def test_forced_tail_on_and_off_agree(E, dense):
    """Explicit fork depths so that a compacted stage with live queries exists. A query forced at the FIRST fork has taken the
    same launches as in the plain loop up to there and contributes nothing afterwards: equal with ==. A query
    that walks on in a compacted stage runs its later steps with fewer rows than the plain loop, which may take another GEMM
    route there: the bound of the golden test instead."""
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    try:
        ctx.set_forced_tail(0)
        plain = E.search(*args, margins=True)
        ctx.set_forced_tail(1)
        ctx.set_fork_depths([3, 5])
        forked = E.search(*args, margins=True)
        torch.cuda.synchronize()
        stats = ctx.last_fork_stats()
    finally:
        ctx.set_forced_tail(1)
        ctx.set_fork_depths(None)
    assert stats[0]["forced"] > 0 and stats[0]["left"] > 0, stats   # a tail pass, and a compacted stage with live queries
    a, b = plain.margins.cpu().numpy(), forked.margins.cpu().numpy()
    assert np.isfinite(a).sum() >= d["Q"] // 2, "the fixture has too few finite margins to say anything"
    _within_bound(b, a, "forks [3, 5] vs plain loop")
    assert int((a == b).sum()) >= stats[0]["forced"], (int((a == b).sum()), stats)


def test_lane_split_on_and_off_agree(E, dense):
    """Each half writes its own slice of out_margin. A half batch may take another GEMM route than the whole one
    (tests/test_gpu_edges.py: scores within summation-order noise), so split vs unsplit is held to the bound of the golden
    test; replay and eager launches of the split call itself agree with ==."""
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"][:37], d["mask"][:37], d["B"], d["L"])   # an odd batch: halves of 19 and 18
    saved = ctx.lane_split()
    try:
        ctx.set_lane_split(64)
        if ctx.lane_split() == 0:                # lane_split() creates the two masked streams itself, once per ctx
            pytest.skip("CU-masked streams unavailable on this device")
        ctx.set_lane_split(0)
        whole = E.search(*args, margins=True)
        torch.cuda.synchronize()
        ctx.set_lane_split(64)
        split = E.search(*args, margins=True)
        again = E.search(*args, margins=True, use_graph=False)
        torch.cuda.synchronize()
        # two lanes ran: the lanes exist (their creation is remembered by the ctx, so the search found them too) and the
        # batch of 370 decoder rows is above the threshold in force
        assert ctx.lane_split() == 64 and args[2].shape[0] * d["B"] >= 64
    finally:
        ctx.set_lane_split(saved if saved else 10240)
    assert torch.equal(split.tokens, whole.tokens)
    _within_bound(split.margins.cpu().numpy(), whole.margins.cpu().numpy(), "two lanes vs one")
    assert torch.equal(split.margins, again.margins)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------
def test_fewer_docs_than_beams_gives_inf(E, built):
    g, ctx, model, trie = built("g1_mini_b10_l8_tiny_trie")
    got = _margins(E, g, model, trie)
    assert np.isinf(got).all() and (got > 0).all(), got
    assert np.isinf(prune_margins(g)[0]).all()


def _search_margins_into(E, model, trie, ids, mask, B, L, out_margin):
    """rpr_search_margins straight through the binding, into a caller-prepared out_margin"""
    ctx = model.ctx
    dev = ctx.device
    ids = ids.to(device=dev, dtype=torch.int32).contiguous()
    mask = mask.to(device=dev, dtype=torch.int32).contiguous()
    Q, Lq = ids.shape
    pad = (-Lq) % 8                       # the padded length E.search would pass: the same launches
    ids, mask = torch.nn.functional.pad(ids, (0, pad)).contiguous(), torch.nn.functional.pad(mask, (0, pad)).contiguous()
    Lq += pad
    tokens = torch.empty((Q, B, L), dtype=torch.int32, device=dev)
    scores = torch.empty((Q, B), dtype=torch.float32, device=dev)
    lo = torch.empty((Q, B), dtype=torch.int64, device=dev)
    hi = torch.empty((Q, B), dtype=torch.int64, device=dev)
    E.check(ctx.lib.rpr_search_margins(ctx.handle, model.handle, trie.handle, ids.data_ptr(), mask.data_ptr(), Q, Lq, B, L, 0,
                                       tokens.data_ptr(), scores.data_ptr(), lo.data_ptr(), hi.data_ptr(), out_margin.data_ptr(),
                                       None, E._stream_ptr(dev)), "rpr_search_margins")
    torch.cuda.synchronize()
    return tokens, scores


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_equal_codebook_rows_tie_exactly_and_single_query(E, prec):
    """Position-0 output codebook rows all equal: every child of the root carries the same logit, the root has more than B
    children, so rank B-1 and rank B tie exactly at step 0 and the margin is 0.0 — for one query (Q = 1) and for several, with
    out_margin poisoned with NaN before the call (it must be written, never read)."""
    from ripor_amd.utils import synth
    L, V, B, N = 6, 256, 4, 2000
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    sd = dict(synth.make_state_dict(dims, seed=9))
    w = np.array(sd["list_output_embeds.0.weight"], copy=True)
    w[:] = w[0]
    sd["list_output_embeds.0.weight"] = w
    codes = synth.make_codes(N, L, V, seed=9)
    assert len(np.unique(codes[:, 0])) > B
    ctx = E.Context.get(0)
    model, trie = E.DeviceModel(ctx, sd, dims), E.DeviceTrie.from_codes(ctx, codes, V)
    ids, mask = synth.make_queries(5, vocab_size=dims.vocab_size, seed=9, max_len=10)
    ctx.set_precision(prec)
    try:
        for Q in (1, 5):
            out = torch.full((Q,), float("nan"), dtype=torch.float64, device=ctx.device)
            _search_margins_into(E, model, trie, torch.from_numpy(ids[:Q]), torch.from_numpy(mask[:Q]), B, L, out)
            got = out.cpu().numpy()
            assert (got == 0.0).all() and not np.signbit(got).any(), (prec, Q, got)
    finally:
        ctx.set_precision("f16x2")


def test_out_margin_is_written_not_read(E, built):
    g, ctx, model, trie = built("g1_mini_b4_l8")
    want = _margins(E, g, model, trie, use_graph=False)
    for fill in (float("nan"), -1.0):
        out = torch.full((g.Q,), fill, dtype=torch.float64, device=ctx.device)
        _search_margins_into(E, model, trie, torch.from_numpy(g.input_ids), torch.from_numpy(g.attention_mask), g.B, g.L, out)
        got = out.cpu().numpy()
        assert not np.isnan(got).any() and (got >= 0).all()
    assert (got == want).all(), (got, want)


# ---- 5. the default search is unchanged --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_search_and_search_margins_return_the_same_bits(E, built, name):
    g, ctx, model, trie = built(name)
    for kw in ({}, {"use_graph": False}):
        assert _same_result(_run(E, g, model, trie, **kw), _run(E, g, model, trie, margins=True, **kw)), (name, kw)
    assert _run(E, g, model, trie).margins is None


# ---- 6. the near-tie guard -------------------------------------------------------------------------------------------------------
def _f32_search(E, ctx, *args, **kw):
    ctx.set_precision("f32")
    try:
        res = E.search(*args, **kw)
        torch.cuda.synchronize()
    finally:
        ctx.set_precision("f16x2")
    return res


def test_guard_off_is_the_unguarded_search(E, dense):
    d = dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    res = E.search_guarded(*args).result()
    assert res.margins is None and res.rerun is None and res.margins_f32 is None
    plain = E.search(*args)
    torch.cuda.synchronize()
    assert _same_result(res, plain)


def test_guard_inf_reruns_everything_in_f32(E, dense):
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    res = E.search_guarded(*args, margin_guard=float("inf")).result()
    assert ctx.get_precision() == "f16x2"
    assert bool(res.rerun.all()) and res.margins_f32.shape[0] == d["Q"]
    want = _f32_search(E, ctx, *args, margins=True)
    assert _same_result(res, want)
    assert torch.equal(res.margins_f32, want.margins)


def test_guard_threshold_between_two_margins(E, dense):
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    base = E.search(*args, margins=True)
    torch.cuda.synchronize()
    m = base.margins.cpu().numpy()
    srt = np.unique(m[np.isfinite(m)])
    assert len(srt) >= 6
    eps = float((srt[2] + srt[3]) / 2)              # three queries (or more, on ties) below it
    res = E.search_guarded(*args, margin_guard=eps).result()
    assert ctx.get_precision() == "f16x2"
    rerun = res.rerun.numpy()
    assert (rerun == (m < eps)).all() and 0 < rerun.sum() < d["Q"]
    assert torch.equal(res.margins, base.margins)
    keep = torch.from_numpy(~rerun).to(base.tokens.device)
    for got, ref in ((res.tokens, base.tokens), (res.scores, base.scores), (res.row_lo, base.row_lo), (res.row_hi, base.row_hi)):
        assert torch.equal(got[keep], ref[keep]), "a row outside the re-run changed"
    sel = torch.from_numpy(rerun)
    sub = _f32_search(E, ctx, d["model"], d["trie"], d["ids"][sel], d["mask"][sel], d["B"], d["L"], margins=True)
    pick = sel.to(base.tokens.device)
    for got, ref in ((res.tokens, sub.tokens), (res.scores, sub.scores), (res.row_lo, sub.row_lo), (res.row_hi, sub.row_hi)):
        assert torch.equal(got[pick], ref), "a re-run row is not the f32 search of the sub-batch"
    assert torch.equal(res.margins_f32, sub.margins)


def test_guard_rerun_is_exact_on_an_optimistic_ctx(E, dense):
    """A ctx in the optimistic forced-tail mode (ctx.set_forced_tail(2)) with fork depths that leave queries behind at the last
    fork (forks [1, 2] on this trie, tests/test_gpu_forced_tail.py): a search of the re-run sub-batch in that mode raises
    STATUS_TAIL_LEFTOVER and its rows are unspecified. The guard's re-run is reported as the exact fp32 result, so it must run
    in the exact mode: its rows equal an exact-mode f32 search of that sub-batch, and mode and precision come back."""
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    try:
        ctx.set_fork_depths([1, 2])
        ctx.set_forced_tail(1)
        base = E.search(*args, margins=True)
        torch.cuda.synchronize()
        m = base.margins.cpu().numpy()
        srt = np.unique(m[np.isfinite(m)])
        assert len(srt) >= 6
        eps = float((srt[len(srt) // 2 - 1] + srt[len(srt) // 2]) / 2)      # about half of the batch below it
        ctx.set_forced_tail(2)
        ctx.status(clear=True)
        guard = E.search_guarded(*args, margin_guard=eps)
        res = guard.result()
        assert guard.repeated                      # the first search itself left queries behind: repeated in the exact mode
        assert ctx.forced_tail() == 2 and ctx.get_precision() == "f16x2"
        assert torch.equal(res.margins, base.margins)
        rerun = res.rerun.numpy()
        assert (rerun == (m < eps)).all() and 0 < rerun.sum() < d["Q"]
        sel = torch.from_numpy(rerun)
        sub_args = (d["model"], d["trie"], d["ids"][sel], d["mask"][sel], d["B"], d["L"])
        # the fixture does what it is for: in the optimistic mode the sub-batch leaves a query behind
        _f32_search(E, ctx, *sub_args, margins=True)
        assert ctx.last_fork_stats()[-1]["left"] > 0
        assert ctx.status(clear=True) & E._lib.STATUS_TAIL_LEFTOVER
        ctx.set_forced_tail(1)
        sub = _f32_search(E, ctx, *sub_args, margins=True)
        assert ctx.status(clear=True) == 0
        pick = sel.to(base.tokens.device)
        for got, ref in ((res.tokens, sub.tokens), (res.scores, sub.scores), (res.row_lo, sub.row_lo), (res.row_hi, sub.row_hi)):
            assert torch.equal(got[pick], ref), "a re-run row is not the exact-mode f32 search of the sub-batch"
        assert torch.equal(res.margins_f32, sub.margins)
        keep = torch.from_numpy(~rerun).to(base.tokens.device)
        assert torch.equal(res.tokens[keep], base.tokens[keep]) and torch.equal(res.scores[keep], base.scores[keep])
    finally:
        ctx.set_fork_depths(None)
        ctx.set_forced_tail(1)
        ctx.set_precision("f16x2")
        ctx.status(clear=True)
        ctx._leftover_streak, ctx._exact_calls_left = 0, 0     # the lost bet above is this test's own


def test_guard_on_an_f32_context_reruns_nothing(E, dense):
    ctx, d = dense["ctx"], dense
    args = (d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"])
    ctx.set_precision("f32")
    try:
        res = E.search_guarded(*args, margin_guard=float("inf")).result()
        assert ctx.get_precision() == "f32"
    finally:
        ctx.set_precision("f16x2")
    assert not bool(res.rerun.any()) and res.margins_f32.numel() == 0 and res.margins.shape[0] == d["Q"]
    assert _same_result(res, _f32_search(E, ctx, *args))


def test_guard_restores_the_precision_when_the_rerun_raises(E, dense, monkeypatch):
    ctx, d = dense["ctx"], dense
    guard = E.search_guarded(d["model"], d["trie"], d["ids"], d["mask"], d["B"], d["L"], margin_guard=float("inf"))

    def boom(*a, **k):
        assert ctx.get_precision() == "f32"
        raise RuntimeError("re-run failed")

    monkeypatch.setattr(E, "search", boom)
    with pytest.raises(RuntimeError, match="re-run failed"):
        guard.result()
    assert ctx.get_precision() == "f16x2"


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_near_tie_guard_writes_near_tie_json(tmp_path):
    from test_gpu_cli import _make_world, _run as _cli
    ckpt, d2s_path, qdir, codes, queries, dims = _make_world(str(tmp_path))
    B, L = 5, 8
    common = ["-m", "t5_pretrainer.evaluate", f"--pretrained_path={ckpt}", "--task=t5seq_aq_retrieve_docids",
              f"--docid_to_smtid_path={d2s_path}", "--q_collection_paths=" + json.dumps([qdir]), "--batch_size=4",
              f"--max_new_token_for_docid={L}", f"--topk={B}"]
    plain_dir, guard_dir = os.path.join(str(tmp_path), "plain"), os.path.join(str(tmp_path), "guarded")
    out_plain = _cli(common + [f"--out_dir={plain_dir}"])
    assert sorted(os.listdir(os.path.join(plain_dir, "MSMARCO"))) == ["run_0.json"]      # today's files, nothing else
    out_guard = _cli(common + [f"--out_dir={guard_dir}", "--near_tie_guard=0.5"])
    assert sorted(os.listdir(os.path.join(guard_dir, "MSMARCO"))) == ["near_tie.json", "run_0.json"]
    rec = json.load(open(os.path.join(guard_dir, "MSMARCO", "near_tie.json")))
    assert rec["threshold"] == 0.5 and rec["queries"] == len(queries)
    # the guard fired: with 600 docs the root has far more than 5 children, so every query drops live candidates at step 0,
    # and rank 4 and rank 5 of some 200 sorted mini-model scores are not 0.5 apart (a flag ignored downstream gives 0 here)
    assert 0 < rec["rerun_fp32"] == len(rec["rerun_qids"]) <= rec["queries"]
    assert rec["still_under_threshold_fp32"] == len(rec["still_under_threshold_qids"]) <= rec["rerun_fp32"]
    assert set(rec["still_under_threshold_qids"]) <= set(rec["rerun_qids"]) <= {int(q) for q in queries}
    # the extra report goes to stderr: stdout has the lines of a run without the flag (timings aside)
    strip = lambda s: [ln for ln in s.splitlines() if not ln.startswith(("timing", "out_dir"))]   # noqa: E731
    assert strip(out_guard) == strip(out_plain)
    run_p = json.load(open(os.path.join(plain_dir, "MSMARCO", "run_0.json")))
    run_g = json.load(open(os.path.join(guard_dir, "MSMARCO", "run_0.json")))
    assert set(run_g) == set(run_p) == set(queries)
