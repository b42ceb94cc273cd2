"""not-gpu: the host side of the pruning margins and the near-tie guard — the ABI entry is declared, bound and exported;
the splice of the re-run rows; the CLI flag; and the numpy restatement of the margin (tests/prune_margin_ref.py) pinned to
conftest.prune_margins through the oracle's own per-step record."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import SCORE_TOL, golden_names, prune_margins
from prune_margin_ref import prune_margin_ref, step_gaps, unpack_valid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_binds_and_exports_rpr_search_margins():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    m = re.search(r"\bint rpr_search_margins\(([^;]*)\);", hdr)
    s = re.search(r"\bint rpr_search\(([^;]*)\);", hdr)
    assert m and s
    # the arguments of rpr_search plus double* out_margin
    assert m.group(1).count(",") == s.group(1).count(",") + 1 and "double* out_margin" in m.group(1)
    assert len(_lib.SIGNATURES["rpr_search_margins"][1]) == len(_lib.SIGNATURES["rpr_search"][1]) + 1
    assert hasattr(C.CDLL(ge.LIB), "rpr_search_margins") and hasattr(C.CDLL(ge.LIB_DEV), "rpr_search_margins")
    assert C.sizeof(_lib.DebugTaps) == 6 * C.sizeof(C.c_void_p)   # no new tap field


def _canned(as_torch):
    full = (np.arange(5 * 3 * 2).reshape(5, 3, 2).astype(np.int32), np.arange(15, dtype=np.float32).reshape(5, 3),
            np.arange(15, dtype=np.int64).reshape(5, 3), np.arange(15, dtype=np.int64).reshape(5, 3) + 1)
    conv = (lambda a: torch.from_numpy(a.copy())) if as_torch else (lambda a: a.copy())
    return tuple(conv(a) for a in full)


@pytest.mark.parametrize("as_torch", [False, True])
def test_splice_rows(as_torch):
    from ripor_amd.engine import splice_rows
    full = _canned(as_torch)
    keep = [np.asarray(f).copy() for f in full]
    mask = np.array([False, True, False, False, True])
    mask_in = torch.from_numpy(mask) if as_torch else mask
    sub = tuple((-(f[mask_in] + 100)) for f in full)
    out = splice_rows(full, mask_in, sub)
    for o, f, x in zip(out, keep, sub):
        o, x = np.asarray(o), np.asarray(x)
        assert o.dtype == f.dtype and o.shape == f.shape
        assert (o[~mask] == f[~mask]).all(), "an unmasked row changed"
        assert (o[mask] == x).all(), "a masked row is not the re-run's"
    for f, k in zip(full, keep):
        assert (np.asarray(f) == k).all(), "the inputs were modified in place"
    # empty mask: the inputs themselves; full mask: the re-run itself
    none = mask_in & ~mask_in
    out = splice_rows(full, none, tuple(f[none] for f in full))
    assert all(o is f for o, f in zip(out, full))
    every = ~none
    sub = tuple(f + 7 for f in full)
    out = splice_rows(full, every, sub)
    assert all(o is x for o, x in zip(out, sub))
    with pytest.raises(AssertionError):
        splice_rows(full, mask_in, tuple(f[:1] for f in full))


def test_cli_accepts_near_tie_guard_and_is_unchanged_without_it():
    import argparse
    from ripor_amd import evaluate as ev
    base = ["--task", "t5seq_aq_retrieve_docids", "--out_dir", "o", "--topk", "10"]
    a = ev.get_args(base)
    b = ev.get_args(base + ["--near_tie_guard", "1e-3"])
    assert not hasattr(a, "near_tie_guard")
    assert b.near_tie_guard == 1e-3
    del b.near_tie_guard
    assert a == b
    # today's namespace: the fields of the parser before this flag existed
    assert set(vars(a)) == {"pretrained_path", "out_dir", "task", "docid_to_smtid_path", "q_collection_paths", "eval_qrel_path",
                            "eval_metric", "batch_size", "gather_results", "search_batch_size", "max_new_token_for_docid", "topk",
                            "local_rank", "max_new_token", "train_query_dir", "mmap_dir", "index_dir", "num_subvectors_for_pq",
                            "codebook_bits", "apply_log_softmax_for_scores"}
    assert isinstance(a, argparse.Namespace)


def test_near_tie_log_counts(tmp_path):
    import json
    from ripor_amd.evaluate import NearTieLog
    log = NearTieLog(1e-3)
    log.note([11, 12, 13], torch.tensor([5e-4, 1.0, 1e-5], dtype=torch.float64), torch.tensor([True, False, True]),
             torch.tensor([2e-3, 1e-6], dtype=torch.float64))
    log.note([14], torch.tensor([np.inf], dtype=torch.float64), torch.tensor([False]), torch.empty(0, dtype=torch.float64))
    log.write(str(tmp_path))
    rec = json.load(open(tmp_path / "near_tie.json"))
    assert rec == {"threshold": 1e-3, "queries": 4, "rerun_fp32": 2, "still_under_threshold_fp32": 1, "rerun_qids": [11, 13],
                   "still_under_threshold_qids": [13]}


def test_unpack_valid_bit_order():
    w = np.zeros((1, 2), dtype=np.int64)
    w[0, 0] = 1 | (1 << 5)
    w[0, 1] = np.int64(-2 ** 63)            # bit 63 of word 1 = item 127
    v = unpack_valid(w, 2, 64)
    assert v.shape == (1, 2, 64) and v.sum() == 3 and v[0, 0, 0] and v[0, 0, 5] and v[0, 1, 63]


def test_restatement_on_canned_steps():
    # Q = 1, B = 2, V = 4, two steps; beam 1 is dead at step 0
    lg = np.array([[[1.0, 3.0, 2.0, 0.5], [9.0, 9.0, 9.0, 9.0]], [[1.0, 0.0, 0.0, 0.0], [0.25, 0.0, 0.0, 5.0]]], dtype=np.float32)
    ok = np.zeros((2, 1, 2, 4), dtype=bool)
    ok[0, 0, :, :3] = True                  # the root has three children
    ok[1, 0, 0, 0] = ok[1, 0, 1, 0] = True  # one child each afterwards: rank B is masked
    scores = np.array([[[3.0, 2.0]], [[4.0, 2.25]]])
    g = step_gaps(lg, ok, scores, 2)
    assert g[0, 0] == 1.0 and g[1, 0] == np.inf
    assert prune_margin_ref(lg, ok, scores, 2)[0] == 1.0
    # an exact tie across the boundary gives 0; a padding column is no candidate
    lg[0, 0, 0] = 2.0
    assert step_gaps(lg, ok, np.array([[[3.0, 2.0]], [[4.0, 2.25]]]), 2)[0, 0] == 0.0
    assert step_gaps(lg, ok, scores, 2, Vreal=2)[0, 0] == np.inf   # two live candidates, two beams: nothing live is dropped


def _oracle_taps(g, L):
    """The oracle's own per-step record of the first L steps, in the layout of the device taps."""
    from oracle import beam_ref, t5_ref
    from ripor_amd.utils import synth
    pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(g.codes)), g.V)
    rec = {}
    torch.set_num_threads(8)
    beam_ref.beam_search_ref(t5_ref.T5RefCached(g.state_dict, g.dims), pm, g.input_ids, g.attention_mask, g.B, L,
                             g.log_softmax, use_kv_cache=True, record=rec)
    Q, B, V = g.Q, g.B, g.V
    assert len(rec["steps"]) == L
    logits = np.stack([s["logits"] for s in rec["steps"]])                     # [L, Q*B, V] float32
    if g.log_softmax:
        logits = np.stack([torch.log_softmax(torch.from_numpy(s["logits"]), dim=-1).numpy() for s in rec["steps"]])
    scores = np.stack([s["top_scores"][:, :B] for s in rec["steps"]])          # [L, Q, B] float64
    valid = np.zeros((L, Q, B, V), dtype=bool)
    ids = np.zeros((Q * B, 1), dtype=np.int64)
    for t, s in enumerate(rec["steps"]):
        valid[t] = pm(ids).reshape(Q, B, V) > 0
        parent = (np.arange(Q)[:, None] * B + s["top_beam"][:, :B]).reshape(-1)
        ids = np.concatenate([ids[parent], s["top_tok"][:, :B].reshape(-1, 1)], axis=1)
    own = np.stack([s["top_scores"] for s in rec["steps"]])                    # [L, Q, 2B] float64, sorted
    return logits, valid, scores, own


@pytest.mark.parametrize("name", [n for n in golden_names()])
def test_restatement_reproduces_prune_margins_from_the_oracle_taps(golden_cache, name):
    g = golden_cache(name)
    assert "top_scores" in g.z.files
    want, _ = prune_margins(g)
    # The oracle walks the steps up to two past the last one at which the reference dropped a live candidate: by the golden's
    # own record every later gap is +inf, so the minimum over the walked steps IS prune_margins(g), and the t5-large goldens
    # do not spend their time on steps that cannot move it.
    ts = g.z["top_scores"]
    live = np.isfinite(ts[:, :, g.B]) & (ts[:, :, g.B] > -1e8) if ts.shape[2] > g.B else np.zeros(ts.shape[:2], dtype=bool)
    steps = min(g.L, (int(np.nonzero(live.any(axis=1))[0].max()) + 3) if live.any() else 2)
    assert not live[steps:].any()
    logits, valid, scores, own = _oracle_taps(g, steps)
    got = prune_margin_ref(logits, valid, scores, g.B)
    # (a) the same float64 adds as the oracle's own sorted candidates: equal bit for bit
    if own.shape[2] > g.B:
        gap = np.where(own[:, :, g.B] > -1e8, own[:, :, g.B - 1] - own[:, :, g.B], np.inf)
        assert (got == gap.min(axis=0)).all(), (got, gap.min(axis=0))
    # (b) the reference's goldens: the KV-cached oracle reproduces the reference's cumulative scores within SCORE_TOL (the
    # project's bound on a beam score), a margin is the difference of two of them
    assert (np.isinf(got) == np.isinf(want)).all(), (got, want)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    print(f"[margin-ref] {name}: {int(fin.sum())} finite margins of {g.Q}, worst difference to the reference {err:.3g}")
    assert err <= 2 * SCORE_TOL
