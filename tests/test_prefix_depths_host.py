"""One search that also reports its beams at shorter prefix lengths (rpr_search_prefixes), the parts that need no GPU: the plan
(ripor_amd/csrc/search_plan.h through tests/prefix_depths_plan_driver.cpp, compiled here with the host C++ compiler), the
ABI, the --prefix_out_dirs flag of the rank-data task and what constrained_decode_smtid writes for every prefix length.
Every expectation is worked out by hand from the planner's rules and the reference's rank-data format."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("prefix_depths_plan") / "prefix_depths_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "prefix_depths_plan_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def plan(driver, **kw):
    def fmt(v):
        return ",".join(repr(float(x)) for x in v) if isinstance(v, (list, tuple)) else str(int(v) if isinstance(v, bool) else v)
    out = subprocess.run([driver, "plan"] + [f"{k}={fmt(v)}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


# 600 queries x 10 beams of 16 tokens, automatic mode. Trie statistics per depth: f = share of single-sequence nodes, mu = mean
# extra sequences per node. First fork: the first depth with f^10 >= 1/2 -> depth 2 (0.95^10 = 0.599; 0.5^10 is not), and
# 14 >= 8 positions remain (6000 > 4096 decoder rows). Extras: automatic, 6000 > 4096 rows and fewer than 32 beams -> budget 4,
# pool 600 / 32 = 18. Second fork with that budget: depth 3 leaves 600 * P[Poisson(0.01) > 4] + E[(Poisson(5.97) - 18)+] << 0.05
# queries behind -> [2, 3]. WITHOUT extras depth 3 would leave 600 * (1 - 0.999^10) = 5.97 queries and the second fork would be
# depth 4 (f = 1): the call with prefix lengths must keep [2, 3] — the forks of the same call without them — and carry no extras.
STATS = dict(f=[0.0, 0.5, 0.95, 0.999] + [1.0] * 13, mu=[5.0, 1.0, 0.06, 0.001] + [0.0] * 13)
CALL = dict(Q=600, Lq=16, B=10, L=16)
TODAY = {"Q": 600, "Lq": 16, "B": 10, "L": 16, "flags": 0, "lane": -1, "cus": 0, "prec": 1, "margins": 0, "l0": 0, "mfma16": 1,
         "extras": 4, "pool": 18, "forks": [2, 3], "drop_last": 0, "tail_rank_replay": 0, "select_radix": -1}


def test_plan_without_depths_is_todays_plan(driver):
    p = plan(driver, **CALL, **STATS)
    assert p == dict(TODAY, depths=[], n_depths=0)


def test_plan_with_depths_keeps_the_forks_and_drops_the_extras(driver):
    p = plan(driver, **CALL, **STATS, depths=[4, 8])
    assert p == dict(TODAY, extras=0, pool=0, depths=[4, 8], n_depths=2)
    # the optimistic mode drops the last stage exactly as without prefix lengths
    a, b = plan(driver, **CALL, **STATS, forced_tail=2), plan(driver, **CALL, **STATS, forced_tail=2, depths=[4])
    assert a["forks"] == b["forks"] and a["drop_last"] == b["drop_last"] == 1 and b["extras"] == b["pool"] == 0
    # explicit fork depths still win, and an explicit extras budget does not apply either
    p = plan(driver, **CALL, **STATS, depths=[3, 4, 8], n_fork_override=2, fork0=2, fork1=5, tail_extras=6)
    assert p["forks"] == [2, 5] and p["extras"] == 0 and p["pool"] == 0 and p["depths"] == [3, 4, 8]
    # no forced tail: nothing but the prefix lengths differs from the plain plan
    a, b = plan(driver, **CALL, **STATS, forced_tail=0), plan(driver, **CALL, **STATS, forced_tail=0, depths=[4, 8])
    assert a["forks"] == [] and dict(a, depths=[4, 8], n_depths=2) == b


def test_depths_are_part_of_the_key(driver):
    r = json.loads(subprocess.run([driver, "key"], check=True, capture_output=True, text=True).stdout)
    names, eq, lt = r["names"], r["eq"], r["lt"]
    assert names[:2] == ["base", "copy"] and set(names[2:]) == {"no depths", "depth0", "depth1", "depth2", "n_depths"}
    n = len(names)
    for i in range(n):
        for j in range(n):
            same = i == j or {i, j} == {0, 1}
            assert eq[i][j] == int(same), (names[i], names[j])
            assert lt[i][j] + lt[j][i] == int(not same), (names[i], names[j])      # a strict order: graphs never collide
    # a plan without prefix lengths sorts before the same plan with them (zeros in the key's last fields)
    assert lt[names.index("no depths")][0] == 1


def test_abi_exports_the_symbol_and_keeps_its_version():
    from ripor_amd import _lib
    assert "rpr_search_prefixes" in _lib.SIGNATURES and _lib.ABI_VERSION == 5
    res, args = _lib.SIGNATURES["rpr_search_prefixes"]
    assert len(args) == len(_lib.SIGNATURES["rpr_search"][1]) - 1 + 6      # rpr_search's without the taps + n, depths, 4 arrays
    lib = _lib.load()
    assert hasattr(lib, "rpr_search_prefixes") and lib.rpr_abi_version() == 5
    header = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    assert "int rpr_search_prefixes(" in header


def _args(*extra):
    from ripor_amd import evaluate
    return evaluate.get_args(["--task=t5seq_aq_get_qid_to_smtid_rankdata", "--max_new_token=16"] + list(extra))


def test_prefix_out_dirs_is_parsed_and_bad_values_are_refused():
    from ripor_amd import evaluate
    assert not hasattr(_args(), "prefix_out_dirs") and evaluate.check_rankdata_flags(_args()) is None
    assert evaluate.check_rankdata_flags(_args('--prefix_out_dirs={"4": "/x/d4", "8": "/x/d8"}')) == {4: "/x/d4", 8: "/x/d8"}
    for bad in ('{"3": "/x"}', '{"16": "/x"}', "not json", "{}", '{"4": ""}', '[4]'):
        with pytest.raises(SystemExit):
            evaluate.check_rankdata_flags(_args(f"--prefix_out_dirs={bad}"))
    with pytest.raises(SystemExit):
        evaluate.check_rankdata_flags(_args('--prefix_out_dirs={"4": "/x"}', "--near_tie_guard=1e-3"))
    with pytest.raises(SystemExit):   # a key must be below --max_new_token
        evaluate.check_rankdata_flags(evaluate.get_args(["--max_new_token=8", '--prefix_out_dirs={"8": "/x"}']))
    # the task refuses before it loads anything: a checkpoint path that does not exist is never touched
    with pytest.raises(SystemExit):
        evaluate.main(["--task=t5seq_aq_get_qid_to_smtid_rankdata", "--max_new_token=16", "--pretrained_path=/nonexistent",
                       '--prefix_out_dirs={"3": "/x"}'])


def test_constrained_decode_smtid_writes_every_prefix_directory(tmp_path, monkeypatch):
    """generate_for_constrained_prefix_beam_search stubbed with fixed outputs: 2 queries, 2 beams, 8 tokens, prefix length 4."""
    from ripor_amd import evaluate
    perm = np.array([3, 1, 0, 2, 4], dtype=np.int64)                     # sorted row -> docid index
    table = evaluate.DocidTable([f"d{i}" for i in range(5)])
    proc = types.SimpleNamespace(trie=lambda device: types.SimpleNamespace(perm=perm))
    seq8 = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 9, 5, 6, 7, 8], [0, 7, 7, 7, 7, 1, 1, 1, 1], [0, 6, 6, 6, 6, 2, 2, 2, 2]])
    seq4 = torch.tensor([[0, 1, 2, 3, 4], [0, 1, 2, 3, 9], [0, 6, 6, 6, 6], [0, 7, 7, 7, 7]])
    out8 = types.SimpleNamespace(sequences=seq8, sequences_scores=torch.tensor([0.5, 0.25, 1.0, -2.0]),
                                 row_lo=torch.tensor([0, 1, 2, 4]), row_hi=torch.tensor([1, 2, 4, 5]), near_tie=None)
    out8.prefix_outputs = {4: types.SimpleNamespace(sequences=seq4, sequences_scores=torch.tensor([1.5, 0.75, 3.0, -1.0]),
                                                    row_lo=torch.tensor([0, 1, 4, 2]), row_hi=torch.tensor([1, 3, 5, 4]))}
    seen = {}

    def stub(model, processor, **kw):
        seen.update(kw)
        return out8

    monkeypatch.setattr(evaluate, "generate_for_constrained_prefix_beam_search", stub)
    loader = [{"id": torch.tensor([11, 12]), "input_ids": torch.ones((2, 3), dtype=torch.long),
               "attention_mask": torch.ones((2, 3), dtype=torch.long)}]
    main_dir, d4 = str(tmp_path / "main"), str(tmp_path / "deep" / "d4")
    os.makedirs(main_dir)
    evaluate.constrained_decode_smtid(None, loader, proc, table, 8, "cpu", main_dir, 0, topk=2, prefix_out_dirs={4: d4})
    assert seen["prefix_lengths"] == (4,) and seen["max_new_tokens"] == 8 and "near_tie_guard" not in seen
    got8 = json.load(open(os.path.join(main_dir, "qid_smtid_rankdata_0.json")))
    got4 = json.load(open(os.path.join(d4, "qid_smtid_rankdata_0.json")))
    assert got8 == {"11": {"1_2_3_4_5_6_7_8": {"d3": 4.0}, "1_2_3_9_5_6_7_8": {"d1": 2.0}},
                    "12": {"7_7_7_7_1_1_1_1": {"d0": 8.0, "d2": 8.0}, "6_6_6_6_2_2_2_2": {"d4": -16.0}}}
    # smtids of 4 codes, score = rel_score * 4, docids = perm[lo:hi]
    assert got4 == {"11": {"1_2_3_4": {"d3": 6.0}, "1_2_3_9": {"d1": 3.0, "d0": 3.0}},
                    "12": {"6_6_6_6": {"d4": 12.0}, "7_7_7_7": {"d0": -4.0, "d2": -4.0}}}
    # without the flag: the call and the file of today, no other directory
    seen.clear()
    plain_dir = str(tmp_path / "plain")
    os.makedirs(plain_dir)
    evaluate.constrained_decode_smtid(None, loader, proc, table, 8, "cpu", plain_dir, 0, topk=2)
    assert "prefix_lengths" not in seen
    assert json.load(open(os.path.join(plain_dir, "qid_smtid_rankdata_0.json"))) == got8
    # the reference's dict of smtid strings knows one length only; the near-tie guard has no margins for the shorter ones
    with pytest.raises(ValueError):
        evaluate.constrained_decode_smtid(None, loader, proc, {"1_2_3_4_5_6_7_8": ["d3"]}, 8, "cpu", main_dir, 0, topk=2,
                                          prefix_out_dirs={4: d4})
    with pytest.raises(ValueError):
        evaluate.constrained_decode_smtid(None, loader, proc, table, 8, "cpu", main_dir, 0, topk=2, prefix_out_dirs={4: d4},
                                          near_tie_guard=1e-3)
