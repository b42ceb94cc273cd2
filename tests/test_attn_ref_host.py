"""not-gpu: the fp64 attention reference of tests/attn_ref.py and the inputs of tests/test_gpu_attn_direct.py, checked on
the CPU: the bucket restatement against the library's table, every case's expected kernel against the planner, the plain
numpy fp32 evaluation inside the a-priori bound, and — the point of the file — that the inputs discriminate: every mutant of
the definition (a shifted bias table, a neighbour head's bias, a dropped key, an ignored mask or ancestry, a wrong offset
...) exceeds the bound by at least 30x in at least one row of every (query, head) it applies to.

A mutant applies to a (query, head) when it changes something that enters the definition there (attn_ref.same_definition):
a prefix mask has no hole for `last_as_count` to miss, query 0 is packed at the padded offset, position 0 has no ancestry.
Every mutant must apply somewhere at every site that knows it (test_every_mutant_applies_somewhere). The 30x is a condition on the inputs,
not a measurement: a case that misses it gets other inputs, not another factor. Run with -s to see the smallest ratios."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import attn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 30.0
# which mutants can mean anything at a site
SITE_MUTANTS = {
    "enc": ("bias_shift", "bias_head", "drop_last", "drop_16", "mask_ignored", "causal_off", "next_query", "padded_offset"),
    "self": ("bias_shift", "bias_head", "drop_last", "drop_16", "anc_ignored", "next_query"),
    "cross": ("drop_last", "drop_16", "mask_ignored", "last_as_count", "next_query", "padded_offset"),
    "tail_self": ("bias_shift", "bias_head", "drop_last", "drop_16", "anc_ignored", "causal_off", "next_query", "kvq_as_flist"),
}
_smallest = {}       # mutant -> (ratio, case)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    return _lib.load()


def test_bucket_restatement_matches_the_library(lib):
    for bid in (0, 1):
        for nb, md in ((32, 128), (16, 64), (8, 32)):
            for rel in range(-255, 256):
                assert R.hf_bucket(rel, bool(bid), nb, md) == lib.rpr_rel_bucket(rel, bid, nb, md), (bid, nb, md, rel)


def test_kernel_names_match_the_route_header(lib):
    src = open(os.path.join(REPO, "ripor_amd", "csrc", "attn_route.h")).read()
    body = src[src.index("#define RPR_ATTN_KERNELS(X)"):src.index("enum AttnKernel")]
    names = re.findall(r"\bX\((\w+)\)", body)
    assert lib.rpr_attn_kernel_count() == len(names)
    assert [lib.rpr_attn_kernel_name(i).decode() for i in range(len(names))] == names
    assert lib.rpr_attn_kernel_name(len(names)) is None and lib.rpr_attn_kernel_name(-1) is None
    covered = {c.kernel for c in R.CASES}
    assert R.OUT_OF_SCOPE <= set(names)
    assert set(names) - R.OUT_OF_SCOPE == covered, (set(names) - R.OUT_OF_SCOPE) ^ covered


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_direct") / "attn_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "attn_route_driver.cpp")], check=True,
                   capture_output=True, text=True)
    return exe


def test_every_case_takes_the_kernel_it_names(driver):
    """The planner (attn_route.h, compiled for the host) on every row of the table, many-waves rows included."""
    for c in R.CASES:
        site, kw = R.planner_query(c)
        p = json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)
        assert (p["kernel"], p["invalid"]) == (c.kernel, 0), (c.name, p)
    by = {c.name: c for c in R.CASES}
    site, kw = R.planner_query(by["step_cross_many_waves"])
    p = json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)
    assert (p["tiles"], p["tpw"], p["groups"]) == (9, 8, 2), p          # groups of 8 + 1 tiles
    site, kw = R.planner_query(by["tail_cross_many_waves"])
    p = json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)
    assert (p["tiles"], p["tpw"], p["groups"]) == (32, 9, 4), p         # groups of 9 + 9 + 9 + 5 tiles
    site, kw = R.planner_query(by["block_cross_L64_B100"])
    p = json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)
    assert (p["bchunk"], p["grid"][1]) == (32, 4), p                    # a last chunk of 4 rows
    site, kw = R.planner_query(by["block_cross_L256_B5"])
    p = json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)
    assert (p["bchunk"], p["grid"][1]) == (1, 5), p


def _ratio(diff, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(diff > 0, diff / bound, 0.0).max())


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_inputs_discriminate(case):
    inp = R.make_inputs(case)
    pairs = R.sample_pairs(case, inp) or R.all_pairs(inp)
    gather = R.GATHER[case.site]
    worst32, n_live = 0.0, 0
    smallest = {}
    for g, h in pairs:
        G0 = gather(inp, g, h)
        if G0 is None:
            continue
        n_live += 1
        o0, b0 = R.attend(G0.q, G0.K, G0.V, G0.bias, G0.ok)
        o32, _ = R.attend(G0.q, G0.K, G0.V, G0.bias, G0.ok, np.float32, want_bound=False)
        assert np.isfinite(o0).all() and np.isfinite(b0).all()
        worst32 = max(worst32, _ratio(np.abs(o32.astype(np.float64) - o0), b0))
        for mut in SITE_MUTANTS[case.site]:
            G1 = gather(inp, g, h, mut)
            if R.same_definition(G0, G1):
                continue
            o1, _ = R.attend(G1.q, G1.K, G1.V, G1.bias, G1.ok, want_bound=False)
            r = _ratio(np.abs(o1 - o0), b0)
            if r < smallest.get(mut, (np.inf,))[0]:
                smallest[mut] = (r, g, h)
    assert n_live > 0
    print(f"\n{case.name}: {n_live} (query, head) pairs, fp32 / bound {worst32:.4f}; smallest mutant ratio per (query, head): " +
          ", ".join(f"{m} {v[0]:.3g}" for m, v in smallest.items()))
    assert worst32 <= 1.0, worst32
    for m, (r, g, h) in smallest.items():
        if r < _smallest.get(m, (np.inf, ""))[0]:
            _smallest[m] = (r, case.name)
        assert r >= FACTOR, (m, r, g, h)


def test_every_mutant_applies_somewhere():
    """No mutant may be a no-op on the whole table: each one changes the definition of some (query, head) of a case of every
    site that knows it (looked at on head 0 of every query of the small cases; on its own, not through the runs above)."""
    seen = set()
    for case in R.CASES:
        if case.sample:
            continue
        inp = R.make_inputs(case)
        gather = R.GATHER[case.site]
        for g in range(R.n_groups(inp)):
            G0 = gather(inp, g, 0)
            for mut in SITE_MUTANTS[case.site]:
                if (case.site, mut) not in seen and G0 is not None and not R.same_definition(G0, gather(inp, g, 0, mut)):
                    seen.add((case.site, mut))
    want = {(s, m) for s, ms in SITE_MUTANTS.items() for m in ms}
    assert seen == want, want - seen
    assert {m for _, m in want} == set(R.MUTANTS)
    if _smallest:
        print("\nsmallest ratio per mutant over the cases run: " + ", ".join(f"{m} {r:.3g} ({c})" for m, (r, c) in sorted(_smallest.items())))
