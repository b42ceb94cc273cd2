"""not-gpu: the fp64 reference of the training step's attention (tests/attn_train_ref.py) and the inputs of
tests/test_gpu_attn_train_direct.py, checked on the CPU:
  * the definition against torch.autograd in float64 through a plain restatement of softmax(Q K^T + bias[bucket]) * mul . V, to
    1e-12 of every tensor's largest element, on every (shape, rate) of the table: it is not only its author's algebra;
  * the plain numpy fp32 evaluation, in two summation orders, inside the a-priori bound on every case;
  * that the inputs discriminate: every mutant of the definition lies FACTOR = 10x or more beyond the bound somewhere in every
    (group, head) it applies to (dbias: per head). It applies where it moves some output of the fp64 definition by more than
    u = 2^-24 of the larger of 1 (the scale of K, V and dO) and the output's largest element there: less than that no fp32 result
    can show, whatever the bound (a keep bit that differs on a key of weight e^-40, key 32 of a causal length 33 that only the
    last row attends and that row is peaked elsewhere);
  * every case's expected kernel against the planner (tests/attn_route_driver.cpp), the refusals, the side of LDS_MAX every
    shape lies on, and that this table and attn_ref's together name every kernel of RPR_ATTN_KERNELS.
The 10x is a condition on the inputs, not a measurement: a case that misses it gets other inputs, not another factor. Run with -s
to see the ratios."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import attn_ref as R
import attn_train_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 10.0
SHAPE_RATES = [(p, r) for p, _, _ in T.SHAPES for r in ((0.0, T.RATE) if p["drop_rate"] == T.RATE else (p["drop_rate"],))]
IDS = [f"{p['name']}_rate{r}" for p, r in SHAPE_RATES]
OUT = ("O", "dQ", "dK", "dV")
_fp32 = {}           # order -> (worst ratio, case, output)
_smallest = {}       # mutant -> (ratio, case)
_applied = set()


def _ratio(diff, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(diff > 0, diff / bound, 0.0).max(initial=0.0))


# ---------------------------------------------------------------------------------------------- autograd
def _autograd(inp, rate):
    """Gradients of sum(O * dO) by torch.autograd in float64: {(g, h): (O, dQ, dK, dV)} and d rel_bias [NB, H] (self-attention)."""
    H = inp["H"]
    rb = torch.tensor(inp["rel_bias"].astype(np.float64), requires_grad=True) if inp["site"] == "self" else None
    out, loss = {}, 0.0
    leaves = {}
    for g in range(inp["groups"]):
        for h in range(H):
            G = T.gather(inp, g, h, rate)
            if not G.ok.any():
                continue
            q, K, V = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (G.q, G.K, G.V))
            ok = torch.from_numpy(G.ok)
            s = q @ K.T
            if rb is not None:
                s = s + rb[torch.from_numpy(G.bucket), h]
            p = torch.softmax(s.masked_fill(~ok, -float("inf")), dim=1)
            O = (p * torch.from_numpy(G.mul.astype(np.float64))) @ torch.where(ok.any(dim=0)[:, None], V, torch.zeros_like(V))
            loss = loss + (O * torch.from_numpy(G.dO.astype(np.float64))).sum()
            leaves[(g, h)] = (O, q, K, V)
    loss.backward()
    for k, (O, q, K, V) in leaves.items():
        out[k] = dict(O=O.detach().numpy(), dQ=q.grad.numpy(), dK=K.grad.numpy(), dV=V.grad.numpy())
    return out, (rb.grad.numpy() if rb is not None else None)


@pytest.mark.parametrize("p,rate", SHAPE_RATES, ids=IDS)
def test_definition_equals_autograd(p, rate):
    inp = T.make_inputs(p)
    ref = T.reference(p, rate)
    auto, drb = _autograd(inp, rate)
    worst = 0.0
    for k, r in ref["groups"].items():
        if k not in auto:       # no attended key: softmax over nothing has no autograd; the definition gives zeros
            assert not r["ok"].any() and all((r[o] == 0).all() for o in OUT)
            continue
        for o in OUT:
            a = auto[k][o]
            assert np.isfinite(r[o]).all()
            rel = np.abs(r[o] - a).max() / max(np.abs(a).max(), 1e-300)
            worst = max(worst, rel)
            assert rel <= 1e-12, (k, o, rel)
    if drb is not None:
        d = ref["dbias"] - inp["dbias0"].astype(np.float64)
        rel = np.abs(d - drb).max() / max(np.abs(drb).max(), np.abs(inp["dbias0"]).max())
        worst = max(worst, rel)
        assert rel <= 1e-12, ("dbias", rel)
    print(f"\n{p['name']} rate {rate}: worst relative difference to autograd {worst:.3g}")


# ---------------------------------------------------------------------------------------------- fp32 inside the bound
@pytest.mark.parametrize("p,rate", SHAPE_RATES, ids=IDS)
def test_fp32_evaluation_stays_within_the_bound(p, rate):
    ref = T.reference(p, rate)
    for order, seed in (("natural", None), ("permuted", 12345)):
        ev = T.reference(p, rate, dtype=np.float32, perm_seed=seed)
        worst = (0.0, "-")
        for k, r in ref["groups"].items():
            for o in OUT:
                assert np.isfinite(r["b_" + o]).all()
                x = _ratio(np.abs(ev["groups"][k][o].astype(np.float64) - r[o]), r["b_" + o])
                worst = max(worst, (x, o))
        if "dbias" in ref:
            worst = max(worst, (_ratio(np.abs(ev["dbias"].astype(np.float64) - ref["dbias"]), ref["b_dbias"]), "dbias"))
        print(f"\n{p['name']} rate {rate} {order}: fp32 / bound {worst[0]:.4f} ({worst[1]})")
        if worst[0] > _fp32.get(order, (-1.0,))[0]:
            _fp32[order] = (worst[0], f"{p['name']} rate {rate}", worst[1])
        assert worst[0] <= 1.0, (order, worst)


# ---------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("p,rate", SHAPE_RATES, ids=IDS)
def test_inputs_discriminate(p, rate):
    inp = T.make_inputs(p)
    ref = T.reference(p, rate)
    line = []
    for mut in T.MUTANTS:
        if not T.mutant_applies(inp, rate, mut):
            continue
        m = T.reference(p, rate, mut=mut)
        small = (np.inf, None)
        if mut == "dbias_diag":       # changes where dS lands and nothing else: judged per head on dbias
            units = {h: (_ratio(np.abs(m["dbias"][:, h] - ref["dbias"][:, h]), ref["b_dbias"][:, h]),
                         bool(np.abs(m["dbias"][:, h] - ref["dbias"][:, h]).max() > T.U * max(1.0, np.abs(ref["dbias"][:, h]).max())))
                     for h in range(inp["H"])}
        else:
            units = {}
            for k, r in ref["groups"].items():
                diffs = [np.abs(m["groups"][k][o] - r[o]) for o in OUT]
                units[k] = (max(_ratio(d, r["b_" + o]) for d, o in zip(diffs, OUT)),
                            any(d.max() > T.U * max(1.0, np.abs(r[o]).max()) for d, o in zip(diffs, OUT)))
        for k, (x, changed) in units.items():
            if changed and x < small[0]:
                small = (x, k)
        if small[1] is None:
            continue
        _applied.add((inp["site"], mut))
        line.append(f"{mut} {small[0]:.3g}")
        if small[0] < _smallest.get(mut, (np.inf, ""))[0]:
            _smallest[mut] = (small[0], f"{p['name']} rate {rate}")
        assert small[0] >= FACTOR, (mut, small)
    print(f"\n{p['name']} rate {rate}: smallest mutant ratio per unit: " + ", ".join(line))


def test_every_mutant_applies_somewhere():
    """No mutant may be a no-op on the whole table: each one applies to some (group, head) of a case of every site that knows it."""
    want = {(s, m) for s in ("self", "cross") for m in T.MUTANTS
            if not (s == "cross" and m in ("dbias_diag", "tables_swapped")) and not (s == "self" and m == "doc_ignored")}
    if len(_applied) == 0:        # run on its own: the sweep above has not filled the record
        for p, rate in SHAPE_RATES:
            test_inputs_discriminate(p, rate)
    assert _applied == want, want ^ _applied
    print("\nfp32 evaluation / bound, worst per order: " + ", ".join(f"{o} {v[0]:.4f} ({v[1]}, {v[2]})" for o, v in sorted(_fp32.items())))
    print("smallest ratio per mutant over the table: " + ", ".join(f"{m} {r:.3g} ({c})" for m, (r, c) in sorted(_smallest.items())))


def test_rate_09_drops_whole_rows():
    """Rate 0.9 with 3 keys: the reference itself has rows whose kept keys are all dropped — zeros in O, nothing added to dV, dS = 0."""
    for p, _, _ in T.SHAPES:
        if p["drop_rate"] != 0.9:
            continue
        inp = T.make_inputs(p)
        ref = T.reference(p, 0.9)
        dead_rows = 0
        for (g, h), r in ref["groups"].items():
            G = T.gather(inp, g, h, 0.9)
            dead = ((G.mul == 0) | ~G.ok).all(axis=1) & G.ok.any(axis=1)
            dead_rows += int(dead.sum())
            assert (r["O"][dead] == 0).all() and (r["dS"][dead] == 0).all() and (r["dQ"][dead] == 0).all()
            # nothing added to dV: the definition over the other rows alone gives the same dV
            rest = T.Group(G.q[~dead], G.K, G.V, G.dO[~dead], G.bias[~dead] if G.bias is not None else None, G.ok[~dead], G.mul[~dead], None)
            if (~dead).any():
                assert np.abs(T.define(rest, want_bound=False)["dV"] - r["dV"]).max() <= 1e-13 * np.abs(r["dV"]).max()
            else:
                assert (r["dV"] == 0).all()
        assert dead_rows >= 3, (p["name"], dead_rows)


# ---------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_train_direct") / "attn_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "attn_route_driver.cpp")], check=True,
                   capture_output=True, text=True)
    return exe


def _plan(driver, site, **kw):
    return json.loads(subprocess.run([driver, site] + [f"{k}={v}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout)


def test_every_case_takes_the_kernel_it_names(driver):
    for c in T.CASES:
        site, kw = T.planner_query(c)
        p = _plan(driver, site, **kw)
        assert (p["kernel"], p["invalid"]) == (c.kernel, 0), (c.name, p)


def test_every_shape_lies_on_its_side_of_the_carve():
    """cross_attn_bwd_carve and self_attn_bwd_smem recomputed here: resident shapes fit LDS_MAX, tiled ones do not."""
    for p, resident, _ in T.SHAPES:
        carve = T.self_carve(p["Ls"]) if p["site"] == "self" else T.cross_carve(p["n"], p["Lq"])
        assert (carve <= T.LDS_MAX) == resident, (p["name"], carve)
    assert T.self_carve(91) == 163692 and T.self_carve(92) > T.LDS_MAX
    assert T.cross_carve(8, 256) <= T.LDS_MAX < T.cross_carve(16, 256)


def test_refusals(driver):
    """Shapes no training kernel takes: causal beyond the carve, 128-dim heads beyond the carve, the tiles without a key mask, query
    rows that are not whole sequences of drop_L positions."""
    self_kw = dict(S=3, H=3, buckets=T.NB, dkv=64, causal=0, mask=1, drop=0, drop_L=0)
    cross_kw = dict(bz=2, n=16, Lq=256, H=2, dkv=64, mask=1, drop=0, drop_L=0)
    refused = [("train_self_bwd", dict(self_kw, Ls=92, causal=1, mask=0)),
               ("train_self_drop_fwd", dict(self_kw, Ls=92, causal=1, mask=0, drop=1, drop_L=92)),
               ("train_self_bwd", dict(self_kw, Ls=92, dkv=128)),
               ("train_self_drop_fwd", dict(self_kw, Ls=92, dkv=128, drop=1, drop_L=92)),
               ("train_cross_bwd", dict(cross_kw, dkv=128)),
               ("train_cross_drop_fwd", dict(cross_kw, dkv=128, drop=1, drop_L=8)),
               ("train_self_bwd", dict(self_kw, Ls=92, mask=0)),
               ("train_self_drop_fwd", dict(self_kw, Ls=92, mask=0, drop=1, drop_L=92)),
               ("train_cross_bwd", dict(cross_kw, mask=0)),
               ("train_cross_drop_fwd", dict(cross_kw, mask=0, drop=1, drop_L=8)),
               ("train_self_bwd", dict(self_kw, Ls=92, drop=1, drop_L=7)),
               ("train_self_drop_fwd", dict(self_kw, Ls=92, drop=1, drop_L=7)),
               ("train_cross_bwd", dict(cross_kw, drop=1, drop_L=7)),
               ("train_cross_drop_fwd", dict(cross_kw, drop=1, drop_L=7)),
               ("train_cross_bwd", dict(cross_kw, n=8, Lq=5, drop=1, drop_L=3)),
               ("train_cross_drop_fwd", dict(cross_kw, n=8, Lq=5, drop=1, drop_L=3))]
    for site, kw in refused:
        p = _plan(driver, site, **kw)
        assert (p["kernel"], p["invalid"]) == ("NONE", 1), (site, kw, p)
    # and their admitted neighbours
    assert _plan(driver, "train_self_bwd", **dict(self_kw, Ls=91, causal=1, mask=0))["kernel"] == "TRAIN_BWD_VALU"
    assert _plan(driver, "train_self_bwd", **dict(self_kw, Ls=91, dkv=128))["kernel"] == "TRAIN_BWD_VALU128"
    assert _plan(driver, "train_cross_bwd", **dict(cross_kw, drop=1, drop_L=8))["kernel"] == "TRAIN_CROSS_BWD_TILED"


def test_the_two_tables_cover_every_kernel():
    """attn_ref.OUT_OF_SCOPE without NONE and the development-switch kernel is exactly what this table names; with attn_ref's own
    cases that is all of RPR_ATTN_KERNELS."""
    names = set(R.OUT_OF_SCOPE) | {c.kernel for c in R.CASES}
    assert R.OUT_OF_SCOPE - {"NONE", "TAIL_CROSS_G1_NKT1"} == T.KERNELS, (R.OUT_OF_SCOPE - {"NONE", "TAIL_CROSS_G1_NKT1"}) ^ T.KERNELS
    src = open(os.path.join(REPO, "ripor_amd", "csrc", "attn_route.h")).read()
    body = src[src.index("#define RPR_ATTN_KERNELS(X)"):src.index("enum AttnKernel")]
    assert set(re.findall(r"\bX\((\w+)\)", body)) == names
