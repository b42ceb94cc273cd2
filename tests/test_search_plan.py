"""The plan of a constrained beam search (ripor_amd/csrc/search_plan.h), checked on the CPU.

tests/search_plan_driver.cpp includes the header and is compiled here with the host C++ compiler. Every expectation below
was worked out by hand from the search driver as it stood before the planner was split out of it (choose_forks, plan_forks,
tail_extras_budget, tail_extras_pool, PrecGuard and the hand-packed graph key of api.hip / internal.h) — none comes from
running the planner."""
import itertools
import json
import math
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16X2, BF16 = 0, 1, 2
LOG_SOFTMAX = 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("search_plan") / "search_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "search_plan_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def run(driver, *args):
    return subprocess.run([driver] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def plan(driver, **kw):
    def fmt(v):
        return ",".join(repr(float(x)) for x in v) if isinstance(v, (list, tuple)) else str(int(v) if isinstance(v, bool) else v)
    return json.loads(run(driver, "plan", *[f"{k}={fmt(v)}" for k, v in kw.items()]))


@pytest.mark.parametrize("mode,Q,B,margins,budget", [
    (0, 1000, 10, 0, 0),      # off
    (-1, 410, 10, 0, 4),      # automatic: 4100 > 4096 decoder rows
    (-1, 409, 10, 0, 0),      #   4090 rows
    (-1, 2000, 3, 0, 3),      #   never more than the beams
    (8, 5, 4, 0, 4),          # explicit: always, capped by the beams
    (8, 1000, 32, 0, 0),      # 32 beams or more: never
    (4, 1000, 10, 1, 0),      # never with the pruning margins
])
def test_extras_budget(driver, mode, Q, B, margins, budget):
    assert int(run(driver, "budget", mode, Q, B, margins)) == budget


def test_extras_pool(driver):
    """Q / 32, at least 4, at most 64"""
    assert [int(run(driver, "pool", q)) for q in (100, 1075, 4000)] == [4, 33, 64]


EXPLICIT = dict(Q=6, Lq=16, B=4, L=32, n_fork_override=1, fork0=4, logit_bound=1.0)   # passes every gate: forks [4]


def test_gates(driver):
    p = plan(driver, **EXPLICIT)
    assert (p["forks"], p["drop_last"], p["stats_calls"]) == ([4], 0, 0)
    closed = [dict(forced_tail=0), dict(taps=1), dict(L=2, fork0=1), dict(logit_bound="inf"),
              dict(logit_bound=1.5e6)]                       # 1e8 - 32 * 3e6 = 4e6 <= 1e7
    for kw in closed:
        for mode in ({}, dict(forced_tail=2)):
            p = plan(driver, **{**EXPLICIT, **mode, **kw, "tail_extras": 3})
            assert (p["forks"], p["drop_last"], p["extras"], p["pool"], p["stats_calls"]) == ([], 0, 0, 0, 0), kw
    assert plan(driver, **{**EXPLICIT, "logit_bound": 1e6})["forks"] == [4]          # 1e8 - 32 * 2e6 = 3.6e7
    # log-softmax scores add ln V per step: bound 1406248.5 (a float), V = 256: 32 * 2812497 = 89999904 leaves 10000096 > 1e7;
    # 32 * (2812497 + 5.545) = 90000081.4 leaves 9999918.6
    assert 1e8 - 32 * 2 * 1406248.5 > 1e7 >= 1e8 - 32 * (2 * 1406248.5 + math.log(256))
    assert plan(driver, **{**EXPLICIT, "logit_bound": 1406248.5, "V": 256})["forks"] == [4]
    assert plan(driver, **{**EXPLICIT, "logit_bound": 1406248.5, "V": 256, "flags": LOG_SOFTMAX})["forks"] == []


def test_explicit_depths(driver):
    base = dict(Q=6, Lq=16, B=4, L=16, logit_bound=1.0)
    for mode in (1, 2):
        p = plan(driver, **base, forced_tail=mode, n_fork_override=2, fork0=4, fork1=40)    # 40 > L - 1: dropped
        assert (p["forks"], p["drop_last"], p["stats_calls"]) == ([4], int(mode == 2), 0)
        p = plan(driver, **base, forced_tail=mode, n_fork_override=2, fork0=4, fork1=15)
        assert (p["forks"], p["drop_last"]) == ([4, 15], int(mode == 2))
        p = plan(driver, **base, forced_tail=mode, n_fork_override=2, fork0=5, fork1=3)     # not ascending: dropped
        assert p["forks"] == [5]
        p = plan(driver, **base, forced_tail=mode, n_fork_override=2, fork0=16, fork1=17)   # nothing left: no drop_last either
        assert (p["forks"], p["drop_last"]) == ([], 0)
        p = plan(driver, **base, forced_tail=mode, n_fork_override=0, fork0=4, tail_extras=2)
        assert (p["forks"], p["drop_last"], p["extras"], p["pool"]) == ([], 0, 0, 0)
    # the budget and the spare entries of a search with a fork: min(2, B) and max(4, Q / 32)
    p = plan(driver, **base, n_fork_override=1, fork0=4, tail_extras=2)
    assert (p["extras"], p["pool"]) == (2, 4)
    p = plan(driver, **{**base, "Q": 1075, "B": 10}, n_fork_override=1, fork0=4)            # automatic: 10750 rows -> 4, 33 entries
    assert (p["extras"], p["pool"]) == (4, 33)
    p = plan(driver, **{**base, "Q": 1075, "B": 10}, n_fork_override=1, fork0=4, margins=1)
    assert (p["extras"], p["pool"], p["margins"]) == (0, 0, 1)


def test_automatic_depths_ask_for_the_statistics_once(driver):
    """Q = 4, B = 2 (8 rows: a fork needs 2 remaining positions), L = 8. f^2 = 0.25, 0.64: first fork at depth 2. Without
    extras 4 * (1 - f^2) = 0.0796 at depth 3 (f = 0.99), 0.008 at depth 4 (f = 0.999): second fork at 4; not under 0.05 at
    depth 2, so the optimistic mode keeps both forks and drops the stage behind them."""
    f = [0, 0.5, 0.8, 0.99, 0.999, 1, 1, 1, 1]
    base = dict(Q=4, Lq=8, B=2, L=8, logit_bound=1.0, f=f, mu=[0.0] * 9)
    p = plan(driver, **base, tail_extras=0)
    assert (p["forks"], p["drop_last"], p["extras"], p["pool"], p["stats_calls"]) == ([2, 4], 0, 0, 0, 1)
    p = plan(driver, **base, tail_extras=0, forced_tail=2)
    assert (p["forks"], p["drop_last"], p["stats_calls"]) == ([2, 4], 1, 1)
    # budget min(3, B) = 2 with no extras anywhere (mu = 0): nobody is expected to stay behind, second fork right at depth 3;
    # optimistic: one fork, nothing behind it
    p = plan(driver, **base, tail_extras=3)
    assert (p["forks"], p["drop_last"], p["extras"], p["pool"]) == ([2, 3], 0, 2, 4)
    p = plan(driver, **base, tail_extras=3, forced_tail=2)
    assert (p["forks"], p["drop_last"], p["extras"], p["pool"]) == ([2], 1, 2, 4)
    # f^2 never reaches one half before depth L - 2: no fork, and then neither budget nor pool
    p = plan(driver, **{**base, "f": [0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 1, 1]}, tail_extras=3)
    assert (p["forks"], p["extras"], p["pool"], p["stats_calls"]) == ([], 0, 0, 1)


def test_precision_lane_and_table(driver):
    base = dict(Q=6, Lq=16, B=4, L=8, n_fork_override=0, lane_cus=128)
    assert [plan(driver, **base, precision=p)["prec"] for p in (F32, F16X2, BF16)] == [F32, F16X2, F16X2]   # bf16 is a training mode
    assert [plan(driver, **base, precision=p, f32_only=1)["prec"] for p in (F32, F16X2, BF16)] == [F32] * 3
    assert [(plan(driver, **base, lane=l)["lane"], plan(driver, **base, lane=l)["cus"]) for l in (-1, 0, 1)] == [(-1, 0), (0, 128), (1, 128)]
    # the table is read when it is current, in the ctx's mode, by a split-precision search only
    assert [plan(driver, **base, l0_current=1, l0_mode=m)["l0"] for m in (0, 1, 2)] == [0, 1, 2]
    assert plan(driver, **base, l0_current=0, l0_mode=2)["l0"] == 0
    assert plan(driver, **base, l0_current=1, l0_mode=2, precision=F32)["l0"] == 0
    p = plan(driver, **base, flags=3, margins=1, tail_rank_replay=7, select_radix=2)
    assert (p["Q"], p["Lq"], p["B"], p["L"], p["flags"], p["margins"], p["tail_rank_replay"], p["select_radix"]) == (6, 16, 4, 8, 3, 1, 1, 2)
    assert plan(driver, **base)["select_radix"] == -1


def test_key_tells_every_field_apart(driver):
    k = json.loads(run(driver, "key"))
    names, eq, lt = k["names"], k["eq"], k["lt"]
    n = len(names)
    assert names[:2] == ["base", "copy"] and {"prec", "margins", "l0", "extras", "fork0", "fork1", "drop_last", "lane", "tail_rank_replay",
                                              "select_radix", "flag log_softmax", "flag no_graph"} <= set(names)
    for i, j in itertools.product(range(n), repeat=2):
        same = i == j or {i, j} == {0, 1}
        assert eq[i][j] == int(same), (names[i], names[j])
        # a strict weak order whose equivalence is ==: irreflexive, and exactly one of <, >, == holds
        assert lt[i][j] + lt[j][i] + eq[i][j] == 1, (names[i], names[j])
    for i, j, l in itertools.product(range(n), repeat=3):       # transitive (with the above: also through equal plans)
        assert not (lt[i][j] and lt[j][l]) or lt[i][l], (names[i], names[j], names[l])
