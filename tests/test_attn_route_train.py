"""The planners of the training step's four attention sites (ripor_amd/csrc/attn_route.h: plan_train_self_attn_bwd,
plan_train_self_attn_drop_fwd, plan_train_cross_attn_bwd, plan_train_cross_attn_drop_fwd) and the admission helper
(train_attn_admitted), swept on the CPU against the launcher logic they replaced. tests/attn_route_train_driver.cpp prints a whole
grid in one process; the expectations below restate, branch by branch, what launch_self_attn_bwd,
launch_cross_attn_bwd, launch_self_attn_drop_fwd, launch_cross_attn_drop_fwd (train_kernels.hip), run_attn_bwd_tiled,
run_attn_drop_fwd_tiled (attn_mfma.hip) and train_setup (train_api.hip) did by hand before the planners existed — none of it is
read from the header.

LDS in floats (x 4 bytes), against the 40 960 of a CU:
  self carve     4 Ls 65 + 2 Ls (Ls + 1) + 64 + 5 Ls            the resident backward and, asking for the same, its drop-forward
  cross carve    2 n 65 + 2 Lq 65 + 2 n (Lq + 1) + Lq
  MFMA tile      2 (3 x 2048 + 64 + 96 + 64 + 64) = 12 864       two waves per block, 128 threads
  tiles          self backward 20 480, self forward 17 152, cross backward 17 408, cross forward 16 640 (test_attn_route_long.py)
Refusals compare as the empty plan: NONE, invalid, grid 0, block 256, no LDS."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
S, BZ, H = 2, 2, 12
REFUSED = ("NONE", 1, 0, 256, 0)
MFMA_LDS = 2 * (3 * 32 * 64 + 64 + 96 + 64 + 64) * 4
TILED_LDS = {"TRAIN_SELF_BWD_TILED": 20480 * 4, "TRAIN_SELF_DROP_FWD_TILED": 17152 * 4, "TRAIN_CROSS_BWD_TILED": 17408 * 4,
             "TRAIN_CROSS_DROP_FWD_TILED": 16640 * 4}


def self_carve(Ls):
    return 4 * (4 * Ls * 65 + 2 * Ls * (Ls + 1) + 64 + 5 * Ls)


def cross_carve(n, Lq):
    return 4 * (2 * n * 65 + 2 * Lq * 65 + 2 * n * (Lq + 1) + Lq)


def tiled(kernel, seqs, nq, nk, buckets, dkv, mask, drop, drop_L):
    """plan_attn_tiled followed by the checks of run_attn_bwd_tiled / run_attn_drop_fwd_tiled: 64-dim heads, 1 .. 256 query rows and
    keys, a key mask, and with dropout whole sequences of drop_L rows. One block of 256 threads per (sequence, head)."""
    if dkv != 64 or nq < 1 or nk < 1 or nq > 256 or nk > 256 or buckets > 64 or not mask:
        return REFUSED
    if drop and (drop_L < 1 or nq % drop_L):
        return REFUSED
    return (kernel, 0, seqs * H, 256, TILED_LDS[kernel])


def old_self_bwd(Ls, dkv, causal, mask, drop, drop_L, buckets):
    """launch_self_attn_bwd: the resident plan; where it refuses, the tiles if the carve is what refused and the launch is
    bidirectional; with dropout the VALU kernel whatever the resident plan said."""
    carve = self_carve(Ls)
    if carve > LDS or buckets > 64 or Ls < 1 or dkv not in (64, 128):
        if causal or carve <= LDS:
            return REFUSED
        return tiled("TRAIN_SELF_BWD_TILED", S, Ls, Ls, buckets, dkv, mask, drop, drop_L)
    if dkv == 128:
        return ("TRAIN_BWD_VALU128", 0, S * H, 256, carve)
    if not drop and Ls <= 32:
        return ("TRAIN_BWD_MFMA", 0, (S * H + 1) // 2, 128, MFMA_LDS)
    return ("TRAIN_BWD_VALU", 0, S * H, 256, carve)


def old_self_drop_fwd(Ls, dkv, causal, mask, drop, drop_L, buckets):
    """launch_self_attn_drop_fwd (always with dropout: ``drop`` is not read). The resident kernel asks for the backward's carve and
    does not look at drop_L."""
    carve = self_carve(Ls)
    if carve > LDS and dkv == 64 and not causal and mask:
        return tiled("TRAIN_SELF_DROP_FWD_TILED", S, Ls, Ls, buckets, dkv, mask, True, drop_L)
    if carve > LDS or buckets > 64 or Ls < 1 or Ls > 256 or (not causal and not mask) or dkv not in (64, 128):
        return REFUSED
    return ("TRAIN_SELF_DROP_FWD128" if dkv == 128 else "TRAIN_SELF_DROP_FWD", 0, S * H, 256, carve)


def old_cross_bwd(n, Lq, dkv, mask, drop, drop_L):
    """launch_cross_attn_bwd. Resident with dropout it also stopped at 256 keys (a few decoder rows fit the carve beyond them)."""
    carve = cross_carve(n, Lq)
    if carve > LDS:
        return tiled("TRAIN_CROSS_BWD_TILED", BZ, n, Lq, 0, dkv, mask, drop, drop_L) if dkv == 64 else REFUSED
    if dkv not in (64, 128):
        return REFUSED
    if drop and (drop_L < 1 or n % drop_L or Lq > 256):
        return REFUSED
    return ("TRAIN_CROSS_BWD128" if dkv == 128 else "TRAIN_CROSS_BWD", 0, BZ * H, 256, carve)


def old_cross_drop_fwd(n, Lq, dkv, mask, drop, drop_L):
    """launch_cross_attn_drop_fwd (always with dropout)."""
    carve = cross_carve(n, Lq)
    if carve > LDS:
        return tiled("TRAIN_CROSS_DROP_FWD_TILED", BZ, n, Lq, 0, dkv, mask, True, drop_L) if dkv == 64 else REFUSED
    if drop_L < 1 or n % drop_L or dkv not in (64, 128):
        return REFUSED
    return ("TRAIN_CROSS_DROP_FWD128" if dkv == 128 else "TRAIN_CROSS_DROP_FWD", 0, BZ * H, 256, carve)


OLD = {"self_bwd": old_self_bwd, "self_drop_fwd": old_self_drop_fwd, "cross_bwd": old_cross_bwd, "cross_drop_fwd": old_cross_drop_fwd}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_route_train") / "attn_route_train_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "attn_route_train_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def sweep(driver, what):
    """-> {(site, *shape): (kernel, invalid, grid, block, smem)} of one sweep of the driver, and its number of lines (drop_L = Ls
    names 0 and 7 twice)."""
    rows, lines = {}, 0
    for line in subprocess.run([driver, "sweep", what], check=True, capture_output=True, text=True).stdout.splitlines():
        shape, plan = line.split(" | ")
        site, *ints = shape.split()
        kernel, *launch = plan.split()
        key = (site,) + tuple(map(int, ints))
        lines += 1
        assert rows.setdefault(key, (kernel,) + tuple(map(int, launch))) == (kernel,) + tuple(map(int, launch)), key
    return rows, lines


def check(rows):
    wrong = [(k, v, OLD[k[0]](*k[1:])) for k, v in rows.items() if v != OLD[k[0]](*k[1:])]
    assert not wrong, (len(wrong), wrong[:5])


def test_self_attention_planners_decide_as_the_launchers_did(driver):
    """Ls 0 .. 258, d_kv 32 / 64 / 128, causal, key mask, dropout with drop_L 0 / Ls / 7, 32 / 64 / 65 buckets, both sites:
    259 x 3 x 2 x 2 x 6 x 3 x 2 = 111 888 plans. The boundaries pinned by hand elsewhere lie on their sides: 32 | 33 between the MFMA
    tile and the VALU kernel, 91 | 92 between the carve (163 692 bytes) and the tiles or the refusal."""
    rows, lines = sweep(driver, "self")
    assert lines == 259 * 3 * 2 * 2 * 6 * 3 * 2
    check(rows)
    assert rows[("self_bwd", 32, 64, 1, 0, 0, 0, 32)] == ("TRAIN_BWD_MFMA", 0, 12, 128, 51456)
    assert rows[("self_bwd", 33, 64, 1, 0, 0, 0, 32)] == ("TRAIN_BWD_VALU", 0, 24, 256, 44212)
    assert rows[("self_bwd", 32, 64, 1, 0, 1, 32, 32)] == ("TRAIN_BWD_VALU", 0, 24, 256, self_carve(32))     # dropout: never the tile
    assert rows[("self_bwd", 91, 64, 0, 1, 0, 0, 32)] == ("TRAIN_BWD_VALU", 0, 24, 256, 163692)
    assert rows[("self_bwd", 92, 64, 0, 1, 0, 0, 32)] == ("TRAIN_SELF_BWD_TILED", 0, 24, 256, 81920)
    assert rows[("self_bwd", 92, 64, 1, 1, 0, 0, 32)] == REFUSED and rows[("self_bwd", 92, 128, 0, 1, 0, 0, 32)] == REFUSED
    assert rows[("self_bwd", 91, 128, 0, 1, 1, 91, 32)] == ("TRAIN_BWD_VALU128", 0, 24, 256, 163692)
    assert rows[("self_drop_fwd", 91, 64, 0, 1, 1, 0, 32)] == ("TRAIN_SELF_DROP_FWD", 0, 24, 256, 163692)    # drop_L is not read
    assert rows[("self_drop_fwd", 92, 64, 0, 1, 1, 92, 32)] == ("TRAIN_SELF_DROP_FWD_TILED", 0, 24, 256, 68608)
    assert rows[("self_drop_fwd", 92, 64, 0, 1, 1, 7, 32)] == REFUSED                                        # 92 % 7: the tiles read it
    kernels = {v[0] for v in rows.values()}
    assert kernels == {"NONE", "TRAIN_BWD_MFMA", "TRAIN_BWD_VALU", "TRAIN_BWD_VALU128", "TRAIN_SELF_BWD_TILED", "TRAIN_SELF_DROP_FWD",
                       "TRAIN_SELF_DROP_FWD128", "TRAIN_SELF_DROP_FWD_TILED"}


def test_cross_attention_planners_decide_as_the_launchers_did(driver):
    """n of 1, 8, 16, 32, 64, 128, 256, 257 decoder rows, Lq 1 .. 258, d_kv 32 / 64 / 128, key mask, dropout with drop_L 0 / 8 / 7,
    both sites: 8 x 258 x 3 x 2 x 6 x 2 = 148 608 plans. n = 64: 8448 + 259 Lq floats, Lq 125 (40 823) resident, 126 (41 082) tiled;
    n = 16 at Lq 129: 23 139 floats, resident; at Lq 256: 43 840, tiled."""
    rows, lines = sweep(driver, "cross")
    assert lines == len(rows) == 8 * 258 * 3 * 2 * 6 * 2
    check(rows)
    assert rows[("cross_bwd", 64, 125, 64, 1, 0, 0)] == ("TRAIN_CROSS_BWD", 0, 24, 256, 40823 * 4)
    assert rows[("cross_bwd", 64, 126, 64, 1, 0, 0)] == ("TRAIN_CROSS_BWD_TILED", 0, 24, 256, 69632)
    assert rows[("cross_bwd", 64, 126, 128, 1, 0, 0)] == REFUSED
    assert rows[("cross_bwd", 16, 256, 64, 1, 1, 8)] == ("TRAIN_CROSS_BWD_TILED", 0, 24, 256, 69632)
    assert rows[("cross_drop_fwd", 16, 256, 64, 1, 1, 8)] == ("TRAIN_CROSS_DROP_FWD_TILED", 0, 24, 256, 66560)
    for site, kernel in (("cross_bwd", "TRAIN_CROSS_BWD"), ("cross_drop_fwd", "TRAIN_CROSS_DROP_FWD")):
        assert rows[(site, 16, 129, 64, 1, 1, 8)] == (kernel, 0, 24, 256, 23139 * 4)
        assert rows[(site, 16, 129, 128, 1, 1, 8)] == (kernel + "128", 0, 24, 256, 23139 * 4)
        assert rows[(site, 16, 129, 64, 1, 1, 7)] == REFUSED
    # eight rows fit the carve beyond 256 keys (Lq 257: 38 835 floats): the backward with dropout stops there, nothing else does
    assert rows[("cross_bwd", 8, 257, 64, 1, 0, 0)] == ("TRAIN_CROSS_BWD", 0, 24, 256, 38835 * 4)
    assert rows[("cross_bwd", 8, 257, 64, 1, 1, 8)] == REFUSED
    assert rows[("cross_drop_fwd", 8, 257, 64, 1, 1, 8)] == ("TRAIN_CROSS_DROP_FWD", 0, 24, 256, 38835 * 4)
    kernels = {v[0] for v in rows.values()}
    assert kernels == {"NONE", "TRAIN_CROSS_BWD", "TRAIN_CROSS_BWD128", "TRAIN_CROSS_BWD_TILED", "TRAIN_CROSS_DROP_FWD",
                       "TRAIN_CROSS_DROP_FWD128", "TRAIN_CROSS_DROP_FWD_TILED"}


def test_admission_agrees_with_the_expression_it_replaced(driver):
    """train_setup admitted a step with tiled_ok || (self carve of max(L, Lq) fits && cross carve of (docs L, Lq) fits), tiled_ok =
    64-dim heads with 1 .. 256 decoder rows per query and 1 .. 256 tokens and at most 64 buckets. train_attn_admitted asks the planners
    for every attention launch of the step instead. d_kv 64 / 128, 1 / 2 / 4 / 8 docs, L 1 / 8 / 32 / 64, Lq 1 .. 256, 2 / 32 / 64
    buckets — what rpr_load_model lets through: 2 x 4 x 4 x 256 x 3 = 24 576 steps, and they agree on every one. They would differ
    beyond 64 buckets, which the old expression ignored on its resident side and every planner refuses; no such model is loaded, so
    that never reaches train_setup."""
    lines = subprocess.run([driver, "sweep", "admit"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 2 * 4 * 4 * 256 * 3
    wrong, admitted = [], 0
    for line in lines:
        shape, got = line.split(" | ")
        dkv, docs, L, Lq, buckets = map(int, shape.split())
        tiled_ok = dkv == 64 and 1 <= docs * L <= 256 and 1 <= Lq <= 256 and buckets <= 64
        old = tiled_ok or (self_carve(max(L, Lq)) <= LDS and cross_carve(docs * L, Lq) <= LDS)
        admitted += old
        if int(got) != int(old):
            wrong.append((shape, got, old))
    assert not wrong, (len(wrong), wrong[:5])
    assert 0 < admitted < len(lines)


def test_the_launchers_hold_no_route_of_their_own():
    """The literal 160 * 1024 and the second copy of the cross carve are gone from the training sources, and every launch of a
    training attention kernel stands in a switch over the plan's kernel."""
    csrc = os.path.join(REPO, "ripor_amd", "csrc")
    for name in ("train_kernels.hip", "train_api.hip", "common.h"):
        src = open(os.path.join(csrc, name)).read()
        assert "160 * 1024" not in src and "cross_attn_bwd_smem" not in src, name
    kernels = ("self_attn_bwd_kernel", "cross_attn_bwd_kernel", "self_attn_drop_fwd_kernel", "cross_attn_drop_fwd_kernel",
               "attn_bwd_tiled_kernel", "attn_drop_fwd_tiled_kernel")
    launches = 0
    for name in ("train_kernels.hip", "attn_mfma.hip"):
        lines = open(os.path.join(csrc, name)).read().splitlines()
        for i, line in enumerate(lines):
            if "hipLaunchKernelGGL" in line and any(k in line for k in kernels):
                launches += 1
                assert "case ATTN_TRAIN_" in lines[i] + lines[i - 1], (name, i + 1, line)
    assert launches == 12
