"""The plans of the training attention beyond the one-head LDS carve (ripor_amd/csrc/attn_route.h: plan_*_tiled), checked on the
CPU: tests/attn_route_long_driver.cpp includes the header and is compiled here with the host C++ compiler. The expectations are
worked out by hand from the carve stated in the header — none comes from running the planner.

One block of four waves (256 threads) per (sequence, head), whatever the length. LDS in floats:
  per wave    two 32 x 64 strips = 4096; the self-attention backward adds the wave's 512 diagonal sums
  per block   key mask 256; a backward adds the three row statistics of 256 queries = 768; a relative bias adds the bias per
              diagonal (512) and, in the backward, the block's diagonal sums (512)
  self backward   4 (4096 + 512) + 768 + 256 + 1024 = 20 480 floats = 81 920 B    (two blocks in the 160 KB of a CU)
  self forward    4 x 4096 + 256 + 512              = 17 152 floats = 68 608 B
  cross backward  4 x 4096 + 768 + 256              = 17 408 floats = 69 632 B
  cross forward   4 x 4096 + 256                    = 16 640 floats = 66 560 B
The launchers (train_kernels.hip) ask the resident plan first and come here only when it refuses the length and d_kv = 64."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH = ("kernel", "invalid", "grid", "block", "smem")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_route_long") / "attn_route_long_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "attn_route_long_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def plan(driver, site, **kw):
    argv = [driver, site] + [f"{k}={int(v)}" for k, v in kw.items()]
    return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)


def got(p, *keys):
    return tuple(p[k] for k in keys)


def test_tiled_self_attention_plans(driver):
    """2 sequences x 12 heads = 24 blocks of 256 threads at every length from the first the resident plan refuses (92) over a
    ragged last tile (129 = four tiles and one row) to the maximum (256); the LDS does not depend on the length. 257 tokens,
    128-dim heads, more than 64 buckets and an empty sequence are refused."""
    base = dict(S=2, H=12, buckets=32)
    for Ls in (92, 129, 256):
        assert got(plan(driver, "self_bwd_tiled", Ls=Ls, **base), *LAUNCH) == ("TRAIN_SELF_BWD_TILED", 0, [24, 1], 256, 81920), Ls
        assert got(plan(driver, "self_fwd_tiled", Ls=Ls, **base), *LAUNCH) == ("TRAIN_SELF_DROP_FWD_TILED", 0, [24, 1], 256, 68608), Ls
    assert 2 * 81920 <= 160 * 1024
    for site in ("self_bwd_tiled", "self_fwd_tiled"):
        assert plan(driver, site, Ls=257, **base)["invalid"] == 1
        assert plan(driver, site, Ls=0, **base)["invalid"] == 1
        assert plan(driver, site, Ls=129, dkv=128, **base)["invalid"] == 1
        assert plan(driver, site, Ls=129, S=2, H=12, buckets=65)["invalid"] == 1
    # t5-large: 16 heads, a batch of 64
    assert got(plan(driver, "self_bwd_tiled", S=64, Ls=256, H=16, buckets=32), "grid", "smem") == ([1024, 1], 81920)


def test_the_resident_self_plan_answers_as_before(driver):
    """plan_self_attn_bwd: Ls 32 -> the one-wave MFMA tile, two waves per block: (24 + 1) / 2 = 12 blocks of 128 threads,
    2 (3 x 2048 + 64 + 96 + 64 + 64) x 4 = 51 456 B. Ls 33 -> the VALU kernel, a block per (sequence, head):
    (4 x 33 x 65 + 2 x 33 x 34 + 64 + 5 x 33) x 4 = 11 053 x 4 = 44 212 B. Ls 91: 23 660 + 16 744 + 64 + 455 = 40 923 floats =
    163 692 B <= 163 840. Ls 92: 23 920 + 17 112 + 64 + 460 = 41 556 floats: refused, for both head sizes."""
    base = dict(S=2, H=12, buckets=32)
    assert got(plan(driver, "self_bwd", Ls=32, **base), *LAUNCH) == ("TRAIN_BWD_MFMA", 0, [12, 1], 128, 51456)
    assert got(plan(driver, "self_bwd", Ls=33, **base), *LAUNCH) == ("TRAIN_BWD_VALU", 0, [24, 1], 256, 44212)
    assert got(plan(driver, "self_bwd", Ls=91, **base), *LAUNCH) == ("TRAIN_BWD_VALU", 0, [24, 1], 256, 163692)
    assert got(plan(driver, "self_bwd", Ls=91, dkv=128, **base), *LAUNCH) == ("TRAIN_BWD_VALU128", 0, [24, 1], 256, 163692)
    for dkv in (64, 128):
        p = plan(driver, "self_bwd", Ls=92, dkv=dkv, **base)
        assert got(p, "invalid", "resident", "carve") == (1, 0, 41556 * 4)
    assert plan(driver, "self_bwd", Ls=91, **base)["resident"] == 1


def test_tiled_cross_attention_plans_and_the_carve_boundary(driver):
    """The resident carve of n decoder rows against Lq keys is 2 n 65 + 2 Lq 65 + 2 n (Lq + 1) + Lq floats against the 40 960 of
    a CU. n = 64 (the ranking step at L 32): 8448 + 259 Lq — Lq 125: 40 823 fits, Lq 126: 41 082 does not. The shapes of
    tests/test_gpu_long_queries.py: n 64, Lq 129 -> 41 859 (tiled); n 16, Lq 256 -> 43 840 (tiled); the seq2seq steps, n 32 at
    Lq 129 -> 4160 + 16 770 + 8320 + 129 = 29 379 and n 8 at Lq 256 -> 1040 + 33 280 + 4112 + 256 = 38 688: resident.
    The tiled plan: a block per (query, head) = 2 x 12."""
    base = dict(bz=2, H=12)
    for n, Lq, floats, resident in ((64, 125, 40823, 1), (64, 126, 41082, 0), (64, 129, 41859, 0), (16, 256, 43840, 0),
                                    (32, 129, 29379, 1), (8, 256, 38688, 1)):
        p = plan(driver, "cross_bwd_tiled", n=n, Lq=Lq, **base)
        assert got(p, "carve", "resident") == (floats * 4, resident), (n, Lq)
        assert got(p, *LAUNCH) == ("TRAIN_CROSS_BWD_TILED", 0, [24, 1], 256, 69632), (n, Lq)
        assert got(plan(driver, "cross_fwd_tiled", n=n, Lq=Lq, **base), *LAUNCH) == ("TRAIN_CROSS_DROP_FWD_TILED", 0, [24, 1], 256, 66560)
    for site in ("cross_bwd_tiled", "cross_fwd_tiled"):
        assert plan(driver, site, n=64, Lq=257, **base)["invalid"] == 1
        assert plan(driver, site, n=257, Lq=128, **base)["invalid"] == 1
        assert plan(driver, site, n=64, Lq=129, dkv=128, **base)["invalid"] == 1
        assert plan(driver, site, n=128, Lq=256, **base)["invalid"] == 0      # two documents of 64 codes: the most a query has
