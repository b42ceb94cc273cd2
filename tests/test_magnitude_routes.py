"""The cases of tests/test_gpu_magnitude.py take the kernel family their names say (host only): the route planner
(ripor_amd/csrc/gemm_route.h, through tests/gemm_route_driver.cpp) is asked for the plan of every first launch as the hook
`rpr_op_linear_h2` issues it — split-K scratch of 9 M floats lent, no device-side row count — in x-stream mode (planes out,
residual planes in, row sums out), and for the pinned tiles of the development library."""
import json
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magnitude_probe as mp  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK = dict(part=1, mid_split=1, part_cap=9 << 20)          # api.hip: rpr_op_linear_h2 lends c->ws.part (9 << 20 floats)
X_PLANES = dict(out_h=1, resid_h=1, ssq_out=1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("magnitude_routes") / "gemm_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "gemm_route_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def _plan(driver, **kw):
    argv = [driver, "plan"] + [f"{k}={int(v)}" for k, v in kw.items()]
    return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)


@pytest.mark.parametrize("name", list(mp.ROUTED))
def test_default_route_of_the_case(driver, name):
    (M, N, K), want = mp.ROUTED[name]
    p = _plan(driver, M=M, N=N, K=K, **HOOK, **X_PLANES)
    assert not p["invalid"] and len(p["steps"]) == 1, p
    s = p["steps"][0]
    assert (s["family"], s["bm"], s["bn"], s["ksplit"], s["reduce"]) == want, (name, s)
    assert name.split()[-1] == f"{M}x{N}x{K}"


@pytest.mark.parametrize("tile", list(mp.TILED))
def test_pinned_tile_of_the_case(driver, tile):
    for (M, N, K) in mp.TILED_SHAPES:
        for kw in (dict(M=M, N=N, K=K, **X_PLANES), dict(M=M, N=N, K=N, row_ssq=1)):     # both launches of the chain
            p = _plan(driver, force_tile=tile, **HOOK, **kw)
            assert not p["invalid"] and len(p["steps"]) == 1, p
            s = p["steps"][0]
            assert (s["family"], s["bm"], s["bn"], s["ksplit"]) == mp.TILED[tile] + (1,), (tile, s)
            assert not s["full"] and s["tiles_m"] >= 2, "a ragged last row tile"


def test_every_row_sum_producer_has_a_case():
    """gemm_h2.hip adds to ssq_out in six places: the 128-row LDS-DMA kernel (tiles 128x64, 128x128), the ping-pong kernel (both
    MFMA bodies), skinny16, wave-split, and the one- and four-column split-K epilogues."""
    fams = {(w[0], w[4]) for _, w in mp.ROUTED.values()}
    assert {("skinny16", "none"), ("wsplit", "none"), ("dma", "fused"), ("dma", "fused4")} <= fams
    assert set(mp.TILED) == {64, 128, 256} and len(mp.tiled_names(256)) == 4 and len(mp.tiled_names(64)) == 2
    src = open(os.path.join(REPO, "ripor_amd", "csrc", "gemm_h2.hip")).read() + \
        open(os.path.join(REPO, "ripor_amd", "csrc", "gemm_h2_pp_body.inc")).read()
    assert src.count("atomicAdd(g.ssq_out") == 6, "a producer of row sums was added or removed: give it a case in magnitude_probe.py"
