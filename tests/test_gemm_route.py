"""The shape -> route table of the split-precision GEMM (ripor_amd/csrc/gemm_route.h), checked on the CPU.

tests/gemm_route_driver.cpp includes the header and is compiled here with the host C++ compiler. Every expectation below
was worked out by hand from launch_gemm_h2 as it stood before the planner was split out of it (the arithmetic is in the
comments), or is a number its comments and tools/rowsplit_bench.sh record — none comes from running the planner."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 16 << 20          # floats of split-K scratch lent by the caller
SEARCH = dict(part=1, mid_split=1, part_cap=CAP)   # what the search path's projections set (passes.hip: linear)
INT_MAX = 0x7fffffff


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "gemm_route_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def run(driver, mode, *args, **kw):
    argv = [driver, mode] + list(args) + [f"{k}={int(v)}" for k, v in kw.items()]
    return subprocess.run(argv, check=True, capture_output=True, text=True).stdout


def plan(driver, **kw):
    return json.loads(run(driver, "plan", **kw))


def step(s, *keys):
    return tuple(s[k] for k in keys)


SHAPE = ("family", "bm", "bn", "stages", "full", "ksplit", "reduce", "grid")
ROWS = ("rows", "m_base")


def test_beam1000_search_product_is_row_split(driver):
    """M = 27000, N = 768: ceil(27000 / 256) * 3 = 318 tiles of 256^2, round efficiency 318 / 512 = 0.62 >= 0.6: ping-pong.
    One whole round = 256 tiles = 85 row panels of 3 -> 21760 rows; the 5240 rows behind them are 41 * 6 = 246 tiles of
    128^2: 1 + 0.43 * 1 + 6 / 78 = 1.51 < 0.9 * 2, so the launch is split (tools/rowsplit_bench.sh names 21760 / 5240)."""
    p = plan(driver, M=27000, N=768, K=768, **SEARCH)
    assert (p["invalid"], p["cls"], len(p["steps"])) == (0, "gemm", 2)
    a, b = p["steps"]
    assert step(a, *ROWS) == (21760, 0) and step(b, *ROWS) == (5240, 21760)
    assert step(a, *SHAPE) == ("pp", 256, 256, 0, 1, 1, "none", [255, 1]) and a["block"] == 512 and a["tile_cw"] == 0
    assert step(b, *SHAPE) == ("dma", 128, 128, 2, 0, 1, "none", [246, 1]) and b["block"] == 256   # 246 > 128 blocks: two stages
    # a lane stream with half the chip: two whole rounds of 128 and 246 tiles of 128^2 = two more rounds of those:
    # 2 + 0.43 * 2 + 0.08 = 2.94 > 0.9 * 3: one launch
    assert [step(s, "family", *ROWS) for s in plan(driver, M=27000, N=768, K=768, cus=128, **SEARCH)["steps"]] == [("pp", 27000, 0)]


def test_rowsplit_switch(driver):
    p = plan(driver, M=27000, N=768, K=768, row_split=0, **SEARCH)     # off: one ragged ping-pong launch, 256 persistent blocks
    assert [step(s, *SHAPE) for s in p["steps"]] == [("pp", 256, 256, 0, 0, 1, "none", [256, 1])] and p["cls"] == "gemm"
    # = 2: every ping-pong launch with two or more row tiles is split in the middle, no_row_split or not.
    # M = 16384, N = 768: 64 * 3 = 192 tiles (efficiency 0.75), under one round: not split by default
    assert len(plan(driver, M=16384, N=768, K=768)["steps"]) == 1
    for nrs in (0, 1):
        p = plan(driver, M=16384, N=768, K=768, row_split=2, no_row_split=nrs)
        assert [step(s, "family", "bn", *ROWS) for s in p["steps"]] == [("pp", 256, 8192, 0), ("dma", 128, 8192, 8192)]
    assert [s["family"] for s in plan(driver, M=256, N=768 * 40, K=768, out_h=1, row_split=2)["steps"]] == ["pp"]   # one row tile


def test_round_efficiency_bar(driver):
    """M = 8192, N = 2304: 32 * 9 = 288 tiles, round efficiency 288 / 512 = 0.5625 < 0.6: 128 x 128 tiles for an fp32 output
    (64 * 18 = 1152 of them); with an f16-plane output the ping-pong kernel whatever the efficiency, and the row split:
    256 / 9 = 28 row panels = 7168 rows + 1024 (8 * 18 = 144 tiles of 128^2: 1.51 < 1.8)."""
    p = plan(driver, M=8192, N=2304, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 128, 2, 1, 1, "none", [1152, 1])] and p["cls"] == "gemm_small"
    p = plan(driver, M=8192, N=2304, K=768, out_h=1, **SEARCH)
    assert [step(s, "family", "bn", "full", "grid", *ROWS) for s in p["steps"]] == [("pp", 256, 1, [252, 1], 7168, 0), ("dma", 128, 1, [144, 1], 1024, 7168)]
    assert p["steps"][0]["tile_cw"] == 0 and p["steps"][1]["stages"] == 2       # 252 tiles on 252 blocks: nothing to order
    # no_row_split (packed encoder): one launch, 288 tiles on 256 persistent blocks, super-tiles of 3 columns (9 % 3 == 0) x
    # (256 / 8) / 3 = 10 row panels
    p = plan(driver, M=8192, N=2304, K=768, out_h=1, no_row_split=1, **SEARCH)
    assert [step(s, *SHAPE, "tile_cw", "tile_rb") for s in p["steps"]] == [("pp", 256, 256, 0, 1, 1, "none", [256, 1], 3, 10)]
    p = plan(driver, M=8192, N=2304, K=768, out_h=1, no_row_split=1, supertile=0, **SEARCH)   # RPR_PP_SUPERTILE=0: row-major
    assert step(p["steps"][0], "tile_cw", "tile_rb") == (0, 0)
    p = plan(driver, M=8192, N=3072, K=768, out_h=1, no_row_split=1)            # 12 column tiles: groups of 4, 32 / 4 = 8 row panels
    assert step(p["steps"][0], "tile_cw", "tile_rb") == (4, 8)


def test_few_rows(driver):
    """One query in flight: the 16-row skinny kernel, N / 16 column tiles x ceil(M / 16) row tiles."""
    p = plan(driver, M=16, N=768, K=768, **SEARCH)
    assert [step(s, "family", "full", "grid", "block") for s in p["steps"]] == [("skinny16", 1, [48, 1], 256)] and p["cls"] == "gemm_small"
    assert plan(driver, M=32, N=768, K=768, m_dev=1)["steps"][0]["full"] == 0 and plan(driver, M=32, N=768, K=768)["steps"][0]["grid"] == [48, 2]
    # 33 rows, N = K = 768 (choose_wsplit by hand: 32 x 32: 2 * 24 = 48 blocks, one round, 5 + 3 + 196.6 KB / 48 = 12.1 us;
    # 64 x 32: 14.1; 64 x 64: 17.6; a K split adds 4.5 us for the reduction and saves less): 32 x 32, four stages, no split
    p = plan(driver, M=33, N=768, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 32, 32, 4, 0, 1, "none", [48, 1])]
    # 352 rows: 32 x 32 needs 264 blocks = two rounds (19.2 us), 64 x 32 144 blocks in one (5 + 3 + 294.9 / 48 = 14.1), 64 x 64 with
    # three splits 15.7: 64 x 32, three stages
    p = plan(driver, M=352, N=768, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 64, 32, 3, 0, 1, "none", [144, 1])]


def test_wave_split_only_within_one_round(driver):
    # 400 rows, N = 768: 64 x 32 tiles = 7 * 24 = 168 blocks, one round (14.1 us, the best shape): wave-split
    p = plan(driver, M=400, N=768, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 64, 32, 3, 0, 1, "none", [168, 1])]
    # 640 rows, N = 2304: the best wave-split shape (64 x 64, 360 blocks) needs two rounds -> the 128 x 64 fused split-K route:
    # 5 * 36 = 180 tiles, ks = min(ceil(384 / 180) = 3, 4, 768 / 128) = 3, fused epilogue four columns per thread (2304 % 256 == 0)
    p = plan(driver, M=640, N=2304, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 2, 1, 3, "fused4", [180, 3])] and p["cls"] == "gemm_small"
    # 1400 rows, N = 3072: 11 * 48 = 528 tiles of 128 x 64 >= 256 CUs: no split; 11 * 24 = 264 >= 256 tiles of 128^2: 128 x 128
    p = plan(driver, M=1400, N=3072, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 128, 2, 0, 1, "none", [264, 1])]
    # without the search path's scratch the 640-row product has no K split: 5 * 18 = 90 < 256 tiles of 128^2 -> 128 x 64, 180 > 128 blocks
    p = plan(driver, M=640, N=2304, K=768)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 2, 1, 1, "none", [180, 1])]
    # N = 352 is no multiple of 64: no K split; 11 * 3 = 33 < 256 tiles of 128^2 -> 11 * 6 = 66 <= 128 blocks of 128 x 64, four stages deep
    p = plan(driver, M=1401, N=352, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 4, 0, 1, "none", [66, 1])]
    assert plan(driver, M=1500, N=64, K=768)["steps"][0]["stages"] == 4          # 12 blocks <= 128
    for n in (256, 768, 2304, 3072):                                             # 1401 rows: never wave-split
        assert plan(driver, M=1401, N=n, K=768, **SEARCH)["steps"][0]["family"] == "dma"
        assert plan(driver, M=1400, N=n, K=768, wsplit_max=0, **SEARCH)["steps"][0]["family"] == "dma"
    # 1401 rows, N = 768: 11 * 12 = 132 tiles of 128 x 64 -> ks = 3, ragged
    p = plan(driver, M=1401, N=768, K=768, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 2, 0, 3, "fused4", [132, 3])]


def test_wave_split_switches(driver):
    # RPR_GEMM_WSPLIT_MAX=0: 400 rows take the route behind: 4 * 12 = 48 tiles of 128 x 64, ks = min(ceil(384 / 48), 4, 6) = 4
    p = plan(driver, M=400, N=768, K=768, wsplit_max=0, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 2, 0, 4, "fused4", [48, 4])]
    p = plan(driver, M=33, N=768, K=768, wsplit_max=0, **SEARCH)                 # at most 352 rows: the skinny route's 32 x 32 tiles
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 32, 32, 4, 0, 1, "none", [48, 1])]
    # RPR_WSPLIT_CFG / RPR_WSPLIT_KS force shape and split, and the route itself where the model would leave it
    p = plan(driver, M=400, N=768, K=768, wsplit_cfg=2, wsplit_ks=2, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 64, 64, 2, 0, 2, "fused4", [84, 2])]
    p = plan(driver, M=640, N=2304, K=768, wsplit_cfg=0, wsplit_ks=1, **SEARCH)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 32, 32, 4, 1, 1, "none", [1440, 1])]
    p = plan(driver, M=400, N=768, K=768, wsplit_cfg=1, wsplit_ks=3)             # no scratch: the forced split is not taken
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 64, 32, 3, 0, 1, "none", [168, 1])]
    p = plan(driver, M=400, N=800, K=768, wsplit_cfg=2, wsplit_ks=2, **SEARCH)   # N % 64 != 0: no K split
    assert step(p["steps"][0], "ksplit", "reduce") == (1, "none")
    p = plan(driver, M=400, N=832, K=768, wsplit_cfg=2, wsplit_ks=2, **SEARCH)   # N % 256 != 0: one column per thread
    assert step(p["steps"][0], "ksplit", "reduce") == (2, "fused")


def test_tile_switch(driver):
    p = plan(driver, M=640, N=768, K=768, force_tile=256, **SEARCH)              # RPR_GEMM_TILE=256: ping-pong whatever the shape
    assert [step(s, *SHAPE) for s in p["steps"]] == [("pp", 256, 256, 0, 0, 1, "none", [9, 1])] and p["cls"] == "gemm"
    assert len(plan(driver, M=27000, N=768, K=768, force_tile=256, **SEARCH)["steps"]) == 1    # and no row split
    for m in (16, 400, 27000):                                                   # = 64 / 128: that tile of the 128-row kernel
        p = plan(driver, M=m, N=768, K=768, force_tile=64, **SEARCH)
        assert [step(s, "family", "bn", "ksplit") for s in p["steps"]] == [("dma", 64, 1)] and p["cls"] == "gemm_small"
        p = plan(driver, M=m, N=768, K=768, force_tile=128, **SEARCH)
        assert [step(s, "family", "bn", "ksplit") for s in p["steps"]] == [("dma", 128, 1)]


def test_compacted_stage(driver):
    """m_dev, small_live = 1024, capacity 8192 rows: three launches gated on the live count. 32 * 3 = 96 tiles of 256^2 < 112 and
    64 * 6 = 384 tiles of 128^2: the large-tile launch is 128 x 128; 1024 rows are 8 * 12 = 96 <= 128 tiles of 128 x 64 (four
    stages); at most min(352, 1024) rows go to 32 x 32 wave-split tiles, M = 352 already a multiple of 32."""
    p = plan(driver, M=8192, N=768, K=768, m_dev=1, small_live=1024, **SEARCH)
    assert [step(s, *SHAPE, "rows", "live_lo", "live_hi") for s in p["steps"]] == [
        ("dma", 128, 128, 2, 0, 1, "none", [384, 1], 8192, 1024, INT_MAX),
        ("dma", 128, 64, 4, 0, 1, "none", [96, 1], 1024, 352, 1024),
        ("wsplit", 32, 32, 4, 0, 1, "none", [264, 1], 352, -1, 352)]
    assert p["cls"] == "gemm_small" and all(s["m_base"] == 0 for s in p["steps"])
    # small_live = 100: no middle launch, the skinny launch's M rounded up to 128; 27000 rows: the large launch is the ping-pong
    # kernel and sets the profile class
    p = plan(driver, M=27000, N=768, K=768, m_dev=1, small_live=100, no_row_split=1, **SEARCH)
    assert [step(s, "family", "rows", "live_lo", "live_hi") for s in p["steps"]] == [("pp", 27000, 100, INT_MAX), ("wsplit", 128, -1, 100)]
    assert p["cls"] == "gemm"
    # the large launch of a compacted stage is row-split like any other (its small_live is spent): four launches
    p = plan(driver, M=27000, N=768, K=768, m_dev=1, small_live=1024, **SEARCH)
    assert [step(s, "family", "bn", "rows", "m_base", "live_lo", "live_hi") for s in p["steps"]] == [
        ("pp", 256, 21760, 0, 1024, INT_MAX), ("dma", 128, 5240, 21760, 1024, INT_MAX), ("dma", 64, 1024, 0, 352, 1024), ("wsplit", 32, 352, 0, -1, 352)]
    # at most small_live rows of capacity: an ordinary launch with the caller's window (no K split with m_dev: 64 x 64 tiles are
    # the one shape with a single round, 16 * 12 = 192 blocks)
    p = plan(driver, M=1024, N=768, K=768, m_dev=1, small_live=1024, **SEARCH)
    assert [step(s, "family", "bn", "stages", "live_lo", "live_hi") for s in p["steps"]] == [("wsplit", 64, 2, 0, 0)]


def test_bf16(driver):
    p = plan(driver, M=8192, N=768, K=768, bf16=1, out_b=1)
    assert [step(s, "family", "full", "bf16", "grid") for s in p["steps"]] == [("pp", 1, 1, [96, 1])] and p["cls"] == "gemm"
    for kw in (dict(M=8192, N=700), dict(M=8200, N=768), dict(M=8192, N=768, resid=1), dict(M=8192, N=768, outb_al=0)):
        assert plan(driver, K=768, bf16=1, out_b=1, **kw) == {"invalid": 1, "cls": "gemm_small", "steps": []}
    assert plan(driver, M=8192, N=768, K=768, bf16=1, out_h=1)["invalid"] == 1
    # weight gradient K = 8192, M = N = 768: 9 tiles of 256^2, 128 K-tiles of 64: ks = min(256 / 9 = 28, 128 / 4 = 32, cap) = 28,
    # trimmed until every split owns a K-tile: 28 and 27 splits of 5 K-tiles overshoot 128, 26 do not
    p = plan(driver, M=768, N=768, K=8192, bf16=1, part=1, part_cap=CAP)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("pp", 256, 256, 0, 1, 26, "sum", [9, 26])] and p["cls"] == "gemm"
    p = plan(driver, M=768, N=768, K=8192, bf16=1, part=1, part_cap=10 * 768 * 768)      # scratch for 10 partial results
    assert step(p["steps"][0], "ksplit", "grid") == (10, [9, 10])
    # not a multiple of 256: the 128 x 64 split-K: 6 * 11 = 66 tiles, ks = min(ceil(640 / 66) = 10, 8192 / 1024 = 8) = 8
    p = plan(driver, M=768, N=700, K=8192, bf16=1, part=1, part_cap=CAP)
    assert [step(s, *SHAPE, "bf16") for s in p["steps"]] == [("dma", 128, 64, 2, 0, 8, "sum", [66, 8], 1)] and p["cls"] == "gemm_small"
    # 200 or more tiles of 256^2: ping-pong (32 * 12 = 384); 96 tiles: 384 >= 256 tiles of 128^2 -> 128 x 128
    p = plan(driver, M=8192, N=3072, K=768, bf16=1)
    assert [step(s, *SHAPE, "tile_cw", "tile_rb") for s in p["steps"]] == [("pp", 256, 256, 0, 1, 1, "none", [256, 1], 4, 8)]
    assert plan(driver, M=12800, N=1024, K=768, bf16=1)["steps"][0]["family"] == "pp"        # 50 * 4 = 200
    assert plan(driver, M=12544, N=1024, K=768, bf16=1)["steps"][0]["family"] == "dma"       # 49 * 4 = 196
    p = plan(driver, M=8192, N=768, K=768, bf16=1)
    assert [step(s, *SHAPE, "bf16") for s in p["steps"]] == [("dma", 128, 128, 2, 1, 1, "none", [384, 1], 1)]


def test_refused_and_empty(driver):
    assert plan(driver, M=0, N=768, K=768) == {"invalid": 0, "cls": "gemm_small", "steps": []}
    for kw in (dict(K=760), dict(K=0), dict(K=768, ab_al8=0)):
        assert plan(driver, M=64, N=768, **kw)["invalid"] == 1


def test_fp32_long_reduction(driver):
    # training in split precision, dW = dY^T X with 2304 x 768 outputs: 27 tiles of 256^2, 256 K-tiles of 32:
    # ks = min(256 / 27 = 9, 256 / 4, cap / (2304 * 768) = 9) = 9 (8 * 29 < 256: nothing to trim)
    p = plan(driver, M=2304, N=768, K=8192, part=1, part_cap=CAP)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("pp", 256, 256, 0, 1, 9, "sum", [27, 9])] and p["cls"] == "gemm"
    # a ReLU rules the plain sum out: no split; 18 * 6 = 108 < 256 tiles of 128^2 -> 128 x 64, 216 blocks, two stages
    p = plan(driver, M=2304, N=768, K=8192, relu=1, part=1, part_cap=CAP)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("dma", 128, 64, 2, 1, 1, "none", [216, 1])] and p["cls"] == "gemm_small"
    # 768 rows are within the wave-split range, which comes first: 64 x 64 tiles are the one shape with a single round (144 blocks)
    p = plan(driver, M=768, N=768, K=8192, part=1, part_cap=CAP)
    assert [step(s, *SHAPE) for s in p["steps"]] == [("wsplit", 64, 64, 2, 1, 1, "none", [144, 1])]


def test_group_order(driver):
    def order(*mn):
        return [int(x) for x in run(driver, "group", *[f"{m}:{n}" for m, n in mn]).split()]
    # one 3 x 3 product is one super-tile in row-major order; 9 tiles in 8 runs: the last run has two
    assert order((768, 768)) == [0, 1, 2, 3, 4, 5, 6, 7] + [-1] * 7 + [8]
    # the six weight gradients of a t5-base layer (q, k, v, o, wi, wo) at 8192 rows: 4 * 9 + 36 + 36 = 108 tiles
    prods = [(768, 768)] * 4 + [(3072, 768), (768, 3072)]
    asg = order(*prods)
    assert len(asg) % 8 == 0
    tiles = sorted(v for v in asg if v >= 0)
    assert tiles == sorted((i << 16) | t for i, (m, n) in enumerate(prods) for t in range((m // 256) * (n // 256))) and len(tiles) == 108
    runs = [[v for v in asg[x::8]] for x in range(8)]
    lens = [sum(v >= 0 for v in r) for r in runs]
    assert max(lens) - min(lens) <= 1 and len(asg) == 8 * max(lens)
    for r, n in zip(runs, lens):
        assert all(v >= 0 for v in r[:n]) and all(v == -1 for v in r[n:])
    flat = [v for r, n in zip(runs, lens) for v in r[:n]]
    assert [v >> 16 for v in flat] == sorted(v >> 16 for v in flat)      # the runs, one after the other, walk the products in order
    # wi [3072, 768] = 12 x 3 tiles: super-tiles of 4 x 3, each row-major
    wi = [v & 0xffff for v in flat if v >> 16 == 4]
    assert wi == list(range(36))
    # wo [768, 3072] = 3 x 12 tiles: super-tiles of 3 x 4
    wo = [v & 0xffff for v in flat if v >> 16 == 5]
    assert wo[:12] == [0, 1, 2, 3, 12, 13, 14, 15, 24, 25, 26, 27] and wo[12:16] == [4, 5, 6, 7]


@pytest.mark.parametrize("flags", [dict(SEARCH), dict(part=1, part_cap=1 << 20), dict(), dict(out_h=1, no_row_split=0),
                                   dict(m_dev=1, small_live=1024, **SEARCH), dict(bf16=1, part=1, part_cap=CAP)],
                         ids=["search", "train", "plain", "planes", "compacted", "bf16"])
def test_steps_cover_the_rows_once(driver, flags):
    """M in 1..60000, N in {256, 768, 2304, 3072}, K in {768, 3072}: the steps of a plan cover rows [0, M) exactly once — for a
    compacted stage the live windows partition the live counts [0, max] and every windowed step has the rows its window admits —
    and a K split never needs more scratch than the caller lent."""
    cap = flags.get("part_cap", 0)
    compact = flags.get("small_live", 0)
    n_lines = 0
    for line in run(driver, "sweep", **flags).splitlines():
        f = [int(x) for x in line.split()]
        M, N, K, invalid, n = f[:5]
        steps = [f[5 + 5 * i: 10 + 5 * i] for i in range(n)]
        n_lines += 1
        assert not invalid and 1 <= n <= 4, line
        for rows, m_base, lo, hi, ks in steps:
            assert ks == 1 or ks * M * N <= cap, line
        if compact and M > compact:
            # windows (lo, hi] from the top down: (small_live, max], .., [0, ..]
            wins = sorted({(lo, hi) for _, _, lo, hi, _ in steps}, reverse=True)
            assert wins[0][1] == INT_MAX and wins[-1][0] == -1 and all(a[0] == b[1] for a, b in zip(wins, wins[1:])), line
            for lo, hi in wins:
                part = sorted((m_base, rows) for rows, m_base, l, h, _ in steps if (l, h) == (lo, hi))
                end = 0
                for m_base, rows in part:
                    assert m_base == end, line
                    end += rows
                assert end >= min(hi, M) and (hi == INT_MAX) == (end == M), line
        else:
            end = 0
            for rows, m_base, lo, hi, ks in steps:
                assert m_base == end and rows > 0 and (lo, hi) == (0, 0), line
                end += rows
            assert end == M, line
    assert n_lines == 60000 * 4 * 2
