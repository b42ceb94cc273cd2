"""The issue order of the MFMAs in the K-loop of the 256 x 256 split-precision GEMM (ripor_amd/csrc/gemm_h2_pp_body.inc, PP16_MMA48
and PP_MMA24; DESIGN.md §5a "Chained triples"). The 16x16x32 body gives an accumulator its three products lo*hi, hi*lo, hi*hi back
to back instead of sixteen MFMAs apart; the 32x32x16 body keeps them eight apart (chaining did not pay there). Per accumulator the
products and their order are what they were, so every output of either body must keep its BITS: tests/golden/gemm_pp_order_bits.json
holds the sha256 of every output buffer below as the library gave it before the order changed (written once by
tools/gemm_pp_order_record.py from a build of that commit).

One child process loads the development build with RPR_GEMM_TILE=256 (every split-precision launch on the ping-pong kernel,
as tests/test_gpu_gemm_mfma16.py does) and calls single products through the test hook rpr_op_linear_h2:
  * M in {256, 257, 600}: one full row tile, one live row in a second tile, a ragged third tile;
  * N in {256, 768}: one and three column tiles;
  * K in {32, 64, 96, 768}: one K-tile (no DMA slot in the loop is live), two, an odd count, the model's;
  * both MFMA shapes (mfma16 0 / 1);
  * the epilogues "x planes + residual + row sums of squares" and "fp32 out";
  * 600 x 768 x 96 once more with a device-side live row count below M.
Inputs come from synth.uniform_f32 (a hash of name and index: the same bits on every machine).
Reference semantics: torch.nn.Linear inside T5Attention / T5DenseActDense (t5_pretrainer/modeling/t5_generative_retriever.py)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "gemm_pp_order_bits.json")
pytestmark = pytest.mark.gpu

MS, NS, KS = (256, 257, 600), (256, 768), (32, 64, 96, 768)
LIVE_SHAPE, LIVE_ROWS = (600, 768, 96), 600 - 37
EPILOGUES = ["x_planes", "f32"]
# of the largest output, against the fp64 product of the decoded planes: the split-precision bar of tests/test_gpu_gemm_mfma16.py
# for every K, and the tighter figure at the model's K = 768
BOUND, BOUND_K768 = 2e-5, 4e-6

_SCRIPT = r"""
import hashlib, json, sys, torch
sys.path.insert(0, %r)
from ripor_amd import engine as E
from ripor_amd.utils import synth
MS, NS, KS, LIVE_SHAPE, LIVE_ROWS = %r
ctx = E.Context.get(0)
dev = "cuda"
XS, WS = 1.0 / 16, 256.0     # csrc/common.h: X_PLANE_SCALE, W_PLANE_SCALE
def planes(x, s):
    hi = (x * s).half(); lo = (x * s - hi.float()).half()
    return hi, lo
def dec(x, s):
    hi, lo = planes(x, s)
    return (hi.double() + lo.double()) / s
def sha(t): return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
def gen(name, shape, scale): return torch.from_numpy(synth.uniform_f32(name, shape, scale, seed=20)).to(dev)
def err(got, ref): return {"err": (got - ref).abs().max().item(), "scale": max(1.0, ref.abs().max().item())}
out = {}
for M in MS:
    for N in NS:
        for K in KS:
            A = gen(f"order.A.{M}.{K}", (M, K), 1.0); W = gen(f"order.W.{N}.{K}", (N, K), (3.0 / K) ** 0.5)
            R = gen(f"order.R.{M}.{N}", (M, N), 1.0)
            C = dec(A, 1.0) @ dec(W, WS).t()
            for mfma16 in (0, 1):
                pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev); ssq = torch.zeros(M, dtype=torch.int64, device=dev)
                ctx.linear_h2(A, W, 1, mfma16, resid=R, out_planes=pl, ssq_out=ssq)
                o0 = torch.full((M, N), 12345.0, device=dev)
                ctx.linear_h2(A, W, 0, mfma16, out0=o0)
                torch.cuda.synchronize()
                out[f"{M}x{N}x{K} m{mfma16} x_planes"] = dict(err((pl[0].double() + pl[1].double()) / XS, C + dec(R, XS)),
                                                              sha={"planes": sha(pl), "ssq": sha(ssq)})
                out[f"{M}x{N}x{K} m{mfma16} f32"] = dict(err(o0.double(), C), sha={"out": sha(o0)})
                if (M, N, K) == tuple(LIVE_SHAPE):
                    md = torch.tensor([LIVE_ROWS], dtype=torch.int32, device=dev)
                    o0 = torch.full((M, N), 12345.0, device=dev)
                    ctx.linear_h2(A, W, 5, mfma16, m_dev=md, out0=o0)
                    torch.cuda.synchronize()
                    out[f"{M}x{N}x{K} m{mfma16} live_rows"] = dict(err(o0[:LIVE_ROWS].double(), C[:LIVE_ROWS]), sha={"out": sha(o0)},
                                                                   dead_rows_untouched=bool((o0[LIVE_ROWS:] == 12345.0).all()))
print("RESULT " + json.dumps(out))
"""


def run_cases(repo=REPO):
    """Every case in one child process on the development build of `repo`: {case: {err, scale, sha: {buffer: sha256}}}."""
    e = dict(os.environ, RPR_DEV_LIB="1", RPR_GEMM_TILE="256")   # development switches: live only in libripor_hip_dev.so
    script = _SCRIPT % (repo, (MS, NS, KS, LIVE_SHAPE, LIVE_ROWS))
    p = subprocess.run([sys.executable, "-c", script], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def cases():
    return run_cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


def _keys(mfma16, epilogue):
    if epilogue == "live_rows":
        return ["%dx%dx%d m%d live_rows" % (*LIVE_SHAPE, mfma16)]
    return [f"{M}x{N}x{K} m{mfma16} {epilogue}" for M in MS for N in NS for K in KS]


@pytest.mark.parametrize("mfma16", [0, 1])
@pytest.mark.parametrize("epilogue", EPILOGUES + ["live_rows"])
def test_products_meet_the_fp64_bound(cases, epilogue, mfma16):
    """Within 2e-5 of the largest output of the fp64 product of the decoded planes, and within 4e-6 at K = 768; rows past the
    device-side live count keep their sentinel."""
    for key in _keys(mfma16, epilogue):
        v = cases[key]
        bound = (BOUND_K768 if key.split()[0].endswith("x768") else BOUND) * v["scale"]
        print(f"[order] {key}: err {v['err']:.3g} (bound {bound:.3g})")
        assert v["err"] < bound, (key, v)
        assert v.get("dead_rows_untouched", True), key


@pytest.mark.parametrize("mfma16", [0, 1])
@pytest.mark.parametrize("epilogue", EPILOGUES + ["live_rows"])
def test_outputs_keep_the_bits_of_the_interleaved_order(cases, golden, epilogue, mfma16):
    """sha256 of every output buffer (planes and row sums, or the fp32 output with its sentinel rows) equals the record of the
    library before the issue order changed."""
    for key in _keys(mfma16, epilogue):
        assert cases[key]["sha"] == golden[key], key


def test_the_record_holds_exactly_these_cases(golden):
    want = {k for m in (0, 1) for e in EPILOGUES + ["live_rows"] for k in _keys(m, e)}
    assert set(golden) == want
    assert len(want) == 2 * (2 * len(MS) * len(NS) * len(KS) + 1)
