"""The register epilogue of the 16x16x32 body of the 256 x 256 split-precision GEMM (ripor_amd/csrc/gemm_h2.hip,
h2_direct16_planes / h2_direct16_fp32). The tail-pass instantiation has its W rows DMA'd into LDS in an order that
puts a lane's four MFMA tiles side by side in the output (one order for fp32 outputs, one for plane outputs), and stores 16-byte
row pieces from its accumulators — no staging strips; plane outputs trade half-pieces between lanes c and c ^ 8 first. One wrong
term of the order, of the trade or of the row-sum reduction shows as a column, a row or a lane group in the wrong place.

The processes below load the development build with RPR_GEMM_TILE=256 (every split-precision launch on the ping-pong kernel) and
call single products through `Context.linear_h2(..., mfma16=1)`, as tests/test_gpu_gemm_mfma16.py does.
  * exact placement: operands for which every product and sum is exact in the planes and in fp32, so the outputs equal the
    integer product bit for bit;
  * blocks that walk several tiles (more tiles than CUs, odd and even K-tile counts, both tile orders), random operands against
    fp64;
  * one small search with a tail pass, setting 1 against setting 0.
Reference semantics: torch.nn.Linear inside T5Attention / T5DenseActDense (t5_pretrainer/modeling/t5_generative_retriever.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ROUTE_TOL = 3e-5     # scores after a change of GEMM route (tests/test_gpu_gemm_mfma16.py)
MARGIN_MIN = 1e-3

# 257 x 320 x 32: one K-tile, a ragged second row tile with one live row, a second column tile with 64 live columns (FULL = false);
# 600 x 768 x 96: three K-tiles, three column tiles
EXACT_SHAPES = [(257, 320, 32), (600, 768, 96)]
# the four epilogues a tail pass runs (fused-norm fp32, x planes + residual + row sums, ReLU FF planes, a device-side live row
# count) and the plain fp32 output; the K/V scatter and the fp32 residual keep the staged strips (tests/test_gpu_gemm_mfma16.py)
EXACT_MODES = ["f32", "fused_norm", "x_planes", "ff_planes", "live_rows"]

_EXACT_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, %r)
from ripor_amd import engine as E
ctx = E.Context.get(0)
dev = "cuda"
XS, FFS, FIX = 1.0 / 16, 1.0 / 16, 65536.0     # csrc/common.h: X_PLANE_SCALE, FF_PLANE_SCALE, SSQ_FIX
def dec_out(pl, s): return (pl[0].double() + pl[1].double()) / s
def where(bad):
    i = torch.nonzero(bad)
    return [] if i.numel() == 0 else i[0].tolist()
out = {}
for (M, N, K) in %r:
    gen = torch.Generator(device="cpu").manual_seed(M + N + K)
    # A in {-1, 0, 1}, 256 W in {-2 .. 2}, R in {-1, 0, 1}: the planes hold them exactly (lo = 0), a product is an integer / 256 of
    # magnitude <= 2 K / 256 <= 0.75, x = product + R is an integer / 256 below 2, and 65536 x^2 summed over a wave's 64 columns
    # stays below 2^24: every fp32 step of the kernel, the row sums included, is exact
    A = torch.randint(-1, 2, (M, K), generator=gen).float().to(dev)
    W = (torch.randint(-2, 3, (N, K), generator=gen).float() / 256).to(dev)
    R = torch.randint(-1, 2, (M, N), generator=gen).float().to(dev)
    C = A.double() @ W.double().t()
    live = M - 37
    for mode in %r:
        m = {}
        o0 = torch.full((M, N), 12345.0, device=dev)
        if mode == "f32":
            ctx.linear_h2(A, W, 0, 1, out0=o0)
            bad = o0.double() != C
        elif mode == "fused_norm":
            # row scale rsqrt(row_ssq / (K SSQ_FIX) + 0) = 2, 1, 1/2 by row (row_ssq = K SSQ_FIX 4^j); the hook takes A as x-stream planes
            j = (torch.arange(M, device=dev) %% 3) - 1
            rs = (K * FIX * 4.0 ** j.double()).to(torch.int64)
            ctx.linear_h2(A, W, 4, 1, row_ssq=rs, eps=0.0, out0=o0)
            ref = C * (2.0 ** -j.double())[:, None]
            # the scale is one v_rsq_f32 (1 ulp) of K SSQ_FIX 4^j times the fp32 reciprocal of K SSQ_FIX (half an ulp), the output
            # one more rounding: 2^-22 relative. A misplaced element is off by a multiple of 2^-9.
            bad = (o0.double() - ref).abs() > 2.0 ** -22 * ref.abs()
        elif mode == "x_planes":
            pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev); ssq = torch.zeros(M, dtype=torch.int64, device=dev)
            ctx.linear_h2(A, W, 1, 1, resid=R, out_planes=pl, ssq_out=ssq)
            x = C + R.double()
            bad = dec_out(pl, XS) != x
            want = torch.round((x * x).sum(1) * FIX).to(torch.int64)
            m["ssq_exact"] = bool(torch.equal(ssq, want)); m["ssq_first_bad"] = where(ssq != want)
        elif mode == "ff_planes":
            pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev)
            ctx.linear_h2(A, W, 2, 1, out_planes=pl)
            bad = dec_out(pl, FFS) != torch.relu(C)
        elif mode == "live_rows":
            md = torch.tensor([live], dtype=torch.int32, device=dev)
            ctx.linear_h2(A, W, 5, 1, m_dev=md, out0=o0)
            bad = o0[:live].double() != C[:live]
            m["dead_rows_untouched"] = bool((o0[live:] == 12345.0).all())
        torch.cuda.synchronize()
        m["mismatches"] = int(bad.sum().item()); m["first_bad"] = where(bad)
        out[f"{M}x{N}x{K} {mode}"] = m
print("RESULT " + json.dumps(out))
"""

# more tiles than the 256 CUs, so blocks walk a second tile with their registers and LDS as the first left them; the buffer the last
# K-tile sits in depends on the parity of the K-tile count (3 and 2). 4353 x 4096: 18 x 16 = 288 tiles in super-tile order;
# 22100 x 768: 87 x 3 = 261 tiles row-major, a ragged last row panel
WALK_SHAPES = [(4353, 4096, 96), (4353, 4096, 64), (22100, 768, 96), (22100, 768, 64)]
WALK_MODES = ["x_planes", "fused_norm"]

_WALK_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, %r)
from ripor_amd import engine as E
ctx = E.Context.get(0)
dev = "cuda"
XS, WS, FIX = 1.0 / 16, 256.0, 65536.0
def planes(x, s):
    hi = (x * s).half(); lo = (x * s - hi.float()).half()
    return hi, lo
def dec(x, s):
    hi, lo = planes(x, s)
    return (hi.double() + lo.double()) / s
def dec_out(pl, s): return (pl[0].double() + pl[1].double()) / s
out = {}
for (M, N, K) in %r:
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=dev); W = torch.randn(N, K, device=dev) * K ** -0.5
    R = torch.randn(M, N, device=dev)
    Wd = dec(W, WS)
    for mode in %r:
        runs = []
        for rep in range(2):
            if mode == "x_planes":
                pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev); ssq = torch.zeros(M, dtype=torch.int64, device=dev)
                ctx.linear_h2(A, W, 1, 1, resid=R, out_planes=pl, ssq_out=ssq); runs.append((pl, ssq))
            else:
                xd = dec(A, XS)
                rs = torch.round((xd * xd).sum(1) * FIX).to(torch.int64)
                o0 = torch.full((M, N), 12345.0, device=dev)
                ctx.linear_h2(A, W, 4, 1, row_ssq=rs, eps=1e-6, out0=o0); runs.append((o0, rs))
            torch.cuda.synchronize()
        m = {"repeat": bool(torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]))}
        if mode == "x_planes":
            got, ref = dec_out(runs[0][0], XS), dec(A, 1.0) @ Wd.t() + dec(R, XS)
            # the row sums against the sums over the decoded planes, to the planes' quantum (tests/test_gpu_gemm_mfma16.py)
            xq = torch.maximum(torch.full_like(got, 2.0 ** -20), got.abs() * 2.0 ** -21)
            own = (got * got).sum(1)
            tol = (2 * got.abs() * xq + xq * xq).sum(1) + (N / 64) * 0.5 / FIX + 1e-5 * own
            m["ssq_own_excess"] = ((runs[0][1].double() / FIX - own).abs() - tol).max().item()
        else:
            got = runs[0][0].double()
            ref = (dec(A, XS) @ Wd.t()) * torch.rsqrt(runs[0][1].double() / (FIX * K) + 1e-6)[:, None]
        m["err"] = (got - ref).abs().max().item(); m["scale"] = max(1.0, ref.abs().max().item())
        out[f"{M}x{N}x{K} {mode}"] = m
        del got, ref
print("RESULT " + json.dumps(out))
"""

_SEARCH_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from ripor_amd import engine as E
from ripor_amd.utils import synth
out_path, Q, B, L, V, N, seed = sys.argv[1], *[int(x) for x in sys.argv[2:8]]
dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
ctx = E.Context.get(0)
model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=seed), dims)
trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(N, L, V, seed=seed), V)
ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=seed, max_len=12)
ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
out = {}
ctx.set_fork_depths([3])
for mfma16 in (0, 1):
    ctx.set_gemm_mfma16(mfma16)
    res = E.search(model, trie, ti, tm, B, L, margins=True)
    torch.cuda.synchronize()
    for k in ("tokens", "scores", "row_lo", "row_hi", "margins"):
        out[f"m{mfma16}_{k}"] = getattr(res, k).cpu().numpy()
    out[f"m{mfma16}_forced"] = np.int64(sum(f["forced"] for f in ctx.last_fork_stats()))
ctx.set_fork_depths(None); ctx.set_gemm_mfma16(1)
np.savez(out_path, **out)
"""


def _dev_run(script, *argv, timeout=600):
    e = dict(os.environ, RPR_DEV_LIB="1", RPR_GEMM_TILE="256")   # development switches: live only in libripor_hip_dev.so
    p = subprocess.run([sys.executable, "-c", script, *[str(a) for a in argv]], env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return p.stdout


def _result(out):
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def exact():
    return _result(_dev_run(_EXACT_SCRIPT % (REPO, EXACT_SHAPES, EXACT_MODES)))


@pytest.mark.parametrize("mode", EXACT_MODES)
def test_exact_operands_land_in_their_rows_and_columns(exact, mode):
    """Operands whose products and sums are exact (integers, integer multiples of 2^-8): the fp32 output, the decoded x planes and
    FF planes equal the integer product, and ssq_out equals SSQ_FIX times the row's sum of squares, bit for bit (the fused-norm
    output to the rounding of its row scale, 2^-22); rows past the device-side live count keep their sentinel."""
    for (M, N, K) in EXACT_SHAPES:
        v = exact[f"{M}x{N}x{K} {mode}"]
        print(f"[direct] {M}x{N}x{K} {mode}: {v}")
        assert v["mismatches"] == 0, (M, N, K, v)
        assert v.get("ssq_exact", True), (M, N, K, v)
        assert v.get("dead_rows_untouched", True), (M, N, K, v)


@pytest.fixture(scope="module")
def walks():
    return _result(_dev_run(_WALK_SCRIPT % (REPO, WALK_SHAPES, WALK_MODES)))


@pytest.mark.parametrize("mode", WALK_MODES)
def test_blocks_that_walk_several_tiles(walks, mode):
    """288 and 261 tiles on 256 CUs, three and two K-tiles, super-tile and row-major order: within the split-precision bar
    (2e-5 of the largest output) of the fp64 product of the decoded planes, the same bits on a second call, the row sums within
    the planes' quantum of the sums over the decoded outputs."""
    for (M, N, K) in WALK_SHAPES:
        v = walks[f"{M}x{N}x{K} {mode}"]
        print(f"[direct] {M}x{N}x{K} {mode}: err {v['err']:.3g} (bound {2e-5 * v['scale']:.3g})")
        assert v["err"] < 2e-5 * v["scale"], (M, N, K, v)
        assert v["repeat"], (M, N, K)
        assert v.get("ssq_own_excess", -1.0) <= 0.0, (M, N, K, v)


SEARCH = dict(Q=16, B=4, L=8, V=256, N=3000, seed=11)   # tests/test_gpu_gemm_mfma16.py


def test_small_search_with_a_fork_agrees_with_the_other_shape(tmp_path):
    """A fork at depth 3 (five positions in the tail pass), setting 1 against setting 0: tokens and ranges equal and scores
    within 3e-5 on the queries whose pruning margin is above 1e-3 at both settings, at least 80 % of them; the margins equal bit
    for bit, because the steps in front of the fork are untouched."""
    out = str(tmp_path / "search.npz")
    _dev_run(_SEARCH_SCRIPT % REPO, out, *[SEARCH[k] for k in ("Q", "B", "L", "V", "N", "seed")])
    d = dict(np.load(out))
    keep = (d["m0_margins"] > MARGIN_MIN) & (d["m1_margins"] > MARGIN_MIN)
    assert keep.mean() >= 0.8, (d["m0_margins"], d["m1_margins"])
    assert d["m1_forced"] > 0.5 * SEARCH["Q"], "the fork forced too few queries for the tail pass to matter"
    for k in ("tokens", "row_lo", "row_hi"):
        assert (d[f"m0_{k}"][keep] == d[f"m1_{k}"][keep]).all(), k
    err = float(np.abs(d["m0_scores"][keep].astype(np.float64) - d["m1_scores"][keep]).max())
    print(f"[direct] search fork3: max score difference {err:.3g} on {int(keep.sum())} of {keep.size} queries")
    assert err <= ROUTE_TOL, err
    assert d["m0_margins"].tobytes() == d["m1_margins"].tobytes()
