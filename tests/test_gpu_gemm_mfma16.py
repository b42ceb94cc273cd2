"""The 16x16x32 body of the 256 x 256 split-precision GEMM (ripor_amd/csrc/gemm_h2_pp_body.inc, M16): the tail
passes of a search run the ping-pong kernel on v_mfma_f32_16x16x32_f16 (`Context.set_gemm_mfma16(1)`, the default), everything
else and setting 0 on v_mfma_f32_32x32x16_f16. Same tiles, same three products per element; the 32 columns of a K-tile are
summed in another order, so the two settings agree to rounding, not bit for bit. A tail pass scores sequences that are already
chosen; the launches that decide which sequences survive the steps (encoder, steps, the layer-0 table) keep their bits at either
setting. One pruning decision does read tail-pass scores: a query forced with extras keeps the best B of B + extras sequences.

The processes below load the development build with RPR_GEMM_TILE=256 (read once, when the library loads), which pins every
split-precision launch to the ping-pong kernel whatever its shape; the setting itself belongs to the ctx, so one process
compares 0 and 1.
  * single products through the test hook rpr_op_linear_h2 (`Context.linear_h2`: rpr_op_linear's operands, plus the epilogue of
    the launch and the MFMA shape): fp32 out, x-stream planes with residual and row sums of squares, ReLU with FF-scaled
    planes, the K/V-cache scatter, a fused-norm input, a device-side live row count — each shape, each mode, both settings,
    against the fp64 product of the decoded planes;
  * one small search with a tail pass, 0 against 1, and the gated layer-0 table beside the new shape;
  * queries forced WITH EXTRAS, 0 against 1: the one pruning decision that reads tail-pass scores (tail_rank_extras).
Reference semantics: torch.nn.Linear inside T5Attention / T5DenseActDense (t5_pretrainer/modeling/t5_generative_retriever.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ROUTE_TOL = 3e-5     # scores after a change of GEMM route (tests/test_gpu_layer0_table.py)
MARGIN_MIN = 1e-3    # queries whose pruning margin is above this cannot change rank under a 3e-5 perturbation

# 257 x 256 x 32: one K-tile (no next-tile DMA), a ragged second row tile with one live row; 600 x 768 x 96: three K-tiles,
# three column tiles, clamped rows; 1100 x 1280 x 768: five column tiles, 24 K-tiles; 4353 x 4096 x 64: 18 x 16 = 288 tiles on
# 256 CUs — blocks that walk a second tile (accumulators cleared, strips reused) in super-tile order, a ragged last row panel
SHAPES = [(257, 256, 32), (600, 768, 96), (1100, 1280, 768), (4353, 4096, 64)]

MODES = ["f32", "f32_relu_resid", "x_planes", "ff_planes", "kv_scatter", "fused_norm", "live_rows"]

_PRODUCT_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, %r)
from ripor_amd import engine as E
ctx = E.Context.get(0)
dev = "cuda"
XS, FFS, WS, FIX = 1.0 / 16, 1.0 / 16, 256.0, 65536.0     # csrc/common.h: X_PLANE_SCALE, FF_PLANE_SCALE, W_PLANE_SCALE, SSQ_FIX
def planes(x, s):      # split_f16: hi = f16(s x), lo = f16(s x - hi)
    hi = (x * s).half(); lo = (x * s - hi.float()).half()
    return hi, lo
def dec(x, s):         # the value the two planes carry, in fp64
    hi, lo = planes(x, s)
    return (hi.double() + lo.double()) / s
def dec_out(pl, s): return (pl[0].double() + pl[1].double()) / s
out = {}
for (M, N, K) in %r:
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=dev); W = torch.randn(N, K, device=dev) * K ** -0.5
    R = torch.randn(M, N, device=dev)
    C = dec(A, 1.0) @ dec(W, WS).t()
    Bm, split_n = 10, 64 * -(-(N // 64) // 3)
    nq, stride = -(-M // Bm), (split_n // 64) * Bm * 64
    m_idx = torch.arange(M, device=dev)[:, None]
    live = M - 37
    for mode in %r:
        res = {}
        for mfma16 in (0, 1):
            runs = []
            for rep in range(2):
                o0 = torch.full((M, N), 12345.0, device=dev); r = {}
                if mode == "f32":
                    ctx.linear_h2(A, W, 0, mfma16, out0=o0); r = dict(val=o0)
                elif mode == "f32_relu_resid":
                    ctx.linear_h2(A, W, 0, mfma16, relu=True, resid=R, out0=o0); r = dict(val=o0)
                elif mode == "x_planes":
                    pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev); ssq = torch.zeros(M, dtype=torch.int64, device=dev)
                    ctx.linear_h2(A, W, 1, mfma16, resid=R, out_planes=pl, ssq_out=ssq); r = dict(val=pl, ssq=ssq)
                elif mode == "ff_planes":
                    pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev)
                    ctx.linear_h2(A, W, 2, mfma16, out_planes=pl); r = dict(val=pl)
                elif mode == "kv_scatter":
                    q = torch.full((M, split_n), 12345.0, device=dev)
                    k = torch.full((nq * stride,), 12345.0, device=dev); v = torch.full((nq * stride,), 12345.0, device=dev)
                    ctx.linear_h2(A, W, 3, mfma16, rm_B=Bm, split_n=split_n, out0=q, out1=k, out2=v); r = dict(val=torch.cat([q.reshape(-1), k, v]), q=q, k=k, v=v)
                elif mode == "fused_norm":
                    xd = dec(A, XS)
                    rs = torch.round((xd * xd).sum(1) * FIX).to(torch.int64)
                    ctx.linear_h2(A, W, 4, mfma16, row_ssq=rs, eps=1e-6, out0=o0); r = dict(val=o0, rs=rs)
                elif mode == "live_rows":
                    md = torch.tensor([live], dtype=torch.int32, device=dev)
                    ctx.linear_h2(A, W, 5, mfma16, m_dev=md, out0=o0); r = dict(val=o0)
                torch.cuda.synchronize()
                runs.append(r)
            r = runs[0]
            m = {"repeat": bool(torch.equal(runs[0]["val"], runs[1]["val"]) and ("ssq" not in r or torch.equal(runs[0]["ssq"], runs[1]["ssq"])))}
            if mode == "f32": got, ref = r["val"].double(), C
            elif mode == "f32_relu_resid": got, ref = r["val"].double(), torch.relu(C) + R.double()
            elif mode == "x_planes": got, ref = dec_out(r["val"], XS), C + dec(R, XS)
            elif mode == "ff_planes": got, ref = dec_out(r["val"], FFS), torch.relu(C)
            elif mode == "fused_norm":
                xd = dec(A, XS)
                got, ref = r["val"].double(), (xd @ dec(W, WS).t()) * torch.rsqrt(r["rs"].double() / (FIX * K) + 1e-6)[:, None]
            elif mode == "live_rows":
                got, ref = r["val"][:live].double(), C[:live]
                m["dead_rows_untouched"] = bool((r["val"][live:] == 12345.0).all())
            elif mode == "kv_scatter":
                parts, untouched = [r["q"].double()[:, :min(split_n, N)]], True
                for oi, buf in ((1, r["k"]), (2, r["v"])):
                    w = min(split_n, N - oi * split_n)
                    if w <= 0:
                        untouched = untouched and bool((buf == 12345.0).all())
                        continue
                    on = torch.arange(w, device=dev)[None, :]
                    idx = (m_idx // Bm) * stride + (m_idx %% Bm) * 64 + (on // 64) * (Bm * 64) + on %% 64
                    parts.append(buf[idx].double())
                    seen = torch.zeros_like(buf, dtype=torch.bool); seen[idx.reshape(-1)] = True
                    untouched = untouched and bool((buf[~seen] == 12345.0).all())
                got, ref = torch.cat(parts, 1), C
                m["unaddressed_untouched"] = untouched
            m["err"] = (got - ref).abs().max().item(); m["scale"] = max(1.0, ref.abs().max().item())
            if mode == "x_planes":
                # the kernel adds, per 64-column piece of a row, fix(sum of x^2) of the fp32 values x BEFORE they are split into planes;
                # a decoded value is within q = max(2^-20, 2^-21 |x|) of it (f16 lo plane at scale 1/16, subnormal below 0.125)
                xq = torch.maximum(torch.full_like(got, 2.0 ** -20), got.abs() * 2.0 ** -21)
                own = (got * got).sum(1)
                tol = (2 * got.abs() * xq + xq * xq).sum(1) + (N / 64) * 0.5 / FIX + 1e-5 * own   # + fp32 summation of the pieces
                m["ssq_own_excess"] = ((r["ssq"].double() / FIX - own).abs() - tol).max().item()
                res[mfma16] = (got, xq, r["ssq"])
            else:
                res[mfma16] = (r["val"],)
            out[f"{M}x{N}x{K} {mode} {mfma16}"] = m
        pair = {"same_bits": bool(torch.equal(res[0][0], res[1][0]))} if mode != "x_planes" else {}
        if mode == "x_planes":
            # the two settings: every piece's sum moves by at most sum(2 |x| d + d^2), d = |x0 - x1| + 2 q, and is then rounded to a unit
            g0, q0, s0 = res[0]; g1, q1, s1 = res[1]
            d = (g0 - g1).abs() + q0 + q1
            bound = FIX * (2 * torch.maximum(g0.abs(), g1.abs()) * d + d * d).sum(1) + N / 64
            pair = {"ssq_pair_excess": ((s0 - s1).abs().double() - bound).max().item(), "ssq_pair_max_units": int((s0 - s1).abs().max().item()),
                    "same_bits": bool(torch.equal(g0, g1))}
        out[f"{M}x{N}x{K} {mode} pair"] = pair
print("RESULT " + json.dumps(out))
"""

_EXTRAS_SCRIPT = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
from ripor_amd import engine as E
from test_gpu_tail_extras import World, CONFIGS
c = dict(CONFIGS["b4"]); budget = c.pop("budget")
w = World(E, seed=4, **c)
qa, qb, qc = w.targets([1, 1, 2])
Lt = w.L - w.T
w.split(w.private[qa][0], 2, at=0)
w.split(w.private[qb][0], 2, at=Lt - 1)
nodes = w.private[qc][:budget]
for i, n in enumerate(nodes):
    w.split(n, 1 + budget // len(nodes) + (i < budget %% len(nodes)))
trie = w.trie()
ctx = w.ctx
out = {}
ctx.set_forced_tail(False)
plain = E.search(w.model, trie, w.ti, w.tm, w.B, w.L)
ctx.set_forced_tail(1); ctx.set_fork_depths([w.T]); ctx.set_tail_extras(budget)
for mfma16 in (0, 1):
    ctx.set_gemm_mfma16(mfma16)
    res = E.search(w.model, trie, w.ti, w.tm, w.B, w.L)
    torch.cuda.synchronize()
    for k in ("tokens", "scores", "row_lo", "row_hi"):
        out[f"m{mfma16}_{k}"] = getattr(res, k).cpu().numpy()
    out[f"m{mfma16}_forced"] = np.int64(ctx.last_fork_stats()[0]["forced"])
for k in ("tokens", "scores"):
    out[f"plain_{k}"] = getattr(plain, k).cpu().numpy()
forced, ex = w.predicted_forced(budget)
out["pred_forced"] = forced; out["extras"] = ex
ctx.set_gemm_mfma16(1); ctx.set_tail_extras(-1); ctx.set_fork_depths(None); ctx.set_forced_tail(True)
np.savez(sys.argv[1], **out)
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
def run(tag, mfma16, l0, forks, profile=False):
    ctx.set_gemm_mfma16(mfma16); ctx.set_l0_table(l0); ctx.set_fork_depths(forks)
    if profile:
        ctx.profile_enable(True); ctx.profile_reset()
    res = E.search(model, trie, ti, tm, B, L, margins=not profile)
    torch.cuda.synchronize()
    for k in ("tokens", "scores", "row_lo", "row_hi"):
        out[f"{tag}_{k}"] = getattr(res, k).cpu().numpy()
    if not profile:
        out[f"{tag}_margins"] = res.margins.cpu().numpy()
    out[f"{tag}_table_bytes"] = np.int64(ctx.l0_table_bytes(model))
    out[f"{tag}_forced"] = np.int64(sum(f["forced"] for f in ctx.last_fork_stats()))
    if profile:
        p = ctx.profile_get()
        out[f"{tag}_gemm_launches"] = np.int64(p["gemm"]["launches"] + p["gemm_small"]["launches"])
        ctx.profile_enable(False)
for forks, ft in ((None, "auto"), ([3], "fork3")):
    for mfma16 in (0, 1):
        run(f"{ft}_m{mfma16}", mfma16, 1, forks)
# the gated layer-0 table on the new shape: table off against table on, and the launch it saves
run("l0off", 1, 0, [3]); run("l0on", 1, 1, [3])
run("l0off_p", 1, 0, [3], profile=True); run("l0on_p", 1, 1, [3], profile=True)
ctx.set_fork_depths(None); ctx.set_l0_table(1); ctx.set_gemm_mfma16(1)
np.savez(out_path, **out)
"""


def _dev_run(script, *argv, timeout=600):
    e = dict(os.environ, RPR_DEV_LIB="1", RPR_GEMM_TILE="256")   # development switches: live only in libripor_hip_dev.so
    p = subprocess.run([sys.executable, "-c", script, *[str(a) for a in argv]], env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return p.stdout


@pytest.fixture(scope="module")
def products():
    out = _dev_run(_PRODUCT_SCRIPT % (REPO, SHAPES, MODES))
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("mfma16", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_single_products_meet_the_split_precision_bar(products, mode, mfma16):
    """Every shape in this output mode at this setting: within the bound of
    tests/test_gpu_parity.py::test_linear_kernel_against_torch_fp32 (2e-5 of the largest output) of the fp64 product of the
    decoded planes; the same call twice gives the same bits; rows past the device-side live count and cache elements no
    output maps to keep their sentinel; the row sums of squares equal the sums over the decoded planes to the planes' quantum."""
    for (M, N, K) in SHAPES:
        v = products[f"{M}x{N}x{K} {mode} {mfma16}"]
        print(f"[mfma16] {M}x{N}x{K} {mode} setting {mfma16}: err {v['err']:.3g} (bound {2e-5 * v['scale']:.3g})")
        assert v["err"] < 2e-5 * v["scale"], (M, N, K, v)
        assert v["repeat"], (M, N, K)
        assert v.get("dead_rows_untouched", True) and v.get("unaddressed_untouched", True), (M, N, K, v)
        assert v.get("ssq_own_excess", -1.0) <= 0.0, (M, N, K, v)


def test_row_sums_of_the_two_settings_agree_to_the_fixed_point_rounding(products):
    """ssq_out at setting 0 against setting 1: one unit of 1 / SSQ_FIX per 64-column piece of a row, plus what the difference
    of the two settings' outputs itself moves the sums by (bound derived in the child from the decoded planes)."""
    for (M, N, K) in SHAPES:
        v = products[f"{M}x{N}x{K} x_planes pair"]
        print(f"[mfma16] {M}x{N}x{K} row sums: largest difference {v['ssq_pair_max_units']} units of 1/65536")
        assert v["ssq_pair_excess"] <= 0.0, (M, N, K, v)


def test_the_setting_selects_another_kernel(products):
    """The two settings sum a K-tile in different orders: at K = 768 the fp32 outputs cannot agree bit for bit — if they do,
    the 16x16x32 instantiation did not run and the other tests here compare a kernel with itself."""
    for mode in ("f32", "f32_relu_resid", "kv_scatter", "fused_norm", "live_rows"):
        assert not products[f"1100x1280x768 {mode} pair"]["same_bits"], mode


SEARCH = dict(Q=16, B=4, L=8, V=256, N=3000, seed=11)


@pytest.fixture(scope="module")
def searches(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mfma16") / "search.npz")
    _dev_run(_SEARCH_SCRIPT % REPO, out, *[SEARCH[k] for k in ("Q", "B", "L", "V", "N", "seed")])
    return dict(np.load(out))


def _oracle_margins():
    """Pruning margins of the exact-fp32 CPU oracle: per query the smallest gap, over the steps, between the last kept and
    the first dropped live candidate (tests/conftest.py: prune_margins)."""
    from oracle import beam_ref, t5_ref
    from ripor_amd.utils import synth
    s = SEARCH
    dims = synth.mini_dims(L=s["L"], V=s["V"], enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=s["seed"])
    codes = synth.make_codes(s["N"], s["L"], s["V"], seed=s["seed"])
    ids, mask = synth.make_queries(s["Q"], vocab_size=dims.vocab_size, seed=s["seed"], max_len=12)
    pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(codes)), s["V"])
    rec = {}
    seqs, sc = beam_ref.beam_search_ref(t5_ref.T5RefCached(sd, dims), pm, ids, mask, s["B"], s["L"], use_kv_cache=True, record=rec)
    B = s["B"]
    top = np.stack([st["top_scores"] for st in rec["steps"]])          # [L, Q, 2B] float64, sorted descending
    gap = np.where(top[:, :, B] > -1e8, top[:, :, B - 1] - top[:, :, B], np.inf)
    return gap.min(axis=0), seqs.numpy().reshape(s["Q"], B, s["L"] + 1)[:, :, 1:], sc.numpy().reshape(s["Q"], B)


def test_small_search_agrees_between_the_settings(searches):
    """Setting 0 against setting 1, with the automatic forks and with a fork at depth 3 (five positions in the tail pass):
    tokens and row ranges equal, scores within 3e-5, on the queries whose pruning margin (rpr_search_margins, both runs) is
    above 1e-3. The seed keeps at least 90 % of the queries by the exact-fp32 oracle's margins alone, and the kept queries
    match the oracle. The steps in front of the fork keep their arithmetic, so the margins are the same bits."""
    ref_margin, ref_tok, ref_sc = _oracle_margins()
    assert (ref_margin > MARGIN_MIN).mean() >= 0.9, ref_margin
    for ft in ("auto", "fork3"):
        a = {k: searches[f"{ft}_m0_{k}"] for k in ("tokens", "scores", "row_lo", "row_hi", "margins")}
        b = {k: searches[f"{ft}_m1_{k}"] for k in ("tokens", "scores", "row_lo", "row_hi", "margins")}
        keep = (a["margins"] > MARGIN_MIN) & (b["margins"] > MARGIN_MIN) & (ref_margin > MARGIN_MIN)
        assert keep.mean() >= 0.8, (ft, a["margins"], b["margins"])
        for k in ("tokens", "row_lo", "row_hi"):
            assert (a[k][keep] == b[k][keep]).all(), (ft, k)
        err = float(np.abs(a["scores"][keep].astype(np.float64) - b["scores"][keep]).max())
        print(f"[mfma16] search {ft}: max score difference {err:.3g} on {int(keep.sum())} of {keep.size} queries")
        assert err <= ROUTE_TOL, (ft, err)
        assert (a["margins"] == b["margins"]).all(), ft       # pruning happens in the steps: untouched by the setting
        if ft == "fork3":
            assert searches["fork3_m1_forced"] > 0.5 * SEARCH["Q"], "the fork forced too few queries for the tail pass to matter"
            assert not np.array_equal(a["scores"], b["scores"]), "the two settings gave the same bits: the 16x16x32 body did not run"
        assert (b["tokens"][keep] == ref_tok[keep]).all(), ft
        assert np.abs(b["scores"][keep] - ref_sc[keep]).max() < 1e-4, ft


def test_gated_layer0_table_gives_the_bits_of_the_projection_on_the_new_shape(searches):
    """Setting 1, every launch on the ping-pong kernel: the table against the projection it replaces, in the steps and in
    the tail pass whose other launches run the 16x16x32 body — every output bit for bit, with fewer GEMM launches in the
    profile counters (the check of tests/test_gpu_layer0_table.py beside the new shape: the table and the tail's layer-0
    projection both stay on 32x32x16)."""
    assert searches["l0off_table_bytes"] == 0 and searches["l0on_table_bytes"] > 0
    for on, off in (("l0on", "l0off"), ("l0on_p", "l0off"), ("l0off_p", "l0off"), ("l0on", "fork3_m1")):
        for k in ("tokens", "row_lo", "row_hi", "scores"):
            assert searches[f"{on}_{k}"].tobytes() == searches[f"{off}_{k}"].tobytes(), (on, off, k)
    assert searches["l0on_p_gemm_launches"] < searches["l0off_p_gemm_launches"]


def test_queries_forced_with_extras_agree_between_the_settings(tmp_path):
    """tail_rank_extras keeps the best B of a query's B + extras sequences by their tail-pass scores: the one pruning decision
    that sees the new shape's rounding. The table of tests/test_gpu_tail_extras.py (b4, seed 4: extras diverging at the first
    and at the last tail position, and a query with the whole budget), extras forced on, setting 0 against 1 and both against
    the plain loop, by that file's criterion: identical sequences and ranges at every rank outside score near-ties (2e-4),
    scores within 3e-5 of each other and within 0.3 of the parity tolerance of the plain loop."""
    out = str(tmp_path / "extras.npz")
    _dev_run(_EXTRAS_SCRIPT % (REPO, REPO), out)
    d = dict(np.load(out))
    with_extras = d["pred_forced"] & (d["extras"] > 0)
    assert int(with_extras.sum()) >= 3 and d["m0_forced"] == d["m1_forced"] == int(d["pred_forced"].sum()), (d["extras"], d["m0_forced"])
    live = d["plain_scores"] > -1e6
    for a, b, tol in (("m0", "m1", ROUTE_TOL), ("m1", "plain", 0.3e-4), ("m0", "plain", 0.3e-4)):
        same = (d[f"{a}_tokens"] == d[f"{b}_tokens"]).all(axis=2)
        diff = np.abs(d[f"{a}_scores"].astype(np.float64) - d[f"{b}_scores"])
        assert (same | (diff <= 2e-4) | ~live).all(), (a, b)
        print(f"[mfma16] extras {a} against {b}: max score difference {float((diff * live).max()):.3g}, {int(same.sum())}/{same.size} ranks identical")
        assert float((diff * live).max()) <= tol, (a, b)
        if b != "plain":
            both = same & live
            assert (d[f"{a}_row_lo"][both] == d[f"{b}_row_lo"][both]).all() and (d[f"{a}_row_hi"][both] == d[f"{b}_row_hi"][both]).all()
            assert not np.array_equal(d["m0_scores"], d["m1_scores"]), "same bits: the 16x16x32 body did not run"
