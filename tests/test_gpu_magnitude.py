"""-m gpu: the split-precision search path across activation magnitudes, against the operation in fp64 and against the CPU
oracle at the same magnitude.

The path carries the un-normalised residual stream in two f16 planes at a FIXED scale (csrc/common.h X_PLANE_SCALE = 2^-4: an
absolute step of 2^-20 below |x| = 2) and each row's sum of squares as a fixed-point count of 2^-16 units (SSQ_FIX), one
rounded partial per 16- to 256-column piece of a row. Both are absolute resolutions, so the path has a floor as well as the
ceiling tests/test_gpu_edges.py walks up to: a row whose RMS is far below 1 loses relative precision in its planes and in its
norm scale, while the normalised output it feeds is O(1) whatever the stream's size. Every other GEMM test draws O(1) inputs
and allows an absolute error, which a small row passes whatever the kernel does.

What this file establishes, for every magnitude s of the grid 2^4 .. 2^-10 and every kernel family that writes row sums
(tests/magnitude_probe.py; the routes are pinned on the host by tests/test_magnitude_routes.py):
  * either the result is within the project's bar — 2e-5 max(1, max |y|) for a product, 1e-4 for a beam score — or the call
    raised the sticky RPR_STATUS_SMALL_STREAM, which the boundaries act on like on saturation (repeat in exact fp32);
    silence outside the bar is the bug. (A pass tests its row totals with one kernel, csrc/passes.hip Pass::check_ssq; the hook
    behind the product tests runs that kernel on the row sums it is given, the model tests go through the passes themselves);
  * at and above the floor (FLOOR for the products, whose rows have RMS sqrt(2) s; MODEL_FLOOR for a model's stream_scale)
    the error is at most HALF the bar — the factor 2 is for inputs other than these seeds' — and no flag is raised; the
    unit-RMS goldens and the bench model are a factor 8 clear of it;
  * rows of different magnitudes in one launch meet the bar they meet alone (nothing in a tile is shared across rows);
  * the fp32 RMSNorm kernel has no floor: rtol 1e-5 against fp64 down to rows with mean(x^2) << eps.
The measured table (family x s -> error / bar, flag) is printed by test_floor_of_the_products; a GPU run's copy is
profiles/r23_magnitude_summary.txt. Reference semantics: T5LayerNorm + torch.nn.Linear of the T5 blocks
(t5_pretrainer/modeling/t5_generative_retriever.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magnitude_probe as mp  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRID = mp.GRID
FLOOR = 2.0 ** -3           # products: at and above it every family is within half the bar, unflagged (row RMS sqrt(2) s = 0.18)
MODEL_FLOOR = 2.0 ** -2     # models: stream_scale (= RMS of the embeddings) at and above which embed and search are within their bars, unflagged
SMALL, SAT = mp.STATUS_SMALL_STREAM, mp.STATUS_SATURATED
MARGIN_MIN = 1e-3           # tests/test_gpu_gemm_mfma16.py: a query whose oracle pruning margin is under it may change a sequence
STEP_LOGIT_TOL = 5e-4       # tests/test_gpu_heads128.py: embedding logits against the oracle
SCALES = [1.0, 2.0 ** -2, 2.0 ** -3, 2.0 ** -5, 2.0 ** -7]


def _pw(s):
    return f"2^{int(np.log2(s))}"


# ---------------------------------------------------------------------------------------------- products

@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    c = E.Context.get(0)
    c.set_precision("f16x2")
    c.status(clear=True)
    yield c
    c.set_precision("f16x2"); c.set_forced_tail(True); c.set_fork_depths(None)
    c.status(clear=True)


@pytest.fixture(scope="module")
def routed(ctx):
    """The default-route cases in this process (the product library)."""
    assert ctx.lib.rpr_abi_version() >= 4
    return {name: mp.sweep(ctx, *shape) for name, (shape, _) in mp.ROUTED.items()}


_TILED = {}


def _tiled(tile):
    """The pinned-tile cases: one fresh process per tile on the development library (RPR_GEMM_TILE is read once, when it loads)."""
    if tile not in _TILED:
        e = dict(os.environ, RPR_DEV_LIB="1", RPR_GEMM_TILE=str(tile))
        p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "magnitude_probe.py"), str(tile)], env=e, capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        _TILED[tile] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return _TILED[tile]


def _check_family(name, res):
    for s in GRID:
        v = res[repr(s)]
        print(f"[magnitude] {name} s={_pw(s)} (row RMS {v['rms']:.3g}): y err/bar {v['err']:.3f}  planes/bound {v['plane']:.3f}  "
              f"row sums/bound {v['ssq']:.3f}  flags {v['flags']}")
    for s in GRID:
        v = res[repr(s)]
        assert not v["flags"] & SAT, (name, s)
        assert not v["flags_producer"] & SMALL, (name, s, "the producer reads no row total")
        # the planes carry x to their steps and the products' 22 bits (magnitude_probe.chain), and the row sums are the sums of x^2 to their pieces' rounding, at every magnitude
        assert v["plane"] <= 1.0, (name, s, v)
        assert v["ssq"] <= 1.0, (name, s, v)
        if s >= FLOOR:
            assert v["err"] <= 0.5 and not v["flags"] & SMALL, (name, s, v)
        else:
            assert v["err"] <= 1.0 or v["flags"] & SMALL, (name, s, v, "outside the bar and no flag")
    m = res["mixed"]
    print(f"[magnitude] {name} mixed rows: y err/bar per s " + " ".join(f"{_pw(s)}:{e:.3f}" for s, e in zip(GRID, m["row_err"])) +
          f"  flags {m['flags']}")
    assert not m["flags"] & SAT and m["plane"] <= 1.0 and m["ssq"] <= 1.0, (name, m)
    assert m["flags"] & SMALL, (name, "rows under the floor went unreported in a launch that also holds large rows")
    for s, e in zip(GRID, m["row_err"]):
        if s >= FLOOR:
            assert e <= 0.5, (name, s, e, "a row in mixed company misses the bar it meets alone")


@pytest.mark.parametrize("name", list(mp.ROUTED))
def test_products_by_default_route(routed, name):
    """x = resid + A W^T into planes and row sums, then y = norm(x) W2^T from them, against fp64 of the fp32 inputs."""
    _check_family(name, routed[name])


@pytest.mark.parametrize("tile", list(mp.TILED))
def test_products_by_pinned_tile(tile):
    """The 128 x 64 and 128 x 128 LDS-DMA tiles and the 256 x 256 ping-pong kernel on both MFMA bodies, 300 and 257 rows."""
    res = _tiled(tile)
    assert sorted(res) == sorted(mp.tiled_names(tile))
    for name in mp.tiled_names(tile):
        _check_family(name, res[name])


def test_floor_of_the_products(routed):
    """The table of the run, and the floor it shows: the smallest s at and above which every family is within half its bar."""
    fams = dict(routed)
    for tile in mp.TILED:
        fams.update(_tiled(tile))
    w = max(len(n) for n in fams)
    print("\n[magnitude] y error / bar (bar = 2e-5 max(1, max |y|)); * = RPR_STATUS_SMALL_STREAM raised")
    print("[magnitude] " + "family".ljust(w) + " " + " ".join(_pw(s).rjust(8) for s in GRID))
    for n, r in fams.items():
        print("[magnitude] " + n.ljust(w) + " " + " ".join((f"{r[repr(s)]['err']:.3f}" + ("*" if r[repr(s)]["flags"] & SMALL else "")).rjust(8) for s in GRID))
    worst = [max(r[repr(s)]["err"] for r in fams.values()) for s in GRID]
    floor = GRID[0] * 2
    for s, e in zip(GRID, worst):      # descending
        if e > 0.5:
            break
        floor = s
    print(f"[magnitude] floor found: s = {_pw(floor)} (row RMS {2 ** 0.5 * floor:.3g}); documented {_pw(FLOOR)}")
    assert floor <= FLOOR <= 2.0 ** -2, (floor, worst)       # (2^-2: the unit-RMS goldens and the bench model stay a factor 4 clear)


# ---------------------------------------------------------------------------------------------- the fp32 RMSNorm kernel

@pytest.mark.parametrize("rows,d", [(1, 768), (77, 1024), (33, 256)])
def test_rmsnorm_kernel_has_no_floor(ctx, rows, d):
    """rpr_op_rmsnorm (exact-fp32 mode's norm) against fp64 for every s of the grid, for 2^-16 and 2^-20 (mean(x^2) = 2e-10 and
    1e-12 against eps = 1e-6) and with the rows cycling through all of them: fp32 products of finite values, rtol 1e-5."""
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x0, w = torch.randn(rows, d, generator=g), 1.0 + 0.2 * (2 * torch.rand(d, generator=g) - 1)
    mags = GRID + [2.0 ** -16, 2.0 ** -20]
    cases = [(_pw(s), x0 * s) for s in mags] + [("mixed", x0 * torch.tensor([mags[r % len(mags)] for r in range(rows)])[:, None])]
    for tag, x in cases:
        got = ctx.rmsnorm(x.cuda(), w.cuda(), mp.EPS).cpu().double()
        xd = x.double()
        want = w.double() * (xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + mp.EPS))
        rel = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
        print(f"[magnitude] rmsnorm {rows}x{d} s={tag}: max relative error {rel:.2e}")
        assert rel <= 1e-5, (tag, rel)
    assert ctx.status(clear=True) == 0


# ---------------------------------------------------------------------------------------------- models

L, V, N_DOCS, B, Q = 8, 256, 1000, 4, 5


@pytest.fixture(scope="module")
def world(ctx):
    """The oracle at every stream_scale (computed once), and the pieces the device runs share."""
    from oracle import beam_ref, t5_ref
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=L, V=V, enc_layers=2, d_ff=128, vocab_size=512)
    codes = synth.make_codes(N_DOCS, L, V, seed=91)
    ids, mask = synth.make_queries(Q, vocab_size=512, seed=92, max_len=12)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(codes)), V)
    w = dict(E=E, ti=ti, tm=tm, trie=E.DeviceTrie.from_codes(ctx, codes, V), scales={})
    for s in SCALES:
        sd = synth.make_state_dict(dims, seed=91, stream_scale=s)
        ref = t5_ref.T5RefCached(sd, dims)
        rec = {}
        seqs, sc = beam_ref.beam_search_ref(ref, pm, ids, mask, B, L, use_kv_cache=True, record=rec)
        top = np.stack([st["top_scores"] for st in rec["steps"]])          # [L, Q, 2B] float64, sorted descending
        margin = np.where(top[:, :, B] > -1e8, top[:, :, B - 1] - top[:, :, B], np.inf).min(axis=0)
        with torch.no_grad():
            logits = ref.last_logits(torch.full((Q, 1), -1, dtype=torch.long), ref.encode(ti.long(), tm.long()), tm.long()).numpy()
        w["scales"][s] = dict(sd=sd, dims=dims, margin=margin, tok=seqs.numpy().reshape(Q, B, L + 1)[:, :, 1:],
                              sc=sc.numpy().reshape(Q, B).astype(np.float64), logits=logits, e0=ref.out_embed(0).double().numpy(),
                              rms=float(np.sqrt((sd["shared.weight"].astype(np.float64) ** 2).mean())))
    return w


def _grade(o, tok, sc):
    """(sets of sequences equal on the queries the oracle decides clearly, max |score - oracle| over the sequences in both)."""
    keep = o["margin"] > MARGIN_MIN
    same, err = True, 0.0
    for q in range(Q):
        got = {tuple(t): s for t, s in zip(tok[q].tolist(), sc[q])}
        want = {tuple(t): s for t, s in zip(o["tok"][q].tolist(), o["sc"][q])}
        if keep[q]:
            same = same and got.keys() == want.keys()
        err = max([err] + [abs(got[k] - want[k]) for k in want if k in got])
    return same, err


def test_premise_the_oracle_decides_these_queries_clearly(world):
    for s, o in world["scales"].items():
        assert (o["margin"] < MARGIN_MIN).sum() <= 1, (s, o["margin"])
        assert abs(o["rms"] / s - 1.0) < 5e-3, (s, o["rms"])               # the stream really is that small


@pytest.mark.parametrize("s", SCALES, ids=[_pw(s) for s in SCALES])
def test_model_at_stream_scale(ctx, world, s):
    """E.embed and E.search (forced tail off, and on with a fork at depth 2: the tail passes have their own epilogues) in f16x2
    and f32 against the oracle at the same stream_scale; the status is cleared and read around every call."""
    E, o = world["E"], world["scales"][s]
    model = E.DeviceModel(ctx, o["sd"], o["dims"])
    assert not model.f32_only
    seen = {}
    try:
        for prec in ("f16x2", "f32"):
            ctx.set_precision(prec)
            ctx.status(clear=True)
            emb = E.embed(model, world["ti"], world["tm"]).cpu().double().numpy()
            flags = ctx.status(clear=True)
            err = float(np.abs(emb @ o["e0"].T - o["logits"]).max())
            print(f"[magnitude] model {_pw(s)} {prec} embed: max |logit - oracle| {err:.2e}  flags {flags}")
            seen[(prec, "embed")] = (err <= STEP_LOGIT_TOL, flags)
            for tail, forks in ((False, None), (True, [2])):
                ctx.set_forced_tail(tail); ctx.set_fork_depths(forks)
                ctx.status(clear=True)
                res = E.search(model, world["trie"], world["ti"], world["tm"], B, L)
                torch.cuda.synchronize()
                flags = ctx.status(clear=True)
                tok, sc = res.tokens.cpu().numpy(), res.scores.cpu().numpy().astype(np.float64)
                same, err = _grade(o, tok, sc)
                print(f"[magnitude] model {_pw(s)} {prec} search tail={'fork@2' if tail else 'off'}: sequences {'equal' if same else 'DIFFER'}  "
                      f"max |score - oracle| {err:.2e}  flags {flags}")
                seen[(prec, tail)] = (same and err <= 1e-4, flags, sc)
        for tail in (False, True):
            d = float(np.abs(seen[("f16x2", tail)][2] - seen[("f32", tail)][2]).max())
            print(f"[magnitude] model {_pw(s)} tail={tail}: max |score(f16x2) - score(f32)| {d:.2e}")
            seen[("pair", tail)] = d
    finally:
        ctx.set_precision("f16x2"); ctx.set_forced_tail(True); ctx.set_fork_depths(None)
    for key in (("f32", "embed"), ("f32", False), ("f32", True)):                  # the exact mode has no floor
        assert seen[key][0] and not seen[key][1], (key, seen[key][:2])
    for key in (("f16x2", "embed"), ("f16x2", False), ("f16x2", True)):
        ok, flags = seen[key][:2]
        assert not flags & SAT, key
        if s >= MODEL_FLOOR:
            assert ok and not flags & SMALL, (key, ok, flags)
        else:
            assert ok or flags & SMALL, (key, "outside the bar and no flag")
        if key[1] != "embed":
            assert seen[("pair", key[1])] <= 5e-5 or flags & SMALL, (key, seen[("pair", key[1])])


@pytest.mark.parametrize("s", [x for x in SCALES if x < MODEL_FLOOR], ids=[_pw(x) for x in SCALES if x < MODEL_FLOOR])
def test_boundary_repeats_a_small_stream_in_fp32(ctx, world, s):
    """Below the floor the Python boundary returns oracle-grade results: search_guarded sees the flag and repeats the batch in fp32."""
    E, o = world["E"], world["scales"][s]
    model = E.DeviceModel(ctx, o["sd"], o["dims"])
    with pytest.warns(UserWarning, match="fp32"):
        g = E.search_guarded(model, world["trie"], world["ti"], world["tm"], B, L)
        res = g.result()
    torch.cuda.synchronize()
    assert g.repeated and ctx.get_precision() == "f16x2"
    same, err = _grade(o, res.tokens.cpu().numpy(), res.scores.cpu().numpy().astype(np.float64))
    print(f"[magnitude] model {_pw(s)} through search_guarded: max |score - oracle| {err:.2e}")
    assert same and err <= 1e-4
    assert ctx.status(clear=True) == 0


def test_all_zero_rows_raise_no_flag(ctx):
    """A row of zeros has the total 0 and the output 0: nothing to report (rows past a device-side live count, whose slots are
    zeroed at the start of a pass, read as such rows or are not read at all: the fork runs of test_model_at_stream_scale and
    the flag-free suite cover them). The same launch with a few small rows does report."""
    dev = ctx.device
    M, K, Nn = 80, 768, 768
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(Nn, K, generator=g) * K ** -0.5).to(dev)
    A = torch.randn(M, K, generator=g)
    A[3] = 0.0; A[40:] = 0.0
    ssq = torch.round((A.double() ** 2).sum(1) * mp.SSQ_FIX).to(torch.int64).to(dev)
    out = torch.full((M, Nn), 12345.0, device=dev)
    ctx.status(clear=True)
    ctx.linear_h2(A.to(dev), W, 4, 0, row_ssq=ssq, eps=mp.EPS, out0=out)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    assert float(out[3].abs().max()) == 0.0 and float(out[40:].abs().max()) == 0.0
    A2 = A.clone(); A2[50:] = torch.randn(M - 50, K, generator=g) * 2.0 ** -7
    ssq2 = torch.round((A2.double() ** 2).sum(1) * mp.SSQ_FIX).to(torch.int64).to(dev)
    ctx.linear_h2(A2.to(dev), W, 4, 0, row_ssq=ssq2, eps=mp.EPS, out0=out)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == SMALL
