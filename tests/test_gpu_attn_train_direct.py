"""-m gpu: every attention kernel of the training step on its own, against the fp64 definition.

Each case of tests/attn_train_ref.py (CASES) goes through the site's test hook (rpr_op_train_self_attn_bwd,
rpr_op_train_self_attn_drop_fwd, rpr_op_train_cross_attn_bwd, rpr_op_train_cross_attn_drop_fwd: the site's own planner and
launcher) and must
  * report the kernel the table names and leave the ctx status at 0;
  * stay within the a-priori fp32 bound of attn_train_ref.define, element by element, with no factor on top: dQ | dK | dV and
    dbias (added to a nonzero start), or O;
  * leave the NaN-payload canary in everything it must not write: the rows behind the last row of every output (for dqkv that
    includes their K | V columns), the row behind dbias, the gap columns of dxk / dxv (xld beyond 2 inner; the same columns of
    the K | V input hold NaN and must not be read);
  * write every row the definition owns (no canary left there); the dK and dV rows of masked keys exactly 0 — their bound is 0,
    as is that of every output of a sequence without an attended key: zeros, no NaN;
  * give the same bits when launched again (dbias from the same start).
With dropout, the drop-forward and the backward of one {seed, step, site} are held to the same numpy mask (tests/dropout_mask.py
through attn_train_ref.gather): the only place where "the backward redraws the forward's mask" is checked at the kernel.
tests/test_attn_train_ref_host.py shows on the CPU that these inputs tell a wrong kernel from a right one (every mutant of the
definition lies 10x or more beyond the bound in every (group, head) it applies to). One test per hook checks a refused plan. The
last test asserts that every kernel of the table was reported by a case of this run and prints the worst |got - ref| / bound per
kernel and output (run with -s)."""
import numpy as np
import pytest
import torch

import attn_train_ref as T

pytestmark = pytest.mark.gpu

CANARY32 = 0x7FC0BEEF       # a quiet NaN with a payload
PAD_ROWS = 3
_seen = {}                  # kernel -> [case names]
_worst = {}                 # (kernel, output) -> (ratio, case)
_dev = {}                   # shape name -> device copies of its inputs


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = E.Context.get(0)
    c.status(clear=True)
    return c


def _canary(rows, cols):
    return torch.full((rows, cols), CANARY32, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_canary(a):
    return a.view(np.int32) == CANARY32


def _device(inp):
    if inp["name"] not in _dev:
        _dev[inp["name"]] = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items() if isinstance(v, np.ndarray)}
    return _dev[inp["name"]]


def _drop(inp, rate):
    if rate == 0:
        return None
    if inp["site"] == "self":
        return (rate, T.SEED, T.STEP, T.SITE_SELF, inp["Ls"])
    return (rate, T.SEED, T.STEP, T.SITE_CROSS, inp["L"])


def launch(ctx, case, inp):
    """One hook call into fresh canary buffers -> (kernel name, {buffer name: numpy array}, status)."""
    d, H, D, inner = _device(inp), inp["H"], inp["D"], inp["inner"]
    drop = _drop(inp, case.rate)
    if inp["site"] == "self":
        S, Ls, rows = inp["S"], inp["Ls"], inp["S"] * inp["Ls"]
        kw = dict(dkv=D, num_buckets=T.NB, max_distance=T.MAXD, causal=inp["causal"])
        if case.op == "bwd":
            dqkv = _canary(rows + PAD_ROWS, 3 * inner)
            dbias = _canary(T.NB + 1, H)
            dbias[:T.NB] = d["dbias0"]
            name = ctx.train_self_attn_bwd(d["qkv"], d["dO"], d.get("mask"), d["rel_bias"], dqkv, dbias, S, Ls, H, drop=drop, **kw)
            bufs = dict(dqkv=dqkv, dbias=dbias)
        else:
            out = _canary(rows + PAD_ROWS, inner)
            name = ctx.train_self_attn_drop_fwd(d["qkv"], d.get("mask"), d["rel_bias"], out, S, Ls, H, drop, **kw)
            bufs = dict(out=out)
    else:
        bz, n, Lq, xld, x = inp["bz"], inp["n"], inp["Lq"], inp["xld"], d["x"]
        if case.op == "bwd":
            dq = _canary(bz * n + PAD_ROWS, inner)
            dx = _canary(bz * Lq + PAD_ROWS, xld)
            name = ctx.train_cross_attn_bwd(d["q"], d["dO"], x, x[:, inner:], xld, d["mask"], dq, dx, dx[:, inner:], bz, n, Lq, H, dkv=D, drop=drop)
            bufs = dict(dq=dq, dx=dx)
        else:
            out = _canary(bz * n + PAD_ROWS, inner)
            name = ctx.train_cross_attn_drop_fwd(d["q"], x, x[:, inner:], xld, d["mask"], out, bz, n, Lq, H, drop, dkv=D)
            bufs = dict(out=out)
    status = ctx.status(clear=True)
    return name, {k: v.cpu().numpy() for k, v in bufs.items()}, status


def _record(kernel, output, ratio, case):
    if ratio > _worst.get((kernel, output), (-1.0, ""))[0]:
        _worst[(kernel, output)] = (ratio, case.name)


def _check(case, kernel, output, got, ref, bound, where):
    got = got.astype(np.float64)
    assert not np.isnan(got).any(), (case.name, output, where, "NaN (or the canary) in an element the kernel must write")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    _record(kernel, output, float(ratio[i]), case)
    assert ratio[i] <= 1.0, (case.name, kernel, output, where, tuple(int(k) for k in i), float(got[i]), float(ref[i]), float(bound[i]), float(ratio[i]))
    return float(ratio[i])


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_case(ctx, case):
    inp = T.make_inputs(case.p)
    ref = T.reference(case.p, case.rate)
    kernel, bufs, status = launch(ctx, case, inp)
    print(f"\n{case.name}: kernel {kernel}")
    _seen.setdefault(kernel, []).append(case.name)
    assert kernel == case.kernel
    assert status == 0, status
    # the same launch again: the same bits
    kernel2, bufs2, _ = launch(ctx, case, inp)
    assert kernel2 == kernel
    for k in bufs:
        assert np.array_equal(bufs[k].view(np.int32), bufs2[k].view(np.int32)), f"two launches differ in {k}"
    H, D, inner, nq, nk = inp["H"], inp["D"], inp["inner"], inp["nq"], inp["nk"]
    groups = inp["groups"]
    worst = {}
    if case.op == "fwd":
        out = bufs["out"]
        assert _is_canary(out[groups * nq:]).all(), "wrote behind the last row"
        assert not _is_canary(out[:groups * nq]).any(), "a row of the output was not written"
        for (g, h), r in ref["groups"].items():
            x = _check(case, kernel, "O", out[g * nq:(g + 1) * nq, h * D:(h + 1) * D], r["O"], r["b_O"], (g, h))
            worst["O"] = max(worst.get("O", 0.0), x)
    else:
        if inp["site"] == "self":
            dqkv, dbias = bufs["dqkv"], bufs["dbias"]
            assert _is_canary(dqkv[groups * nq:]).all(), "wrote behind the last row of dqkv"
            assert not _is_canary(dqkv[:groups * nq]).any(), "an element of dqkv was not written"
            assert _is_canary(dbias[T.NB:]).all(), "wrote behind dbias"
            parts = lambda g, h: (dqkv[g * nq:(g + 1) * nq, h * D:(h + 1) * D], dqkv[g * nq:(g + 1) * nq, inner + h * D:inner + (h + 1) * D],
                                  dqkv[g * nq:(g + 1) * nq, 2 * inner + h * D:2 * inner + (h + 1) * D])
            worst["dbias"] = _check(case, kernel, "dbias", dbias[:T.NB], ref["dbias"], ref["b_dbias"], "dbias")
        else:
            dq, dx = bufs["dq"], bufs["dx"]
            assert _is_canary(dq[groups * nq:]).all(), "wrote behind the last row of dq"
            assert not _is_canary(dq[:groups * nq]).any(), "a row of dq was not written"
            assert _is_canary(dx[groups * nk:]).all(), "wrote behind the last row of dxk / dxv"
            assert _is_canary(dx[:, 2 * inner:]).all(), "wrote into the gap columns of dxk / dxv"
            assert not _is_canary(dx[:groups * nk, :2 * inner]).any(), "an element of dxk / dxv was not written"
            parts = lambda g, h: (dq[g * nq:(g + 1) * nq, h * D:(h + 1) * D], dx[g * nk:(g + 1) * nk, h * D:(h + 1) * D],
                                  dx[g * nk:(g + 1) * nk, inner + h * D:inner + (h + 1) * D])
        for (g, h), r in ref["groups"].items():
            for name, got in zip(("dQ", "dK", "dV"), parts(g, h)):
                worst[name] = max(worst.get(name, 0.0), _check(case, kernel, name, got, r[name], r["b_" + name], (g, h)))
            masked = ~r["ok"].any(axis=0)
            _, dK, dV = parts(g, h)
            assert (dK[masked] == 0).all() and (dV[masked] == 0).all(), ((g, h), "dK / dV of a masked key is not exactly 0")
    print("  worst |got - ref| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ---- refused plans: an error that says so, nothing launched ------------------------------------------------------------------
def _refused(call, bufs):
    from ripor_amd._lib import RiporHipError
    with pytest.raises(RiporHipError, match="planner refuses"):
        call()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b.view(torch.int32) == CANARY32).all()), "a refused launch wrote"


def test_self_bwd_refuses_128_dim_heads_beyond_the_carve(ctx):
    from ripor_amd._lib import RiporHipError
    S, Ls, H, D = 1, 92, 1, 128
    qkv, dO = torch.zeros(S * Ls, 3 * H * D, device="cuda"), torch.zeros(S * Ls, H * D, device="cuda")
    mask = torch.ones(S, Ls, dtype=torch.int32, device="cuda")
    rb = torch.zeros(T.NB, H, device="cuda")
    dqkv, dbias = _canary(S * Ls, 3 * H * D), _canary(T.NB, H)
    _refused(lambda: ctx.train_self_attn_bwd(qkv, dO, mask, rb, dqkv, dbias, S, Ls, H, dkv=D), (dqkv, dbias))
    with pytest.raises(RiporHipError, match="causal"):      # a causal launch takes no mask (and at most 64 positions)
        ctx.train_self_attn_bwd(qkv, dO, mask, rb, dqkv, dbias, S, 8, H, dkv=D, causal=True)
    assert ctx.train_self_attn_bwd(qkv, dO, mask, rb, dqkv, dbias, S, 91, H, dkv=D) == "TRAIN_BWD_VALU128"


def test_self_drop_fwd_refuses_rows_that_are_no_whole_sequences(ctx):
    from ripor_amd._lib import RiporHipError
    S, Ls, H, D = 1, 92, 1, 64
    qkv = torch.zeros(S * Ls, 3 * H * D, device="cuda")
    mask = torch.ones(S, Ls, dtype=torch.int32, device="cuda")
    rb = torch.zeros(T.NB, H, device="cuda")
    out = _canary(S * Ls, H * D)
    _refused(lambda: ctx.train_self_attn_drop_fwd(qkv, mask, rb, out, S, Ls, H, (0.1, 1, 2, T.SITE_SELF, 7)), (out,))
    with pytest.raises(RiporHipError, match="rate > 0"):
        ctx.train_self_attn_drop_fwd(qkv, mask, rb, out, S, Ls, H, (0.0, 1, 2, T.SITE_SELF, Ls))
    assert bool((out.view(torch.int32) == CANARY32).all())
    assert ctx.train_self_attn_drop_fwd(qkv, mask, rb, out, S, Ls, H, (0.1, 1, 2, T.SITE_SELF, 46)) == "TRAIN_SELF_DROP_FWD_TILED"


def _cross_zeros(bz, n, Lq, H, D):
    inner = H * D
    x = torch.zeros(bz * Lq, 2 * inner + 8, device="cuda")
    return (torch.zeros(bz * n, inner, device="cuda"), torch.zeros(bz * n, inner, device="cuda"), x,
            torch.ones(bz, Lq, dtype=torch.int32, device="cuda"))


def test_cross_bwd_refuses_128_dim_heads_beyond_the_carve(ctx):
    bz, n, Lq, H, D = 1, 16, 256, 1, 128
    inner = H * D
    q, dO, x, mask = _cross_zeros(bz, n, Lq, H, D)
    dq, dx = _canary(bz * n, inner), _canary(bz * Lq, 2 * inner + 8)
    _refused(lambda: ctx.train_cross_attn_bwd(q, dO, x, x[:, inner:], 2 * inner + 8, mask, dq, dx, dx[:, inner:], bz, n, Lq, H, dkv=D), (dq, dx))
    _refused(lambda: ctx.train_cross_attn_bwd(q, dO, x, x[:, inner:], 2 * inner + 8, mask, dq, dx, dx[:, inner:], bz, 8, Lq, H, dkv=D,
                                              drop=(0.1, 1, 2, T.SITE_CROSS, 3)), (dq, dx))
    assert ctx.train_cross_attn_bwd(q, dO, x, x[:, inner:], 2 * inner + 8, mask, dq, dx, dx[:, inner:], bz, 8, Lq, H, dkv=D) == "TRAIN_CROSS_BWD128"


def test_cross_drop_fwd_refuses_rows_that_are_no_whole_sequences(ctx):
    from ripor_amd._lib import RiporHipError
    bz, n, Lq, H, D = 1, 8, 5, 1, 64
    inner = H * D
    q, _, x, mask = _cross_zeros(bz, n, Lq, H, D)
    out = _canary(bz * n, inner)
    _refused(lambda: ctx.train_cross_attn_drop_fwd(q, x, x[:, inner:], 2 * inner + 8, mask, out, bz, n, Lq, H, (0.1, 1, 2, T.SITE_CROSS, 3)), (out,))
    with pytest.raises(RiporHipError, match="rate > 0"):
        ctx.train_cross_attn_drop_fwd(q, x, x[:, inner:], 2 * inner + 8, mask, out, bz, n, Lq, H, (0.0, 1, 2, T.SITE_CROSS, 4))
    assert bool((out.view(torch.int32) == CANARY32).all())
    assert ctx.train_cross_attn_drop_fwd(q, x, x[:, inner:], 2 * inner + 8, mask, out, bz, n, Lq, H, (0.1, 1, 2, T.SITE_CROSS, 4)) == "TRAIN_CROSS_DROP_FWD"


def test_every_kernel_was_reached(ctx):
    """Every kernel of the table (attn_ref.OUT_OF_SCOPE without NONE and the development-switch kernel) was reported by a case
    above; the per-kernel record."""
    print("\nkernel | cases | worst |got - ref| / bound per output (case)")
    for k in sorted(_seen):
        w = ", ".join(f"{o} {v[0]:.4f} ({v[1]})" for (kk, o), v in sorted(_worst.items()) if kk == k)
        print(f"{k} | {len(_seen[k])} | {w}")
    assert T.R.OUT_OF_SCOPE - {"NONE", "TAIL_CROSS_G1_NKT1"} == T.KERNELS == set(_seen), T.KERNELS ^ set(_seen)
