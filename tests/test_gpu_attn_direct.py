"""-m gpu: every attention kernel of the search path on its own, against the fp64 definition.

Each case of tests/attn_ref.py (CASES) goes through the site's test hook (rpr_op_enc_attn, rpr_op_dec_self_attn,
rpr_op_cross_attn, rpr_op_tail_self_attn: the site's own planner and launcher) and must
  * report the kernel the table names;
  * stay within the a-priori fp32 bound of attn_ref.attend, element by element, with no factor on top;
  * leave the NaN-payload canary in everything it must not write: rows behind the last row, rows of queries >= *nq_dev and
    of sequences >= *nseq_dev, the rows a packed encoder does not have (the output rows are H * dkv wide with no gap, so
    there are no gap columns to keep; the gap columns of the K | V input rows hold NaN and must not be read);
  * give the same bits when launched again;
  * with plane output, write exactly split_f16(out * 16) of the fp32 launch (hi = float16(x), lo = float16(x - hi), both
    round-to-nearest-even) and the plane canary elsewhere. TRAIN_SELF_MFMA takes fp32 output only: its plane launch is routed
    to ENC_VALU64, whose planes are compared with an fp32 launch of the same route;
  * raise RPR_STATUS_EMPTY_QUERY exactly when a cross-attention query attends to nothing (its rows are zeros), and no other
    status.
tests/test_attn_ref_host.py shows on the CPU that these inputs tell a wrong kernel from a right one (every mutant of the
definition lies 30x or more beyond the bound on every (query, head) it applies to).

Out of scope, so that the uncovered names are explicit (attn_ref.OUT_OF_SCOPE): TAIL_CROSS_G1_NKT1 is reachable only with a
development switch; TRAIN_BWD_MFMA / _VALU / _VALU128, TRAIN_CROSS_BWD(128), TRAIN_SELF_DROP_FWD(128), TRAIN_CROSS_DROP_FWD(128)
and the four *_TILED kernels are the training backward and the forward with dropout: tests/test_gpu_attn_train_direct.py takes
each of them through a hook of its own against the fp64 definition of tests/attn_train_ref.py (test_gpu_train.py, test_gpu_dropout.py,
test_gpu_heads128.py and test_gpu_long_queries.py check them through whole steps against autograd, test_gpu_train_bits.py holds
the steps bit for bit). The last test of the file asserts
that every other name of RPR_ATTN_KERNELS was reported by a case of this run and prints the worst |got - ref| / bound per
kernel (run with -s)."""
import numpy as np
import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

CANARY32 = 0x7FC0BEEF       # a quiet NaN with a payload
CANARY16 = 0x7EAD           # a float16 NaN
A_PLANE_SCALE = np.float32(16.0)
KINDS = ("flat", "peaked", "near-zero q")
_seen = {}                  # kernel -> [case names]
_worst = {}                 # kernel -> (ratio, case, row kind, attended keys)
_plane_mismatch = []


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = E.Context.get(0)
    c.status(clear=True)
    return c


def _dev(a):
    if a is None:
        return None
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _canary_out(rows, cols):
    return torch.full((rows, cols), CANARY32, dtype=torch.int32, device="cuda").view(torch.float32)


def _canary_planes(rows, cols):
    return torch.full((2, rows, cols), CANARY16, dtype=torch.int16, device="cuda").view(torch.float16)


class Launch:
    """The device copies of a case's inputs and one hook call per output mode."""

    def __init__(self, ctx, case, inp):
        self.ctx, self.case, self.inp = ctx, case, inp
        self.rows, self.cols = R.out_shape(inp)
        self.d = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
        if case.site in ("self", "cross"):
            self.d["nq_dev"] = torch.tensor([inp["nq"]], dtype=torch.int32, device="cuda")
        if case.site == "tail_self":
            self.d["nseq_dev"] = torch.tensor([inp["nseq"]], dtype=torch.int32, device="cuda")

    def run(self, planes=False, **over):
        inp, d, ctx = self.inp, self.d, self.ctx
        out = None if planes else _canary_out(self.rows, self.cols)
        pl = _canary_planes(self.rows, self.cols) if planes else None
        kw = dict(out=out, out_planes=pl, plane_stride=self.rows * self.cols, dkv=inp["D"])
        site = self.case.site
        if site == "enc":
            name = ctx.enc_attn(d["qkv"], d.get("mask"), d["rel_bias"], inp["Q"], inp["Lq"], inp["H"], num_buckets=R.NB, max_distance=R.MAXD,
                                causal=inp["causal"], mfma=over.get("mfma", inp["mfma"]), offs=d.get("offs"), lens=d.get("lens"), **kw)
        elif site == "self":
            name = ctx.dec_self_attn(d["q"], d["kcache"], d["vcache"], inp["strides"], d["anc"], d["rel_bias"], inp["Q"], inp["B"], inp["H"],
                                     inp["t"], num_buckets=R.NB, max_distance=R.MAXD, nq_dev=d["nq_dev"], **kw)
        elif site == "cross":
            x, inner = d["x"], inp["H"] * inp["D"]
            name = ctx.cross_attn(inp["cross_site"], d["q"], x, x[:, inner:], inp["xld"], d["mask"], inp["Q"], inp["B"], inp["H"], inp["Lq"],
                                  offs=d.get("offs"), nq_dev=d["nq_dev"], **kw)
        else:
            name = ctx.tail_self_attn(d["qkv"], d["kcache"], d["vcache"], inp["strides"], d["anc"], d["flist"], d.get("kvq"), d["nseq_dev"],
                                      d["rel_bias"], inp["ncap"], inp["B"], inp["H"], inp["T"], inp["L"], num_buckets=R.NB,
                                      max_distance=R.MAXD, **kw)
        return name, (pl if planes else out), ctx.status(clear=True)


def split_f16(x32):
    """numpy restatement of split_f16(out * A_PLANE_SCALE) (csrc/common.h) for values inside the f16 range: uint16 bits."""
    x = x32.astype(np.float32) * A_PLANE_SCALE
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def _expected_status(case, inp):
    from ripor_amd import _lib
    return _lib.STATUS_EMPTY_QUERY if case.site == "cross" and (inp["mask"].sum(axis=1) == 0).any() else 0


def _check_bound(case, kernel, inp, res, fetch):
    """|got - ref| <= bound on every (group, head) of res; fetch(rows, cols) -> the kernel's output there. Records the worst ratio."""
    D = inp["D"]
    worst = (0.0, None)
    for (g, h), (rows, o, b) in res.items():
        got = fetch(rows, slice(h * D, (h + 1) * D)).astype(np.float64)
        assert not np.isnan(got).any(), (case.name, g, h, "NaN (or the canary) in a row the kernel must write")
        err = np.abs(got - o)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / b, 0.0)
        r, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        if ratio[r, c] > worst[0]:
            worst = (float(ratio[r, c]), (g, h, int(r), int(c), float(got[r, c]), float(o[r, c]), float(b[r, c])))
    if worst[1] is not None:
        g, h, r, c = worst[1][:4]
        G = R.GATHER[case.site](inp, g, h)
        kind = KINDS[(r + g + h) % 3] if len(G.rows) >= 3 else KINDS[0]
        rec = (worst[0], case.name, kind, int(G.ok[r].sum()))
        if rec[0] > _worst.get(kernel, (-1.0,))[0]:
            _worst[kernel] = rec
    else:
        _worst.setdefault(kernel, (0.0, case.name, "-", 0))
    print(f"  worst |got - ref| / bound {worst[0]:.4f}" + (f" at (group, head, row, col, got, ref, bound) {worst[1]}" if worst[1] else ""))
    assert worst[0] <= 1.0, (case.name, kernel, worst)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(ctx, case):
    inp = R.make_inputs(case)
    L = Launch(ctx, case, inp)
    want_status = _expected_status(case, inp)
    kernel, out, status = L.run()
    print(f"\n{case.name}: kernel {kernel}")
    _seen.setdefault(kernel, []).append(case.name)
    assert kernel == case.kernel
    assert status == want_status, (status, want_status)
    # the same launch again: the same bits
    kernel2, out2, _ = L.run()
    assert kernel2 == kernel and torch.equal(out.view(torch.int32), out2.view(torch.int32)), "two launches differ"
    del out2
    pairs = R.sample_pairs(case, inp)
    res = R.reference(inp, pairs)
    assert res, "no live (group, head) pair"
    if pairs is None:
        got = out.cpu().numpy()
        _, _, written = R.assemble(inp, res)
        assert written.any()
        assert (got.view(np.int32)[~written] == CANARY32).all(), "wrote where it must not (or skipped the canary check)"
        _check_bound(case, kernel, inp, res, lambda r, c: got[r, c])
    else:   # many waves: every row of a live query is written (no NaN left), the rows behind them keep the canary; bound on the sample
        live = inp["nq"] * inp["B"]
        assert not torch.isnan(out[:live]).any() and bool((out[live:].view(torch.int32) == CANARY32).all())
        _check_bound(case, kernel, inp, res, lambda r, c: out[torch.from_numpy(r).cuda()][:, c].cpu().numpy())
    # plane output
    kp, planes, status = L.run(planes=True)
    assert status == want_status, (status, want_status)
    base = out
    if kernel == "TRAIN_SELF_MFMA":     # fp32 output only: planes come from the VALU route, compared with that route's fp32 launch
        assert kp == "ENC_VALU64"
        kb, base, _ = L.run(mfma=False)
        assert kb == "ENC_VALU64"
        _seen.setdefault(kb, []).append(case.name + " (planes)")
        _check_bound(case, kb, inp, res, lambda r, c, b=base.cpu().numpy(): b[r, c])
    else:
        assert kp == kernel
    if pairs is None:
        hi, lo = split_f16(np.where(written, base.cpu().numpy(), 0))
        pb = planes.view(torch.int16).cpu().numpy().view(np.uint16)
        ok = (np.where(written, pb[0] == hi, pb[0] == CANARY16) & np.where(written, pb[1] == lo, pb[1] == CANARY16))
    else:
        x = base[:live] * 16.0
        hi = x.half()
        lo = (x - hi.float()).half()
        ok = (torch.equal(planes[0, :live].view(torch.int16), hi.view(torch.int16)) and torch.equal(planes[1, :live].view(torch.int16), lo.view(torch.int16))
              and bool((planes[:, live:].view(torch.int16) == CANARY16).all()))
        r = res[next(iter(res))][0]       # and the numpy restatement on the first sampled group's rows
        hn, ln = split_f16(base[torch.from_numpy(r).cuda()].cpu().numpy())
        pr = planes[:, torch.from_numpy(r).cuda()].view(torch.int16).cpu().numpy().view(np.uint16)
        ok = np.array(ok and (pr[0] == hn).all() and (pr[1] == ln).all())
    if not ok.all():
        _plane_mismatch.append(case.name)
    assert ok.all(), f"planes differ from split_f16(out * 16) in {int((~ok).sum())} elements"


# ---- exact inputs: the exponential's cut, saturation ------------------------------------------------------------------------
GAPS = (80.0, 87.4, 100.0, 103.2, 103.3)     # the losing scores lie this far under the winner; exp_nonpos cuts below -103.279
EXACT_SITES = ((0, "CROSS_BLOCK64"), (1, "STEP_CROSS16_ONE"), (2, "TAIL_CROSS_V2_TPW1"))


def _exact_cross(v00=1.0):
    """One query, two rows, H 4, 8 keys of which 6 attended: q = e_0, K[j, 0] = -gap_j (exact fp32 scores), V[j, j] = 1."""
    H, D, Lq, B = 4, 64, 8, 2
    inner = H * D
    x = np.zeros((Lq, 2 * inner + 8), np.float32)
    q = np.zeros((B, inner), np.float32)
    mask = np.zeros((1, Lq), np.int32)
    mask[0, :6] = 1
    for h in range(H):
        q[:, h * D] = 1.0
        x[1:6, h * D] = -np.array(GAPS, np.float32)
        for j in range(Lq):
            x[j, inner + h * D + j] = 1.0
        x[0, inner + h * D] = v00
    return dict(site="cross", H=H, D=D, Q=1, B=B, Lq=Lq, nq=1, x=x, xld=x.shape[1], q=q, mask=mask, offs=None, out_rows=B + 3)


@pytest.mark.parametrize("site,kernel", EXACT_SITES)
def test_exp_cut_against_its_claim(ctx, site, kernel):
    """exp_nonpos (kernel_utils.h) claims the bits of expf down to its cut at -103.279 and 0 below. Weights of e^-80 .. e^-103.2
    (from 1e-35 down into the subnormals) must stay within the bound — which the 2^-120 term dominates there: the claim checked is
    that nothing larger than that comes out — and on the kernels that use exp_nonpos the weight at -103.3 must be exactly 0."""
    inp = _exact_cross()
    inp["cross_site"] = site
    case = R.Case(f"exact_cross_site{site}", "cross", kernel)
    name, out, status = Launch(ctx, case, inp).run()
    assert name == kernel and status == 0
    got = out.cpu().numpy()
    res = R.reference(inp)
    _check_bound(case, kernel, inp, res, lambda r, c: got[r, c])
    for (g, h), (rows, o, b) in res.items():
        w = got[rows, h * 64:h * 64 + 8]
        print(f"  head {h} weights {w[0]}  (fp64 {o[0, :8]})")
        assert (w[:, 6:] == 0).all() and abs(w[0, 0] - 1.0) <= 1e-6
        if site != 0:      # the block kernel calls expf: a weight of one subnormal ulp at -103.3 is its right answer
            assert (w[:, 5] == 0).all()


@pytest.mark.parametrize("site,kernel", EXACT_SITES)
def test_saturation_is_reported_with_planes_only(ctx, site, kernel):
    """A V element of 5000 on the key that takes weight 1: out = 5000, out * 16 leaves the f16 range. Plane output clamps to
    65504 and raises RPR_STATUS_SATURATED; fp32 output does neither."""
    from ripor_amd import _lib
    inp = _exact_cross(v00=5000.0)
    inp["cross_site"] = site
    L = Launch(ctx, R.Case(f"sat_cross_site{site}", "cross", kernel), inp)
    name, out, status = L.run()
    assert name == kernel and status == 0
    assert (out.cpu().numpy()[:2, 0::64] == 5000.0).all()
    name, planes, status = L.run(planes=True)
    assert name == kernel and status == _lib.STATUS_SATURATED
    p = planes.cpu().numpy()
    assert (p[0][:2, 0::64] == np.float16(65504.0)).all() and (p[1][:2, 0::64] == 0).all()


def test_refused_plan_is_an_error(ctx):
    """A shape the site's planner refuses (a tail without a position: T = L) returns an error that says so and launches
    nothing: the output keeps its canary."""
    from ripor_amd._lib import RiporHipError
    case = next(c for c in R.CASES if c.name == "tail_self_L9_T3")
    inp = R.make_inputs(case)
    L = Launch(ctx, case, inp)
    inp["T"] = inp["L"]
    with pytest.raises(RiporHipError, match="planner refuses"):
        L.run()
    inp["T"] = case.p["T"]
    name, out, _ = L.run()
    assert name == case.kernel


def test_every_kernel_was_reached(ctx):
    """Every name of RPR_ATTN_KERNELS outside attn_ref.OUT_OF_SCOPE was reported by a case above; the per-kernel record."""
    names = {ctx.lib.rpr_attn_kernel_name(i).decode() for i in range(ctx.lib.rpr_attn_kernel_count())}
    print("\nkernel | cases | worst |got - ref| / bound (case, row kind, attended keys)")
    for k in sorted(_seen):
        w = _worst.get(k, (0.0, "-", "-", 0))
        print(f"{k} | {len(_seen[k])}: {', '.join(_seen[k])} | {w[0]:.4f} ({w[1]}, {w[2]}, {w[3]} keys)")
    print("plane mismatches:", _plane_mismatch or "none")
    assert names - R.OUT_OF_SCOPE == set(_seen), (names - R.OUT_OF_SCOPE) ^ set(_seen)
