"""-m gpu: every row-wise kernel of the training step on its own, against the fp64 definition.

Each case of tests/train_rows_ref.py (cases()) goes through rpr_op_train_rows — the launch_* function the step itself calls — and
must
  * stay within the a-priori fp32 bound of the definition, element by element, with no factor on top, or match it bit for bit
    where the output is no approximation (bf16 roundings, transposes, indices, the ReLU gate, maxima, copied rows, zero padding);
  * leave the canary in front of and behind every output buffer, and in every element of a buffer the launcher does not own
    (the columns behind Rpad of a transposed operand, the gap between two planes, the second slot of a one-tensor absmax2);
  * write every element it owns (no canary left there);
  * give the same bits when the whole case is launched again from fresh buffers.
rmsnorm_bf16_T is the bf16 rounding of an fp32 value with a bound of its own: an element may be either neighbour where the bound
straddles a rounding boundary; elements that differ from bf16(reference) are counted and capped at 1 % of the case.
tests/test_train_rows_ref_host.py shows on the CPU that these inputs tell a wrong kernel from a right one. The last test asserts
that every launcher of the table was reached and prints the worst |got - ref| / bound per launcher and output and the scatter's
measured error per source magnitude (run with -s)."""
import numpy as np
import pytest
import torch

import train_rows_ref as T

pytestmark = pytest.mark.gpu

PAD = 64                    # canary elements in front of and behind every output
_seen = {}                  # launcher -> [case names]
_worst = {}                 # (launcher, output) -> (ratio, case)
_scatter = {}               # magnitude exponent -> [(max |err| / max |ref|, median |err| / |ref|, case)]
_flips = {}                 # case -> (differing elements, elements)

_CANARY = {4: T.CANARY32, 2: T.CANARY16, 8: T.CANARY64}
_UINT = {4: np.uint32, 2: np.uint16, 8: np.uint64}
_TORCH_INT = {4: torch.int32, 2: torch.int16, 8: torch.int64}


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = E.Context.get(0)
    c.status(clear=True)
    return c


def _padded(n, size, init=None):
    """A device buffer of n elements of `size` bytes between two canary regions -> (whole, view of the n elements)."""
    raw = np.full(n + 2 * PAD, _CANARY[size], _UINT[size])
    if init is not None:
        raw[PAD:PAD + n] = np.ascontiguousarray(init).reshape(-1).view(_UINT[size])
    whole = torch.from_numpy(raw.view({4: np.int32, 2: np.int16, 8: np.int64}[size])).cuda()
    return whole, whole[PAD:PAD + n]


def run_case(ctx, case):
    """All launches of a case into fresh buffers -> {output name: raw unsigned bits, canary regions included}."""
    dst_names = {n for L in case.launches for n in L.dst if n}
    dev, whole = {}, {}
    for name, arr in case.bufs.items():
        if name in dst_names:
            whole[name], dev[name] = _padded(arr.size, arr.dtype.itemsize, arr)
        else:
            dev[name] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(_UINT[arr.dtype.itemsize]).view(
                {4: np.int32, 2: np.int16, 8: np.int64}[arr.dtype.itemsize])).cuda()
    for name, (shape, dtype) in case.outs.items():
        whole[name], dev[name] = _padded(int(np.prod(shape)), np.dtype(dtype).itemsize)
    for L in case.launches:
        ctx.train_rows(L.op, [dev[n] if n else None for n in L.src], [dev[n] if n else None for n in L.dst], L.dims, L.f)
    torch.cuda.synchronize()
    return {name: w.cpu().numpy().view(_UINT[w.element_size()]) for name, w in whole.items()}


def _record(kernel, output, ratio, case):
    if ratio > _worst.get((kernel, output), (-1.0, ""))[0]:
        _worst[(kernel, output)] = (ratio, case.name)


def check_output(case, name, raw):
    ex = case.expect[name]
    size = raw.dtype.itemsize
    can = _CANARY[size]
    assert (raw[:PAD] == can).all(), (case.name, name, "wrote in front of the buffer")
    assert (raw[-PAD:] == can).all(), (case.name, name, "wrote behind the buffer")
    got = raw[PAD:-PAD]
    ref = np.asarray(ex.ref)
    if ex.bound is None:                                    # bit equality (the canary where the launcher owns nothing)
        want = np.ascontiguousarray(ref).reshape(-1).view(_UINT[size])
        same = got == want
        if ex.flips is not None:
            lo, hi = ex.flips[0].reshape(-1), ex.flips[1].reshape(-1)
            key = T.bf16_order(got)
            bad = ~same & ~((key >= lo) & (key <= hi))
            n_diff = int((~same).sum())
            _flips[case.name + "/" + name] = (n_diff, got.size)
            assert not bad.any(), (case.name, name, "beyond both bf16 neighbours the bound admits", int(np.argmax(bad)))
            assert n_diff <= 0.01 * got.size, (case.name, name, n_diff, got.size)
        else:
            i = int(np.argmax(~same))
            assert same.all(), (case.name, name, "bits differ", i, hex(int(got[i])), hex(int(want[i])), int((~same).sum()))
        _record(case.kernel, name, 0.0, case)
        return 0.0
    written = np.ones(got.size, bool) if ex.written is None else ex.written.reshape(-1)
    assert (got[~written] == can).all(), (case.name, name, "wrote an element it does not own")
    assert not (got[written] == can).any(), (case.name, name, "an element it owns was not written")
    typed = got.view({4: np.float32, 2: np.float16, 8: np.uint64}[size])
    vals = ex.decode(typed) if ex.decode is not None else typed.astype(np.float64)
    vals, refv, bound = vals.reshape(-1)[written], ref.reshape(-1)[written].astype(np.float64), np.asarray(ex.bound).reshape(-1)[written]
    assert not np.isnan(vals).any(), (case.name, name, "NaN")
    err = np.abs(vals - refv)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    i = int(np.argmax(ratio))
    _record(case.kernel, name, float(ratio[i]), case)
    print(f"  {name}: worst |got - ref| / bound {ratio[i]:.4f}")
    assert ratio[i] <= 1.0, (case.name, name, i, float(vals[i]), float(refv[i]), float(bound[i]), float(ratio[i]))
    return float(ratio[i])


@pytest.mark.parametrize("case", T.cases(), ids=[c.name for c in T.cases()])
def test_case(ctx, case):
    print(f"\n{case.name}: {case.kernel}")
    first = run_case(ctx, case)
    again = run_case(ctx, case)
    assert ctx.status(clear=True) == 0
    for name in first:
        assert np.array_equal(first[name], again[name]), f"two launches differ in {name}"
    _seen.setdefault(case.kernel, []).append(case.name)
    for name in case.expect:
        check_output(case, name, first[name])
    if case.kernel.startswith("launch_scatter"):
        got = first["table"][PAD:-PAD].view(np.float32).astype(np.float64)
        ref = case.expect["table"].ref.reshape(-1)
        nz = ref != 0
        err = np.abs(got - ref)
        rel = (float(err.max() / np.abs(ref).max()), float(np.median(err[nz] / np.abs(ref[nz]))))
        print(f"  scatter at 2^-{case.p['mag_exp']}: max |err| / max |ref| {rel[0]:.3e}, median |err| / |ref| {rel[1]:.3e}")
        _scatter.setdefault(case.p["mag_exp"], []).append(rel + (case.name,))


def test_refused_shapes_launch_nothing(ctx):
    from ripor_amd._lib import RiporHipError
    x = torch.zeros(4, 36, device="cuda")
    whole, out = _padded(4 * 36, 4)
    w = torch.ones(36, device="cuda")
    for op, src, dst, dims, f in (("RMSNORM_BWD", [x, w, x, None], [out, out, None], (4, 34, 0), (1e-6, 1.0)),     # d % 4
                                  ("RMSNORM_BWD", [x, None, x, None], [out, out, None], (4, 36, 0), (1e-6, 1.0)),  # no weight
                                  ("RMSNORM_BF16_T", [x, w], [out, out], (4, 2048, 32, 32), (1e-6, 1.0)),          # d > 1024
                                  ("S2S_HEAD_FWD", [x, x, x], [out, out, None, out], (1, 1, 32, 96), ()),          # V % 64
                                  ("TO_BF16_T", [x, None], [out, None], (4, 36, 36, 5, 0), ()),                    # odd Rpad
                                  ("COLSUM_MULTI", [x], [out], (36, 5, 1), ())):                                   # five sites
        with pytest.raises(RiporHipError, match="invalid argument"):
            ctx.train_rows(op, src, dst, dims, f)
    torch.cuda.synchronize()
    assert bool((whole == T.CANARY32).all()), "a refused launch wrote"


def test_every_launcher_was_reached(ctx):
    print("\nlauncher | cases | worst |got - ref| / bound per output (case); 0.0000 = bit equality")
    for k in sorted(_seen):
        w = ", ".join(f"{o} {v[0]:.4f} ({v[1]})" for (kk, o), v in sorted(_worst.items()) if kk == k)
        print(f"{k} | {len(_seen[k])} | {w}")
    for me in sorted(_scatter):
        rows = _scatter[me]
        print(f"scatter + flush, sources x 2^-{me}: max |err| / max |ref| {max(r[0] for r in rows):.3e}, "
              f"median |err| / |ref| up to {max(r[1] for r in rows):.3e} ({len(rows)} cases)")
    for k, (n, tot) in sorted(_flips.items()):
        print(f"{k}: {n} of {tot} elements are the other bf16 neighbour")
    assert set(_seen) == T.LAUNCHERS, set(_seen) ^ T.LAUNCHERS
    both = {c.name for c in T.cases() if c.kernel == "launch_rmsnorm_bwd"}
    assert any("_d1024" in n for n in both) and any("_d1028" in n for n in both)
