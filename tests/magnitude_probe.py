"""Measurements behind tests/test_gpu_magnitude.py: the split-precision residual GEMM and the fused-RMSNorm GEMM behind it,
chained through the test hook `Context.linear_h2`, against the operation in fp64 — at one activation magnitude s, or with the
rows of one launch cycling through every s of the grid.

    x = resid + A W^T            mode RPR_LIN_X_PLANES: x leaves the epilogue as two f16 planes (X_PLANE_SCALE) + fixed-point row sums
    y = x rsqrt(mean(x^2) + eps) W2^T     mode RPR_LIN_FUSED_NORM on exactly those planes and those row sums

The reference is fp64 arithmetic on the ORIGINAL fp32 inputs, so what is measured is the operation, not the kernel against its
own quantisation. y does not depend on s (up to eps), so its bar does not either.

Importable without a GPU (the case table is shared with tests/test_magnitude_routes.py); run as a script it measures the cases
named on the command line in this process — the tile-pinned cases need the development library, whose switches are read once
when it loads — and prints one line "RESULT <json>"."""
import json
import sys

GRID = [2.0 ** e for e in (4, 2, 0, -1, -2, -3, -4, -5, -7, -10)]
EPS = 1e-6
X_PLANE_SCALE, SSQ_FIX = 1.0 / 16, 65536.0          # csrc/common.h
BAR = 2e-5                                           # tests/test_gpu_parity.py::test_linear_kernel_against_torch_fp32: 2e-5 max(1, max |ref|)
STATUS_SATURATED, STATUS_SMALL_STREAM = 1, 8         # ripor_amd/_lib.py

# name -> (M, N, K) of the first launch, the kernel family writing ssq_out that the default route gives it (hook: scratch lent),
# as tests/gemm_route_driver prints it: (family, bm, bn, ksplit, reduce). The second launch is (M, N, N).
ROUTED = {
    "skinny16 10x768x768": ((10, 768, 768), ("skinny16", 16, 16, 1, "none")),
    "wsplit32x32 80x768x768": ((80, 768, 768), ("wsplit", 32, 32, 1, "none")),
    "wsplit64x32 600x768x768": ((600, 768, 768), ("wsplit", 64, 32, 1, "none")),
    "wsplit64x64 600x1024x1024": ((600, 1024, 1024), ("wsplit", 64, 64, 1, "none")),
    "wsplit32x32 300x256x768": ((300, 256, 768), ("wsplit", 32, 32, 1, "none")),
    "dma128x64+splitk_epilogue4 1500x768x768": ((1500, 768, 768), ("dma", 128, 64, 3, "fused4")),
    "dma128x64+splitk_epilogue 1500x832x768": ((1500, 832, 768), ("dma", 128, 64, 3, "fused")),
}
# RPR_GEMM_TILE of the development library -> (family, bm, bn), the shapes it runs (ragged second / third row tile) and the MFMA bodies
TILED = {64: ("dma", 128, 64), 128: ("dma", 128, 128), 256: ("pp", 256, 256)}
TILED_SHAPES = [(300, 768, 768), (257, 768, 768)]


def tiled_names(tile):
    fam, bm, bn = TILED[tile]
    return [f"{fam}{bm}x{bn}{' mfma16=%d' % m16 if tile == 256 else ''} {M}x{N}x{K}"
            for (M, N, K) in TILED_SHAPES for m16 in ((0, 1) if tile == 256 else (0,))]


def _inputs(M, N, K, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5,
            torch.randn(N, N, generator=g) * N ** -0.5)


def chain(ctx, M, N, K, s=None, mfma16=0, seed=0):
    """One chained pair of launches. s: the magnitude of the whole launch (resid = s randn, W = s randn K^-0.5), or None: row m
    carries GRID[m % len(GRID)] (resid and A scaled by rows; W is shared by the rows and stays at 1). Returns the figures the
    tests assert on, every one as measured / bound."""
    import torch
    dev = ctx.device
    R0, A, W, W2 = _inputs(M, N, K, seed)
    if s is None:
        srow = torch.tensor([GRID[m % len(GRID)] for m in range(M)])
        resid, A = R0 * srow[:, None], A * srow[:, None]
    else:
        srow = torch.full((M,), float(s))
        resid, W = R0 * s, W * s                       # powers of two: exact
    x = resid.double() + A.double() @ W.double().t()
    y = (x * torch.rsqrt((x * x).mean(1, keepdim=True) + EPS)) @ W2.double().t()

    Ad, Wd, Rd, W2d = (t.to(dev).contiguous() for t in (A, W, resid, W2))
    pl = torch.zeros((2, M, N), dtype=torch.float16, device=dev)
    ssq = torch.zeros(M, dtype=torch.int64, device=dev)
    ctx.status(clear=True)
    ctx.linear_h2(Ad, Wd, 1, mfma16, resid=Rd, out_planes=pl, ssq_out=ssq)
    torch.cuda.synchronize()
    st1 = ctx.status(clear=True)
    dec = (pl[0].double() + pl[1].double()) / X_PLANE_SCALE
    Adec = dec.float()
    assert torch.equal(Adec.double(), dec), "the decoded planes are fp32 values"
    out = torch.full((M, N), 12345.0, device=dev)
    ctx.linear_h2(Adec.contiguous(), W2d, 4, mfma16, row_ssq=ssq, eps=EPS, out0=out)
    torch.cuda.synchronize()
    st2 = ctx.status(clear=True)

    dec, got, own = dec.cpu(), out.double().cpu(), ssq.double().cpu() / SSQ_FIX
    # What the planes may differ from x by. A value v goes into planes at X_PLANE_SCALE to half a step: h(v) = max(2^-21, 2^-22 |v|)
    # (f16 lo plane: a step of 2^-20 below |v| = 2, 22 bits above). x is rounded twice — the residual on its way in, the sum on
    # its way out: h(resid) + h(x), which is the max(2^-20, 2^-21 |x|) of tests/test_gpu_gemm_mfma16.py where resid ~ x. That
    # file compares with the fp32 value in front of the split; against the TRUE x the K products count too, each operand
    # carried to half a step of ITS planes (A unscaled, W at W_PLANE_SCALE = 2^8: 22 bits, or 2^-25 / scale where the lo plane
    # is subnormal — the small rows of the mixed launch): first order, sum_k (dA_k |w_k| + |a_k| dW_k). The fp32 accumulation,
    # a random walk of 2^-24 per step, stays inside it (measured: at most 0.5 of this term).
    h = lambda v, scale=X_PLANE_SCALE: torch.maximum(torch.full_like(v, 2.0 ** -25 / scale), v.abs() * 2.0 ** -22)
    Aa, Wa = A.double().abs(), W.double().abs()
    xq = h(resid.double()) + h(x) + h(Aa, 1.0) @ Wa.t() + Aa @ h(Wa, 256.0).t()
    # row sums: what that moves them by, half a unit per piece a kernel adds (the narrowest tile has 16 columns), the fp32 sums
    true = (x * x).sum(1)
    ssq_tol = (2 * x.abs() * xq + xq * xq).sum(1) + (N / 16) * 0.5 / SSQ_FIX + 1e-5 * true
    row_err = (got - y).abs().max(1).values
    bar = BAR * max(1.0, float(y.abs().max()))
    return dict(plane=float(((dec - x).abs() / xq).max()), ssq=float(((own - true).abs() / ssq_tol).max()),
                err=float(row_err.max()) / bar, bar=bar, flags=int(st1 | st2), flags_producer=int(st1),
                row_err=[float(row_err[srow == g].max()) / bar for g in GRID] if s is None else None,
                rms=float(true.div(N).sqrt().median()))


def sweep(ctx, M, N, K, mfma16=0):
    """Every s of the grid alone, then the mixed launch."""
    seed = M * 7 + N * 3 + K + mfma16
    out = {repr(s): chain(ctx, M, N, K, s, mfma16, seed) for s in GRID}
    out["mixed"] = chain(ctx, M, N, K, None, mfma16, seed + 1)
    return out


def main(argv):
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    from ripor_amd import engine as E
    ctx = E.Context.get(0)
    tile = int(argv[1])
    out = {}
    for (M, N, K) in TILED_SHAPES:
        for m16 in ((0, 1) if tile == 256 else (0,)):
            fam, bm, bn = TILED[tile]
            out[f"{fam}{bm}x{bn}{' mfma16=%d' % m16 if tile == 256 else ''} {M}x{N}x{K}"] = sweep(ctx, M, N, K, m16)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main(sys.argv)
