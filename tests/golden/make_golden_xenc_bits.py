"""Records tests/golden/xenc_bits.npz: the fp32 scores of ``engine.xenc_score`` on the MI355X, bit for bit, for the
fixture batches of CASES in both precisions (tests/test_gpu_xenc_bits.py compares against them). Needs the GPU and a built
library; run by hand, and only from a commit whose scores are trusted (for instance after a toolchain change):

  python tests/golden/make_golden_xenc_bits.py --commit $(git rev-parse HEAD)

The file also holds that commit and the ``hipcc --version`` string of the build."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import xenc_half_ref as href  # noqa: E402

# x1/e: 512 tokens; x2/c: heads of 64; x2/f: a short batch; x3/a: lengths 1 .. 256 (full, ragged and multi-tile attention)
CASES = [("x1", "b"), ("x1", "e"), ("x2", "c"), ("x2", "f"), ("x3", "a")]
PRECISIONS = ("f32", "f16")


def score_all(ctx):
    """-> {"<model>_<key>_<precision>": float32 scores}; every model is loaded once and switched between the modes."""
    from ripor_amd import engine as E
    out = {}
    for name in sorted({m for m, _ in CASES}):
        fx = href.load(name)
        model = E.XencModel(ctx, fx["weights"], fx["cfg"])
        for prec in PRECISIONS:
            model.set_precision(prec)
            for m, key in CASES:
                if m != name:
                    continue
                b = fx["batches"][key]
                got = E.xenc_score(model, torch.from_numpy(b["ids"]), torch.from_numpy(b["types"]), torch.from_numpy(b["mask"]))
                out[f"{m}_{key}_{prec}"] = got.cpu().numpy().astype(np.float32, copy=False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "xenc_bits.npz"))
    args = ap.parse_args()
    from ripor_amd import engine as E
    import __graft_entry__ as ge
    hipcc = subprocess.run([ge._hipcc(), "--version"], capture_output=True, text=True, check=True).stdout.strip()
    scores = score_all(E.Context.get(0))
    assert all(np.isfinite(v).all() for v in scores.values())
    np.savez(args.out, commit=np.array(args.commit), hipcc_version=np.array(hipcc), **scores)
    for k, v in scores.items():
        print(f"[xenc bits] {k}: {len(v)} scores, first {v[0]!r}")
    print(f"[xenc bits] wrote {args.out} ({os.path.getsize(args.out)} bytes) at {args.commit}")


if __name__ == "__main__":
    main()
