#!/usr/bin/env python
"""GPU box: write tests/golden/gemm_pp_order_bits.json, the sha256 of every output buffer of the cases of
tests/test_gpu_gemm_issue_order.py. Run it ONCE, in a tree whose libraries were built from the commit BEFORE the K-loop's MFMA
issue order changed (copy this file and the test file into that tree); the test then holds every later build to those bits.

    python tools/gemm_pp_order_record.py [--out PATH] [--tree TREE_WHOSE_LIBRARY_RUNS] [--commit ITS_COMMIT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import test_gpu_gemm_issue_order as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--commit", default="", help="the commit the library was built from (recorded as text)")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    cases = T.run_cases(tree)
    for k in sorted(cases):
        print(f"{k}: err {cases[k]['err']:.3g} scale {cases[k]['scale']:.3g}")
    rec = {"what": "sha256 of the output buffers of tests/test_gpu_gemm_issue_order.py, from the library with the interleaved "
                   "MFMA order (lo*hi, hi*lo, hi*hi of an accumulator 16 / 8 MFMAs apart)",
           "library_commit": a.commit,
           "sha256": {k: cases[k]["sha"] for k in sorted(cases)}}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(cases)} cases, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
