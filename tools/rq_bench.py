"""Residual-quantization benchmark (docid creation): trains M x K codebooks on the training sample of N synthetic
embeddings and encodes all N rows on the device (rpr_rq_train / rpr_rq_encode), each timed on its own, and reports the
achieved fp32 rate against the 157.3 TF/s fp32 MFMA peak of the MI355X. One JSON line on stdout.

  python tools/rq_bench.py --n 8841823 --d 768 --M 32 --K 256

The embeddings are generated on the device (anisotropic Gaussian, seeded); the host memmap path of the CLI is not part of
the timed region."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_TFLOPS = 157.3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--niter", type=int, default=25)
    ap.add_argument("--chunk_rows", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args(argv)
    from ripor_amd import engine as E

    ctx = E.Context.get(0)
    N, d, M, K = args.n, args.d, args.M, args.K
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.empty((N, d), dtype=torch.float32, device="cuda")
    scale = torch.linspace(0.25, 2.0, d, device="cuda")
    for lo in range(0, N, 1 << 20):
        X[lo:lo + (1 << 20)] = torch.randn((min(1 << 20, N - lo), d), generator=g, device="cuda") * scale
    S, init = E.rq_training_plan(N, M, K)
    Xs = X[torch.from_numpy(S).cuda()].contiguous()
    n_train = len(S)

    # warm-up of every shape the timed region uses
    E.rq_train(ctx, Xs, M, K, init, niter=1)
    E.rq_encode(ctx, X[:min(N, args.chunk_rows)], torch.zeros((M, K, d), device="cuda"), chunk_rows=args.chunk_rows)
    torch.cuda.synchronize()

    train_s, enc_s = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        books, mse = E.rq_train(ctx, Xs, M, K, init, niter=args.niter)   # ends in a stream synchronisation
        torch.cuda.synchronize()
        train_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        codes, enc_mse = E.rq_encode(ctx, X, books, chunk_rows=args.chunk_rows)
        torch.cuda.synchronize()
        enc_s.append(time.perf_counter() - t0)
    train_flop = 2.0 * n_train * K * d * M * (args.niter + 1)
    enc_flop = 2.0 * N * K * d * M
    tr, en = min(train_s), min(enc_s)
    out = dict(metric="rq_docid_creation", n=N, d=d, M=M, K=K, niter=args.niter, n_train=n_train,
               train_s=round(tr, 4), encode_s=round(en, 4), train_s_all=[round(t, 4) for t in train_s],
               encode_s_all=[round(t, 4) for t in enc_s],
               train_tflops=round(train_flop / tr / 1e12, 2), encode_tflops=round(enc_flop / en / 1e12, 2),
               encode_frac_of_f32_peak=round(enc_flop / en / 1e12 / PEAK_F32_TFLOPS, 3),
               train_frac_of_f32_peak=round(train_flop / tr / 1e12 / PEAK_F32_TFLOPS, 3),
               train_level_mse_first_last=[float(mse[0]), float(mse[-1])],
               encode_level_mse_first_last=[float(enc_mse[0]), float(enc_mse[-1])],
               unique_smtid_frac=float(len(np.unique(codes, axis=0)) / N) if N <= 2_000_000 else None)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
