"""Residual-quantization benchmark (docid creation): trains M x K codebooks on the training sample of N synthetic
embeddings and encodes all N rows on the device (rpr_rq_train / rpr_rq_encode), each timed on its own, and reports the
achieved fp32 rate against the 157.3 TF/s fp32 MFMA peak of the MI355X. One JSON line on stdout.

  python tools/rq_bench.py --n 8841823 --d 768 --M 32 --K 256 [--beam 5]

--beam N encodes with a beam of N candidate encodings per row (rpr_rq_encode_beam; the training stays greedy); the encode
rate then counts the distance work of the beam, (1 + (M - 1) N) / M times the greedy one.

The embeddings are generated on the device (anisotropic Gaussian, seeded); the host memmap path of the CLI is not part of
the timed region.

  python tools/rq_bench.py --search --n 8841823 --d 768 --M 32 --K 256 --Q 128 --topk 200

times rpr_rq_search alone over seeded random codes: the first call (cold: scratch allocation, code objects)
and the best and median of --repeats warm calls by device events, the code bytes per second it streams (one read of the
code matrix per pass) and the LUT lookups per second it sustains (Q N M per pass), and as the yardstick on the same card
a plain torch path: the LUT by matmul, per chunk of queries the level sum of LUT columns gathered by the codes, torch.topk.

  python tools/rq_bench.py --flat --n 8841823 --d 768 --M 32 --K 256 --Q 128 --topks 200 1000

times the exact search (FlatIndex.search -> rpr_flat_search) over the same synthetic embeddings held on the
device in blocks of at most 4 GB: cold and warm by device events per topk, the fp32 rate of its 2 Q N d flops against the
peak, and as the yardstick on the same card a plain torch path (torch.matmul per block, torch.topk, merge by a second
topk). Then it trains greedy codebooks on the same embeddings, encodes them, and reports recall@10 / 100 / 200 of
rpr_rq_search against the exact result."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_TFLOPS = 157.3


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def search_leg(args, E):
    ctx = E.Context.get(0)
    N, d, M, K, Q, topk = args.n, args.d, args.M, args.K, args.Q, args.topk
    g = torch.Generator(device="cuda").manual_seed(0)
    books = torch.randn((M, K, d), generator=g, device="cuda") * torch.linspace(1.0, 0.05, M, device="cuda")[:, None, None]
    q = torch.randn((Q, d), generator=g, device="cuda")
    codes = torch.randint(0, K, (N, M), generator=g, device="cuda", dtype=torch.int16)
    torch.cuda.synchronize()
    cold, _ = _timed(lambda: E.rq_search(ctx, q, books, codes, topk))
    warm = []
    for _ in range(max(3, args.repeats)):
        t, (idx, sc) = _timed(lambda: E.rq_search(ctx, q, books, codes, topk))
        warm.append(t)

    def torch_path():
        lut = (q @ books.reshape(M * K, d).T).reshape(Q, M, K)
        out_i, out_s = [], []
        for q0 in range(0, Q, args.torch_chunk):
            part = lut[q0:q0 + args.torch_chunk]
            s = torch.zeros((part.shape[0], N), device="cuda")
            for m in range(M):
                s += part[:, m].index_select(1, codes_l[:, m])
            v, i = torch.topk(s, topk, dim=1)
            out_i.append(i); out_s.append(v)
        return torch.cat(out_i), torch.cat(out_s)

    codes_l = codes.long()
    _timed(torch_path)   # warm-up of every shape
    t_torch, (ti, ts) = min((_timed(torch_path) for _ in range(2)), key=lambda r: r[0])
    best, med = min(warm), sorted(warm)[len(warm) // 2]
    same = float((ti == idx).float().mean())
    out = dict(metric="rq_search", n=N, d=d, M=M, K=K, Q=Q, topk=topk, cold_s=round(cold, 5), warm_s=round(best, 5),
               warm_median_s=round(med, 5), warm_s_all=[round(t, 5) for t in warm],
               queries_per_s=round(Q / best, 1),
               # per pass over the rows: the code matrix once from HBM (the other query groups hit the caches), Q N M lookups
               code_gb_per_s_per_pass_time=round(N * M * 2 / best / 1e9, 1),
               lut_lookups_per_s_per_pass_time=float("%.4g" % (Q * N * M / best)),
               torch_s=round(t_torch, 5), torch_over_rq_search=round(t_torch / best, 2),
               idx_equal_to_torch_frac=round(same, 6), max_score_diff_to_torch=float((ts - sc).abs().max()))
    print(json.dumps(out), flush=True)


def flat_leg(args, E):
    from ripor_amd.tasks.dense_indexer import FLAT_BLOCK_BYTES, FlatIndex
    ctx = E.Context.get(0)
    N, d, M, K, Q = args.n, args.d, args.M, args.K, args.Q
    g = torch.Generator(device="cuda").manual_seed(0)
    scale = torch.linspace(0.25, 2.0, d, device="cuda")
    rows = max(1, FLAT_BLOCK_BYTES // (d * 4))
    blocks = []
    for lo in range(0, N, rows):
        xb = torch.empty((min(rows, N - lo), d), dtype=torch.float32, device="cuda")
        for p in range(0, xb.shape[0], 1 << 20):
            xb[p:p + (1 << 20)] = torch.randn((min(1 << 20, xb.shape[0] - p), d), generator=g, device="cuda") * scale
        blocks.append((lo, xb))
    q = torch.randn((Q, d), generator=g, device="cuda") * scale
    index = FlatIndex.from_blocks(ctx, blocks)
    torch.cuda.synchronize()
    out = dict(metric="flat_search", n=N, d=d, Q=Q, blocks=len(blocks), scratch_bytes=E.FLAT_SCRATCH_BYTES)
    exact = None
    for topk in args.topks:
        cold, _ = _timed(lambda: index.search(q, topk))
        warm = []
        for _ in range(max(3, args.repeats)):
            t, (idx, sc) = _timed(lambda: index.search(q, topk))
            warm.append(t)

        def torch_path():
            state = None
            for lo, xb in blocks:
                v, i = torch.topk(torch.matmul(q, xb.T), min(topk, xb.shape[0]), dim=1)
                i = i + lo
                if state is not None:
                    v, i = torch.cat([state[0], v], dim=1), torch.cat([state[1], i], dim=1)
                    v, o = torch.topk(v, min(topk, v.shape[1]), dim=1)
                    i = i.gather(1, o)
                state = (v, i)
            return state

        _timed(torch_path)   # warm-up of every shape
        t_torch, (tv, ti) = min((_timed(torch_path) for _ in range(2)), key=lambda r: r[0])
        best = min(warm)
        tf = 2.0 * Q * N * d / best / 1e12
        out[f"top{topk}"] = dict(cold_s=round(cold, 5), warm_s=round(best, 5), warm_median_s=round(sorted(warm)[len(warm) // 2], 5),
                                 warm_s_all=[round(t, 5) for t in warm], queries_per_s=round(Q / best, 1), tflops=round(tf, 2),
                                 frac_of_f32_peak=round(tf / PEAK_F32_TFLOPS, 3), torch_s=round(t_torch, 5),
                                 torch_over_flat_search=round(t_torch / best, 3),
                                 idx_equal_to_torch_frac=round(float((ti == idx).float().mean()), 6),
                                 max_score_diff_to_torch=float((tv - sc).abs().max()))
        if exact is None:
            exact = idx
    if args.recall:
        S, init = E.rq_training_plan(N, M, K)
        St = torch.from_numpy(S).cuda()
        Xs = torch.cat([xb[St[(St >= lo) & (St < lo + xb.shape[0])] - lo] for lo, xb in blocks])
        books, _ = E.rq_train(ctx, Xs, M, K, init, niter=args.niter)
        del Xs
        codes = np.concatenate([E.rq_encode(ctx, xb, books, chunk_rows=args.chunk_rows)[0] for _, xb in blocks])
        ri, _ = E.rq_search(ctx, q, books, codes, max(200, args.topks[0]))
        ri, ex = ri.cpu().numpy(), exact.cpu().numpy()
        out["rq_search_recall_vs_exact"] = {f"recall@{k}": round(float(np.mean([len(set(ri[i, :k]) & set(ex[i, :k])) / k
                                                                                  for i in range(Q)])), 4)
                                             for k in (10, 100, 200) if k <= ex.shape[1]}
        out["rq"] = dict(M=M, K=K, niter=args.niter, n_train=int(len(S)))
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--niter", type=int, default=25)
    ap.add_argument("--chunk_rows", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--beam", type=int, default=1, help="beam of the encode leg (1: greedy rpr_rq_encode; else rpr_rq_encode_beam)")
    ap.add_argument("--search", action="store_true", help="time rpr_rq_search instead of training / encoding")
    ap.add_argument("--flat", action="store_true", help="time the exact search (rpr_flat_search) and the recall of rpr_rq_search against it")
    ap.add_argument("--topks", type=int, nargs="+", default=[200, 1000], help="--flat: the topk values timed (recall uses the first)")
    ap.add_argument("--recall", type=int, default=1, help="--flat: 0 skips the quantizer training and the recall figures")
    ap.add_argument("--Q", type=int, default=128)
    ap.add_argument("--topk", type=int, default=200)
    ap.add_argument("--torch_chunk", type=int, default=8, help="queries per chunk of the torch yardstick")
    args = ap.parse_args(argv)
    from ripor_amd import engine as E
    if args.search:
        return search_leg(args, E)
    if args.flat:
        return flat_leg(args, E)

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
    E.rq_encode(ctx, X[:min(N, args.chunk_rows)], torch.zeros((M, K, d), device="cuda"), chunk_rows=args.chunk_rows,
                beam=args.beam)
    torch.cuda.synchronize()

    train_s, enc_s = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        books, mse = E.rq_train(ctx, Xs, M, K, init, niter=args.niter)   # ends in a stream synchronisation
        torch.cuda.synchronize()
        train_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        codes, enc_mse = E.rq_encode(ctx, X, books, chunk_rows=args.chunk_rows, beam=args.beam)
        torch.cuda.synchronize()
        enc_s.append(time.perf_counter() - t0)
    train_flop = 2.0 * n_train * K * d * M * (args.niter + 1)
    enc_flop = 2.0 * N * K * d * (1 + (M - 1) * args.beam)   # level 0 scores the row, every later level its beam entries
    tr, en = min(train_s), min(enc_s)
    out = dict(metric="rq_docid_creation", n=N, d=d, M=M, K=K, niter=args.niter, n_train=n_train, beam=args.beam,
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
