#!/usr/bin/env python3
"""Time the headline-shape search (beam 10, length 32, 2150 queries per step, the MS MARCO-size trie) on a gated-GELU model
at google/t5-v1_1-base dims (d_ff 2048, wo(gelu_new(wi_0 x) * wi_1 x)) and on a ReLU control with the same d_ff 2048, one
JSON line each: queries/s of warm hipGraph replays and, from an eager profile pass, the time per kernel class (the gate
kernel is accounted under "other").

The share of the gated run's KERNEL time the gate kernel takes comes from a trace of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o gated -- python tools/gated_ff_timing.py --which gated --steps 2
    python tools/rocpd_summary.py DIR/.../gated_results.db stats.csv     (when the run wrote a rocpd database)
    python tools/gated_ff_timing.py --share stats.csv                    (no GPU: reads the per-kernel stats)

Usage: python tools/gated_ff_timing.py [--which gated|relu|both] [--steps 3] [--warmup 1] [--batch 2150] [--docs N]"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MSMARCO_DOCS = 8_841_823


def share(path):
    """gate kernel share of the total kernel time in a per-kernel stats CSV (Name, Calls, TotalDurationNs | TotalDuration(us))."""
    total = gate = 0.0
    calls = 0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            dur = float(row.get("TotalDurationNs") or row.get("TotalDuration(us)") or row.get("TotalDuration") or 0.0)
            total += dur
            if "gated_gelu_kernel" in name:
                gate += dur
                calls += int(float(row.get("Calls") or 0))
    print(json.dumps({"stats": path, "gate_kernel_calls": calls, "gate_kernel_share_of_kernel_time": gate / total if total else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="both", choices=["gated", "relu", "both"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=2150)
    ap.add_argument("--beams", type=int, default=10)
    ap.add_argument("--len", type=int, default=32, dest="L")
    ap.add_argument("--docs", type=int, default=MSMARCO_DOCS)
    ap.add_argument("--share", default=None, metavar="STATS_CSV")
    args = ap.parse_args()
    if args.share:
        return share(args.share)
    import numpy as np
    import torch
    from ripor_amd import _lib
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    L, V, B, Q, W, K = args.L, 256, args.beams, args.batch, args.warmup, args.steps
    dims = synth.t5_v11_base_dims(L=L, V=V)
    ctx = E.Context.get(0)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes_fast(args.docs, L, V), V)
    pool_ids, pool_mask = synth.make_queries(6980, vocab_size=dims.vocab_size)
    sels = [[(s * Q + i) % 6980 for i in range(Q)] for s in range(W + K)]
    lq = (max(int(pool_mask[sel].sum(1).max()) for sel in sels) + 7) // 8 * 8
    batches = []
    for sel in sels:
        ids = np.pad(pool_ids[sel], ((0, 0), (0, max(0, lq - pool_ids.shape[1]))))[:, :lq]
        mask = np.pad(pool_mask[sel], ((0, 0), (0, max(0, lq - pool_mask.shape[1]))))[:, :lq]
        batches.append((torch.from_numpy(ids).to("cuda", torch.int32), torch.from_numpy(mask).to("cuda", torch.int32)))
    for kind in (["gated-gelu", "relu"] if args.which == "both" else ["gated-gelu" if args.which == "gated" else "relu"]):
        model = E.DeviceModel(ctx, synth.make_state_dict(dims, feed_forward_proj=kind), dims)
        ctx.status(clear=True)
        for i in range(W):
            E.search(model, trie, *batches[i], B, L)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            E.search(model, trie, *batches[W + i], B, L)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / K
        flags = ctx.status(clear=True)
        ctx.profile_reset(); ctx.profile_enable(True)
        E.search(model, trie, *batches[W], B, L)
        torch.cuda.synchronize()
        st = ctx.profile_get(); ctx.profile_enable(False)
        print(json.dumps({"task": "constrained beam search, t5-v1.1-base dims (d_ff 2048)", "feed_forward_proj": kind, "queries_per_step": Q,
                          "beams": B, "len": L, "docs": int(trie.N), "enc_len_padded": lq, "ms_per_step": dt * 1e3, "queries_per_s": Q / dt,
                          "status_flags": int(flags), "fork_stats": ctx.last_fork_stats(), "workspace_mb": ctx.workspace_bytes() / 1e6,
                          "profile_kernel_ms": {k: round(v["total_ms"], 3) for k, v in st.items()},
                          "profile_other_launches": int(st[_lib.KERNEL_CLASS_NAMES[_lib.K_OTHER]]["launches"])}), flush=True)
        del model


if __name__ == "__main__":
    main()
