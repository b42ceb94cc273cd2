#!/usr/bin/env python3
"""Record of what the forward passes (csrc/passes.hip) launch and compute, for comparing two builds of the library after a
host-side refactor: a fixed list of eager calls with the library profile on; per call the profile records without their
time fields (launches, flops, bytes per kernel class) and a sha256 of every output array, as JSON. Two builds agree when
their files are equal byte for byte. (With the profile on, rpr_search enqueues eagerly whatever its graph flag says. An
optimistic forced-tail search that leaves a query unforced returns that query's rows as the workspace held them: the
hashes of those cases are those of this call list in this order, which is fixed.)

Covers: precision f16x2 and f32; forced tail off / exact / optimistic with one and two forks; log-softmax scores; debug
taps; 1, 10 and 40 beams (radix selection); a decoder vocab size that is not a multiple of 64; scaleup_output_hidden; a
d_kv = 128 model; a batch split over the two lanes; DeviceModel.encode; lngknp_forward.

Usage: tools/pass_equivalence.py [--out OUT.json] [--time OUT_TIMES.json]
--time: the wall time per call (median of 50 after 5 warm-up calls, f16x2) of the two entry points that enqueue
eagerly in production: lngknp_forward at t5-base dims (bz 4, 2 docs, L 32) and DeviceModel.encode at 64 queries."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripor_amd import engine as E  # noqa: E402
from ripor_amd.utils import synth  # noqa: E402


def digest(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def arg(flag):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None


def record_calls(ctx, out_path):
    records = {}

    def record(name, fn):
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            outs = fn()
            torch.cuda.synchronize()
            prof = ctx.profile_get()
        finally:
            ctx.profile_enable(False)
        ctx.status(clear=True)
        records[name] = dict(
            profile={k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in prof.items()},
            forks=ctx.last_fork_stats() if name.startswith("search") else None,
            sha256={k: digest(v) for k, v in outs.items()})
        print(name, sum(v["launches"] for v in prof.values()), "launches", flush=True)

    def build(dims, N, seed, **kw):
        sd = synth.make_state_dict(dims, seed=seed, **kw)
        L, V = len(dims.decoder_vocab_sizes), dims.decoder_vocab_sizes[0]
        return E.DeviceModel(ctx, sd, dims), E.DeviceTrie.from_codes(ctx, synth.make_codes(N, L, V, seed=seed), V), L

    def search(model, trie, Q, B, L, seed, vocab=512, log_softmax=False, taps=False):
        ids, mask = synth.make_queries(Q, vocab_size=vocab, seed=seed, max_len=14)
        r = E.search(model, trie, torch.from_numpy(ids), torch.from_numpy(mask), B, L,
                     apply_log_softmax_for_scores=log_softmax, taps=taps)
        outs = dict(tokens=r.tokens, scores=r.scores, row_lo=r.row_lo, row_hi=r.row_hi)
        outs.update(r.taps or {})
        return outs

    mini = build(synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=256), 1000, 11)
    v100 = build(synth.mini_dims(L=8, V=100), 1000, 107)
    scale = build(synth.mini_dims(L=5, V=1024, enc_layers=1, d_ff=128, scaleup_output_hidden=True), 700, 41, logit_scale=8.0)
    t3b = build(synth.ModelDims(vocab_size=512, d_model=1024, d_kv=128, d_ff=512, num_layers=1, num_decoder_layers=24,
                                num_heads=32, decoder_vocab_sizes=[256] * 8), 3000, 701)

    for prec in ("f16x2", "f32"):
        ctx.set_precision(prec)
        for ft, forks in ((0, []), (1, [3]), (1, [3, 5]), (2, [3]), (2, [3, 5])):
            ctx.set_forced_tail(ft)
            ctx.set_fork_depths(forks if ft else None)
            for ls in (False, True):
                record(f"search/{prec}/mini/ft{ft}/forks{forks}/logsoftmax{int(ls)}",
                       lambda: search(*mini[:2], 6, 4, mini[2], 21, log_softmax=ls))
        ctx.set_forced_tail(1)
        ctx.set_fork_depths([3])
        record(f"search/{prec}/mini/taps", lambda: search(*mini[:2], 3, 4, mini[2], 22, taps=True))
        for B in (1, 10, 40):
            record(f"search/{prec}/mini/B{B}", lambda: search(*mini[:2], 5, B, mini[2], 23))
        for ls in (False, True):
            record(f"search/{prec}/v100/logsoftmax{int(ls)}", lambda: search(*v100[:2], 4, 4, v100[2], 24, log_softmax=ls))
        ctx.set_lane_split(16)
        record(f"search/{prec}/mini/lanes", lambda: search(*mini[:2], 9, 4, mini[2], 25))
        ctx.set_lane_split(10240)
        ctx.set_fork_depths(None)
        record(f"search/{prec}/scaleup", lambda: search(*scale[:2], 5, 6, scale[2], 42))
        for ft in (0, 1):
            ctx.set_forced_tail(ft)
            record(f"search/{prec}/3b/ft{ft}", lambda: search(*t3b[:2], 4, 10, t3b[2], 26))
        ctx.set_forced_tail(1)

        def encode():
            ids, mask = synth.make_queries(5, vocab_size=512, seed=27, max_len=14)
            return dict(encoder_out=mini[0].encode(torch.from_numpy(ids), torch.from_numpy(mask)))
        record(f"encode/{prec}/mini", encode)

        def lngknp(model=mini[0], L=mini[2], bz=3):
            ids, mask = synth.make_queries(bz, vocab_size=512, seed=28, max_len=14)
            codes = synth.randint("pass_equivalence.codes", (bz, 2, L), 0, 256, seed=28)
            tp = synth.uniform_f32("pass_equivalence.tp", (2, bz), 4.0, seed=28)
            tn = synth.uniform_f32("pass_equivalence.tn", (2, bz), 4.0, seed=29)
            losses, pos = E.lngknp_forward(model, torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(codes),
                                           torch.from_numpy(tp), torch.from_numpy(tn), [L // 2, L])
            return dict(losses=losses, position_scores=pos)
        record(f"lngknp_forward/{prec}/mini", lngknp)
    ctx.set_precision("f16x2")
    with open(out_path, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
    print("wrote", out_path, len(records), "calls")


def time_eager_calls(ctx, out_path):
    def wall(fn, n=50, warm=5):
        ts = []
        for i in range(warm + n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3
    dims = synth.t5_base_dims(L=32, V=256, vocab_size=2048)
    base = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=504), dims)
    ids, mask = synth.make_queries(4, vocab_size=2048, seed=504, max_len=20)
    codes = synth.randint("pass_equivalence.codes", (4, 2, 32), 0, 256, seed=504)
    ids, mask, codes = (torch.from_numpy(a).to("cuda", torch.int32) for a in (ids, mask, codes))
    q_ids, q_mask = (torch.from_numpy(a).to("cuda", torch.int32) for a in synth.make_queries(64, vocab_size=2048, seed=505, max_len=20))
    times = dict(lngknp_forward_ms=wall(lambda: E.lngknp_forward(base, ids, mask, codes)),
                 encode_q64_ms=wall(lambda: base.encode(q_ids, q_mask)))
    with open(out_path, "w") as f:
        json.dump(times, f)
    print(times)


if __name__ == "__main__":
    ctx = E.Context.get(0)
    if arg("--out"):
        record_calls(ctx, arg("--out"))
    if arg("--time"):
        time_eager_calls(ctx, arg("--time"))
