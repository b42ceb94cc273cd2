#!/usr/bin/env python3
"""Times one optimisation step of the two device training steps with and without dropout (the README's training rows and
profiles/r08_train_dropout_summary.txt): t5-base dims, L 32, V 256, queries of 32 tokens, bf16 mode unless --precision says
otherwise; the fine-tune step on 128 examples, the seq2seq step on 256.

    python tools/train_dropout_timing.py [--rates 0,0.1] [--steps 20] [--warmup 5] [--split] [--repo DIR]

Per (step, rate) one JSON line: median / min / max of --steps hipEvent-timed steps and, with --split, the time and the launch
count per kernel class from one profiled step (rpr_profile_*; that pass runs the launches one by one, so its total is above
the timed step). --repo DIR imports the package from another checkout of this repository (to alternate two builds in one
session: a checkout from before the dropout entry points runs at rate 0 only)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rates", default="0,0.1")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--split", action="store_true")
ap.add_argument("--precision", default="bf16")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from ripor_amd import engine as E  # noqa: E402
from ripor_amd.utils import synth  # noqa: E402

ctx = E.Context.get(0)
ctx.set_precision(args.precision)
L, V = 32, 256
dims = synth.t5_base_dims(L=L, V=V, vocab_size=2048)
model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=3), dims)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3))


def split(fn):
    ctx.profile_reset(); ctx.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    st = ctx.profile_get()
    ctx.profile_enable(False)
    return {k: dict(ms=round(v["total_ms"], 3), launches=v["launches"]) for k, v in st.items() if v["launches"]}


for step, bz in (("fine-tune", 128), ("seq2seq", 256)):
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=5, fixed_len=32)
    ids, mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    codes = torch.from_numpy(synth.make_codes(2 * bz, L, V, seed=5).astype(np.int64).reshape(2, bz, L).transpose(1, 0, 2).copy()).cuda()
    prefix = [L, 4, 8, 16]
    tp = torch.from_numpy(np.stack([synth.uniform_f32(f"m/p{k}", (bz,), 30.0) for k in prefix]))
    tn = torch.from_numpy(np.stack([synth.uniform_f32(f"m/n{k}", (bz,), 30.0) for k in prefix]))
    labels = codes[:, 0].contiguous()
    for rate in [float(r) for r in args.rates.split(",")]:
        st = E.TrainState(model, dropout_rate=rate, dropout_seed=1) if rate > 0 else E.TrainState(model)
        if step == "fine-tune":
            def fn():
                E.train_step(model, st, ids, mask, codes, tp, tn, prefix, lr=1e-6)
        else:
            def fn():
                E.seq2seq_train_step(model, st, ids, mask, labels, lr=1e-6)
        r = dict(tag=args.tag, step=step, examples=bz, rate=rate, precision=args.precision, **timed(fn))
        if args.split:
            r["split"] = split(fn)
        print("TIMING " + json.dumps(r), flush=True)
