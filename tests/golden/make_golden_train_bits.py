"""Records tests/golden/train_bits.json: what the training step (csrc/train_api.hip) computes and launches on the MI355X for
the batches of CASES, bit for bit (tests/test_gpu_train_bits.py replays them and compares exactly). Per call: the sha256 of
the flat gradient buffer, the losses as float32 bit patterns, the (offset, numel) list of the gradient buckets in hand-over
order, and the launch count per kernel class of the library profile. Needs the GPU and a built library; run by hand, and
only from a commit whose gradients are trusted by other means (tests/test_gpu_train.py, test_gpu_seq2seq.py):

  python tests/golden/make_golden_train_bits.py --commit $(git rev-parse HEAD)

The file names that commit. A change that alters the training arithmetic or its launch sequence on purpose re-records it with
this script and says so; a restructuring never does.

CASES, the smallest that reach every branch of the layer walk:
  mini   2 encoder + 12 decoder layers of t5-base width, d_ff 256, bz 3, Lq <= 14, L 8 (T = 42 and R = 48 rows, both padded to
         64), in f32, f16x2 and bf16: the ranking step (two docs per query) and the seq2seq step (one), both with the dry-run
         bucket hook. Two encoder layers and two / three sub-blocks per layer (an even and an odd count) exercise the dx / dx2
         ping-pong and the layer indexing of both stacks.
  fused  bf16, d_ff 3072, 1 encoder + 2 decoder layers, bz 68, every query 64 tokens, L 32, two docs: R = T = 4352 = 17 * 256
         rows, so the feed-forward products have 17 * 12 = 204 >= 200 tiles of 256 x 256 and fused_ok holds in both stacks: the
         forward hand-over of the FF block's bf16 operands and the backward's pre-converted gradient are on the path (their
         conversion launches are missing from the recorded "other" count).

ROUTE_CASES, one per attention route of the step that the cases above do not reach (csrc/attn_route.h, the training sites;
DESIGN.md §5b'). All in f32 (no attention launcher reads the precision), both steps each: the ranking step with two docs of L = 8
(n = 16 decoder rows per query) and the seq2seq step (n = 8). The dropout cases run at rate 0.1 with a fixed seed and global step.
  drop         the mini batch: the resident backward kernels with the mask (never the MFMA tile) and both resident drop-forwards,
               causal and bidirectional
  d128         3 heads of 128, d_model 256, 1 + 2 layers, bz 3, Lq <= 13 (tests/test_gpu_heads128.py, model A): the <., 128> kernels
  long129      3 heads of 64, 1 + 2 layers, bz 2, queries of 129 and 70 tokens (the key mask matters): the encoder's self-attention
               in tiles, cross-attention resident at a long Lq (n = 16: 23 139 floats)
  long256      the same at 256 and 100 tokens: self-attention and the ranking step's cross-attention in tiles (n = 16: 43 840
               floats, past the carve), the seq2seq step's cross-attention resident (n = 8)
Each carries the commit it was recorded at in its own "commit" key (--extend: the earlier records are replayed first, must come
out as the file has them and are kept byte for byte; every new case is recorded twice and must give the same record)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PRECISIONS = ("f32", "f16x2", "bf16")
STEPS = ("lngknp_backward", "seq2seq_backward")
ROUTE_CASES = ("drop", "d128", "d128drop", "long129", "long129drop", "long256", "long256drop")
CASES = ([(f"mini/{p}/{step}", p) for p in PRECISIONS for step in STEPS] + [("fused/bf16/lngknp_backward", "bf16")] +
         [(f"{c}/f32/{step}", "f32") for c in ROUTE_CASES for step in STEPS])
DROP = dict(dropout_rate=0.1, dropout_seed=0x1234_5678_9ABC_DEF1)   # tests/test_gpu_dropout.py
DROP_STEP = 7


def _job(ctx, E, synth, dims, bz, seed, drop=False, lens=None, **queries):
    """``lens``: the token count of every query, the first the longest (else what make_queries draws); ``drop``: the step at DROP."""
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=seed), dims)
    L, V = len(dims.decoder_vocab_sizes), dims.decoder_vocab_sizes[0]
    if lens:
        queries = dict(fixed_len=lens[0])
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=seed, **queries)
    for i, n in enumerate(lens or ()):   # a shorter query: cut, with the end-of-sequence id last
        ids[i, n - 1], ids[i, n:], mask[i, n:] = 1, 0, 0
    t = torch.from_numpy
    codes = t(synth.randint("train_bits.codes", (bz, 2, L), 0, V, seed=seed))
    tp = t(synth.uniform_f32("train_bits.tp", (2, bz), 4.0, seed=seed))
    tn = t(synth.uniform_f32("train_bits.tn", (2, bz), 4.0, seed=seed + 1))
    return dict(model=model, state=E.TrainState(model, **(DROP if drop else {})), step=DROP_STEP if drop else None, ids=t(ids), mask=t(mask),
                codes=codes, tp=tp, tn=tn, prefix=[L, L // 2])


def _record(ctx, E, job, step):
    ex = E.GradExchange(job["state"].grads, dry_run=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        if step == "lngknp_backward":
            losses = E.lngknp_backward(job["model"], job["state"], job["ids"], job["mask"], job["codes"], job["tp"], job["tn"], job["prefix"],
                                       exchange=ex, global_step=job["step"])
        else:
            losses = E.seq2seq_backward(job["model"], job["state"], job["ids"], job["mask"], job["codes"][:, 0].contiguous(), exchange=ex,
                                        global_step=job["step"])
        ex.finish()
        torch.cuda.synchronize()
        prof = ctx.profile_get()
    finally:
        ctx.profile_enable(False)
    ctx.status(clear=True)
    grads = np.ascontiguousarray(job["state"].grads.detach().cpu().numpy())
    assert np.isfinite(grads).all()
    return dict(grads_sha256=hashlib.sha256(grads.tobytes()).hexdigest(),
                loss_bits=[int(v) for v in losses.detach().cpu().numpy().astype(np.float32, copy=False).view(np.uint32)],
                buckets=[[int(o), int(n)] for o, n in ex.history],
                launches={k: int(v["launches"]) for k, v in sorted(prof.items()) if v["launches"]})


def _route_jobs(ctx, E, synth):
    """(case, job) of ROUTE_CASES, one at a time."""
    heads128 = synth.mini_dims(L=8, V=64, enc_layers=1, d_ff=128, d_model=256, d_kv=128, num_heads=3, num_decoder_layers=2)
    heads64 = synth.mini_dims(L=8, V=64, enc_layers=1, d_ff=128, d_model=256, d_kv=64, num_heads=3, num_decoder_layers=2)
    yield "drop", _job(ctx, E, synth, synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=256), 3, 41, drop=True, max_len=14)
    for drop in (False, True):
        tail = "drop" if drop else ""
        yield "d128" + tail, _job(ctx, E, synth, heads128, 3, 43, drop=drop, mean_len=9, std_len=3, min_len=5, max_len=13)
        yield "long129" + tail, _job(ctx, E, synth, heads64, 2, 44, drop=drop, lens=[129, 70])
        yield "long256" + tail, _job(ctx, E, synth, heads64, 2, 45, drop=drop, lens=[256, 100])


def record_routes(ctx):
    """-> {case name: record} of ROUTE_CASES, in f32."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    before = ctx.get_precision()
    out = {}
    try:
        ctx.set_precision("f32")
        for case, job in _route_jobs(ctx, E, synth):
            for step in STEPS:
                out[f"{case}/f32/{step}"] = _record(ctx, E, job, step)
    finally:
        ctx.set_precision(before)
        ctx.lib.rpr_set_train_dropout(ctx.handle, 0.0, 0, 0)
    return out


def record_all(ctx, precisions=PRECISIONS):
    """-> {case name: record} for every case of CASES whose precision is in ``precisions``; the calls run in CASES order."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    before = ctx.get_precision()
    out = {}
    try:
        for prec in precisions:
            ctx.set_precision(prec)
            mini = _job(ctx, E, synth, synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=256), 3, 41, max_len=14)
            for step in ("lngknp_backward", "seq2seq_backward"):
                out[f"mini/{prec}/{step}"] = _record(ctx, E, mini, step)
            del mini
        if "bf16" in precisions:
            ctx.set_precision("bf16")
            dims = synth.ModelDims(vocab_size=512, num_layers=1, num_decoder_layers=2, decoder_vocab_sizes=[256] * 32)
            fused = _job(ctx, E, synth, dims, 68, 42, fixed_len=64)
            out["fused/bf16/lngknp_backward"] = _record(ctx, E, fused, "lngknp_backward")
    finally:
        ctx.set_precision(before)
    if "f32" in precisions:
        out.update(record_routes(ctx))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "train_bits.json"))
    ap.add_argument("--extend", action="store_true",
                    help="keep the records --out holds (they must reproduce) and its commit; add the cases it lacks, each with --commit")
    args = ap.parse_args()
    from ripor_amd import engine as E
    ctx = E.Context.get(0)
    records = record_all(ctx)
    again = record_routes(ctx)
    assert all(records[k] == v for k, v in again.items()), [k for k, v in again.items() if records[k] != v]
    commit = args.commit
    if args.extend:
        with open(args.out) as f:
            old = json.load(f)
        moved = [k for k, v in old["cases"].items() if records[k] != {f: v[f] for f in records[k]}]
        assert not moved, f"records of {old['commit']} that this build does not reproduce: {moved}"
        commit = old["commit"]
        records = {k: old["cases"].get(k) or dict(v, commit=args.commit) for k, v in records.items()}
    with open(args.out, "w") as f:
        json.dump(dict(commit=commit, cases=records), f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in records.items():
        print(f"[train bits] {k}: grads {v['grads_sha256'][:16]}, {len(v['buckets'])} buckets, launches {v['launches']}")
    print(f"[train bits] wrote {args.out} ({os.path.getsize(args.out)} bytes) at {args.commit}")


if __name__ == "__main__":
    main()
