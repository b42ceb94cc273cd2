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
         conversion launches are missing from the recorded "other" count)."""
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
CASES = [(f"mini/{p}/{step}", p) for p in PRECISIONS for step in ("lngknp_backward", "seq2seq_backward")] + [("fused/bf16/lngknp_backward", "bf16")]


def _job(ctx, E, synth, dims, bz, seed, **queries):
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=seed), dims)
    L, V = len(dims.decoder_vocab_sizes), dims.decoder_vocab_sizes[0]
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=seed, **queries)
    t = torch.from_numpy
    codes = t(synth.randint("train_bits.codes", (bz, 2, L), 0, V, seed=seed))
    tp = t(synth.uniform_f32("train_bits.tp", (2, bz), 4.0, seed=seed))
    tn = t(synth.uniform_f32("train_bits.tn", (2, bz), 4.0, seed=seed + 1))
    return dict(model=model, state=E.TrainState(model), ids=t(ids), mask=t(mask), codes=codes, tp=tp, tn=tn, prefix=[L, L // 2])


def _record(ctx, E, job, step):
    ex = E.GradExchange(job["state"].grads, dry_run=True)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        if step == "lngknp_backward":
            losses = E.lngknp_backward(job["model"], job["state"], job["ids"], job["mask"], job["codes"], job["tp"], job["tn"], job["prefix"],
                                       exchange=ex)
        else:
            losses = E.seq2seq_backward(job["model"], job["state"], job["ids"], job["mask"], job["codes"][:, 0].contiguous(), exchange=ex)
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "train_bits.json"))
    args = ap.parse_args()
    from ripor_amd import engine as E
    records = record_all(E.Context.get(0))
    with open(args.out, "w") as f:
        json.dump(dict(commit=args.commit, cases=records), f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in records.items():
        print(f"[train bits] {k}: grads {v['grads_sha256'][:16]}, {len(v['buckets'])} buckets, launches {v['launches']}")
    print(f"[train bits] wrote {args.out} ({os.path.getsize(args.out)} bytes) at {args.commit}")


if __name__ == "__main__":
    main()
