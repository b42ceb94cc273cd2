#!/usr/bin/env python3
"""Record of what the training step (csrc/train_api.hip) launches and computes, for comparing two builds of the library
after a host-side refactor: a fixed list of eager calls with the library profile on; per call the profile records without
their time fields (launches, flops, bytes per kernel class), the (offset, numel) sequence of the gradient buckets handed
over where a bucket hook is given, and a sha256 of every output: losses, label log-probabilities, the flat gradient
buffer, and the parameters plus both AdamW moments after rpr_adamw_step. JSON; two builds agree when their files are
equal byte for byte. Synthetic inputs only (ripor_amd.utils.synth); the calls run in this order on ONE context, so the
side stream's set rotation and pending marks carry from each call into the next.

Which case reaches which route of the weight-gradient products (Bwd::dxdw_*, WGradSide):
  mini/*      12 decoder + 2 encoder layers of t5-base width, d_ff 256, bz 3: f32 (both products on the main stream), f16x2
              (per-product route, rotating sets) and bf16 (grouped route: the first product of a layer finds the group
              empty, the others join it; the feed-forward fusion is off, fused_ok false). Entry points: lngknp_backward
              without and with a bucket hook (GradExchange dry run), seq2seq_forward alone, seq2seq_backward without and
              with the hook, train_step twice on one context (rotation and pending marks across passes), then a step on a
              second model (the bf16 weight-cache table is rebuilt) and the first model again.
  base/*      t5-base dims, bz 128, L 32 (R = 8192 rows: the decoder's feed-forward dX products have 32 x 12 = 384 >= 200
              tiles, fused_ok true): in bf16 the dX product of Wo leaves the next product's dY converted (the pre
              hand-over); seq2seq_backward at R = 4096 (192 tiles: grouped, not fused).
  wide/*      24 decoder layers of d_model 1024 (16 heads of 64), one encoder layer: the cross-K/V product has
              xld = 49152, 192 x 4 = 768 tiles > MAX_TILES: in bf16 it leaves the group for the per-product route with the
              forward's saved X^T and the cached W^T.
  tallff/*    d_ff 20480 at d_model 768, R = 768 rows: Wo's and Wi's weight gradients have 240 tiles each, so Wi's does not
              fit the group Wo's opened (480 > MAX_TILES): the open group is flushed and Wi's starts the next one; fused_ok
              is true (3 x 80 = 240 tiles) and the reservation of the pre slot is refused for the same reason.
  switch/*    the precision changes between steps on one context and one model: bf16 -> f32 -> f16x2 -> bf16.

Usage: tools/train_equivalence.py --out OUT.json [--only PREFIX]"""
import hashlib
import json
import os
import sys

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


class Job:
    """A model, its optimizer state and one fixed batch."""

    def __init__(self, ctx, dims, bz, seed, vocab, **queries):
        self.model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=seed), dims)
        self.state = E.TrainState(self.model)
        L, V = len(dims.decoder_vocab_sizes), dims.decoder_vocab_sizes[0]
        ids, mask = synth.make_queries(bz, vocab_size=vocab, seed=seed, **queries)
        t = torch.from_numpy
        self.ids, self.mask = t(ids), t(mask)
        self.codes = t(synth.randint("train_equivalence.codes", (bz, 2, L), 0, V, seed=seed))
        self.labels = self.codes[:, 0].contiguous()
        self.prefix = [L, L // 2]
        self.tp = t(synth.uniform_f32("train_equivalence.tp", (2, bz), 4.0, seed=seed))
        self.tn = t(synth.uniform_f32("train_equivalence.tn", (2, bz), 4.0, seed=seed + 1))

    def lngknp(self, hook=False):
        ex = E.GradExchange(self.state.grads, dry_run=True) if hook else None
        losses = E.lngknp_backward(self.model, self.state, self.ids, self.mask, self.codes, self.tp, self.tn, self.prefix, exchange=ex)
        return self._done(dict(losses=losses, grads=self.state.grads), ex)

    def s2s_forward(self):
        loss, lp = E.seq2seq_forward(self.model, self.ids, self.mask, self.labels)
        return dict(loss=loss, label_logprobs=lp)

    def s2s_backward(self, hook=False):
        ex = E.GradExchange(self.state.grads, dry_run=True) if hook else None
        loss = E.seq2seq_backward(self.model, self.state, self.ids, self.mask, self.labels, exchange=ex)
        return self._done(dict(loss=loss, grads=self.state.grads), ex)

    def step(self):
        losses = E.train_step(self.model, self.state, self.ids, self.mask, self.codes, self.tp, self.tn, self.prefix, lr=1e-4)
        params = {}   # every packed tensor once, in the order the model lists them (not by address: that moves from run to run)
        for _, t, _ in self.model.named_device_params():
            params.setdefault(t.data_ptr(), t)
        return dict(losses=losses, grads=self.state.grads, exp_avg=self.state.exp_avg, exp_avg_sq=self.state.exp_avg_sq,
                    grad_norm=self.state.grad_norm, params=torch.cat([t.reshape(-1).float() for t in params.values()]))

    @staticmethod
    def _done(outs, ex):
        if ex is not None:
            ex.finish()
            outs["buckets"] = [list(b) for b in ex.history]
        return outs


def record_calls(ctx, out_path, only):
    records = {}

    def record(name, fn):
        if only and not name.startswith(only):
            return
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            outs = fn()
            torch.cuda.synchronize()
            prof = ctx.profile_get()
        finally:
            ctx.profile_enable(False)
        ctx.status(clear=True)
        buckets = outs.pop("buckets", None)
        records[name] = dict(
            profile={k: {f: v[f] for f in ("launches", "flops", "bytes")} for k, v in prof.items()},
            buckets=buckets,
            sha256={k: digest(v) for k, v in outs.items()})
        print(name, sum(v["launches"] for v in prof.values()), "launches", flush=True)

    mini_dims = synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=256)
    for prec in ("f32", "f16x2", "bf16"):
        ctx.set_precision(prec)
        mini = Job(ctx, mini_dims, 3, 31, 512, max_len=14)
        record(f"mini/{prec}/lngknp_backward", mini.lngknp)
        record(f"mini/{prec}/lngknp_backward_buckets", lambda: mini.lngknp(hook=True))
        record(f"mini/{prec}/seq2seq_forward", mini.s2s_forward)
        record(f"mini/{prec}/seq2seq_backward", mini.s2s_backward)
        record(f"mini/{prec}/seq2seq_backward_buckets", lambda: mini.s2s_backward(hook=True))
        record(f"mini/{prec}/train_step_1", mini.step)
        record(f"mini/{prec}/train_step_2", mini.step)
        other = Job(ctx, synth.mini_dims(L=8, V=256, enc_layers=1, d_ff=128), 2, 32, 512, max_len=10)
        record(f"mini/{prec}/second_model_step", other.step)
        record(f"mini/{prec}/first_model_again", mini.lngknp)
        del mini, other

    base_dims = synth.t5_base_dims(L=32, V=256, vocab_size=2048)
    ctx.set_precision("f16x2")
    base = Job(ctx, base_dims, 128, 5, 2048, mean_len=16, std_len=5, min_len=6, max_len=64)
    record("base/f16x2/lngknp_backward", base.lngknp)
    ctx.set_precision("bf16")
    record("base/bf16/lngknp_backward", base.lngknp)
    record("base/bf16/lngknp_backward_buckets", lambda: base.lngknp(hook=True))
    record("base/bf16/seq2seq_backward", base.s2s_backward)
    record("base/bf16/train_step_1", base.step)
    record("base/bf16/train_step_2", base.step)
    del base

    wide_dims = synth.ModelDims(vocab_size=512, d_model=1024, d_kv=64, d_ff=256, num_layers=1, num_decoder_layers=24,
                                num_heads=16, decoder_vocab_sizes=[256] * 8)
    for prec in ("f16x2", "bf16"):
        ctx.set_precision(prec)
        wide = Job(ctx, wide_dims, 4, 33, 512, max_len=14)
        record(f"wide/{prec}/lngknp_backward_buckets", lambda: wide.lngknp(hook=True))
        record(f"wide/{prec}/train_step", wide.step)
        del wide

    tall_dims = synth.ModelDims(vocab_size=512, d_ff=20480, num_layers=1, num_decoder_layers=2, decoder_vocab_sizes=[256] * 8)
    ctx.set_precision("bf16")
    tall = Job(ctx, tall_dims, 48, 35, 512, max_len=14)
    record("tallff/bf16/lngknp_backward", tall.lngknp)
    record("tallff/bf16/train_step", tall.step)
    del tall

    sw = Job(ctx, mini_dims, 3, 34, 512, max_len=14)
    for i, prec in enumerate(("bf16", "f32", "f16x2", "bf16")):
        ctx.set_precision(prec)
        record(f"switch/{i}_{prec}/train_step", sw.step)
    ctx.set_precision("f16x2")
    with open(out_path, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
    print("wrote", out_path, len(records), "calls")


if __name__ == "__main__":
    record_calls(E.Context.get(0), arg("--out") or "train_equivalence.json", arg("--only"))
