"""TEST INFRASTRUCTURE. Float64 restatement of the dense first-stage step (loss_type t5seq_pretrain_margin_mse; reference
T5SeqPretrainEncoder.forward, modeling/t5_generative_retriever.py:708-757, with one decoder position) on the CPU oracle's
``T5Ref.encode`` / ``decode_full``, and the ``pre_*`` fixtures of tests/golden/make_golden_pretrain.py.

The weights are float64. The one place where HF's T5 leaves the model dtype, the variance of T5LayerNorm (always float32), is
float32 here as well (``oracle.t5_ref.rmsnorm``); the softmax runs in the dtype of the scores, as HF's eager attention does
(``_attn`` below: ``T5Ref._attn`` casts the scores to float32, a no-op for its float32 weights). So the restatement meets a
float64 run of the reference to 1e-9.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from gated_ref import GatedT5Ref
from oracle.t5_ref import T5Ref

PRE_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("pre_") and f.endswith(".npz") and f != "pre_data.npz")
GROUPS = ("q", "pd", "nd")   # queries, positive documents, negative documents: the order of the device step's [3, bz, Lt]


class PreGolden:
    def __init__(self, name):
        from ripor_amd.utils import synth
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.spec = json.loads(str(self.z["spec"]))
        self.dims = synth.ModelDims(**self.spec["dims"])
        self.bz, self.seed = self.spec["bz"], self.spec["seed"]
        self.kind = self.spec.get("feed_forward_proj", "relu")
        self.state_dict = synth.make_state_dict(self.dims, seed=self.seed, feed_forward_proj=self.kind)

    def tok(self, g):
        t = torch.from_numpy
        return {"input_ids": t(self.z[g + "_ids"]), "attention_mask": t(self.z[g + "_mask"]),
                "decoder_input_ids": torch.full((self.bz, 1), -1, dtype=torch.long)}

    def inputs(self):
        """The batch as MarginMSEforPretrainCollator emits it."""
        return {"tokenized_pos_query": self.tok("q"), "tokenized_neg_query": self.tok("q"), "tokenized_pos_doc": self.tok("pd"),
                "tokenized_neg_doc": self.tok("nd"), "teacher_pos_score": torch.from_numpy(self.z["teacher_pos"]),
                "teacher_neg_score": torch.from_numpy(self.z["teacher_neg"])}

    def stacked(self):
        """(input_ids, attention_mask) [3, bz, Lt] int64: the three groups padded to the longest."""
        Lt = max(self.z[g + "_ids"].shape[1] for g in GROUPS)
        ids, mask = np.zeros((3, self.bz, Lt), np.int64), np.zeros((3, self.bz, Lt), np.int64)
        for k, g in enumerate(GROUPS):
            n = self.z[g + "_ids"].shape[1]
            ids[k, :, :n], mask[k, :, :n] = self.z[g + "_ids"], self.z[g + "_mask"]
        return ids, mask

    def ref_model(self, cls=None):
        return ref64(self.state_dict, self.dims, self.kind, cls)


class _Attn64:
    """``T5Ref._attn`` with the softmax in the dtype of the scores."""

    def _attn(self, prefix, x, kv, bias):
        B, Tq, _ = x.shape
        Tk = kv.shape[1]
        sd, H, dkv = self.sd, self.H, self.dkv
        q = (x @ sd[prefix + ".q.weight"].t()).view(B, Tq, H, dkv).transpose(1, 2)
        k = (kv @ sd[prefix + ".k.weight"].t()).view(B, Tk, H, dkv).transpose(1, 2)
        v = (kv @ sd[prefix + ".v.weight"].t()).view(B, Tk, H, dkv).transpose(1, 2)
        scores = q @ k.transpose(2, 3) + bias
        w = torch.softmax(scores, dim=-1)
        o = (w @ v).transpose(1, 2).reshape(B, Tq, H * dkv)
        return o @ sd[prefix + ".o.weight"].t()


def ref64(state_dict, dims, kind="relu", cls=None):
    """The CPU oracle (ReLU or gated feed-forward) with float64 weights."""
    base = cls or (GatedT5Ref if kind == "gated-gelu" else T5Ref)
    model = type(base.__name__ + "64", (_Attn64, base), {})(state_dict, dims)
    model.sd = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in state_dict.items()}
    return model


def dense_reps(model, input_ids, attention_mask):
    """rep(x) = decoder_last_hidden_state[:, 0] of the encoder plus one decoder position fed with the start embedding."""
    ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    mask = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)
    enc = model.encode(ids, mask)
    return model.decode_full(torch.full((ids.shape[0], 1), -1, dtype=torch.long), enc, mask)[:, 0]


def _margin_mse(q, qn, dp, dn, teacher_pos, teacher_neg):
    scores = torch.stack([(q * dp).sum(-1), (qn * dn).sum(-1)], dim=1)
    margin = scores[:, 0] - scores[:, 1]
    teacher = torch.as_tensor(np.asarray(teacher_pos)).to(margin.dtype) - torch.as_tensor(np.asarray(teacher_neg)).to(margin.dtype)
    return torch.nn.functional.mse_loss(margin, teacher), scores, torch.cat([q, dp, dn], 0)


def dense_margin_mse(model, groups, teacher_pos, teacher_neg):
    """groups: [(ids, mask)] of the queries, the positive and the negative documents (each padded to its own longest, or all to
    one length: padding changes nothing). Returns (loss, scores [bz, 2], reps [3 bz, d]).
    The query goes through the model twice, as the reference's tokenized_pos_query and tokenized_neg_query do: the same values
    forward, but in the backward each pass rounds the gradient of its float32 layer-norm variances on its own — 1e-7 of a gradient
    tensor's scale against one pass that receives the sum (what the device step does, far inside its bars)."""
    q, dp, dn = (dense_reps(model, ids, mask) for ids, mask in groups)
    return _margin_mse(q, dense_reps(model, *groups[0]), dp, dn, teacher_pos, teacher_neg)


def dense_margin_mse_stacked(model, input_ids, attention_mask, teacher_pos, teacher_neg):
    """The same loss as the device step computes it: ONE pass over the 3 bz sequences of input_ids / attention_mask [3, bz, Lt]
    (sequence s of the pass = row s of the flattened batch: the coordinates dropout masks are drawn by), the query encoded once."""
    ids, mask = np.asarray(input_ids), np.asarray(attention_mask)
    q, dp, dn = dense_reps(model, ids.reshape(-1, ids.shape[-1]), mask.reshape(-1, ids.shape[-1])).chunk(3)
    return _margin_mse(q, q, dp, dn, teacher_pos, teacher_neg)


def dense_grads(model, fn, *args):
    """Autograd of fn = dense_margin_mse or dense_margin_mse_stacked: (loss, grads: state-dict name -> tensor, global norm)."""
    for t in model.sd.values():
        t.requires_grad_(True)
        t.grad = None
    loss, _, _ = fn(model, *args)
    loss.backward()
    grads = {k: t.grad.detach().clone() for k, t in model.sd.items() if t.grad is not None}
    for t in model.sd.values():
        t.requires_grad_(False)
        t.grad = None
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    return float(loss.detach()), grads, gn


def golden_groups(g: PreGolden):
    return [(g.z[k + "_ids"], g.z[k + "_mask"]) for k in GROUPS]
