"""TEST INFRASTRUCTURE. The CPU oracle (oracle.t5_ref.T5Ref, float32 torch) in training mode: the five kinds of dropout
site of HF ``T5Stack`` — stack input, attention probabilities, sub-block output, the feed-forward's inner activation, stack
output — with the masks of tests/dropout_mask.py multiplied in as constants, so torch autograd differentiates exactly the
function the device step computes (ripor_amd/csrc/dropout.h draws the same masks).

``DropoutRef`` overrides ``encode`` and ``decode_full`` only, so everything written against ``T5Ref`` runs unchanged on it:
``oracle.train_ref.train_step`` (two decoder passes: document 0 = the positive, 1 = the negative, over ONE encoder mask) and
``tests/test_seq2seq_host.seq2seq_grads`` (one decoder pass). Call ``begin(n_docs)`` before each step: decoder pass number k
of the step is document k % n_docs, row b of it sequence b * n_docs + doc.
"""
from __future__ import annotations

import numpy as np
import torch

import dropout_mask as dm
from oracle.t5_ref import NEG_MASK, T5Ref, relative_position_bucket, rmsnorm


class DropoutRef(T5Ref):
    def __init__(self, state_dict, dims, rate: float, seed: int, step: int):
        super().__init__(state_dict, dims)
        self.rate, self.seed, self.step = float(rate), int(seed), int(step)
        self.begin(1)

    def begin(self, n_docs: int):
        self.n_docs, self._dec_calls = int(n_docs), 0

    # ---- masks as constants -------------------------------------------------------------------------------------------------
    def _act(self, x: torch.Tensor, site: int, seqs) -> torch.Tensor:
        if self.rate == 0.0:
            return x
        return x * torch.from_numpy(dm.act_mask(self.rate, self.seed, self.step, site, seqs, x.shape[1], x.shape[2]))

    def _attn_drop(self, prefix, x, kv, bias, site, seqs):
        B, Tq, _ = x.shape
        Tk = kv.shape[1]
        sd, H, dkv = self.sd, self.H, self.dkv
        q = (x @ sd[prefix + ".q.weight"].t()).view(B, Tq, H, dkv).transpose(1, 2)
        k = (kv @ sd[prefix + ".k.weight"].t()).view(B, Tk, H, dkv).transpose(1, 2)
        v = (kv @ sd[prefix + ".v.weight"].t()).view(B, Tk, H, dkv).transpose(1, 2)
        w = torch.softmax((q @ k.transpose(2, 3) + bias).float(), dim=-1)
        if self.rate != 0.0:
            w = w * torch.from_numpy(dm.attn_mask(self.rate, self.seed, self.step, site, seqs, H, Tq, Tk))
        o = (w @ v).transpose(1, 2).reshape(B, Tq, H * dkv)
        return o @ sd[prefix + ".o.weight"].t()

    def _ff_drop(self, prefix, x, site, seqs):
        sd = self.sd
        return self._act(torch.relu(x @ sd[prefix + ".wi.weight"].t()), site, seqs) @ sd[prefix + ".wo.weight"].t()

    # ---- the two stacks -----------------------------------------------------------------------------------------------------
    def encode(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        sd, d = self.sd, self.dims
        Q, Lq = input_ids.shape
        seqs = np.arange(Q)
        x = self._act(sd["shared.weight"][input_ids], dm.site_input(0), seqs)
        pos = torch.arange(Lq)
        bucket = relative_position_bucket(pos[None, :] - pos[:, None], True, d.relative_attention_num_buckets,
                                          d.relative_attention_max_distance)
        tab = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        bias = tab[bucket].permute(2, 0, 1)[None] + torch.where(attention_mask[:, None, None, :] > 0, 0.0, NEG_MASK)
        for i in range(d.num_layers):
            p = f"encoder.block.{i}.layer"
            h = rmsnorm(x, sd[p + ".0.layer_norm.weight"], self.eps)
            x = x + self._act(self._attn_drop(p + ".0.SelfAttention", h, h, bias, dm.site_mid(0, i, 0), seqs), dm.site_sub_out(0, i, 0), seqs)
            h = rmsnorm(x, sd[p + ".1.layer_norm.weight"], self.eps)
            x = x + self._act(self._ff_drop(p + ".1.DenseReluDense", h, dm.site_mid(0, i, 1), seqs), dm.site_sub_out(0, i, 1), seqs)
        return self._act(rmsnorm(x, sd["encoder.final_layer_norm.weight"], self.eps), dm.site_output(0), seqs)

    def decode_full(self, ids: torch.Tensor, enc: torch.Tensor, enc_mask: torch.Tensor) -> torch.Tensor:
        sd, d = self.sd, self.dims
        doc = self._dec_calls % self.n_docs
        self._dec_calls += 1
        seqs = np.arange(ids.shape[0]) * self.n_docs + doc
        x = self._act(self.decoder_inputs_embeds(ids), dm.site_input(1), seqs)
        R, T, _ = x.shape
        pos = torch.arange(T)
        bucket = relative_position_bucket(pos[None, :] - pos[:, None], False, d.relative_attention_num_buckets,
                                          d.relative_attention_max_distance)
        tab = sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        causal = torch.where(pos[None, :] <= pos[:, None], 0.0, NEG_MASK)
        self_bias = tab[bucket].permute(2, 0, 1)[None] + causal[None, None]
        cross_bias = torch.where(enc_mask[:, None, None, :] > 0, 0.0, NEG_MASK)
        for i in range(d.num_decoder_layers):
            p = f"decoder.block.{i}.layer"
            h = rmsnorm(x, sd[p + ".0.layer_norm.weight"], self.eps)
            x = x + self._act(self._attn_drop(p + ".0.SelfAttention", h, h, self_bias, dm.site_mid(1, i, 0), seqs), dm.site_sub_out(1, i, 0), seqs)
            h = rmsnorm(x, sd[p + ".1.layer_norm.weight"], self.eps)
            x = x + self._act(self._attn_drop(p + ".1.EncDecAttention", h, enc, cross_bias, dm.site_mid(1, i, 1), seqs), dm.site_sub_out(1, i, 1), seqs)
            h = rmsnorm(x, sd[p + ".2.layer_norm.weight"], self.eps)
            x = x + self._act(self._ff_drop(p + ".2.DenseReluDense", h, dm.site_mid(1, i, 2), seqs), dm.site_sub_out(1, i, 2), seqs)
        x = self._act(rmsnorm(x, sd["decoder.final_layer_norm.weight"], self.eps), dm.site_output(1), seqs)
        if d.scaleup_output_hidden:
            x = x * (d.d_model ** -0.5)
        return x
