"""Golden vectors of the two training steps WITH dropout, from the *imported* reference on CPU.

Same rules as make_golden.py (whose helpers this imports). The reference classes ``T5SeqAQEncoderForLngKnpMarginMSE`` and
``T5SeqAQEncoderForSeq2Seq`` run unmodified in ``train()`` mode at ``dropout_rate`` 0.1, as the reference's trainer runs them
(tasks/trainer.py:221). torch's RNG stream cannot be matched by a stateless device mask, so for the duration of the forward
``torch.nn.functional.dropout`` is replaced by a function that multiplies by OUR mask (tests/dropout_mask.py, the numpy
restatement of ripor_amd/csrc/dropout.h): HF's call order inside one ``T5ForDocIDGeneration.forward`` is mapped to the site
ids — encoder input, per block (attention probabilities, sub-block output, relu(h Wi^T), sub-block output), encoder output,
then the decoder likewise with its three sub-blocks. The k-th forward of a step is document k % n_docs; its encoder sites
repeat the first forward's (one encoder mask per query: the device computes the encoder once), its decoder rows are sequence
b * n_docs + doc. What is stored is data: seeds and dims to regenerate the inputs, rate / seed / step of the masks, and the
reference's losses, per-position scores and gradients.

Fixture names start with ``drop_`` (never ``g``, ``f4_`` or ``s2s_``: other tests enumerate those prefixes).

Usage:  python tests/golden/make_golden_dropout.py [--only NAME]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import build_reference_model, grad_samples, load_reference, synth  # noqa: E402
import dropout_mask as dm  # noqa: E402

RATE, SEED, STEP = 0.1, 0x1234_5678_9ABC_DEF1, 7
PREFIX_KEYS = {8: ["", "smtid_4_"], 16: ["", "smtid_4_", "smtid_8_"]}

CASES = {
    "drop_f4_bz3_l8": dict(step="lngknp", bz=3, L=8, V=256, seed=811),
    "drop_f4_bz3_l16": dict(step="lngknp", bz=3, L=16, V=256, seed=812),
    "drop_f4_bz3_l8_shared": dict(step="lngknp", bz=3, L=8, V=256, seed=815, shared=True),
    "drop_s2s_bz3_l8": dict(step="seq2seq", bz=3, L=8, V=256, seed=814),
}


class MaskInjector:
    """Stands in for torch.nn.functional.dropout while a reference model runs in train() mode."""

    def __init__(self, dims, rate, seed, step, n_docs):
        self.dims, self.rate, self.seed, self.step, self.n_docs = dims, rate, seed, step, n_docs
        self.forwards, self.queue, self.calls = 0, [], 0

    def _stack_sites(self, dec, layers, nsub):
        out = [("act", dm.site_input(dec), dec)]
        for i in range(layers):
            for j in range(nsub):
                ff = j == nsub - 1
                out.append(("act" if ff else "attn", dm.site_mid(dec, i, j), dec))
                out.append(("act", dm.site_sub_out(dec, i, j), dec))
        return out + [("act", dm.site_output(dec), dec)]

    def begin_forward(self, *_):
        assert not self.queue, f"{len(self.queue)} dropout sites of the previous forward were never reached"
        self.doc = self.forwards % self.n_docs
        self.forwards += 1
        self.queue = self._stack_sites(0, self.dims.num_layers, 2) + self._stack_sites(1, self.dims.num_decoder_layers, 3)

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        assert abs(p - self.rate) < 1e-12, p
        kind, site, dec = self.queue.pop(0)
        self.calls += 1
        seqs = np.arange(x.shape[0]) * (self.n_docs if dec else 1) + (self.doc if dec else 0)
        if kind == "attn":
            assert x.dim() == 4, (kind, site, tuple(x.shape))
            m = dm.attn_mask(self.rate, self.seed, self.step, site, seqs, x.shape[1], x.shape[2], x.shape[3])
        else:
            assert x.dim() == 3, (kind, site, tuple(x.shape))
            m = dm.act_mask(self.rate, self.seed, self.step, site, seqs, x.shape[1], x.shape[2])
        return x * torch.from_numpy(m)


def train_mode(base, rate):
    """model.train() at ``rate``: build_reference_model builds at rate 0 (the other fixtures), so every dropout gets its p here."""
    base.config.dropout_rate = rate
    for mod_ in base.modules():
        if isinstance(mod_, torch.nn.Dropout):
            mod_.p = rate
        elif isinstance(getattr(mod_, "dropout", None), float):
            mod_.dropout = rate
    base.train()


def make_case(name, spec, mod):
    bz, L, V, seed = spec["bz"], spec["L"], spec["V"], spec["seed"]
    kw = dict(shared_output_input_embeds=True) if spec.get("shared") else {}
    dims = synth.mini_dims(L=L, V=V, **kw)
    t0 = time.time()
    sd = synth.make_state_dict(dims, seed=seed)
    base = build_reference_model(mod, dims, sd)
    base.config.decoding = False
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=seed, mean_len=9, std_len=3, min_len=5, max_len=13)
    assert len(set(mask.sum(1).tolist())) > 1, "unequal query lengths wanted (padding)"
    start = np.full((bz, 1), -1, dtype=np.int64)

    def tq(codes):
        return {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask),
                "decoder_input_ids": torch.from_numpy(np.concatenate([start, codes[:, :-1]], axis=1))}

    lngknp = spec["step"] == "lngknp"
    out = dict(input_ids=ids, attention_mask=mask, rate=np.float64(RATE), mask_seed=np.uint64(SEED), mask_step=np.uint64(STEP))
    if lngknp:
        Cls = mod.T5SeqAQEncoderForLngKnpMarginMSE
        m = Cls.__new__(Cls)
        torch.nn.Module.__init__(m)
        m.base_model, m.config, m.loss_fn = base, base.config, torch.nn.MSELoss()
        codes = synth.make_codes(2 * bz, L, V, seed=seed).astype(np.int64)
        pos, neg = codes[:bz], codes[bz:]
        teacher = {f"{k}teacher_{side}_scores": synth.uniform_f32(f"drop/{name}/{k}{side}", (bz,), 30.0, seed)
                   for k in PREFIX_KEYS[L] for side in ("pos", "neg")}
        inputs = {"pos_tokenized_query": tq(pos), "neg_tokenized_query": tq(neg), "pos_doc_encoding": torch.from_numpy(pos),
                  "neg_doc_encoding": torch.from_numpy(neg)}
        inputs.update({k: torch.from_numpy(v) for k, v in teacher.items()})
        out.update(pos_doc_encoding=pos, neg_doc_encoding=neg, **teacher)
        n_docs = 2
    else:
        Cls = mod.T5SeqAQEncoderForSeq2Seq
        m = Cls.__new__(Cls)
        torch.nn.Module.__init__(m)
        m.base_model, m.config, m.rank_loss, m.multi_vocab_sizes = base, base.config, torch.nn.CrossEntropyLoss(), False
        labels = synth.make_codes(bz, L, V, seed=seed).astype(np.int64)
        inputs = {"tokenized_query": tq(labels), "labels": torch.from_numpy(labels)}
        out.update(labels=labels)
        n_docs = 1
    train_mode(base, RATE)
    m.train()
    inj = MaskInjector(dims, RATE, SEED, STEP, n_docs)
    hook = base.register_forward_pre_hook(inj.begin_forward)
    real = torch.nn.functional.dropout
    torch.nn.functional.dropout = inj
    try:
        params = {k: p for k, p in base.named_parameters() if p.requires_grad}
        for p in params.values():
            p.grad = None
        losses = m(**inputs)
        names = sorted(losses)
        total = sum(losses[k] for k in names)
        total.backward()
        with torch.no_grad():      # the per-position scores of the same masks (the forwards restart at document 0)
            assert inj.forwards % n_docs == 0
            if lngknp:
                ph = base(**tq(pos)).decoder_last_hidden_state
                nh = base(**tq(neg)).decoder_last_hidden_state
                out["pos_position_scores"] = (ph * m.decode(torch.from_numpy(pos))).sum(-1).numpy().astype(np.float32)
                out["neg_position_scores"] = (nh * m.decode(torch.from_numpy(neg))).sum(-1).numpy().astype(np.float32)
            else:
                h = base(**inputs["tokenized_query"]).decoder_last_hidden_state
                lp = torch.log_softmax(m.get_seq_logits(h), -1).gather(-1, torch.from_numpy(labels)[..., None])[..., 0]
                out["label_logprobs"] = lp.numpy().astype(np.float32)
        assert not inj.queue
    finally:
        torch.nn.functional.dropout = real
        hook.remove()
    per_forward = 4 + 4 * dims.num_layers + 6 * dims.num_decoder_layers   # input + output of each stack, two sites per sub-block
    assert inj.calls == per_forward * inj.forwards, (inj.calls, per_forward, inj.forwards)
    grads = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None and "decoder.embed_tokens" not in k}
    gn = sorted(grads)
    out.update(spec=json.dumps(dict(spec, name=name, dims=dims.__dict__)), loss_names=np.array(names),
               losses=np.array([float(losses[k]) for k in names], dtype=np.float64), total_loss=np.float64(float(total)),
               grad_names=np.array(gn), grad_norms=np.array([float(grads[k].double().norm()) for k in gn]),
               grad_samples=np.concatenate([grads[k].reshape(-1)[torch.from_numpy(grad_samples(k, grads[k].shape))].numpy()
                                            for k in gn]).astype(np.float32),
               grad_sample_counts=np.array([len(grad_samples(k, grads[k].shape)) for k in gn]),
               grad_global_norm=np.float64(float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[golden] {name}: {time.time() - t0:.1f}s losses {dict((k, float(losses[k])) for k in names)}, {inj.calls} masked "
          f"dropout calls -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.set_num_threads(1)
    _, mod, _, _ = load_reference()
    for name, spec in CASES.items():
        if args.only and name != args.only:
            continue
        make_case(name, spec, mod)


if __name__ == "__main__":
    main()
