"""Golden vectors of the seq2seq docid step (loss_type t5seq_aq_encoder_seq2seq) from the *imported* reference on CPU.

Same rules as make_golden.py (whose helpers this imports): the reference's own ``T5SeqAQEncoderForSeq2Seq.forward``
(modeling/t5_generative_retriever.py:968-1019), ``Seq2SeqForT5SeqAQDataset`` (dataset/dataset.py:527-550) and
``Seq2SeqForT5SeqAQCollator`` (dataset/data_collator.py:90-113) run unmodified; what is stored is data — seeds and dims
to regenerate the inputs with ripor_amd.utils.synth, and the reference's outputs.

Fixture names start with ``s2s_`` (never ``g`` or ``f4_``: conftest feeds those prefixes to the search and ranking tests).

Usage:  python tests/golden/make_golden_seq2seq.py [--only NAME]
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

from make_golden import (WordTokenizer, build_reference_model, grad_samples, load_reference,  # noqa: E402
                         synth)
import make_golden  # noqa: E402

S2S_CASES = {
    "s2s_mini_bz4_l8": dict(kind="mini", bz=4, L=8, V=256, seed=701),
    "s2s_mini_bz4_l16": dict(kind="mini", bz=4, L=16, V=256, seed=702),
    "s2s_mini_bz4_l32": dict(kind="mini", bz=4, L=32, V=256, seed=703),
    "s2s_mini_bz3_l16_v1024": dict(kind="mini", bz=3, L=16, V=1024, seed=704),
    "s2s_mini_bz4_l8_shared": dict(kind="mini", bz=4, L=8, V=256, seed=705, shared=True),
    "s2s_base_bz4_l32": dict(kind="base", bz=4, L=32, V=256, seed=706),
}


def s2s_batch(dims, bz, L, V, seed):
    """Seeded batch in the layout Seq2SeqForT5SeqAQCollator emits: labels = smtid[1:], decoder_input_ids = smtid[:-1]."""
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=seed, max_len=20)
    labels = synth.make_codes(bz, L, V, seed=seed).astype(np.int64)
    return ids, mask, labels


def make_s2s_case(name, spec, mod):
    kind, bz, L, V, seed = spec["kind"], spec["bz"], spec["L"], spec["V"], spec["seed"]
    kw = dict(shared_output_input_embeds=True) if spec.get("shared") else {}
    dims = synth.mini_dims(L=L, V=V, **kw) if kind == "mini" else synth.t5_base_dims(L=L, V=V, vocab_size=2048, **kw)
    t0 = time.time()
    sd = synth.make_state_dict(dims, seed=seed)
    base = build_reference_model(mod, dims, sd)
    base.config.decoding = False      # T5SeqAQEncoder.__init__: no logits in training
    Cls = mod.T5SeqAQEncoderForSeq2Seq
    m = Cls.__new__(Cls)              # the ctor only loads a checkpoint dir; the forward below is the reference's own
    torch.nn.Module.__init__(m)
    m.base_model, m.config, m.rank_loss, m.multi_vocab_sizes = base, base.config, torch.nn.CrossEntropyLoss(), False
    m.eval()
    ids, mask, labels = s2s_batch(dims, bz, L, V, seed)
    dec_in = np.concatenate([np.full((bz, 1), -1, dtype=np.int64), labels[:, :-1]], axis=1)
    inputs = {"tokenized_query": {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask),
                                  "decoder_input_ids": torch.from_numpy(dec_in)},
              "labels": torch.from_numpy(labels)}
    with torch.no_grad():
        loss = float(m(**inputs)["rank"])
        h = base(**inputs["tokenized_query"]).decoder_last_hidden_state
        logits = m.get_seq_logits(h)
        lp = torch.log_softmax(logits, -1).gather(-1, torch.from_numpy(labels)[..., None])[..., 0].numpy()
        m.multi_vocab_sizes = True        # the per-position form of the loss: the same value with one V everywhere
        loss_multi = float(m(**inputs)["rank"])
        m.multi_vocab_sizes = False
    params = {k: p for k, p in base.named_parameters() if p.requires_grad}
    for p in params.values():
        p.grad = None
    total = m(**inputs)["rank"]
    total.backward()
    grads = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
    keep = {k: g for k, g in grads.items() if "decoder.embed_tokens" not in k}   # transformers-5.x-only unused table
    gn = sorted(keep)
    out = dict(spec=json.dumps(dict(spec, name=name, dims=dims.__dict__)), input_ids=ids, attention_mask=mask, labels=labels,
               loss=np.float64(loss), loss_multi_vocab=np.float64(loss_multi), label_logprobs=lp.astype(np.float32),
               grad_names=np.array(gn), grad_norms=np.array([float(keep[k].double().norm()) for k in gn]),
               grad_samples=np.concatenate([keep[k].reshape(-1)[torch.from_numpy(grad_samples(k, keep[k].shape))].numpy()
                                            for k in gn]).astype(np.float32),
               grad_sample_counts=np.array([len(grad_samples(k, keep[k].shape)) for k in gn]),
               grad_global_norm=np.float64(float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))))
    # one AdamW step after clipping to norm 1.0 (HF Trainer defaults), then the loss on the same batch again
    lr = spec.get("lr", 2e-6)
    opt = torch.optim.AdamW(list(params.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
    before = {k: params[k].detach().clone() for k in gn}
    opt.step()
    out["step_lr"] = np.float64(lr)
    out["param_delta_samples"] = np.concatenate(
        [(params[k].detach() - before[k]).reshape(-1)[torch.from_numpy(grad_samples(k, before[k].shape))].numpy()
         for k in gn]).astype(np.float32)
    with torch.no_grad():
        out["loss_after_step"] = np.float64(float(m(**inputs)["rank"]))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[golden] {name}: {time.time() - t0:.1f}s loss {loss:.6f} -> {float(out['loss_after_step']):.6f} "
          f"({os.path.getsize(path) / 1e3:.1f} KB)")


def s2s_files(root, n_ex=7, L=8, seed=0):
    """The two inputs of Seq2SeqForT5SeqAQDataset: the query -> docid jsonl and docid_to_smtid.json."""
    rng = np.random.RandomState(4321 + L + seed)
    d2s = {}
    for j in range(5):
        d2s[str(2000 + 7 * j)] = [-1] + [int(x) for x in rng.randint(0, 256, size=L)]
    docids = list(d2s)
    lines = [json.dumps({"docid": docids[int(rng.randint(0, len(docids)))],
                         "query": " ".join(f"w{int(x)}" for x in rng.randint(0, 50, size=2 + q))}) for q in range(n_ex)]
    with open(os.path.join(root, "query_to_docid.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "docid_to_smtid.json"), "w") as f:
        json.dump(d2s, f)
    return dict(examples=open(os.path.join(root, "query_to_docid.jsonl")).read(), docid_to_smtid=json.dumps(d2s))


def make_s2s_data_case(name="s2s_data"):
    """The reference's OWN dataset and collator on small seeded files: items in a fixed index order and the collated batch,
    smtid lengths 4 / 8 / 32. AutoTokenizer.from_pretrained is replaced by make_golden's whitespace tokenizer."""
    import importlib
    import tempfile
    ds_mod = importlib.import_module("t5_pretrainer.dataset.dataset")
    dc_mod = importlib.import_module("t5_pretrainer.dataset.data_collator")
    for m_ in (ds_mod, dc_mod):
        assert os.path.realpath(m_.__file__).startswith(make_golden.REF + os.sep), m_.__file__

    class _AT:
        @staticmethod
        def from_pretrained(_path):
            return WordTokenizer()

    dc_mod.AutoTokenizer = _AT
    cases = {}
    for L in (4, 8, 32):
        with tempfile.TemporaryDirectory() as root:
            files = s2s_files(root, L=L)
            ds = ds_mod.Seq2SeqForT5SeqAQDataset(example_path=os.path.join(root, "query_to_docid.jsonl"),
                                                 docid_to_smtid_path=os.path.join(root, "docid_to_smtid.json"))
            order = [3, 0, 6, 1, 2]
            items = [ds[i] for i in order]
            coll = dc_mod.Seq2SeqForT5SeqAQCollator("unused", max_length=5)
            batch = coll(items[:4])
            flat = {f"tokenized_query.{k}": v.tolist() for k, v in batch["tokenized_query"].items()}
            flat["labels"] = batch["labels"].tolist()
            cases[f"L{L}"] = dict(files=files, order=order, items=[list(it) for it in items], batch=flat, length=len(ds), max_length=5)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, cases=np.array(json.dumps(cases)))
    print(f"[golden] {name}: {len(cases)} cases -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    _gen, mod, _utils, _shim = load_reference()
    for name, spec in S2S_CASES.items():
        if args.only and args.only != name:
            continue
        make_s2s_case(name, spec, mod)
    if not args.only or args.only == "s2s_data":
        make_s2s_data_case()


if __name__ == "__main__":
    main()
