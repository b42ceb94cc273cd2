"""Golden vectors of the rank-oriented step (loss_type t5seq_aq_encoder_margin_mse) from the *imported* reference on CPU.

Same rules as make_golden.py (whose helpers this imports): the reference's own ``T5SeqAQEncoderForMarginMSE.forward``
(modeling/t5_generative_retriever.py:857-884), ``MarginMSEforT5SeqAQDataset`` (dataset/dataset.py:552-616) and
``MarginMSEforT5SeqAQCollator`` (dataset/data_collator.py:115-150) run unmodified; what is stored is data — seeds and dims to
regenerate the weights with ripor_amd.utils.synth, the token batches, the teacher scores and the reference's outputs. The
model runs in float64 (``.double()``; HF's T5LayerNorm still takes its variance in float32, as in make_golden_pretrain.py).

Teacher scores and the two conditions on the inputs are make_golden_pretrain.py's: the student's own scores moved by a seeded
3 .. 15 % of the largest |score| in alternating directions, so that every |margin - teacher margin| is at least 1 % of the
largest |score|; every ReLU pre-activation of a real token at least MIN_PREACT from 0. Both are asserted below; seeds were
picked for which the reference alone satisfies them.

Cases: the smtid as long as the model's 8 positions with ragged queries, one of them the single token </s>; 4 codes on a model
of 8 positions (the sub-smtid stage: the codebooks of positions 4 .. 7 receive no gradient, asserted below); input and output
codebooks shared; the gated-GELU feed-forward.

Fixture names start with ``rk_`` (never ``g``, ``f4_``, ``s2s_``, ``drop_``, ``v11_`` or ``pre_``: other tests collect those).

Usage:  python tests/golden/make_golden_rank.py [--only NAME]
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

from make_golden import WordTokenizer, grad_samples, load_reference, synth  # noqa: E402
import make_golden  # noqa: E402
import make_golden_gated  # noqa: E402
from make_golden_pretrain import MIN_PREACT, ragged, watch_relu_inputs  # noqa: E402

RK_CASES = {
    # L = the model's 8 positions; unequal query lengths, the third query is the single token </s>
    "rk_mini_bz4_l8": dict(bz=4, L=8, model_L=8, V=256, seed=1501, q_lens=[9, 4, 1, 6]),
    # 4 codes on a model of 8 positions (full_lng_knp_train_pipline.sh:5-45 at mini size)
    "rk_mini_bz3_l4of8": dict(bz=3, L=4, model_L=8, V=256, seed=1312, q_lens=[5, 11, 3]),
    # decode() reads the INPUT codebooks (reference :821-822)
    "rk_mini_bz3_l8_shared": dict(bz=3, L=8, model_L=8, V=256, seed=1383, q_lens=[7, 2, 10], shared=True),
    "rk_v11_mini_bz3_l8": dict(bz=3, L=8, model_L=8, V=256, seed=1304, q_lens=[6, 12, 3], feed_forward_proj="gated-gelu"),
}


def rk_dims(spec):
    gated = spec.get("feed_forward_proj") == "gated-gelu"
    # the bf16 kernels reduce in tiles of 64 (include/ripor_hip.h: rpr_op_linear_bf16), so make_golden_gated's d_ff of 96 would
    # keep this fixture out of bf16: twice that here (W_in 384 rows, W_out's reduction three tiles), as tests/test_gpu_gated_ff.py
    kw = dict(d_ff=2 * make_golden_gated.D_FF) if gated else {}
    if spec.get("shared"):
        kw["shared_output_input_embeds"] = True
    return synth.mini_dims(L=spec["model_L"], V=spec["V"], **kw), gated


def rk_codes(spec):
    """Seeded smtids, positive rows then negative rows; a negative shares its first two codes with its positive, like the
    hard negatives of beam-search rank data."""
    bz, L = spec["bz"], spec["L"]
    codes = synth.make_codes(2 * bz, L, spec["V"], seed=spec["seed"]).astype(np.int64)
    pos, neg = codes[:bz].copy(), codes[bz:].copy()
    neg[:, :2] = pos[:, :2]
    return pos, neg


def make_rk_case(name, spec, mod):
    bz, L, seed = spec["bz"], spec["L"], spec["seed"]
    dims, gated = rk_dims(spec)
    t0 = time.time()
    sd = synth.make_state_dict(dims, seed=seed, **(dict(feed_forward_proj="gated-gelu") if gated else {}))
    build = make_golden_gated.build_gated_reference_model if gated else make_golden.build_reference_model
    base = build(mod, dims, sd).double()
    base.config.decoding = False
    Cls = mod.T5SeqAQEncoderForMarginMSE
    m = Cls.__new__(Cls)              # the ctor only loads a checkpoint dir; the forward below is the reference's own
    torch.nn.Module.__init__(m)
    m.base_model, m.config, m.loss_fn = base, base.config, torch.nn.MSELoss()
    m.eval()
    q_ids, q_mask = ragged(name, spec["q_lens"], dims.vocab_size, seed)
    pos, neg = rk_codes(spec)
    t = torch.from_numpy
    start = np.full((bz, 1), -1, dtype=np.int64)

    def tq(codes):
        return {"input_ids": t(q_ids), "attention_mask": t(q_mask), "decoder_input_ids": t(np.concatenate([start, codes[:, :-1]], 1))}

    with torch.no_grad():   # per-position student scores from the reference's own hidden states and codebooks
        pos_pp = (base(**tq(pos)).decoder_last_hidden_state * m.decode(t(pos))).sum(-1).numpy()
        neg_pp = (base(**tq(neg)).decoder_last_hidden_state * m.decode(t(neg))).sum(-1).numpy()
    scores = np.stack([pos_pp.sum(-1), neg_pp.sum(-1)], 1)   # [bz, 2]
    top = float(np.abs(scores).max())
    rng = np.random.RandomState(seed)
    sign = np.where(np.arange(bz) % 2 == 0, 1.0, -1.0)
    tp = (scores[:, 0] + sign * rng.uniform(0.03, 0.15, bz) * top).astype(np.float32)
    tn = (scores[:, 1] - sign * rng.uniform(0.03, 0.15, bz) * top).astype(np.float32)
    margin = scores[:, 0] - scores[:, 1]
    assert (np.abs(margin - (tp.astype(np.float64) - tn.astype(np.float64))) >= 0.01 * top).all(), (name, margin, tp, tn, top)
    inputs = {"pos_tokenized_query": tq(pos), "neg_tokenized_query": tq(neg), "pos_doc_encoding": t(pos), "neg_doc_encoding": t(neg),
              "teacher_pos_scores": t(tp).double(), "teacher_neg_scores": t(tn).double()}
    with torch.no_grad():
        if not gated:   # (the gated block's gelu_new has no edge)
            seen, handles = watch_relu_inputs(base, [q_mask, q_mask])
        out = m(**inputs)
        if not gated:
            for h in handles:
                h.remove()
            print(f"[golden] {name}: smallest |feed-forward pre-activation| of a real token {seen['min']:.2e}")
            assert seen["enc_calls"] == 2 * len(base.encoder.block) and seen["min"] >= MIN_PREACT, (name, seen)
        assert set(out) == {"rank"}
        loss = float(out["rank"])
    params = {k: p for k, p in base.named_parameters() if p.requires_grad}
    for p in params.values():
        p.grad = None
    m(**inputs)["rank"].backward()
    grads = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
    for i in range(spec["model_L"]):   # a position past the smtid: its codebooks are never read
        for tab in ("list_decoder_embeds", "list_output_embeds"):
            g = grads.get(f"{tab}.{i}.weight")
            if i >= L:
                assert g is None or not bool(g.any()), (name, tab, i)
    keep = {k: g for k, g in grads.items() if "decoder.embed_tokens" not in k}   # transformers-5.x-only unused table
    gn = sorted(keep)
    out = dict(spec=json.dumps(dict(spec, name=name, dims=dims.__dict__)), loss=np.float64(loss), total_loss=np.float64(loss),
               q_ids=q_ids, q_mask=q_mask, pos_doc_encoding=pos, neg_doc_encoding=neg, teacher_pos_scores=tp, teacher_neg_scores=tn,
               pos_position_scores=pos_pp, neg_position_scores=neg_pp,
               grad_names=np.array(gn), grad_norms=np.array([float(keep[k].norm()) for k in gn]),
               grad_samples=np.concatenate([keep[k].reshape(-1)[torch.from_numpy(grad_samples(k, keep[k].shape))].numpy() for k in gn]),
               grad_sample_counts=np.array([len(grad_samples(k, keep[k].shape)) for k in gn]),
               grad_global_norm=np.float64(float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[golden] {name}: {time.time() - t0:.1f}s loss {loss:.6f}, largest |score| {top:.4g}, {len(gn)} gradient tensors "
          f"({os.path.getsize(path) / 1e3:.1f} KB)")


def rk_files(L=8, seed=0):
    """The inputs of MarginMSEforT5SeqAQDataset in both forms: six example lines over the same candidates (``docids`` to look
    up in docid_to_smtid.json; ``smtids`` of 4 codes for --smtid_as_docid), the queries (raw.tsv) and docid_to_smtid.json."""
    rng = np.random.RandomState(6100 + seed)
    docids = [str(700 + 7 * j) for j in range(9)]
    d2s = {d: [-1] + [int(x) for x in rng.randint(0, 256, size=L)] for d in docids}
    queries = [f"{60 + j}\t {' '.join('w%d' % int(x) for x in rng.randint(0, 50, size=1 + (3 * j) % 7))}  \n" for j in range(6)]
    by_docid, by_smtid = [], []
    for j in range(6):
        pick = [docids[int(i)] for i in rng.permutation(len(docids))[:3 + j % 3]]
        scores = [round(float(x), 4) for x in rng.uniform(-5, 12, size=len(pick))]
        by_docid.append(json.dumps({"qid": str(60 + j), "docids": pick, "scores": scores}))
        by_smtid.append(json.dumps({"qid": str(60 + j), "smtids": ["_".join(str(c) for c in d2s[d][1:5]) for d in pick], "scores": scores}))
    return dict(queries="".join(queries), docid_to_smtid=json.dumps(d2s), examples_docid="\n".join(by_docid) + "\n",
                examples_smtid="\n".join(by_smtid) + "\n")


def write_rk_files(root, files):
    os.makedirs(os.path.join(root, "queries"), exist_ok=True)
    for rel, key in (("queries/raw.tsv", "queries"), ("docid_to_smtid.json", "docid_to_smtid"),
                     ("examples_docid.jsonl", "examples_docid"), ("examples_smtid.jsonl", "examples_smtid")):
        with open(os.path.join(root, rel), "w") as f:
            f.write(files[key])


def make_rk_data_case(name="rk_data"):
    """The reference's OWN dataset and collator on small seeded files, in both forms: items in a fixed index order under a fixed
    ``random.seed`` (the negative is drawn with ``random.sample``) and the collated batch. AutoTokenizer.from_pretrained is
    replaced by make_golden's whitespace tokenizer."""
    import importlib
    import random
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
    files = rk_files()
    for form, max_length in (("docid", 16), ("smtid", 4)):
        with tempfile.TemporaryDirectory() as root:
            write_rk_files(root, files)
            os.makedirs(os.path.join(root, "collection"))     # the reference preloads it and never reads it
            with open(os.path.join(root, "collection", "raw.tsv"), "w") as f:
                f.write("700\tw1 w2\n")
            ds = ds_mod.MarginMSEforT5SeqAQDataset(dataset_path=os.path.join(root, f"examples_{form}.jsonl"),
                                                   document_dir=os.path.join(root, "collection"),
                                                   query_dir=os.path.join(root, "queries"),
                                                   docid_to_smtid_path=os.path.join(root, "docid_to_smtid.json") if form == "docid" else None,
                                                   smtid_as_docid=form == "smtid")
            order = [4, 0, 5, 1, 2, 3, 4]
            random.seed(83)
            items = [ds[i] for i in order]
            batch = dc_mod.MarginMSEforT5SeqAQCollator("unused", max_length=max_length)(items[:5])
            flat = {}
            for key, val in batch.items():
                if isinstance(val, torch.Tensor):
                    flat[key] = val.tolist()
                else:
                    for k, v in val.items():
                        flat[f"{key}.{k}"] = v.tolist()
            cases[form] = dict(order=order, random_seed=83, items=[list(it) for it in items], batch=flat, length=len(ds),
                               max_length=max_length)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, files=np.array(json.dumps(files)), cases=np.array(json.dumps(cases)))
    print(f"[golden] {name}: {len(cases)} cases -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    _gen, mod, _utils, _shim = load_reference()
    for name, spec in RK_CASES.items():
        if args.only and args.only != name:
            continue
        make_rk_case(name, spec, mod)
    if not args.only or args.only == "rk_data":
        make_rk_data_case()


if __name__ == "__main__":
    main()
