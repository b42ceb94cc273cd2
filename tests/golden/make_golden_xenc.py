#!/usr/bin/env python3
"""Fixtures of the cross-encoder teacher (tests/test_xenc_host.py, tests/test_gpu_xenc.py). Runs on the CPU.

x1_xenc.npz / x2_xenc.npz: a seeded HF ``BertForSequenceClassification`` (num_labels = 1) from the installed transformers,
its weights, padded input batches and HF's logits in fp64 (``model.double()``) and in fp32. Data only.

The default init (std 0.02) gives every pair the same score to three digits, so the weights are drawn instead: Linear
weights std 1 / sqrt(hidden), embeddings std 1, LayerNorm weights 1 + 0.2 N(0, 1), every bias 0.1 N(0, 1). To halve the
files the drawn values are rounded to fp16 BEFORE the model sees them and stored as fp16: the stored numbers are exactly
the model's fp32 weights.

  x1: hidden 64, 2 heads of 32, 2 layers, d_ff 96, vocab 200, max_pos 512
  x2: hidden 128, 2 heads of 64, 2 layers, d_ff 160, vocab 200, max_pos 192
Batches: a) one sequence of length 1; b) 13 sequences around the 16-row MFMA block and the 64-row tile; c) 127 / 128 / 129;
d) 70 sequences of 1..5 tokens (offsets across blocks); e) x1 only: 512 and 7; f) 4 rows padded to 24, two of them with a
masked column in the middle, token types 0 / 1 (packing must keep the original position ids).

c10_rerank_callers.json: the reference's callers on a 3-query toy input with fixed fake scores — the preprocess script, the
dataset's triple order (CrossEncRerankForSamePrefixPair), Reranker.triple_ids_to_json_output per 2-rank shard and the
``_2`` merge, imported in place from the reference checkout through make_golden.py's shim (needs that checkout;
``torch.cuda.device_count`` is pinned to the number of shards for the merge's assertion)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

MODELS = {
    "x1": dict(hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=96, vocab_size=200,
               max_position_embeddings=512, seed=101),
    "x2": dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=160, vocab_size=200,
               max_position_embeddings=192, seed=202),
}
LENGTHS = {"a": [1], "b": [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 40], "c": [127, 128, 129],
           "d": [1 + (i * 7) % 5 for i in range(70)], "e": [512, 7]}


def make_model(spec):
    from transformers import BertConfig, BertForSequenceClassification
    spec = dict(spec)
    seed = spec.pop("seed")
    cfg = BertConfig(type_vocab_size=2, num_labels=1, hidden_act="gelu", hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, **spec)
    cfg._attn_implementation = "eager"
    model = BertForSequenceClassification(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    H = cfg.hidden_size
    with torch.no_grad():
        for name, p in model.named_parameters():
            n = torch.randn(p.shape, generator=g)
            if "LayerNorm.weight" in name:
                v = 1.0 + 0.2 * n
            elif name.endswith(".bias"):
                v = 0.1 * n
            elif "embeddings" in name:
                v = n
            else:
                v = n / H ** 0.5
            p.copy_(v.half().float())
    return cfg, model


def make_batch(key, lengths, vocab, seed, pad_to=None, holes=()):
    g = torch.Generator().manual_seed(seed)
    L = pad_to or max(lengths)
    bz = len(lengths)
    ids = torch.randint(0, vocab, (bz, L), generator=g)
    types = torch.zeros((bz, L), dtype=torch.long)
    mask = torch.zeros((bz, L), dtype=torch.long)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
        types[b, n // 2:n] = 1   # query | passage
    for b, col in holes:
        mask[b, col] = 0
    ids = ids * mask   # padding = token 0, like a tokenizer's pad id
    return ids, types, mask


def gen_model(name):
    cfg, model = make_model(MODELS[name])
    out = {"config_json": np.array(json.dumps({k: v for k, v in cfg.to_dict().items() if k in (
        "model_type", "hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size", "vocab_size",
        "max_position_embeddings", "type_vocab_size", "hidden_act", "layer_norm_eps", "position_embedding_type")}
        | {"model_type": "bert", "position_embedding_type": "absolute"}))}
    for k, v in model.state_dict().items():
        if k.endswith("position_ids") or k.endswith("token_type_ids"):
            continue
        assert (v.half().float() == v).all()
        out["w:" + k] = v.half().numpy()
    batches = {k: make_batch(k, v, cfg.vocab_size, 1000 + i) for i, (k, v) in enumerate(LENGTHS.items())
               if not (k == "e" and cfg.max_position_embeddings < 512)}
    batches["f"] = make_batch("f", [24, 20, 24, 9], cfg.vocab_size, 1999, pad_to=24, holes=((0, 11), (1, 5)))
    dev = 0.0
    for key, (ids, types, mask) in batches.items():
        with torch.no_grad():
            y32 = model(input_ids=ids, token_type_ids=types, attention_mask=mask).logits.view(-1)
            y64 = model.double()(input_ids=ids, token_type_ids=types, attention_mask=mask).logits.view(-1)
            model.float()
        out[f"{key}_ids"], out[f"{key}_types"], out[f"{key}_mask"] = (t.numpy().astype(np.int32) for t in (ids, types, mask))
        out[f"{key}_fp64"], out[f"{key}_fp32"] = y64.numpy(), y32.numpy()
        dev = max(dev, float((y32.double() - y64).abs().max()))
        print(f"{name}/{key}: bz {len(y64)}, score std {float(y64.std()) if len(y64) > 1 else 0:.3f}, "
              f"max |fp32 - fp64| {float((y32.double() - y64).abs().max()):.2e}")
    path = os.path.join(HERE, f"{name}_xenc.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KB, max |fp32 - fp64| {dev:.2e}")


# ---- c10: the reference's callers on a toy input ---------------------------------------------------------------------
TOY_RANKDATA = {
    "q7": {"3_1": {"d10": 4.0, "d11": 3.5}, "3_2": {}, "5_0": {"d12": 1.0}},
    "q2": {"9_9": {"d13": 2.0, "d10": 1.5, "d14": 0.5}},
    "q5": {"1_1": {"d11": 9.0}, "1_2": {"d15": 8.0, "d12": 7.0}},
}


def fake_score(qid, docid, smtid):
    return float(int(qid[1:]) * 100 + int(docid[1:]) + 0.25 * int(smtid.split("_")[1]))


def gen_c10():
    import runpy
    import tempfile
    import make_golden
    import importlib
    import importlib.machinery
    import types
    make_golden.load_reference()   # the shim, and the reference's t5_pretrainer in place of this repository's alias package
    try:
        import transformers.trainer  # noqa: F401  (as make_golden.load_reference_evaluate: before the faiss stub exists)
    except Exception:
        pass
    for name in ("faiss", "pytrec_eval"):   # imported by the reference's modules, untouched by what runs here: empty stubs
        if name not in sys.modules:
            m_ = types.ModuleType(name)
            m_.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m_.RelevanceEvaluator = object
            sys.modules[name] = m_
    ds_mod = importlib.import_module("t5_pretrainer.dataset.dataset")
    rr_mod = importlib.import_module("t5_pretrainer.tasks.reranker")
    ref_rerank = importlib.import_module("t5_pretrainer.rerank")
    for m_ in (ds_mod, rr_mod, ref_rerank):
        assert os.path.realpath(m_.__file__).startswith(make_golden.REF + os.sep), m_.__file__
    CrossEncRerankForSamePrefixPair, Reranker = ds_mod.CrossEncRerankForSamePrefixPair, rr_mod.Reranker
    out = {"rankdata": TOY_RANKDATA, "world": 2}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "qid_smtid_rankdata.json"), "w") as f:
            json.dump(TOY_RANKDATA, f)
        argv, sys.argv = sys.argv, ["x", "--root_dir", tmp]
        try:
            runpy.run_path(os.path.join(make_golden.REF, "t5_pretrainer", "aq_preprocess",
                                        "argparse_from_qid_smtid_rank_to_qid_smtid_docids.py"), run_name="__main__")
        finally:
            sys.argv = argv
        with open(os.path.join(tmp, "qid_smtid_docids.train.json")) as f:
            docids = json.load(f)
        out["qid_smtid_docids"] = docids
        with open(os.path.join(tmp, "queries.tsv"), "w") as f:
            for q in docids:
                f.write(f"{q}\tquery {q}\n")
        with open(os.path.join(tmp, "raw.tsv"), "w") as f:
            for d in range(10, 16):
                f.write(f"d{d}\tdoc d{d}\n")
        shards_dir = os.path.join(tmp, "shards")
        os.makedirs(shards_dir)
        out["shards"] = []
        for rank in range(2):
            sampled = {qid: docids[qid] for i, qid in enumerate(docids) if i % 2 == rank}   # rerank.py:597-600
            ds = CrossEncRerankForSamePrefixPair(sampled, os.path.join(tmp, "queries.tsv"), os.path.join(tmp, "raw.tsv"))
            triples = [list(ds[i]["triple_id"]) for i in range(len(ds))]
            scores = [fake_score(*t) for t in triples]
            shard = json.loads(json.dumps(Reranker.triple_ids_to_json_output(scores, [tuple(t) for t in triples])))
            out["shards"].append({"rank": rank, "triples": triples, "scores": scores, "output": shard})
            with open(os.path.join(shards_dir, f"qid_smtid_docids_teacher_score_{rank}.train.json"), "w") as f:
                json.dump(shard, f)
        shard_files = sorted(os.listdir(shards_dir))

        class A:
            out_dir = shards_dir
        count, torch.cuda.device_count = torch.cuda.device_count, lambda: 2
        try:
            ref_rerank.cross_encoder_rerank_for_qid_smtid_docids_2(A)
        finally:
            torch.cuda.device_count = count
        out["shard_files"] = shard_files
        out["after_merge_files"] = sorted(os.listdir(shards_dir))
        with open(os.path.join(shards_dir, "qid_smtid_docids_teacher_score.train.json")) as f:
            merged = json.load(f)
        # the merge walks os.listdir in directory order: per (qid, smtid) the rows are one shard's, so only the key order of
        # the merged dict depends on it (the tests compare it as a dict). Everything else keeps its order in the file.
        out["merged"] = merged
    path = os.path.join(HERE, "c10_rerank_callers.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    what = sys.argv[1:] or ["x1", "x2", "c10"]
    for w in what:
        gen_c10() if w == "c10" else gen_model(w)
