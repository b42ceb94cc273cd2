#!/usr/bin/env python3
"""Fixture of the cross-encoder's f16 mode (tests/test_xenc_half_host.py, tests/test_gpu_xenc_half.py). Runs on the CPU
with the installed transformers. Data only.

xh_xenc.npz: what the reference's setting — HF ``BertForSequenceClassification`` under ``torch.autocast(dtype=float16)`` —
gives on the recorded pairs, so that a test can hold the f16 mode to the reference's own distance from fp64.

  x1, x2: the models of x1_xenc.npz / x2_xenc.npz rebuilt from their stored weights (num_labels 1, dropout 0, eager
          attention); per batch ``<model>_<key>_fp16``, the logits under CPU fp16 autocast. Inputs and fp64 logits stay in
          the x*_xenc.npz files.
  x3:     the MiniLM-L6-H384 dimensions (hidden 384, 12 heads of 32, d_ff 1536, 6 layers, vocab 200, max_pos 256) with
          weights that are NOT stored: tests/xenc_half_ref.py regenerates them from ripor_amd.utils.synth (seed 303). One
          batch of 8 pairs of lengths 1, 17, 64, 65, 130, 256, 33, 200 (T = 766): ids / types / mask, HF's fp64 and
          fp16-autocast logits, and ``x3_checksum``, the fp64 sum of all weights.

Prints, per model, the bar (max |fp16 autocast - fp64|) and what the torch restatement of the f16 mode
(xenc_half_ref.forward_packed_half) reaches against fp64."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import xenc_half_ref as href  # noqa: E402
import xenc_ref as ref  # noqa: E402


def hf_model(hf_config, sd):
    from transformers import BertConfig, BertForSequenceClassification
    keys = ("hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size", "vocab_size", "max_position_embeddings",
            "type_vocab_size", "layer_norm_eps")
    cfg = BertConfig(num_labels=1, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                     **{k: hf_config[k] for k in keys})
    cfg._attn_implementation = "eager"
    model = BertForSequenceClassification(cfg).eval()
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith(("position_ids", "token_type_ids")) for k in res.missing_keys), res
    return model


def logits(model, ids, types, mask):
    kw = dict(input_ids=torch.from_numpy(ids).long(), token_type_ids=torch.from_numpy(types).long(),
              attention_mask=torch.from_numpy(mask).long())
    with torch.no_grad():
        with torch.autocast("cpu", dtype=torch.float16):
            y16 = model(**kw).logits.view(-1).float()
        y64 = model.double()(**kw).logits.view(-1)
        model.float()
    return y64.numpy(), y16.numpy()


def restated(weights, cfg, b):
    from ripor_amd import engine as E
    pk = E.xenc_pack(torch.from_numpy(b["ids"]), torch.from_numpy(b["types"]), torch.from_numpy(b["mask"]))
    return href.forward_packed_half(weights, cfg, *pk).double().numpy()


def main():
    from ripor_amd import engine as E
    from ripor_amd.modeling.cross_encoder import weights_from_state_dict
    out = {}
    for name in ("x1", "x2"):
        fx = ref.load_fixture(name)
        model = hf_model(fx["hf_config"], fx["state_dict"])
        bar = ours = 0.0
        for key, b in fx["batches"].items():
            y64, y16 = logits(model, b["ids"], b["types"], b["mask"])
            assert np.abs(y64 - b["fp64"]).max() <= 1e-9, (name, key)   # the rebuilt model is the recorded one
            out[f"{name}_{key}_fp16"] = y16
            bar = max(bar, float(np.abs(y16 - b["fp64"]).max()))
            ours = max(ours, float(np.abs(restated(fx["weights"], fx["cfg"], b) - b["fp64"]).max()))
        print(f"{name}: bar max |fp16 autocast - fp64| {bar:.3e}, restatement of the f16 mode {ours:.3e}")
    sd = href.x3_state_dict()
    cfg = E.XencConfig(**href.X3)
    ids, types, mask = href.x3_batch()
    y64, y16 = logits(hf_model(href.x3_hf_config(), sd), ids, types, mask)
    b = dict(ids=ids, types=types, mask=mask, fp64=y64, fp16=y16)
    for f, v in b.items():
        out[f"x3_a_{f}"] = v
    out["x3_checksum"] = np.float64(href.checksum(sd))
    ours = float(np.abs(restated(weights_from_state_dict(sd, cfg), cfg, b) - y64).max())
    print(f"x3: bar max |fp16 autocast - fp64| {float(np.abs(y16 - y64).max()):.3e}, restatement of the f16 mode {ours:.3e}; "
          f"score std {float(y64.std()):.3f}")
    path = os.path.join(HERE, "xh_xenc.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
