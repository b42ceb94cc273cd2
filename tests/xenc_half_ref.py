"""Plain-torch restatement of the cross-encoder's f16 mode (``rpr_xenc_set_precision(RPR_XENC_F16)``), the
third fixture model x3, and the loader of ``tests/golden/xh_xenc.npz`` (tests/golden/make_golden_xenc_half.py).

Where the f16 mode may round, and nowhere else (``_h`` below = round to nearest f16, kept as fp32):

* the operands of the four products of a layer: the hidden states entering QKV and FF1, the weights, the attention
  output entering the output projection, the GELU output entering FF2;
* q | k | v (with their biases) as stored for the attention, the softmax probabilities entering P V, the attention output.

Every product accumulates in fp32; the residual stream, LayerNorm, the softmax, bias additions, GELU, embeddings, pooler and
classifier are fp32. The bar of a model is the reference setting's own error on it: max |HF fp16 autocast - HF fp64| over
the model's recorded pairs (``bar``)."""
import math
import os

import numpy as np
import torch

import xenc_ref as ref

X3 = dict(vocab_size=200, hidden=384, layers=6, heads=12, d_ff=1536, max_pos=256, type_vocab=2, ln_eps=1e-12)
X3_LENGTHS = [1, 17, 64, 65, 130, 256, 33, 200]   # T = 766: six 128-row tiles, the last ragged
X3_SEED = 303
MODELS = ("x1", "x2", "x3")


def _h(x):
    return x.half().float()


def forward_packed_half(w, cfg, pk_ids, pk_types, pk_pos, seq_off):
    """The f16 mode over a packed batch -> fp32 logits [bz]."""
    w = {k: v.float() for k, v in w.items()}
    ids, types, pos = (torch.as_tensor(t).long() for t in (pk_ids, pk_types, pk_pos))
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    x = ref._ln(w["word_emb"][ids] + w["type_emb"][types] + w["pos_emb"][pos], w["emb_ln_w"], w["emb_ln_b"], cfg.ln_eps)
    bz = len(seq_off) - 1
    for l in range(cfg.layers):
        qkv = _h(_h(x) @ _h(w["qkv_w"][l]).T + w["qkv_b"][l])
        ctx = torch.empty_like(x)
        for b in range(bz):
            s, e = int(seq_off[b]), int(seq_off[b + 1])
            q, k, v = (t.reshape(e - s, nh, dh).transpose(0, 1) for t in qkv[s:e].split(H, dim=-1))
            p = _h(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1))
            ctx[s:e] = _h((p @ v).transpose(0, 1).reshape(e - s, H))
        x = ref._ln(ctx @ _h(w["ao_w"][l]).T + w["ao_b"][l] + x, w["ln1_w"][l], w["ln1_b"][l], cfg.ln_eps)
        ff = _h(ref._gelu(_h(x) @ _h(w["ff1_w"][l]).T + w["ff1_b"][l]))
        x = ref._ln(ff @ _h(w["ff2_w"][l]).T + w["ff2_b"][l] + x, w["ln2_w"][l], w["ln2_b"][l], cfg.ln_eps)
    first = x[torch.as_tensor(np.asarray(seq_off[:-1])).long()]
    pooled = torch.tanh(first @ w["pool_w"].T + w["pool_b"])
    return pooled @ w["cls_w"] + w["cls_b"][0]


def x3_hf_config():
    return {"model_type": "bert", "hidden_size": X3["hidden"], "num_attention_heads": X3["heads"], "num_hidden_layers": X3["layers"],
            "intermediate_size": X3["d_ff"], "vocab_size": X3["vocab_size"], "max_position_embeddings": X3["max_pos"],
            "type_vocab_size": X3["type_vocab"], "hidden_act": "gelu", "layer_norm_eps": X3["ln_eps"],
            "position_embedding_type": "absolute"}


def x3_state_dict():
    """x3 under HF's BertForSequenceClassification names. Not stored: tensor ``name`` is the draw
    ``synth.uniform_f32("x3:" + name, shape, sqrt(3), seed=303)`` (unit variance), scaled by the rules of make_golden_xenc.py
    (Linear weights u / sqrt(H), embeddings u, LayerNorm weights 1 + 0.2 u, biases 0.1 u) and rounded to fp16."""
    from ripor_amd.utils import synth
    H, F, V = X3["hidden"], X3["d_ff"], X3["vocab_size"]
    shapes = {"bert.embeddings.word_embeddings.weight": (V, H), "bert.embeddings.position_embeddings.weight": (X3["max_pos"], H),
              "bert.embeddings.token_type_embeddings.weight": (X3["type_vocab"], H), "bert.embeddings.LayerNorm.weight": (H,),
              "bert.embeddings.LayerNorm.bias": (H,)}
    for n in range(X3["layers"]):
        p = f"bert.encoder.layer.{n}."
        for lin, (o, i) in (("attention.self.query", (H, H)), ("attention.self.key", (H, H)), ("attention.self.value", (H, H)),
                            ("attention.output.dense", (H, H)), ("intermediate.dense", (F, H)), ("output.dense", (H, F))):
            shapes[p + lin + ".weight"], shapes[p + lin + ".bias"] = (o, i), (o,)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            shapes[p + ln + ".weight"], shapes[p + ln + ".bias"] = (H,), (H,)
    shapes.update({"bert.pooler.dense.weight": (H, H), "bert.pooler.dense.bias": (H,), "classifier.weight": (1, H),
                   "classifier.bias": (1,)})
    sd = {}
    for name, shape in shapes.items():
        u = torch.from_numpy(synth.uniform_f32("x3:" + name, shape, math.sqrt(3.0), seed=X3_SEED))
        if "LayerNorm.weight" in name:
            v = 1.0 + 0.2 * u
        elif name.endswith(".bias"):
            v = 0.1 * u
        elif "embeddings" in name:
            v = u
        else:
            v = u / H ** 0.5
        sd[name] = v.half().float()
    return sd


def x3_batch():
    """ids, types, mask [8, 256] int32: lengths X3_LENGTHS, token types 0 | 1 at the half, padding = token 0."""
    from ripor_amd.utils import synth
    L, bz = max(X3_LENGTHS), len(X3_LENGTHS)
    ids = synth.randint("x3:ids", (bz, L), 0, X3["vocab_size"], seed=X3_SEED)
    types = np.zeros((bz, L), dtype=np.int64)
    mask = np.zeros((bz, L), dtype=np.int64)
    for b, n in enumerate(X3_LENGTHS):
        mask[b, :n] = 1
        types[b, n // 2:n] = 1
    return (ids * mask).astype(np.int32), types.astype(np.int32), mask.astype(np.int32)


def checksum(sd):
    return float(sum(v.double().sum() for v in sd.values()))


_cache = {}


def load(name):
    """-> dict(cfg, weights (stacked layout), state_dict, hf_config, batches={key: dict(ids, types, mask, fp64, fp16)},
    bar = max |fp16 autocast - fp64| over the model's pairs). Loaded once and shared: treat as read-only."""
    if name in _cache:
        return _cache[name]
    from ripor_amd import engine as E
    from ripor_amd.modeling.cross_encoder import weights_from_state_dict
    z = np.load(os.path.join(ref.GOLDEN, "xh_xenc.npz"))
    if name == "x3":
        cfg = E.XencConfig(**X3)
        sd = x3_state_dict()
        got = checksum(sd)
        assert abs(got - float(z["x3_checksum"])) <= 1e-9 * max(1.0, abs(got)), "the regenerated x3 is not the recorded model"
        out = dict(cfg=cfg, state_dict=sd, hf_config=x3_hf_config(), weights=weights_from_state_dict(sd, cfg),
                   batches={"a": {f: z[f"x3_a_{f}"] for f in ("ids", "types", "mask", "fp64", "fp16")}})
    else:
        fx = ref.load_fixture(name)
        out = dict(cfg=fx["cfg"], state_dict=fx["state_dict"], hf_config=fx["hf_config"], weights=fx["weights"],
                   batches={k: dict(b, fp16=z[f"{name}_{k}_fp16"]) for k, b in fx["batches"].items()})
    out["bar"] = max(float(np.abs(b["fp16"].astype(np.float64) - b["fp64"]).max()) for b in out["batches"].values())
    _cache[name] = out
    return out
