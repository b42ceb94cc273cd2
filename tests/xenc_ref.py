"""Plain-torch restatement of the BERT cross-encoder the HIP path computes: post-LayerNorm encoder, absolute
positions, erf GELU, tanh pooler, one logit. Two forms over the stacked weights of ``engine.xenc_weight_shapes``: padded
with a key mask (what HF computes) and packed (what ``rpr_xenc_score`` computes). Also the loader of the ``x*.npz``
fixtures of tests/golden/make_golden_xenc.py."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"x1": ["a", "b", "c", "d", "e", "f"], "x2": ["a", "b", "c", "d", "f"]}


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _cast(w, dtype):
    return {k: v.to(dtype) for k, v in w.items()}


def forward_padded(w, cfg, ids, types, mask, dtype=torch.float64):
    """ids, types, mask [bz, L] -> logits [bz]. Position ids are the columns; masked columns are no keys."""
    w = _cast(w, dtype)
    ids, types, mask = torch.as_tensor(ids).long(), torch.as_tensor(types).long(), torch.as_tensor(mask)
    bz, L = ids.shape
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    x = w["word_emb"][ids] + w["type_emb"][types] + w["pos_emb"][torch.arange(L)][None]
    x = _ln(x, w["emb_ln_w"], w["emb_ln_b"], cfg.ln_eps)
    neg = torch.zeros((bz, 1, 1, L), dtype=dtype).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    for l in range(cfg.layers):
        qkv = x @ w["qkv_w"][l].T + w["qkv_b"][l]
        q, k, v = (t.reshape(bz, L, nh, dh).transpose(1, 2) for t in qkv.split(H, dim=-1))
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh) + neg, dim=-1)
        ctx = (p @ v).transpose(1, 2).reshape(bz, L, H)
        x = _ln(ctx @ w["ao_w"][l].T + w["ao_b"][l] + x, w["ln1_w"][l], w["ln1_b"][l], cfg.ln_eps)
        ff = _gelu(x @ w["ff1_w"][l].T + w["ff1_b"][l])
        x = _ln(ff @ w["ff2_w"][l].T + w["ff2_b"][l] + x, w["ln2_w"][l], w["ln2_b"][l], cfg.ln_eps)
    pooled = torch.tanh(x[:, 0] @ w["pool_w"].T + w["pool_b"])
    return pooled @ w["cls_w"] + w["cls_b"][0]


def forward_packed(w, cfg, pk_ids, pk_types, pk_pos, seq_off, dtype=torch.float64):
    """The packed form: rows [T], sequence b = rows seq_off[b] .. seq_off[b + 1] - 1 -> logits [bz]."""
    w = _cast(w, dtype)
    ids, types, pos = (torch.as_tensor(t).long() for t in (pk_ids, pk_types, pk_pos))
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    x = _ln(w["word_emb"][ids] + w["type_emb"][types] + w["pos_emb"][pos], w["emb_ln_w"], w["emb_ln_b"], cfg.ln_eps)
    bz = len(seq_off) - 1
    for l in range(cfg.layers):
        qkv = x @ w["qkv_w"][l].T + w["qkv_b"][l]
        ctx = torch.empty_like(x)
        for b in range(bz):
            s, e = int(seq_off[b]), int(seq_off[b + 1])
            q, k, v = (t.reshape(e - s, nh, dh).transpose(0, 1) for t in qkv[s:e].split(H, dim=-1))
            p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
            ctx[s:e] = (p @ v).transpose(0, 1).reshape(e - s, H)
        x = _ln(ctx @ w["ao_w"][l].T + w["ao_b"][l] + x, w["ln1_w"][l], w["ln1_b"][l], cfg.ln_eps)
        ff = _gelu(x @ w["ff1_w"][l].T + w["ff1_b"][l])
        x = _ln(ff @ w["ff2_w"][l].T + w["ff2_b"][l] + x, w["ln2_w"][l], w["ln2_b"][l], cfg.ln_eps)
    first = x[torch.as_tensor(np.asarray(seq_off[:-1])).long()]
    pooled = torch.tanh(first @ w["pool_w"].T + w["pool_b"])
    return pooled @ w["cls_w"] + w["cls_b"][0]


_cache = {}


def load_fixture(name):
    """-> dict(cfg=XencConfig, hf_config=dict, state_dict={HF name: fp32 tensor}, weights=stacked layout,
    batches={key: dict(ids, types, mask, fp64, fp32)}). Loaded once and shared: treat as read-only."""
    if name in _cache:
        return _cache[name]
    from ripor_amd import engine as E
    from ripor_amd.modeling.cross_encoder import weights_from_state_dict
    import json
    z = np.load(os.path.join(GOLDEN, f"{name}_xenc.npz"))
    hf = json.loads(str(z["config_json"]))
    cfg = E.XencConfig(vocab_size=hf["vocab_size"], hidden=hf["hidden_size"], layers=hf["num_hidden_layers"],
                       heads=hf["num_attention_heads"], d_ff=hf["intermediate_size"], max_pos=hf["max_position_embeddings"],
                       type_vocab=hf["type_vocab_size"], ln_eps=hf["layer_norm_eps"])
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    batches = {}
    for key in FIXTURES[name]:
        batches[key] = {f: z[f"{key}_{f}"] for f in ("ids", "types", "mask", "fp64", "fp32")}
    out = dict(cfg=cfg, hf_config=hf, state_dict=sd, weights=weights_from_state_dict(sd, cfg), batches=batches)
    _cache[name] = out
    return out


def write_checkpoint(fx, path, with_position_ids=False):
    """The fixture's model as a checkpoint directory CrossEncoder reads (config.json + model.safetensors)."""
    import json
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(fx["hf_config"], f)
    sd = {k: v.contiguous() for k, v in fx["state_dict"].items()}
    if with_position_ids:
        sd["bert.embeddings.position_ids"] = torch.arange(fx["cfg"].max_pos)[None]
    save_file(sd, os.path.join(path, "model.safetensors"))
    return path
