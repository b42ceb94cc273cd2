"""The cross-encoder teacher (reference modeling/cross_encoder.py:7-34): ``CrossEncoder(model_name_or_path)`` scores
(query, passage) pairs with a BERT ``AutoModelForSequenceClassification`` checkpoint such as
``cross-encoder/ms-marco-MiniLM-L-6-v2`` — here on the HIP path (``engine.xenc_score``), in exact fp32 or,
with ``precision="f16"``, with f16 matrix operands and fp32 accumulation (the reference's fp16 autocast), over a packed
batch in which padding does not exist.

Same surface as the reference class for inference: ``from_pretrained``, ``.to(device)``, ``.eval()``,
``forward(**{"qd_kwargs": ...})`` -> logits [bz], ``rerank_forward(qd_kwargs)`` -> ``{"scores": ...}``. Training the teacher
(``labels`` in the inputs) is not built. The checkpoint is a local directory with ``config.json`` and ``model.safetensors``
or ``pytorch_model.bin`` under HF's BERT tensor names; nothing is downloaded."""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import torch

from .. import engine as E


def read_config(path: str) -> E.XencConfig:
    """config.json -> XencConfig; refuses what the kernels do not compute."""
    cfg_path = os.path.join(path, "config.json")
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"{cfg_path} not found: CrossEncoder reads a local checkpoint directory")
    with open(cfg_path) as fin:
        c = json.load(fin)
    if c.get("model_type") != "bert":
        raise ValueError(f"CrossEncoder: model_type {c.get('model_type')!r} is not built; only 'bert' "
                         "(post-LayerNorm encoder, absolute positions, tanh pooler) is")
    if c.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"CrossEncoder: hidden_act {c.get('hidden_act')!r} is not built; only 'gelu' (the erf form) is")
    if c.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"CrossEncoder: position_embedding_type {c.get('position_embedding_type')!r} is not built; only 'absolute' is")
    return E.XencConfig(vocab_size=int(c["vocab_size"]), hidden=int(c["hidden_size"]), layers=int(c["num_hidden_layers"]),
                        heads=int(c["num_attention_heads"]), d_ff=int(c["intermediate_size"]),
                        max_pos=int(c["max_position_embeddings"]), type_vocab=int(c.get("type_vocab_size", 2)),
                        ln_eps=float(c.get("layer_norm_eps", 1e-12)))


def weights_from_state_dict(sd: Dict[str, torch.Tensor], cfg: E.XencConfig) -> Dict[str, torch.Tensor]:
    """HF BertForSequenceClassification tensors -> the stacked layout of ``engine.xenc_weight_shapes``. An old
    ``bert.embeddings.position_ids`` buffer is ignored; a missing tensor or a classifier that is not [1, hidden] raises."""
    def get(name):
        if name not in sd:
            raise KeyError(f"CrossEncoder: the checkpoint has no tensor {name}")
        return sd[name].detach().to(torch.float32).cpu()

    cls_w = get("classifier.weight")
    if tuple(cls_w.shape) != (1, cfg.hidden):
        raise ValueError(f"CrossEncoder: classifier.weight is {tuple(cls_w.shape)}; a single-logit head [1, {cfg.hidden}] is expected "
                         "(num_labels = 1)")
    emb = "bert.embeddings."
    w = {"word_emb": get(emb + "word_embeddings.weight"), "pos_emb": get(emb + "position_embeddings.weight"),
         "type_emb": get(emb + "token_type_embeddings.weight"), "emb_ln_w": get(emb + "LayerNorm.weight"),
         "emb_ln_b": get(emb + "LayerNorm.bias"), "pool_w": get("bert.pooler.dense.weight"), "pool_b": get("bert.pooler.dense.bias"),
         "cls_w": cls_w.reshape(-1), "cls_b": get("classifier.bias").reshape(-1)}
    per = {k: [] for k in ("qkv_w", "qkv_b", "ao_w", "ao_b", "ln1_w", "ln1_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "ln2_w", "ln2_b")}
    for n in range(cfg.layers):
        p = f"bert.encoder.layer.{n}."
        per["qkv_w"].append(torch.cat([get(p + f"attention.self.{x}.weight") for x in ("query", "key", "value")], dim=0))
        per["qkv_b"].append(torch.cat([get(p + f"attention.self.{x}.bias") for x in ("query", "key", "value")], dim=0))
        per["ao_w"].append(get(p + "attention.output.dense.weight")); per["ao_b"].append(get(p + "attention.output.dense.bias"))
        per["ln1_w"].append(get(p + "attention.output.LayerNorm.weight")); per["ln1_b"].append(get(p + "attention.output.LayerNorm.bias"))
        per["ff1_w"].append(get(p + "intermediate.dense.weight")); per["ff1_b"].append(get(p + "intermediate.dense.bias"))
        per["ff2_w"].append(get(p + "output.dense.weight")); per["ff2_b"].append(get(p + "output.dense.bias"))
        per["ln2_w"].append(get(p + "output.LayerNorm.weight")); per["ln2_b"].append(get(p + "output.LayerNorm.bias"))
    w.update({k: torch.stack(v) for k, v in per.items()})
    return w


class CrossEncoder:
    def __init__(self, model_name_or_path: str, precision: str = "f32"):
        from .t5_generative_retriever import _load_checkpoint
        if precision not in E.XENC_PRECISIONS:
            raise ValueError(f"CrossEncoder: precision {precision!r}; one of {sorted(E.XENC_PRECISIONS)} expected")
        self.precision = precision
        self.name_or_path = model_name_or_path
        self.cfg = read_config(model_name_or_path)
        self._weights = weights_from_state_dict(_load_checkpoint(model_name_or_path), self.cfg)
        for name, shape in E.xenc_weight_shapes(self.cfg).items():
            if tuple(self._weights[name].shape) != tuple(shape):
                raise ValueError(f"CrossEncoder: {name} is {tuple(self._weights[name].shape)}, config.json implies {tuple(shape)}")
        self._model: Optional[E.XencModel] = None
        self.model_args = None   # (reference: incompatible with previous models)

    @classmethod
    def from_pretrained(cls, model_name_or_path: str, precision: str = "f32") -> "CrossEncoder":
        return cls(model_name_or_path, precision=precision)

    def set_precision(self, precision: str) -> "CrossEncoder":
        """``"f32"`` or ``"f16"`` (``engine.XencModel.set_precision``); before ``.to(device)`` it is applied there."""
        if precision not in E.XENC_PRECISIONS:
            raise ValueError(f"CrossEncoder: precision {precision!r}; one of {sorted(E.XENC_PRECISIONS)} expected")
        self.precision = precision
        if self._model is not None:
            self._model.set_precision(precision)
        return self

    def to(self, device) -> "CrossEncoder":
        """Binds the weights on a HIP device (an int is a device index, like the reference's ``model.to(local_rank)``)."""
        ctx = E.Context.get(device)
        if self._model is None or self._model.ctx is not ctx:
            self._model = E.XencModel(ctx, self._weights, self.cfg)
        self._model.set_precision(self.precision)
        return self

    def eval(self) -> "CrossEncoder":
        return self

    @property
    def device(self):
        return None if self._model is None else self._model.ctx.device

    def _scores(self, qd_kwargs) -> torch.Tensor:
        if self._model is None:
            raise E.RiporHipError("CrossEncoder: call .to(device) first; the scoring path has no CPU fallback")
        return E.xenc_score(self._model, qd_kwargs["input_ids"], qd_kwargs.get("token_type_ids"), qd_kwargs["attention_mask"])

    def forward(self, **inputs) -> torch.Tensor:
        if "labels" in inputs:
            raise NotImplementedError("CrossEncoder: training the teacher (labels -> BCE loss) is not built; scoring only")
        return self._scores(inputs["qd_kwargs"])

    __call__ = forward

    def rerank_forward(self, qd_kwargs):
        return {"scores": self._scores(qd_kwargs)}
