"""Host-side mirror of the reference's model objects for the generative-retrieval path.

Same names and call surface as reference t5_pretrainer/modeling/t5_generative_retriever.py
(``T5forDocIDConfig`` :45-67, ``T5ForDocIDGeneration`` :70-512, ``T5SeqAQEncoder`` :772-855) as far as
``evaluate.py``'s retrieve tasks use them: ``from_pretrained`` of an HF checkpoint directory,
``.base_model``, ``.config.decoder_vocab_sizes``, ``.eval()``, ``.to(device)``, ``.device``,
``save_pretrained``. The objects only hold weights; all arithmetic of the search happens in
libripor_hip.so (ripor_amd/engine.py binds the weights to an ``rpr_model``). There is no PyTorch
forward here and no CPU fallback: calling the search without a HIP device raises.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch


# config.feed_forward_proj values the device paths run: T5 v1.0's DenseReluDense and v1.1's T5DenseGatedActDense with gelu_new
FEED_FORWARD_KINDS = ("relu", "gated-gelu")


class T5forDocIDConfig:
    """Fields of the reference config (T5Config + docid extras, reference :45-65)."""

    model_type = "t5"

    def __init__(self, decoder_vocab_sizes: Optional[List[int]] = None, decoding: bool = False,
                 decoder_start_token_path: str = "./t5_decoder_start_token_embeds/t5-base.npy",
                 apply_decoder_t5_stack: bool = False, scaleup_output_hidden: bool = False,
                 shared_output_input_embeds: bool = True, vocab_size: int = 32128, d_model: int = 768,
                 d_kv: int = 64, d_ff: int = 3072, num_layers: int = 12, num_decoder_layers: Optional[int] = None,
                 num_heads: int = 12, relative_attention_num_buckets: int = 32,
                 relative_attention_max_distance: int = 128, layer_norm_epsilon: float = 1e-6,
                 feed_forward_proj: str = "relu", dropout_rate: float = 0.1, **kwargs):
        self.decoder_vocab_sizes = list(decoder_vocab_sizes) if decoder_vocab_sizes is not None else [256] * 32
        self.decoding = decoding
        self.decoder_start_token_path = decoder_start_token_path
        self.apply_decoder_t5_stack = apply_decoder_t5_stack
        self.scaleup_output_hidden = scaleup_output_hidden
        self.shared_output_input_embeds = shared_output_input_embeds
        self.vocab_size, self.d_model, self.d_kv, self.d_ff = vocab_size, d_model, d_kv, d_ff
        self.num_layers = num_layers
        self.num_decoder_layers = num_decoder_layers if num_decoder_layers is not None else num_layers
        self.num_heads = num_heads
        self.relative_attention_num_buckets = relative_attention_num_buckets
        self.relative_attention_max_distance = relative_attention_max_distance
        self.layer_norm_epsilon = layer_norm_epsilon
        self.feed_forward_proj = feed_forward_proj
        # T5Config.dropout_rate (HF default 0.1): what the reference trains with (model.train()); unused by inference, applied by
        # the training steps only on request (main.py --dropout=config)
        self.dropout_rate = float(dropout_rate)
        self.tie_word_embeddings = False
        self.max_decoder_length = len(self.decoder_vocab_sizes)
        self.extra = dict(kwargs)
        assert self.apply_decoder_t5_stack == False  # noqa: E712  (reference :67)
        if feed_forward_proj not in FEED_FORWARD_KINDS:
            raise ValueError(f"feed_forward_proj={feed_forward_proj!r} is not supported: the feed-forward block is one of "
                             f"{', '.join(repr(k) for k in FEED_FORWARD_KINDS)}")

    @property
    def is_gated_ff(self) -> bool:
        """wo(gelu_new(wi_0 x) * wi_1 x) (T5 v1.1, Flan-T5, mT5) instead of wo(relu(wi x))."""
        return self.feed_forward_proj == "gated-gelu"

    @classmethod
    def from_pretrained(cls, path: str) -> "T5forDocIDConfig":
        with open(os.path.join(path, "config.json")) as f:
            d = json.load(f)
        d.pop("model_type", None)
        d.pop("tie_word_embeddings", None)
        d.pop("max_decoder_length", None)
        return cls(**d)

    @classmethod
    def from_dims(cls, dims) -> "T5forDocIDConfig":
        """From ripor_amd.utils.synth.ModelDims (synthetic checkpoints)."""
        return cls(decoder_vocab_sizes=dims.decoder_vocab_sizes, vocab_size=dims.vocab_size, d_model=dims.d_model,
                   d_kv=dims.d_kv, d_ff=dims.d_ff, num_layers=dims.num_layers,
                   num_decoder_layers=dims.num_decoder_layers, num_heads=dims.num_heads,
                   relative_attention_num_buckets=dims.relative_attention_num_buckets,
                   relative_attention_max_distance=dims.relative_attention_max_distance,
                   layer_norm_epsilon=dims.layer_norm_epsilon,
                   shared_output_input_embeds=dims.shared_output_input_embeds,
                   scaleup_output_hidden=dims.scaleup_output_hidden,
                   feed_forward_proj=getattr(dims, "feed_forward_proj", "relu"))

    def to_dict(self) -> dict:
        d = {k: v for k, v in self.__dict__.items() if k != "extra"}
        d.update(self.extra)
        d["model_type"] = self.model_type
        return d

    def save_pretrained(self, path: str):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=2)


_IGNORED_KEYS = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight",
                 "decoder.block.0.layer.1.EncDecAttention.relative_attention_bias.weight")


def expected_keys(cfg: T5forDocIDConfig) -> List[str]:
    """State-dict keys the search path reads. A gated feed-forward has wi_0 (the gate) and wi_1 where
    the ReLU block has wi (HF keeps the module name DenseReluDense for both)."""
    wi = ["wi_0", "wi_1"] if cfg.is_gated_ff else ["wi"]
    keys = ["shared.weight", "encoder.final_layer_norm.weight", "decoder.final_layer_norm.weight", "start_token_embed",
            "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
            "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    for i in range(cfg.num_layers):
        p = f"encoder.block.{i}.layer"
        keys += [f"{p}.0.SelfAttention.{w}.weight" for w in "qkvo"]
        keys += [f"{p}.0.layer_norm.weight", f"{p}.1.layer_norm.weight",
                 *[f"{p}.1.DenseReluDense.{w}.weight" for w in wi], f"{p}.1.DenseReluDense.wo.weight"]
    for i in range(cfg.num_decoder_layers):
        p = f"decoder.block.{i}.layer"
        keys += [f"{p}.0.SelfAttention.{w}.weight" for w in "qkvo"]
        keys += [f"{p}.1.EncDecAttention.{w}.weight" for w in "qkvo"]
        keys += [f"{p}.0.layer_norm.weight", f"{p}.1.layer_norm.weight", f"{p}.2.layer_norm.weight",
                 *[f"{p}.2.DenseReluDense.{w}.weight" for w in wi], f"{p}.2.DenseReluDense.wo.weight"]
    for i in range(len(cfg.decoder_vocab_sizes)):
        keys.append(f"list_decoder_embeds.{i}.weight")
        if not cfg.shared_output_input_embeds:
            keys.append(f"list_output_embeds.{i}.weight")
    return keys


def _load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    st = os.path.join(path, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st)
    pt = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(pt):
        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")


def plain_t5_state_dict(sd: Dict[str, torch.Tensor], cfg: T5forDocIDConfig, decoder_start_token_path: str,
                        codebook_seed: int = 0) -> Dict[str, torch.Tensor]:
    """The state dict of a docid-generation model on top of a plain HF T5 checkpoint (reference T5ForDocIDGeneration.__init__
    :80-135 followed by from_pretrained of "t5-base"): the T5 tensors as they are, ``start_token_embed`` [1, 1, d_model] from the
    ``.npy`` file, the codebooks N(0, 1) like a fresh ``nn.Embedding`` from a generator seeded with ``codebook_seed``."""
    if not decoder_start_token_path or not os.path.exists(decoder_start_token_path):
        raise FileNotFoundError(f"a plain T5 checkpoint has no start_token_embed: decoder_start_token_path "
                                f"{decoder_start_token_path!r} must name the .npy file that holds it, [1, 1, {cfg.d_model}] "
                                f"(pass decoder_start_token_path, or set it in config.json)")
    start = torch.from_numpy(np.load(decoder_start_token_path)).float()
    if start.numel() != cfg.d_model:
        raise ValueError(f"{decoder_start_token_path}: {tuple(start.shape)}, expected [1, 1, {cfg.d_model}]")
    out = {k: v for k, v in sd.items() if k.split(".")[0] in ("shared", "encoder", "decoder")}
    out["start_token_embed"] = start.reshape(1, 1, cfg.d_model)
    gen = torch.Generator().manual_seed(int(codebook_seed))
    for i, V in enumerate(cfg.decoder_vocab_sizes):
        out[f"list_decoder_embeds.{i}.weight"] = torch.randn((int(V), cfg.d_model), generator=gen)
        if not cfg.shared_output_input_embeds:
            out[f"list_output_embeds.{i}.weight"] = torch.randn((int(V), cfg.d_model), generator=gen)
    return out


class T5ForDocIDGeneration:
    """Weights of the docid-generation T5 (reference :70-135) bound lazily to the HIP engine."""

    def __init__(self, config: T5forDocIDConfig, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        self.config = config
        self._sd: Dict[str, torch.Tensor] = {}
        self._device = torch.device("cpu")
        self._engine_model = None
        if (config.num_decoder_layers, config.num_heads) not in ((12, 12), (24, 16), (24, 32)):
            # t5-base, t5-large, t5-3b (32 heads of d_kv = 128): reference :116-135
            raise ValueError("the model with decoer layers {} is not supported.".format(config.num_decoder_layers))
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # -- weights --
    def load_state_dict(self, state_dict, strict: bool = True):
        sd = {}
        for k, v in state_dict.items():
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v)
            sd[k] = v.detach().to(torch.float32)
        need = expected_keys(self.config)
        missing = [k for k in need if k not in sd]
        unexpected = [k for k in sd if k not in need and k not in _IGNORED_KEYS]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                               f"unexpected {unexpected[:8]}")
        self._sd = {k: sd[k] for k in need if k in sd}
        self._engine_model = None
        return missing, unexpected

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._sd)

    @classmethod
    def from_pretrained(cls, model_name_or_path: str, config: Optional[T5forDocIDConfig] = None):
        config = config if config is not None else T5forDocIDConfig.from_pretrained(model_name_or_path)
        return cls(config, _load_checkpoint(model_name_or_path))

    def save_pretrained(self, save_dir: str):
        self.config.save_pretrained(save_dir)
        torch.save({k: v.cpu() for k, v in self._sd.items()}, os.path.join(save_dir, "pytorch_model.bin"))

    # -- module-like surface used by evaluate.py --
    def eval(self):
        return self

    def to(self, device):
        device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if device != self._device:
            self._device = device
            self._engine_model = None
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else torch.cuda.current_device()))

    @property
    def device(self) -> torch.device:
        return self._device

    def engine_model(self):
        """The rpr_model bound to this object's weights on its device (built on first use)."""
        if self._engine_model is None:
            from .. import engine as E
            if self._device.type != "cuda":
                raise E.RiporHipError("T5ForDocIDGeneration is on the CPU: move it to a HIP device with .to(local_rank) "
                                      "(the search path has no CPU fallback)")
            ctx = E.Context.get(self._device)
            self._engine_model = E.DeviceModel(ctx, self._sd, self.config)
        return self._engine_model

    def __call__(self, *a, **k):
        raise NotImplementedError("only the constrained beam search path is built: use "
                                  "ripor_amd.tasks.generation.generate_for_constrained_prefix_beam_search")


class T5SeqAQEncoder:
    """reference :772-855 (inference surface only)."""

    def __init__(self, model_name_or_path, shared_output_input_embeds=None, multi_vocab_sizes=None):
        config = T5forDocIDConfig.from_pretrained(model_name_or_path)
        config.decoding = False
        if shared_output_input_embeds is not None:
            assert shared_output_input_embeds in [False, True]
            config.shared_output_input_embeds = shared_output_input_embeds
        self.base_model = T5ForDocIDGeneration.from_pretrained(model_name_or_path, config=config)
        self.config = config
        self.model_args = None

    @classmethod
    def from_pretrained(cls, model_name_or_path=None, shared_output_input_embeds=None, multi_vocab_sizes=False):
        return cls(model_name_or_path, shared_output_input_embeds, multi_vocab_sizes)

    @classmethod
    def from_synthetic(cls, dims, seed=None):
        """Random-init checkpoint of the given dims (no network / no pretrained weights here)."""
        from ..utils import synth
        obj = cls.__new__(cls)
        obj.config = T5forDocIDConfig.from_dims(dims)
        sd = synth.make_state_dict(dims) if seed is None else synth.make_state_dict(dims, seed=seed)
        obj.base_model = T5ForDocIDGeneration(obj.config, sd)
        obj.model_args = None
        return obj

    def eval(self):
        return self

    def to(self, device):
        self.base_model.to(device)
        return self

    def save_pretrained(self, save_dir):
        self.base_model.save_pretrained(save_dir)

    def query_encode(self, **inputs):
        """reference :786-792: ``decoder_last_hidden_state[:, 0, :]`` of the encoder plus one decoder position fed with the
        start embedding (``decoder_input_ids = [-1]``, which is all a query collection carries). -> fp32 [bz, d_model]."""
        from .. import engine as E
        dec = inputs.get("decoder_input_ids")
        if dec is not None and (dec.dim() != 2 or dec.shape[1] != 1 or bool((dec != -1).any())):
            raise ValueError("query_encode embeds with one decoder position fed by the start embedding: decoder_input_ids must be [-1]")
        return E.embed(self.base_model.engine_model(), inputs["input_ids"], inputs["attention_mask"])

    def decode(self, text_encodings, summation=False):
        """reference :811-830: the output-codebook rows of every position's code, [bz, smtid_length, d_model]
        (or their sum over the positions, [bz, d_model])."""
        sd = self.base_model.state_dict()
        name = "list_decoder_embeds" if self.config.shared_output_input_embeds else "list_output_embeds"
        enc = torch.as_tensor(text_encodings).long().cpu()
        embeds = torch.stack([sd[f"{name}.{i}.weight"].cpu()[enc[:, i]] for i in range(enc.shape[1])], dim=1)
        return embeds.sum(dim=1) if summation else embeds

    def _position_pass(self, input_ids, attention_mask, codes, teacher_pos=None, teacher_neg=None, prefix_lens=None):
        """``engine.lngknp_forward`` of ``codes [bz, n_docs, L]`` under the guard of the search path (tasks/generation.py): the
        pass runs on the static-scale f16 planes; an activation outside their range is clamped and flagged (a residual row under
        their RMS floor is flagged too), and the pass is then repeated on the exact-fp32 GEMMs.
        -> (losses [n_prefix] or None, position scores [bz, n_docs, L])."""
        from .. import engine as E
        em = self.base_model.engine_model()
        ctx = em.ctx
        ctx.clear_status_async()
        args = (em, input_ids, attention_mask, codes, teacher_pos, teacher_neg, prefix_lens)
        out = E.lngknp_forward(*args)
        st = ctx.status(clear=True)
        if st & E._lib.STATUS_EMPTY_QUERY:
            raise ValueError("a query has an all-zero attention_mask (no token to attend to)")
        if (st & E._lib.STATUS_NEEDS_F32) and ctx.get_precision() != "f32":
            import warnings
            warnings.warn(("activation outside the f16 plane range" if st & E._lib.STATUS_SATURATED else
                           "residual stream under the RMS floor") + " of the split-precision GEMMs: repeating this forward "
                          "with exact fp32 MFMA (RPR_PRECISION=f32 avoids the retry)")
            saved = ctx.get_precision()   # "f16x2" or "bf16" (a training ctx): whatever it was comes back
            ctx.set_precision("f32")
            try:
                out = E.lngknp_forward(*args)
                ctx.status(clear=True)
            finally:
                ctx.set_precision(saved)
        return out

    def rerank_forward(self, **inputs):
        """reference :794-798: the score of one smtid per query, ``sum_i <decoder_last_hidden_state[:, i], E_out[i][c_i]>``, for
        ``tokenized_query`` (with ``decoder_input_ids`` = the encoding shifted right) and ``doc_encoding [bz, L]``
        -> fp32 ``[bz]``. One teacher-forced pass of ``rpr_lngknp_forward`` without a loss.

        The smtid goes into both document slots of the pass a training forward makes, and the first is read: a score is then
        bit for bit what ``forward`` gives the same (query, smtid) pair as its positive or its negative. With one slot the
        decoder GEMMs would see half the rows, and the split-precision GEMM picks its kernel, and with it the order of its
        sums, by the row count (gemm_route.h: 32 rows and fewer go to the skinny kernel): the last bit of a score would depend
        on whether bz * L crosses that line."""
        tq, codes = inputs["tokenized_query"], inputs["doc_encoding"]
        _check_smtid_length(codes.size(1), self.config)
        _check_shifted_right("tokenized_query", tq["decoder_input_ids"], codes)
        _, pos_scores = self._position_pass(tq["input_ids"], tq["attention_mask"], torch.stack([codes, codes], dim=1))
        return pos_scores[:, 0].sum(dim=-1)


def _check_shifted_right(name, decoder_input_ids, codes):
    if not torch.equal(decoder_input_ids[:, 1:].to(codes.device), codes[:, :-1]):
        raise ValueError(f"{name}: decoder_input_ids must be the doc encoding shifted right (dataset.py:497-500)")


def _check_smtid_length(L, config):
    """An smtid of any length the decoder has positions for. One code alone (the dense view, query_encode) is not a case of
    the teacher-forced passes."""
    n = len(config.decoder_vocab_sizes)
    if L == 1:
        raise ValueError("smtid length 1 is not built: the teacher-forced passes take smtids of 2 codes or more")
    if not 2 <= L <= n:
        raise ValueError(f"not valid length: {L} (the model decodes {n} positions)")


class T5AQEncoder(T5SeqAQEncoder):
    """reference :886-900: the dense view of the same model — ``query_encode`` as above, ``decode`` summed over the levels
    (the vector a residual-quantizer code stands for)."""

    def decode(self, text_encodings):
        return super().decode(text_encodings, summation=True)


class T5SeqPretrainEncoder(T5SeqAQEncoder):
    """reference :558-769: the dense first-stage model. ``doc_encode`` and ``query_encode`` are the same pass: the encoder plus
    one decoder position fed with the start embedding. ``forward(**inputs) -> {"rank": loss}`` is the margin-MSE of loss_type
    ``t5seq_pretrain_margin_mse`` on the batches of ``MarginMSEforPretrainCollator``, in the case the reference's training
    scripts run: ``decoder_input_ids = [-1]`` (no ``--docid_to_smtid_path``). The commit-loss branch (decoder length > 1) is not
    built. The whole pass runs in ``rpr_dense_mse_forward`` / ``rpr_dense_mse_backward`` (engine.py); no autograd graph is
    attached to the returned loss. ``last_scores`` keeps the two dot products of every example, ``[bz, 2]``."""

    def __init__(self, model_name_or_path, model_args=None, decoder_start_token_path=None, codebook_seed=0):
        config = T5forDocIDConfig.from_pretrained(model_name_or_path)
        config.decoding = False
        sd = _load_checkpoint(model_name_or_path)
        if "start_token_embed" not in sd:   # a plain HF T5 directory (what the first training round starts from)
            sd = plain_t5_state_dict(sd, config, decoder_start_token_path or config.decoder_start_token_path, codebook_seed)
        self.base_model = T5ForDocIDGeneration(config, sd)
        self.config = config
        self.model_args = model_args

    @classmethod
    def from_pretrained(cls, model_name_or_path=None, model_args=None, decoder_start_token_path=None, codebook_seed=0):
        """A checkpoint directory of this project's format, or a plain HF T5 directory (``config.json`` of a T5 and its
        ``shared`` / ``encoder.*`` / ``decoder.*`` tensors; ``lm_head`` is ignored). The latter has no ``start_token_embed``: it is
        read from the ``.npy`` named by ``decoder_start_token_path`` (argument, else the config field), and the codebooks —
        which this model never reads — are drawn from a normal seeded with ``codebook_seed``."""
        return cls(model_name_or_path, model_args, decoder_start_token_path, codebook_seed)

    def doc_encode(self, **inputs):
        return self.query_encode(**inputs)

    def _batch(self, inputs):
        pq, nq = inputs["tokenized_pos_query"], inputs["tokenized_neg_query"]
        pd, nd = inputs["tokenized_pos_doc"], inputs["tokenized_neg_doc"]
        if not (torch.equal(pq["input_ids"], nq["input_ids"]) and torch.equal(pq["attention_mask"], nq["attention_mask"])):
            # dataset.py:618-682 builds both from the same query text; two different texts would need two encoder passes
            raise ValueError("tokenized_pos_query and tokenized_neg_query must carry the same query tokens")
        for name, t in (("tokenized_pos_query", pq), ("tokenized_neg_query", nq), ("tokenized_pos_doc", pd), ("tokenized_neg_doc", nd)):
            di = t.get("decoder_input_ids")
            if di is not None and (di.dim() != 2 or di.shape[1] != 1 or bool((di != -1).any())):
                raise ValueError(f"{name}: decoder_input_ids must be [-1] (one decoder position fed with the start embedding); the "
                                 "commit-loss branch of the reference (decoder length > 1, --docid_to_smtid_path) is not built")
        if "pos_prev_smtids" in inputs or "neg_prev_smtids" in inputs:
            raise ValueError("pos_prev_smtids / neg_prev_smtids: the commit-loss branch of the reference is not built")
        groups = (pq, pd, nd)
        bz = pq["input_ids"].shape[0]
        Lt = max(int(t["input_ids"].shape[1]) for t in groups)
        ids = torch.zeros((3, bz, Lt), dtype=torch.int32)
        mask = torch.zeros((3, bz, Lt), dtype=torch.int32)
        for k, t in enumerate(groups):   # one length for the three groups: padded on the host
            if t["input_ids"].shape[0] != bz:
                raise ValueError("queries, positive and negative documents must have the same batch size")
            n = t["input_ids"].shape[1]
            ids[k, :, :n] = t["input_ids"].cpu().to(torch.int32)
            mask[k, :, :n] = t["attention_mask"].cpu().to(torch.int32)
        return ids, mask, inputs["teacher_pos_score"].float().reshape(-1), inputs["teacher_neg_score"].float().reshape(-1)

    def forward(self, **inputs):
        from .. import engine as E
        ids, mask, tp, tn = self._batch(inputs)
        em = self.base_model.engine_model()
        em.ctx.clear_status_async()
        loss, self.last_scores, self.last_reps = E.dense_mse_forward(em, ids, mask, tp, tn)
        if em.ctx.status(clear=True) & E._lib.STATUS_EMPTY_QUERY:
            raise ValueError("a query or a document has an all-zero attention_mask (no token to attend to)")
        return {"rank": loss[0]}

    __call__ = forward

    def train_state(self):
        from .. import engine as E
        if getattr(self, "_train_state", None) is None or self._train_state.model is not self.base_model.engine_model():
            self._train_state = E.TrainState(self.base_model.engine_model())
        return self._train_state

    def backward(self, **inputs):
        """loss.backward() of ``forward``: fills ``train_state().grads``; returns ``{"rank": loss}``."""
        from .. import engine as E
        ids, mask, tp, tn = self._batch(inputs)
        loss = E.dense_mse_backward(self.base_model.engine_model(), self.train_state(), ids, mask, tp, tn)
        return {"rank": loss[0]}

    def training_step(self, lr, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dropout_rate=None,
                      dropout_seed=None, global_step=None, **inputs):
        """One optimisation step (same contract as ``T5SeqAQEncoderForLngKnpMarginMSE.training_step``): backward with the
        data-parallel gradient exchange overlapped, clip_grad_norm_, AdamW in place on the device. Returns ``{"rank": loss}``
        of the batch before the update."""
        from .. import engine as E
        ids, mask, tp, tn = self._batch(inputs)
        loss = E.dense_mse_train_step(self.base_model.engine_model(), self.train_state(), ids, mask, tp, tn, lr, betas=betas, eps=eps,
                                      weight_decay=weight_decay, max_grad_norm=max_grad_norm, dropout_rate=dropout_rate,
                                      dropout_seed=dropout_seed, global_step=global_step)
        return {"rank": loss[0]}


class _MarginMSEOverPrefixes(T5SeqAQEncoder):
    """What the two margin-MSE ranking steps share: the batch guards, the forward through ``rpr_lngknp_forward`` and the training
    step through ``rpr_lngknp_backward`` + ``rpr_adamw_step``. A subclass says which prefixes of the smtid carry a loss:
    ``_prefixes(L) -> [(prefix length, prefix of the teacher-score keys), ...]``, the full length first."""

    def _prefixes(self, L):
        raise NotImplementedError

    def _batch(self, inputs, check_shift=False):
        pos_q, neg_q = inputs["pos_tokenized_query"], inputs["neg_tokenized_query"]
        pos_codes, neg_codes = inputs["pos_doc_encoding"], inputs["neg_doc_encoding"]
        L = pos_codes.size(1)
        prefixes = self._prefixes(L)
        if not torch.equal(pos_q["input_ids"], neg_q["input_ids"]):
            # dataset.py:502-503 builds both from the same query text; two different texts would need two encoder passes
            raise ValueError("pos_tokenized_query and neg_tokenized_query must carry the same query tokens")
        if check_shift:
            for side, q, codes in (("pos", pos_q, pos_codes), ("neg", neg_q, neg_codes)):
                _check_shifted_right(side, q["decoder_input_ids"], codes)
        names = ["rank" if k == L else f"rank_{k}" for k, _ in prefixes]
        tp = torch.stack([inputs[p + "teacher_pos_scores"] for _, p in prefixes]).float()
        tn = torch.stack([inputs[p + "teacher_neg_scores"] for _, p in prefixes]).float()
        return pos_q, torch.stack([pos_codes, neg_codes], dim=1), tp, tn, [k for k, _ in prefixes], names

    def forward(self, **inputs):
        pos_q, codes, tp, tn, prefix_lens, names = self._batch(inputs, check_shift=True)
        losses, self.last_position_scores = self._position_pass(pos_q["input_ids"], pos_q["attention_mask"], codes, tp, tn,
                                                                prefix_lens)
        return {n: losses[i] for i, n in enumerate(names)}

    __call__ = forward

    # ---- training (backward pass + optimizer on the device; reference: HF Trainer around this forward) -----------------
    def train_state(self):
        from .. import engine as E
        if getattr(self, "_train_state", None) is None or self._train_state.model is not self.base_model.engine_model():
            self._train_state = E.TrainState(self.base_model.engine_model())
        return self._train_state

    def backward(self, **inputs):
        """loss = sum of the task losses (ln_to_weight 1, reference arguments.py:109-119; tasks/trainer.py:228-240),
        loss.backward(): fills ``train_state().grads``; returns the task losses like ``forward``."""
        from .. import engine as E
        pos_q, codes, tp, tn, prefix_lens, names = self._batch(inputs)
        losses = E.lngknp_backward(self.base_model.engine_model(), self.train_state(), pos_q["input_ids"],
                                   pos_q["attention_mask"], codes, tp, tn, prefix_lens)
        return {n: losses[i] for i, n in enumerate(names)}

    def training_step(self, lr, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dropout_rate=None,
                      dropout_seed=None, global_step=None, **inputs):
        """One optimisation step as the reference's trainer performs it: backward with the gradient all-reduce across the
        data-parallel ranks overlapped (RCCL when torch.distributed is initialised; engine.GradExchange), clip_grad_norm_,
        AdamW — weights updated in place on the device. Returns the task losses of the batch (before the update).
        ``dropout_rate`` / ``dropout_seed`` / ``global_step``: the dropout of this step (engine.train_step; off by default)."""
        from .. import engine as E
        pos_q, codes, tp, tn, prefix_lens, names = self._batch(inputs)
        losses = E.train_step(self.base_model.engine_model(), self.train_state(), pos_q["input_ids"], pos_q["attention_mask"],
                              codes, tp, tn, prefix_lens, lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm, dropout_rate=dropout_rate, dropout_seed=dropout_seed,
                              global_step=global_step)
        losses = {n: losses[i] for i, n in enumerate(names)}
        return losses


class T5SeqAQEncoderForLngKnpMarginMSE(_MarginMSEOverPrefixes):
    """reference :902-966 — forward of the prefix-oriented ranking fine-tune step, same
    ``forward(**inputs)`` dict interface and return keys (``rank``, ``rank_4``, ``rank_8``, ``rank_16``). The whole
    pass runs in ``rpr_lngknp_forward`` (teacher-forced decoder over all positions of the positive and the negative
    smtid at once, one encoder pass per query). Forward only: no autograd graph is attached to the returned losses."""

    _PREFIXES = {8: [(8, ""), (4, "smtid_4_")], 16: [(16, ""), (4, "smtid_4_"), (8, "smtid_8_")],
                 32: [(32, ""), (4, "smtid_4_"), (8, "smtid_8_"), (16, "smtid_16_")]}

    def _prefixes(self, L):
        if L not in self._PREFIXES:
            raise ValueError("not valid length: {}".format(L))
        return self._PREFIXES[L]


class T5SeqAQEncoderForMarginMSE(_MarginMSEOverPrefixes):
    """reference :857-884 — the rank-oriented step (loss_type ``t5seq_aq_encoder_margin_mse``): one margin-MSE over the whole
    smtid, ``forward(**inputs) -> {"rank": loss}`` on the batches of ``MarginMSEforT5SeqAQCollator``. It is the lng_knp step
    with the single prefix ``[L]``: the same device passes, the same training step. The reference has no table of lengths:
    any smtid length from 2 up to the model's decoder length runs (4 codes on a model of 32 positions is the first rung of
    the prefix curriculum, full_lng_knp_train_pipline.sh:5-45)."""

    def _prefixes(self, L):
        _check_smtid_length(L, self.config)
        return [(L, "")]


class T5SeqAQEncoderForSeq2Seq(T5SeqAQEncoder):
    """reference :968-1019 — the seq2seq docid step (loss_type ``t5seq_aq_encoder_seq2seq``, the first stage of RIPOR's docid
    training): cross-entropy of the per-position codebook logits ``h[:, i] @ E_i^T`` against the docid codes, ``forward(**inputs)
    -> {"rank": loss}`` on the batches of ``Seq2SeqForT5SeqAQCollator``. The whole pass runs in ``rpr_seq2seq_forward`` /
    ``rpr_seq2seq_backward`` (engine.py); no autograd graph is attached to the returned loss. ``multi_vocab_sizes`` is accepted:
    every position has the same codebook size here, where the reference's per-position mean divided by L is the same value."""

    def __init__(self, model_name_or_path, shared_output_input_embeds=None, multi_vocab_sizes=False):
        super().__init__(model_name_or_path, shared_output_input_embeds, multi_vocab_sizes)
        self.multi_vocab_sizes = bool(multi_vocab_sizes)

    def _batch(self, inputs):
        tq, labels = inputs["tokenized_query"], inputs["labels"]
        if labels.dim() != 2:
            raise ValueError(f"labels must be [bz, smtid_length], got {tuple(labels.shape)}")
        V = list(self.config.decoder_vocab_sizes)
        if labels.size(1) > len(V):
            raise ValueError(f"smtid length {labels.size(1)} exceeds the model's {len(V)} codebooks")
        if int(labels.min()) < 0 or int(labels.max()) >= min(V[: labels.size(1)]):
            raise ValueError(f"labels outside [0, {min(V[: labels.size(1)])}) of the codebooks")
        di = tq["decoder_input_ids"]
        start = torch.full((labels.size(0), 1), -1, dtype=labels.dtype)
        if tuple(di.shape) != tuple(labels.shape) or not torch.equal(di.cpu().long(),
                                                                     torch.cat([start, labels[:, :-1]], 1).cpu().long()):
            raise ValueError("decoder_input_ids must be [-1, labels[:, :-1]] (dataset.py:527-550)")
        return tq["input_ids"], tq["attention_mask"], labels

    def forward(self, **inputs):
        from .. import engine as E
        ids, mask, labels = self._batch(inputs)
        loss, self.last_label_logprobs = E.seq2seq_forward(self.base_model.engine_model(), ids, mask, labels)
        return {"rank": loss[0]}

    __call__ = forward

    def train_state(self):
        from .. import engine as E
        if getattr(self, "_train_state", None) is None or self._train_state.model is not self.base_model.engine_model():
            self._train_state = E.TrainState(self.base_model.engine_model())
        return self._train_state

    def backward(self, **inputs):
        """loss.backward() of ``forward``: fills ``train_state().grads``; returns ``{"rank": loss}``."""
        from .. import engine as E
        ids, mask, labels = self._batch(inputs)
        loss = E.seq2seq_backward(self.base_model.engine_model(), self.train_state(), ids, mask, labels)
        return {"rank": loss[0]}

    def training_step(self, lr, max_grad_norm=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dropout_rate=None,
                      dropout_seed=None, global_step=None, **inputs):
        """One optimisation step (same contract as ``T5SeqAQEncoderForLngKnpMarginMSE.training_step``): backward with the
        data-parallel gradient exchange overlapped, clip_grad_norm_, AdamW in place on the device. Returns ``{"rank": loss}``
        of the batch before the update."""
        from .. import engine as E
        ids, mask, labels = self._batch(inputs)
        loss = E.seq2seq_train_step(self.base_model.engine_model(), self.train_state(), ids, mask, labels, lr, betas=betas, eps=eps,
                                    weight_decay=weight_decay, max_grad_norm=max_grad_norm, dropout_rate=dropout_rate,
                                    dropout_seed=dropout_seed, global_step=global_step)
        return {"rank": loss[0]}
