"""TEST INFRASTRUCTURE. The CPU oracles with the gated-GELU feed-forward block of T5 v1.1 / Flan-T5 / mT5
(HF ``T5DenseGatedActDense`` with ``dense_act_fn = "gelu_new"``): ``wo(gelu_new(wi_0 x) * wi_1 x)``. Each class overrides the
feed-forward of its base and nothing else, so everything written against ``T5Ref`` / ``T5RefCached`` / ``DropoutRef``
(``oracle.beam_ref``, ``oracle.train_ref``, the seq2seq gradients) runs on it unchanged.

Also the float64 numpy restatement of the gate and of its backward, the yardstick of the kernel-level hooks
(``rpr_op_gated_gelu``, ``rpr_op_gated_gelu_bwd``).
"""
from __future__ import annotations

import numpy as np
import torch

from dropout_ref import DropoutRef
from oracle.t5_ref import T5Ref, T5RefCached

GELU_C = 0.7978845608028654   # sqrt(2 / pi)
GELU_A = 0.044715


def gelu_new_t(g: torch.Tensor) -> torch.Tensor:
    """HF ``NewGELUActivation`` in the dtype of ``g``."""
    return 0.5 * g * (1.0 + torch.tanh(GELU_C * (g + GELU_A * torch.pow(g, 3.0))))


def _gated_ff(sd, prefix: str, x: torch.Tensor, mask=None) -> torch.Tensor:
    mid = gelu_new_t(x @ sd[prefix + ".wi_0.weight"].t()) * (x @ sd[prefix + ".wi_1.weight"].t())
    if mask is not None:
        mid = mask(mid)
    return mid @ sd[prefix + ".wo.weight"].t()


class GatedT5Ref(T5Ref):
    def _ff(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        return _gated_ff(self.sd, prefix, x)


class GatedT5RefCached(T5RefCached):
    def _ff(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        return _gated_ff(self.sd, prefix, x)


class GatedDropoutRef(DropoutRef):
    """The inner-activation site masks the product [rows, d_ff], as ``T5DenseGatedActDense.forward`` does."""

    def _ff(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        return _gated_ff(self.sd, prefix, x)

    def _ff_drop(self, prefix, x, site, seqs):
        return _gated_ff(self.sd, prefix, x, lambda mid: self._act(mid, site, seqs))


# ---- float64 restatement of the gate kernels ----------------------------------------------------------------------------------
def gelu_new64(g: np.ndarray) -> np.ndarray:
    g = np.asarray(g, dtype=np.float64)
    return 0.5 * g * (1.0 + np.tanh(GELU_C * (g + GELU_A * g ** 3)))


def gelu_new_grad64(g: np.ndarray) -> np.ndarray:
    g = np.asarray(g, dtype=np.float64)
    t = np.tanh(GELU_C * (g + GELU_A * g ** 3))
    return 0.5 * (1.0 + t) + 0.5 * g * (1.0 - t * t) * GELU_C * (1.0 + 3.0 * GELU_A * g * g)


def gate64(gu: np.ndarray) -> np.ndarray:
    """gu [M, 2F] = (g | u) -> gelu_new(g) * u, [M, F] float64."""
    F = gu.shape[1] // 2
    return gelu_new64(gu[:, :F]) * gu[:, F:].astype(np.float64)


def gate_bwd64(gu: np.ndarray, dmid: np.ndarray) -> np.ndarray:
    """-> dgu [M, 2F] = (dmid u gelu_new'(g) | dmid gelu_new(g)) float64."""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].astype(np.float64), gu[:, F:].astype(np.float64), dmid.astype(np.float64)
    return np.concatenate([d * u * gelu_new_grad64(g), d * gelu_new64(g)], axis=1)
