"""TEST INFRASTRUCTURE. The dropout mask of the training step restated in numpy, bit for bit what ripor_amd/csrc/dropout.h
draws on the device (DESIGN.md "Dropout in the training step"): Philox4x32-10 over a counter packed from the LOGICAL
coordinates of an element, keyed by (seed, step). An element is dropped where its 32-bit draw is below round(rate * 2^32);
a kept one is multiplied by float32(1 / (1 - rate)).

    key      k0 = seed[31:0]                 k1 = seed[63:32] ^ step[63:32]
    counter  c1 = sequence                   c3 = step[31:0]
      activation (sequence, position, feature):        c0 = feature >> 2              c2 = site << 16 | position
      attention  (sequence, head, query pos, key pos): c0 = query << 16 | key >> 2    c2 = site << 16 | head
    the element's draw is word (feature & 3) / (key pos & 3) of the block.
"""
from __future__ import annotations

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (broadcast together) and a 64-bit key -> the four output words, each uint32."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK32, n2, p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(rate) -> int:
    return int(np.rint(np.float64(np.float32(rate)) * 4294967296.0))


def scale(rate) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def _key(seed: int, step: int):
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32), step & 0xFFFFFFFF


# ---- sites (16 bits): stack << 11 | code ----
def site_input(dec: int) -> int:
    return (dec << 11) | 0


def site_output(dec: int) -> int:
    return (dec << 11) | 1


def site_mid(dec: int, layer: int, j: int) -> int:
    """attention probabilities / relu(h Wi^T) of sub-block j of a layer"""
    return (dec << 11) | (8 + 8 * layer + 2 * j)


def site_sub_out(dec: int, layer: int, j: int) -> int:
    return (dec << 11) | (8 + 8 * layer + 2 * j + 1)


def act_draws(seed, step, site, seqs, n_pos, n_feat) -> np.ndarray:
    """uint32 draws [len(seqs), n_pos, n_feat] of an activation; seqs = the logical sequence number of every row block."""
    k0, k1, step_lo = _key(seed, step)
    seqs = np.asarray(seqs, dtype=np.uint64).reshape(-1, 1, 1)
    pos = np.arange(n_pos, dtype=np.uint64).reshape(1, -1, 1)
    q = np.arange((n_feat + 3) // 4, dtype=np.uint64).reshape(1, 1, -1)
    w = philox4x32_10(q, seqs, (np.uint64(site) << np.uint64(16)) | pos, np.uint64(step_lo), k0, k1)
    return np.stack(w, axis=-1).reshape(seqs.shape[0], n_pos, -1)[:, :, :n_feat]


def attn_draws(seed, step, site, seqs, n_head, n_q, n_k) -> np.ndarray:
    """uint32 draws [len(seqs), n_head, n_q, n_k] of attention probabilities."""
    k0, k1, step_lo = _key(seed, step)
    seqs = np.asarray(seqs, dtype=np.uint64).reshape(-1, 1, 1, 1)
    head = np.arange(n_head, dtype=np.uint64).reshape(1, -1, 1, 1)
    qp = np.arange(n_q, dtype=np.uint64).reshape(1, 1, -1, 1)
    kq = np.arange((n_k + 3) // 4, dtype=np.uint64).reshape(1, 1, 1, -1)
    w = philox4x32_10((qp << np.uint64(16)) | kq, seqs, (np.uint64(site) << np.uint64(16)) | head, np.uint64(step_lo), k0, k1)
    return np.stack(w, axis=-1).reshape(seqs.shape[0], n_head, n_q, -1)[..., :n_k]


def _mul(draws, rate) -> np.ndarray:
    return np.where(draws.astype(np.uint64) < np.uint64(threshold(rate)), np.float32(0), scale(rate)).astype(np.float32)


def act_mask(rate, seed, step, site, seqs, n_pos, n_feat) -> np.ndarray:
    """float32 multipliers (0 or 1 / (1 - rate)) [len(seqs), n_pos, n_feat]"""
    return _mul(act_draws(seed, step, site, seqs, n_pos, n_feat), rate)


def attn_mask(rate, seed, step, site, seqs, n_head, n_q, n_k) -> np.ndarray:
    return _mul(attn_draws(seed, step, site, seqs, n_head, n_q, n_k), rate)
