"""numpy restatement of the exact top-k inner-product search (rpr_flat_search).

score[q][r] = <queries[q], x[r]> in fp64 (exact for the integer-valued inputs the bit-for-bit tests use, the yardstick of
the derived rounding bound otherwise), ranking by score descending with exact ties to the smaller GLOBAL row, -0.0 = +0.0,
idx -1 / score -inf past the rows there are. ``merge`` folds the result of a block into a running state by the same order,
ignoring idx < 0: any partition of the rows chained through it equals one search over all of them."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_search_ref  # noqa: E402


def scores(queries: np.ndarray, x: np.ndarray) -> np.ndarray:
    """[Q, n] float64."""
    return np.asarray(queries, dtype=np.float64) @ np.asarray(x, dtype=np.float64).T


def topk(sc: np.ndarray, k: int):
    """``rq_search_ref.topk`` (stable sort by (-score, row)), sorting only what can be in the result: the rows at or above
    the k-th largest score, which ``flatnonzero`` lists in ascending order. The same output at N >> k in O(N) per query."""
    Q, N = sc.shape
    if N <= 4 * k:
        return rq_search_ref.topk(sc, k)
    idx = np.empty((Q, k), dtype=np.int64)
    out = np.empty((Q, k), dtype=sc.dtype)
    for q in range(Q):
        kth = np.partition(sc[q], N - k)[N - k]
        cand = np.flatnonzero(sc[q] >= kth)
        order = cand[np.argsort(-sc[q, cand], kind="stable")[:k]]
        idx[q], out[q] = order, sc[q, order]
    return idx, out


def search(queries, x, k: int, row_base: int = 0, out_dtype=np.float32):
    """-> (idx int64 [Q, k] global rows, scores [Q, k] rounded to ``out_dtype`` after the ranking)."""
    idx, sc = topk(scores(queries, x) + 0.0, k)   # + 0.0: -0.0 becomes +0.0
    idx = np.where(idx >= 0, idx + row_base, -1)
    return idx, sc.astype(out_dtype)


def merge(state, block, k: int):
    """Top k of the union of two (idx, scores) results over different rows: score descending, ties to the smaller row."""
    idx = np.concatenate([state[0], block[0]], axis=1)
    sc = np.concatenate([state[1], block[1]], axis=1)
    out_i = np.full((idx.shape[0], k), -1, dtype=np.int64)
    out_s = np.full((idx.shape[0], k), -np.inf, dtype=sc.dtype)
    for q in range(idx.shape[0]):
        live = np.flatnonzero(idx[q] >= 0)
        order = live[np.lexsort((idx[q, live], -sc[q, live]))][:k]
        out_i[q, :len(order)] = idx[q, order]
        out_s[q, :len(order)] = sc[q, order]
    return out_i, out_s


def rounding_bound(queries, x) -> np.ndarray:
    """[Q, n]: 1.01 d 2^-24 sum_i |q_i| |x_i|, the gamma_d bound of a d-term fp32 chain against exact arithmetic."""
    d = np.asarray(queries).shape[1]
    return 1.01 * d * 2.0 ** -24 * scores(np.abs(queries), np.abs(x))
