"""numpy restatement of the top-k inner-product search over residual-quantizer codes (rpr_rq_search).

LUT[q][m][k] = <queries[q], codebooks[m][k]>, score[q][n] = ((LUT[q][0][c_n0] + LUT[q][1][c_n1]) + ...) with the levels in
ascending order, ranking by score descending with exact ties to the smaller row, -1 / -inf past N rows. ``dtype`` is the
arithmetic of both the LUT and the level sum. Given the LUT everything is exact and order-fixed, so the device is compared
bit for bit wherever the LUT is: integer-valued inputs, where every fp32 summation order gives the same entries. float32
here is an fp32 chain in ascending k; the matrix core rounds its own chain differently in the last bits (a numpy chain in
the kernel's staging order 0 4 1 5 2 6 3 7 matched 6-16 % of the entries of a Gaussian LUT bit for bit), so float-valued
cases are checked against float64 and the derived rounding bound instead."""
from __future__ import annotations

import numpy as np


def lut(queries: np.ndarray, books: np.ndarray, dtype=np.float32) -> np.ndarray:
    """[Q, M, K]. float32: acc = fl32(acc + q_k * c_k) for k ascending, the product and the sum carried in fp64 and rounded
    to fp32 once per step; float64: a plain matmul."""
    M, K, d = books.shape
    q = np.asarray(queries)
    if dtype == np.float64:
        return (q.astype(np.float64) @ books.reshape(M * K, d).astype(np.float64).T).reshape(q.shape[0], M, K)
    q64, c64 = q.astype(np.float64), books.reshape(M * K, d).astype(np.float64)
    acc = np.zeros((q.shape[0], M * K), dtype=np.float32)
    for k in range(d):
        acc = (acc.astype(np.float64) + q64[:, k:k + 1] * c64[None, :, k]).astype(np.float32)
    return acc.reshape(q.shape[0], M, K)


def scores(table: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """[Q, N] in the table's dtype: the fixed-order sum over the levels."""
    codes = np.asarray(codes).astype(np.int64)
    s = table[:, 0, codes[:, 0]].copy()
    for m in range(1, table.shape[1]):
        s = s + table[:, m, codes[:, m]]
    return s


def topk(sc: np.ndarray, k: int):
    """Stable sort by (-score, n) -> (idx int64 [Q, k], scores [Q, k]); past N rows idx -1, score -inf."""
    Q, N = sc.shape
    idx = np.full((Q, k), -1, dtype=np.int64)
    out = np.full((Q, k), -np.inf, dtype=sc.dtype)
    n = min(k, N)
    for q in range(Q):
        order = np.argsort(-sc[q], kind="stable")[:n]
        idx[q, :n] = order
        out[q, :n] = sc[q, order]
    return idx, out


def search(queries, books, codes, k: int, dtype=np.float32):
    return topk(scores(lut(queries, books, dtype), codes), k)


def rounding_bound(queries, books, codes) -> np.ndarray:
    """[Q, N]: (d + M) 2^-24 sum_m sum_j |q_j| |C_m[c_m]_j|, the standard bound of a d-term fp32 dot product followed by an
    M-term fp32 sum against exact arithmetic."""
    M, K, d = books.shape
    return (d + M) * 2.0 ** -24 * scores(lut(np.abs(queries), np.abs(books), np.float64), codes)
