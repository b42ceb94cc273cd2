"""numpy restatement of the beam encoder of the residual quantizer (rpr_rq_encode_beam).

A row's beam at level m holds b_m entries (b_0 = 1: the row itself), each an fp32 residual r_s and a code history. Every
candidate (s, k) gets total(s, k) = |r_s|^2 + (|c_k|^2 - 2 r_s.c_k), here all in fp64; the b_{m+1} = min(B, b_m K)
smallest form the next beam, exact ties to the smaller parent slot s, then the smaller k, stored in that order (slot 0 is
the best; nothing is de-duplicated). A child's residual is fp32(r_s - c_k), its history the parent's plus k."""
from __future__ import annotations

import numpy as np


def encode(X: np.ndarray, books: np.ndarray, beam: int = 1, rows_per_step: int = 4096):
    """-> (codes int64 [N, M]: the history of slot 0 after the last level, level_sse float64 [M]: the sum over the rows of
    slot 0's |r|^2 after every level)."""
    X = np.asarray(X, dtype=np.float32)
    books = np.asarray(books, dtype=np.float32)
    M, K, d = books.shape
    N = X.shape[0]
    assert 1 <= beam <= 8 and X.shape[1] == d
    codes = np.empty((N, M), dtype=np.int64)
    sse = np.zeros(M, dtype=np.float64)
    for lo in range(0, N, rows_per_step):
        c, s = _encode_rows(X[lo:lo + rows_per_step], books, beam)
        codes[lo:lo + rows_per_step] = c
        sse += s
    return codes, sse


def _encode_rows(X, books, beam):
    M, K, d = books.shape
    n = X.shape[0]
    R = X[:, None, :].copy()                               # [n, b, d] fp32
    hist = np.zeros((n, 1, 0), dtype=np.int64)             # [n, b, m]
    sse = np.zeros(M, dtype=np.float64)
    rows = np.arange(n)[:, None]
    for m in range(M):
        C64 = books[m].astype(np.float64)
        R64 = R.astype(np.float64)
        b = R.shape[1]
        total = (R64 * R64).sum(2)[:, :, None] + ((C64 * C64).sum(1)[None, None, :] - 2.0 * (R64 @ C64.T))   # [n, b, K]
        nb = min(beam, b * K)
        # a stable sort of the candidates in (s, k) order: equal totals keep the smaller s, then the smaller k, in front
        order = np.argsort(total.reshape(n, b * K), axis=1, kind="stable")[:, :nb]
        s, k = order // K, order % K
        R = (R[rows, s] - books[m][k]).astype(np.float32)
        hist = np.concatenate([hist[rows, s], k[:, :, None]], axis=2)
        sse[m] = (R[:, 0].astype(np.float64) ** 2).sum()
    return hist[:, 0], sse
