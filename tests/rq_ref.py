"""numpy restatement of the greedy residual k-means that creates the docids (rpr_rq_train / rpr_rq_encode; DESIGN.md
"Residual quantization"). Scores and means in fp64, centroids and residuals stored in fp32 as the device stores them."""
from __future__ import annotations

import numpy as np

NITER, SEED, MAX_POINTS_PER_CENTROID = 25, 1234, 256


def plan(N: int, M: int, K: int, seed: int = SEED):
    """Training rows S (sorted) and the initial centroid rows of every level [M, K], from one generator."""
    rng = np.random.default_rng(seed)
    n_train = min(N, MAX_POINTS_PER_CENTROID * K)
    S = np.sort(rng.permutation(N)[:n_train])
    init = np.stack([rng.permutation(n_train)[:K] for _ in range(M)])
    return S, init


def scores(R: np.ndarray, C: np.ndarray) -> np.ndarray:
    """|c_k|^2 - 2 r . c_k in fp64, [n, K]."""
    C64 = C.astype(np.float64)
    return (C64 * C64).sum(1)[None, :] - 2.0 * (R.astype(np.float64) @ C64.T)


def assign(R: np.ndarray, C: np.ndarray) -> np.ndarray:
    return np.argmin(scores(R, C), axis=1)   # np.argmin: the first (smallest) k among equal minima


def update(R: np.ndarray, code: np.ndarray, C: np.ndarray) -> np.ndarray:
    """fp64 mean of every centroid's rows, rounded to fp32 once; a centroid without rows keeps its value."""
    out = C.copy()
    K = C.shape[0]
    sums = np.zeros((K, R.shape[1]), dtype=np.float64)
    np.add.at(sums, code, R.astype(np.float64))
    cnt = np.bincount(code, minlength=K)
    nz = cnt > 0
    out[nz] = (sums[nz] / cnt[nz, None]).astype(np.float32)
    return out


def train(X: np.ndarray, M: int, K: int, niter: int = NITER, seed: int = SEED):
    """-> (codebooks fp32 [M, K, d], level_mse [M], S, init)."""
    X = np.asarray(X, dtype=np.float32)
    S, init = plan(X.shape[0], M, K, seed)
    R = X[S].copy()
    books, mse = [], []
    for m in range(M):
        C = R[init[m]].copy()
        for _ in range(niter):
            C = update(R, assign(R, C), C)
        R = (R - C[assign(R, C)]).astype(np.float32)
        books.append(C)
        mse.append(float((R.astype(np.float64) ** 2).sum(1).mean()))
    return np.stack(books), np.asarray(mse), S, init


def train_on(Xs: np.ndarray, init: np.ndarray, K: int, niter: int = NITER):
    """The same over given training rows and initial rows (what rpr_rq_train receives) -> (codebooks, level_mse)."""
    R = np.asarray(Xs, dtype=np.float32).copy()
    books, mse = [], []
    for m in range(init.shape[0]):
        C = R[init[m]].copy()
        for _ in range(niter):
            C = update(R, assign(R, C), C)
        R = (R - C[assign(R, C)]).astype(np.float32)
        books.append(C)
        mse.append(float((R.astype(np.float64) ** 2).sum(1).mean()))
    return np.stack(books), np.asarray(mse)


def encode(X: np.ndarray, books: np.ndarray):
    """Greedy chain over all rows -> (codes [N, M], level_mse [M])."""
    R = np.asarray(X, dtype=np.float32).copy()
    codes, mse = [], []
    for C in books:
        c = assign(R, C)
        R = (R - C[c]).astype(np.float32)
        codes.append(c)
        mse.append(float((R.astype(np.float64) ** 2).sum(1).mean()))
    return np.stack(codes, 1), np.asarray(mse)
