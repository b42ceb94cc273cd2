"""The row-wise kernels of the training step (train_kernels.hip, dense_head.hip: everything of the step but the GEMMs, the
attention, AdamW, dropout and the gated-GELU gate) from their definitions, in numpy fp64, with an a-priori fp32 error bound per
output element; the inputs and the case table of tests/test_gpu_train_rows_direct.py, which runs every case through
rpr_op_train_rows (the launcher the step calls); the mutants of the definitions that tests/test_train_rows_ref_host.py uses to
show that these inputs tell a wrong kernel from a right one. In the style of tests/attn_train_ref.py. Nothing here follows a
kernel's order of operations: every op is written from the reference model's forward and its autograd (RMSNorm h = post w x rs,
rs = (mean(x^2) + eps)^-1/2; score = <h, E[code]>; margin-MSE; cross-entropy), and the host file compares the differentiable ones
with torch.autograd in float64.

Bounds (first order), u = 2^-24, UF = 2^-126 (a product that leaves the normal range is off by at most UF, flushed or not). A sum of
n terms in ANY order is off by at most (n - 1) u sum |terms|; a product chain of k factors by k u. d = row width.
  e_rs   = ((d + 3) / 2 + 4) u       rs: mean(x^2) + eps has relative error (d + 3) u (squares, any-order sum, the division, the
                                     addition; all terms positive), the power -1/2 halves it, rsqrtf is good to 2 ulp = 4 u
  rmsnorm_bwd   g = dh post w, m = sum(g x) / d, c = rs^3 m, t1 = rs g, t2 = x c, dx = t1 - t2 (+ dres)
      E_c  = rs^3 / d ((d + 3) u sum |dh w x post| + d UF) + |c| (3 e_rs + 4 u)
      b_dx = |t1| (e_rs + 3 u) + |x| E_c + u |t2| + u (|t1| + |t2|) (+ u |dx| with dres) + 4 UF
      a_r  = dh post x rs (the dw term of row r), b_dw = sum_r |a_r| (e_rs + 3 u) + (rows + 2) u sum_r |a_r| + u |dw| + rows UF;
      the 16-row partials (w_part) are held to the same formula over their own rows
  colsum        (n - 1) u sum |part|                      sum_selected: (count + 1) u sum |src| + u |out0 + sum|
  gold score    E_h = |h| (e_rs + 3 u) + UF;  b = sum |e| E_h + (d + 1) u sum |h e| + d UF;  hidden rows: E_h
  gold_score_bwd  de = g h: |de| (e_rs + 4 u) + UF;  dh = g e: u |dh| + UF;  gold_rowdot: (d + 1) u sum |h e| + d UF, u |.| + UF
  margin_mse    E_sm = (k + 1) u (sum |pos| + sum |neg|) (k terms each and the difference), E_dl = E_sm + u |tm| + u |dl|,
                b_loss = mean((2 |dl| E_dl + E_dl^2 + u (|dl| + E_dl)^2)) + u |loss| + UF (the sum itself is in double)
  margin_mse_bwd  term_p = (2 / bz) (m_p - tm_p): E_p = (2 / bz) (u |tm| + u |m - tm|) + 2 u |term_p|; b = sum E_p + np u sum |term_p| + np UF
                fed by the forward launch's own margins (off by up to E_sm + u |m| from the definition's): (2 / bz)(1 + 2 u)(E_sm + u |m|)
                per prefix on top
  dense head    scores as gold_rowdot; margin: E_sp + E_sn + u |m|; g: (2 / bz) (E_m + u |tm| + u |m - tm|) + 2 u |g|; loss as above;
                backward dq = g (d+ - d-): 2 u |dq| + UF, dd+- = +-g q: u |.| + UF
  s2s head      logits l = <h, E_v>: E_l = (d + 1) u sum |h e| + d UF, D = max_v E_l. lse is 1-Lipschitz in the logits (sup norm), expf and
                logf are good to 2 ulp (4 u):  E_lse = D + (spread + 8 + V) u + 4 u log V + u |lse|, spread = max l - min l
                row_loss = lse - l_label: E_lse + E_l(label) + u |row_loss| (label_lp likewise)
                dlogits = (p - onehot) inv_n, p = exp(l - lse): inv_n (p (E_l + E_lse + u |l - lse| + 4 u) + u |p - onehot|) + 2 u |dlogits| + UF
                loss = mean(row_loss), summed in double: mean(b_row_loss) + 2 u |loss|
                dH = dlogits E: (V + 1) u sum |dlogits E| + V UF;  dE = dlogits^T h: (bz + 1) u sum + bz UF
  planes        split_f16 (common.h): hi = f16(xs), lo = f16(xs - hi), xs = x * scale with scale a power of two (X_PLANE_SCALE = 1/16, or
                dyn_plane_scale(amax) = 2^(13 - floor(log2 amax)), which puts amax into [2^13, 2^14): no clamp, xs exact). xs - hi is exact in
                fp32 and at most 2^-11 |xs|; its f16 rounding is off by 2^-11 of it, or by half a subnormal step 2^-25 when it lies under
                2^-14:   |hi + lo - xs| <= max(2^-22 |xs|, 2^-25)
  dec_embed ssq the row's sum of squares of what the planes hold, in 2^-16 units: 65536 ((d + 1) u ss + sum (2 |x| E_x + E_x^2)) + u fix + 1
  scatter+flush count_t 2^-33 + 2 u |result| per table element, count_t the rows that land on it (every addend is rounded to 2^-32 once,
                the integer sum is exact and order-free; the flush rounds to fp32 and adds). The accumulator wraps silently: the bound
                holds while |sum| < 2^31 for every table element.
Exact outputs (bit equality): to_bf16 / to_bf16_T / weights_bf16 (round to nearest even of the fp32 value), transpose_pad, train_indices,
relu_bwd, absmax2, the fp32 rows of train_dec_embed, and every zero-padded row or column. rmsnorm_bf16_T is the bf16 rounding of an fp32
value that carries E_h: an element may be either bf16 neighbour when [h - E_h, h + E_h] straddles a rounding boundary; the elements that
differ from bf16(h) are counted and capped at 1 % of a case.

Inputs: the counter hashes of ripor_amd.utils.synth. Activation rows come in three kinds (row % 3): flat (uniform in [-1, 1)), peaked
(uniform 0.01 with three elements of +-30), near zero (mean(x^2) about eps). Gradient rows carry the row's signature ((row % 61 + 1) / 8)
on column 5 of every eight, weights the column's (1 + (col % 97) / 64) on column 3 of every eight: a row or a column taken from a
neighbour shows."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

from ripor_amd.utils import synth

U = 2.0 ** -24
UF = 2.0 ** -126
EPS = 1e-6
F64, F32 = np.float64, np.float32
X_PLANE_SCALE = 0.0625
SSQ_FIX = 65536.0
GRAD_FIX = 4294967296.0

MUTANTS = ("rs2", "no_mean_div", "post_once", "dres_rows34", "last_block_dw", "colsum_floor16", "prefix_unclamped", "neg_sign_lost",
           "one_over_bz", "inv_n_bz", "codebook_next", "onehot_unclamped", "start_row_scattered", "in_idx_i", "pad_from_neighbour",
           "relu_ge", "lo_dropped")


# ---------------------------------------------------------------------------------------------- inputs
def unif(name, shape, scale=1.0):
    return synth.uniform_f32("train_rows/" + name, shape, scale)


def act_rows(name, rows, d):
    """Activation rows of the three kinds."""
    x = unif(name, (rows, d))
    hot = synth.randint("train_rows/hot/" + name, (rows, 3), 0, d)
    for r in range(rows):
        if r % 3 == 1:
            x[r] *= F32(0.01)
            x[r, hot[r]] = F32(30.0) * np.where(hot[r] % 2 == 0, F32(1), F32(-1))
        elif r % 3 == 2:
            x[r] *= F32(math.sqrt(3.0 * EPS))
    return x


def grad_rows(name, rows, d, scale=1.0):
    g = unif(name, (rows, d), scale)
    sig = ((np.arange(rows) % 61 + 1) / 8.0).astype(F32) * F32(scale)
    g[:, 5::8] = sig[:, None]
    return g


def weight_row(name, d):
    w = (unif(name, (d,), 0.5) + F32(1.0)).astype(F32)
    cols = np.arange(d)[3::8]
    w[3::8] = (1.0 + (cols % 97) / 64.0).astype(F32)
    return w


def _perm(n, perm):
    if perm is None:
        return np.arange(n)
    return np.argsort(synth.hash_u64(f"train_rows/perm/{perm}", n), kind="stable")


def e_rs(d):
    return ((d + 3) / 2.0 + 4.0) * U


A = np.abs


# ---------------------------------------------------------------------------------------------- bf16 and f16 planes, exactly
def bf16_bits(x):
    """Round-to-nearest-even bf16 of fp32 values (finite), as uint16 bit patterns."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(F32)


def bf16_order(bits):
    """Monotone integer key of bf16 bit patterns (sign-magnitude -> ordered)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def dyn_plane_scale(amax):
    """common.h dyn_plane_scale restated."""
    i = int(np.array(amax, F32).view(np.int32))
    e = (i >> 23) & 0xFF
    if e == 0 or e == 255:
        return F32(1.0)
    be = min(254, max(1, 127 + 13 - (e - 127)))
    return np.array(be << 23, np.int32).view(F32)[()]


def split_planes(xs, mut=None):
    """split_f16 of fp32 values xs (|xs| <= 65504) -> (hi, lo) float16."""
    xs = np.asarray(xs, F32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(F32)).astype(np.float16)
    if mut == "lo_dropped":
        lo = np.zeros_like(lo)
    return hi, lo


def plane_bound(xs):
    return np.maximum(2.0 ** -22 * A(np.asarray(xs, F64)), 2.0 ** -25)


# ---------------------------------------------------------------------------------------------- the definitions
# Every definition takes the case's input dict p and returns {output: array} and, in fp64 without perm, {"b_" + output: bound}.
# dt = float32 is the plain numpy fp32 evaluation of the same expressions; perm (a name) evaluates the sums on permuted operands.

def rmsnorm_bwd(p, dt=F64, perm=None, mut=None):
    x, w, dh, dres = p["x"], p["w"], p["dh"], p.get("dres")
    rows, d = x.shape
    pc, pr = _perm(d, perm), _perm(rows, perm)
    inv = np.argsort(pc)
    X, W, G = x[:, pc].astype(dt), w[pc].astype(dt), dh[:, pc].astype(dt)
    post, eps = dt(p["post"]), dt(p["eps"])
    rs = dt(1) / np.sqrt((X * X).sum(1) / dt(d) + eps)
    g = G * post * W
    m = (g * X).sum(1) if mut == "no_mean_div" else (g * X).sum(1) / dt(d)
    rs3 = rs * rs if mut == "rs2" else rs * rs * rs
    c = rs3 * m
    if mut == "post_once":
        c = c / post
    t1, t2 = rs[:, None] * g, X * c[:, None]
    dx = t1 - t2
    if dres is not None:
        R = dres[:, pc].astype(dt)
        if mut == "dres_rows34":
            R = np.where((np.arange(rows) % 16 >= 8)[:, None], dt(0), R)
        dx = dx + R
    a = G * post * X * rs[:, None]
    nblk = (rows + 15) // 16
    w_part = np.stack([a[16 * b:16 * b + 16][_perm(min(16, rows - 16 * b), perm)].sum(0) for b in range(nblk)])
    live = rows - rows % 16 if (mut == "last_block_dw" and rows % 16) else rows
    dw = a[:live][_perm(live, perm)].sum(0) if live else np.zeros(d, dt)
    if mut == "last_block_dw" and rows % 16:
        w_part[-1] = 0
    dw0 = p.get("dw0")
    if dw0 is not None and p.get("accumulate"):
        dw = dw + dw0[pc].astype(dt)
    res = dict(dx=dx[:, inv], w_part=w_part[:, inv], dw=dw[inv])
    if dt is F64 and perm is None and mut is None:
        er = e_rs(d)
        E_c = rs3 / d * ((d + 3) * U * A(G * W * X * post).sum(1) + d * UF) + A(c) * (3 * er + 4 * U)
        b = A(t1) * (er + 3 * U) + A(X) * E_c[:, None] + U * A(t2) + U * (A(t1) + A(t2)) + 4 * UF
        if dres is not None:
            b = b + U * A(dx)
        aa = A(a)
        res["b_dx"] = b
        res["b_w_part"] = np.stack([aa[16 * k:16 * k + 16].sum(0) * (er + 3 * U + 18 * U) + U * A(w_part[k]) + 16 * UF for k in range(nblk)])
        res["b_dw"] = aa.sum(0) * (er + 3 * U + (rows + 2) * U) + U * A(dw) + rows * UF
    return res


def colsum(parts, dt=F64, perm=None, mut=None):
    """out[k] = sum_p parts[p][k]."""
    n = parts.shape[0]
    live = 16 * (n // 16) if mut == "colsum_floor16" else n
    P = parts[:live][_perm(live, perm)].astype(dt)
    out = P.sum(0) if live else np.zeros(parts.shape[1], dt)
    res = dict(out=out)
    if dt is F64 and perm is None and mut is None:
        res["b_out"] = (n - 1) * U * A(P).sum(0)
    return res


def sum_selected(p, dt=F64, perm=None, mut=None):
    src, sel, out0 = p["src"], p["sel"], p["out0"]
    rows = src.shape[0]
    live = 16 * (rows // 16) if mut == "colsum_floor16" else rows
    pr = _perm(live, perm)
    S = np.where((sel[:live][pr] < 0)[:, None], src[:live][pr].astype(dt), dt(0))
    out = out0.astype(dt) + (S.sum(0) if live else 0)
    res = dict(out=out)
    if dt is F64 and perm is None and mut is None:
        cnt = int((sel < 0).sum())
        res["b_out"] = (cnt + 1) * U * A(S).sum(0) + U * A(out)
    return res


def _clamp(c, V):
    return np.clip(c, 0, V - 1)


def norm_rows(x, w, eps, post, dt, pc):
    X, W = x[:, pc].astype(dt), w[pc].astype(dt)
    d = x.shape[1]
    rs = dt(1) / np.sqrt((X * X).sum(1) / dt(d) + dt(eps))
    h = W * (X * rs[:, None])
    if post != 1.0:
        h = h * dt(post)
    return h, rs


def gold_scores(p, dt=F64, perm=None, mut=None):
    """x [S L, d], ln, out_embeds [L, V, d], codes [S, L] -> scores [S L] and the normalised rows (hidden)."""
    x, E, codes = p["x"], p["E"], p["codes"]
    rows, d = x.shape
    L, V = E.shape[0], E.shape[1]
    pc = _perm(d, perm)
    h, _ = norm_rows(x, p["ln"], p["eps"], p["post"], dt, pc)
    pos = np.arange(rows) % L
    if mut == "codebook_next":
        pos = (pos + 1) % L
    e = E[pos, _clamp(codes.reshape(-1), V)][:, pc].astype(dt)
    res = dict(scores=(h * e).sum(1), hidden=h[:, np.argsort(pc)])
    if dt is F64 and perm is None and mut is None:
        E_h = A(h) * (e_rs(d) + 3 * U) + UF
        res["b_hidden"] = E_h
        res["b_scores"] = (A(e) * E_h).sum(1) + (d + 1) * U * A(h * e).sum(1) + d * UF
    return res


def gold_score_bwd(p, dt=F64, perm=None, mut=None):
    x, Ef, idx, g = p["x"], p["E"].reshape(-1, p["x"].shape[1]), p["out_idx"], p["dscores"].astype(dt)
    d = x.shape[1]
    pc = np.arange(d)
    h, _ = norm_rows(x, p["ln"], p["eps"], p["post"], dt, pc)
    e = Ef[idx].astype(dt)
    res = dict(de=g[:, None] * h, dh=g[:, None] * e)
    if dt is F64 and mut is None:
        res["b_de"] = A(res["de"]) * (e_rs(d) + 4 * U) + UF
        res["b_dh"] = U * A(res["dh"]) + UF
    return res


def gold_rowdot(p, dt=F64, perm=None, mut=None):
    hd, Ef, idx = p["hd"], p["E"].reshape(-1, p["hd"].shape[1]), p["out_idx"]
    d = hd.shape[1]
    pc = _perm(d, perm)
    h, e = hd[:, pc].astype(dt), Ef[idx][:, pc].astype(dt)
    g = p["dscores"].astype(dt)
    res = dict(scores=(h * e).sum(1), de=g[:, None] * hd.astype(dt), dh=g[:, None] * Ef[idx].astype(dt))
    if dt is F64 and perm is None and mut is None:
        res["b_scores"] = (d + 1) * U * A(h * e).sum(1) + d * UF
        res["b_de"] = U * A(res["de"]) + UF
        res["b_dh"] = U * A(res["dh"]) + UF
    return res


def _mse_loss_bound(dl, E_dl, loss):
    return (2 * A(dl) * E_dl + E_dl ** 2 + U * (A(dl) + E_dl) ** 2).mean(-1) + U * A(loss) + UF


def margin_mse(p, dt=F64, perm=None, mut=None):
    """scores [bz, 2, L], teacher_pos / teacher_neg [np, bz], prefix_lens [np] -> losses [np], margins [np, bz]."""
    sc, tp, tn, pl = p["scores"], p["teacher_pos"].astype(dt), p["teacher_neg"].astype(dt), p["prefix_lens"]
    bz, _, L = sc.shape
    flat = np.concatenate([sc.reshape(-1), np.zeros(2 * 64, F32)])
    losses, margins, bl, bm = [], [], [], []
    for q, k0 in enumerate(pl):
        k = int(k0) if mut == "prefix_unclamped" else min(int(k0), L)
        if mut == "prefix_unclamped":      # reads on behind the row, into whatever follows
            pos = np.stack([flat[b * 2 * L:b * 2 * L + k] for b in range(bz)])
            neg = np.stack([flat[b * 2 * L + L:b * 2 * L + L + k] for b in range(bz)])
        else:
            pos, neg = sc[:, 0, :k], sc[:, 1, :k]
        pk = _perm(k, perm)
        pos, neg = pos[:, pk].astype(dt), neg[:, pk].astype(dt)
        sm = pos.sum(1) - neg.sum(1)
        tm = tp[q] - tn[q]
        dl = sm - tm
        sq = (dl * dl).astype(F64)          # the kernel adds the squares in double
        loss = sq[_perm(bz, perm)].sum() / bz
        losses.append(dt(loss)); margins.append(sm)
        if dt is F64 and perm is None and mut is None:
            E_sm = (k + 1) * U * (A(pos).sum(1) + A(neg).sum(1))
            E_dl = E_sm + U * A(tm) + U * A(dl)
            bm.append(E_sm); bl.append(_mse_loss_bound(dl, E_dl, loss))
    res = dict(losses=np.array(losses), margins=np.stack(margins))
    if bl:
        res["b_losses"], res["b_margins"] = np.array(bl), np.stack(bm)
    return res


def margin_mse_bwd(p, dt=F64, perm=None, mut=None):
    """margins [np, bz] (given) -> dscores [bz, 2, L]."""
    m, tp, tn, pl = p["margins"].astype(dt), p["teacher_pos"].astype(dt), p["teacher_neg"].astype(dt), p["prefix_lens"]
    bz, L = p["bz"], p["L"]
    npf = len(pl)
    coef = dt(1 if mut == "one_over_bz" else 2) / dt(bz)
    tm = tp - tn
    term = coef * (m - tm)                                             # [np, bz]
    on = (np.arange(L)[None, :] < np.asarray(pl)[:, None]).astype(dt)   # [np, L]
    order = _perm(npf, perm)
    g = np.einsum("pb,pl->bl", term[order], on[order]) if dt is F64 else sum(term[q][:, None] * on[q][None, :] for q in order)
    ds = np.stack([g, g if mut == "neg_sign_lost" else -g], axis=1)
    res = dict(dscores=ds)
    if dt is F64 and perm is None and mut is None:
        E_p = A(coef) * (U * A(tm) + U * A(m - tm)) + 2 * U * A(term)
        b = np.einsum("pb,pl->bl", E_p + npf * U * A(term), on) + npf * UF
        res["b_dscores"] = np.stack([b, b], axis=1)
    return res


def dense_mse(p, dt=F64, perm=None, mut=None):
    """hF [3 bz, d] -> scores [bz, 2], margins, g, loss; dhF from the g given in p["g_in"] (the backward launch's input)."""
    hF, tp, tn = p["hF"], p["teacher_pos"].astype(dt), p["teacher_neg"].astype(dt)
    bz, d = hF.shape[0] // 3, hF.shape[1]
    pc = _perm(d, perm)
    q, dp, dn = (hF[i * bz:(i + 1) * bz][:, pc].astype(dt) for i in range(3))
    sp, sn = (q * dp).sum(1), (q * dn).sum(1)
    m = sp - sn
    tm = tp - tn
    coef = dt(1 if mut == "one_over_bz" else 2) / dt(bz)
    g = coef * (m - tm)
    dl = m - tm
    loss = (dl * dl).astype(F64)[_perm(bz, perm)].sum() / bz
    gi = p["g_in"].astype(dt)[:, None]
    Q, DP, DN = (hF[i * bz:(i + 1) * bz].astype(dt) for i in range(3))
    dhF = np.concatenate([gi * (DP - DN), gi * Q, -gi * Q])
    res = dict(scores=np.stack([sp, sn], 1), margins=m, g=g, loss=np.array([dt(loss)]), dhF=dhF)
    if dt is F64 and perm is None and mut is None:
        E_sp, E_sn = (d + 1) * U * A(q * dp).sum(1) + d * UF, (d + 1) * U * A(q * dn).sum(1) + d * UF
        E_m = E_sp + E_sn + U * A(m)
        E_dl = E_m + U * A(tm) + U * A(dl)
        res.update(b_scores=np.stack([E_sp, E_sn], 1), b_margins=E_m, b_g=A(coef) * E_dl + 2 * U * A(g) + UF,
                   b_loss=np.array([_mse_loss_bound(dl, E_dl, loss)]),
                   b_dhF=np.concatenate([2 * U * A(gi * (DP - DN)) + UF, U * A(gi * Q) + UF, U * A(gi * Q) + UF]))
    return res


def s2s_head(p, dt=F64, perm=None, mut=None):
    """hF [bz L, d], E [L, V, d], labels [bz L] -> dlogits [bz L, V], row_loss, label_lp, loss; dH, dE from the dlogits given in
    p["dl_in"] (the backward launch's input)."""
    hF, E, labels = p["hF"], p["E"], p["labels"]
    L, V, d = E.shape
    n = hF.shape[0]
    bz = n // L
    pc = _perm(d, perm)
    pos = np.arange(n) % L
    Epos = E[(pos + 1) % L] if mut == "codebook_next" else E[pos]          # [n, V, d]
    h = hF[:, pc].astype(dt)
    Ep = Epos[:, :, pc].astype(dt)
    l = np.einsum("nd,nvd->nv", h, Ep) if dt is F64 else (h[:, None, :] * Ep).sum(2)
    pv = _perm(V, perm)
    mx = l.max(1)
    lse = mx + np.log(np.exp(l - mx[:, None])[:, pv].sum(1))
    lab = _clamp(labels, V)
    inv_n = dt(1) / dt(bz if mut == "inv_n_bz" else n)
    pr = np.exp(l - lse[:, None])
    oh = np.zeros((n, V), dt)
    if mut == "onehot_unclamped":
        ok = (labels >= 0) & (labels < V)
        oh[np.arange(n)[ok], labels[ok]] = 1
    else:
        oh[np.arange(n), lab] = 1
    dlg = (pr - oh) * inv_n
    ll = l[np.arange(n), lab]
    row_loss = lse - ll
    loss = row_loss.astype(F64)[_perm(n, perm)].sum() * F64(dt(1) / dt(n))
    dl = p["dl_in"].astype(dt)                                             # [n, V]
    hb, Eb = hF.astype(dt), E.astype(dt)
    pV, pB = _perm(V, perm), _perm(bz, perm)
    dl3, h3 = dl.reshape(bz, L, V), hb.reshape(bz, L, d)
    if dt is F64:
        dH = np.einsum("blv,lvc->blc", dl3[:, :, pV], Eb[:, pV]).reshape(n, d)
        dE = np.einsum("blv,blc->lvc", dl3[pB], h3[pB])
    else:
        dH = np.stack([np.stack([(dl3[b, i, pV][:, None] * Eb[i, pV]).sum(0) for i in range(L)]) for b in range(bz)]).reshape(n, d)
        dE = np.stack([(dl3[pB, i][:, :, None] * h3[pB, i][:, None, :]).sum(0) for i in range(L)])
    res = dict(dlogits=dlg, row_loss=row_loss, label_lp=-row_loss, loss=np.array([dt(loss)]), dH=dH, dE=dE)
    if dt is F64 and perm is None and mut is None:
        E_l = (d + 1) * U * np.einsum("nd,nvd->nv", A(h), A(Ep)) + d * UF
        D = E_l.max(1)
        spread = l.max(1) - l.min(1)
        E_lse = D + (spread + 8 + V) * U + 4 * U * math.log(V) + U * A(lse)
        b_row = E_lse + E_l[np.arange(n), lab] + U * A(row_loss)
        res.update(b_row_loss=b_row, b_label_lp=b_row,
                   b_dlogits=inv_n * (pr * (E_l + E_lse[:, None] + U * A(l - lse[:, None]) + 4 * U) + U * A(pr - oh)) + 2 * U * A(dlg) + UF,
                   b_loss=np.array([b_row.mean() + 2 * U * A(loss)]),
                   b_dH=(V + 1) * U * np.einsum("blv,lvc->blc", A(dl3), A(Eb)).reshape(n, d) + V * UF,
                   b_dE=(bz + 1) * U * np.einsum("blv,blc->lvc", A(dl3), A(h3)) + bz * UF)
    return res


def train_indices(codes, V, mut=None):
    """codes [S, L] -> in_idx, out_idx [S L] (int32)."""
    S, L = codes.shape
    c = _clamp(codes, V)
    i = np.arange(L)[None, :]
    out_idx = (i * V + c).astype(np.int32)
    prev = np.concatenate([np.zeros((S, 1), codes.dtype), c[:, :-1]], 1)
    in_idx = np.where(i == 0, -1, (i - 1) * V + prev).astype(np.int32)
    if mut == "in_idx_i":
        in_idx = np.where(i == 0, -1, i * V + c).astype(np.int32)
    return in_idx.reshape(-1), out_idx.reshape(-1)


def dec_embed(p, mut=None):
    """start [d], in_embeds [L, V, d], codes [S, L] -> the fp32 rows (exact), the planes of rows / 16 and the rows' ssq with bounds."""
    start, T, codes = p["start"], p["in_embeds"], p["codes"]
    L, V, d = T.shape
    in_idx, _ = train_indices(codes, V, mut)
    Tf = T.reshape(-1, d)
    out = np.where((in_idx < 0)[:, None], start[None, :], Tf[np.maximum(in_idx, 0)]).astype(F32)
    xs = out * F32(X_PLANE_SCALE)
    hi, lo = split_planes(xs)
    E_x = plane_bound(xs) / X_PLANE_SCALE
    x64 = out.astype(F64)
    ss = (x64 * x64).sum(1)
    fix = np.floor(ss * SSQ_FIX + 0.5)
    b_plain = SSQ_FIX * (d + 1) * U * ss + U * fix + 1
    return dict(out=out, hi=hi, lo=lo, xs=xs.astype(F64), b_planes=plane_bound(xs), ssq=fix, b_ssq_plain=b_plain,
                b_ssq_planes=b_plain + SSQ_FIX * (2 * A(x64) * E_x + E_x ** 2).sum(1))


def scatter_flush(p, dt=F64, mut=None):
    """src [rows, d], idx [rows] (< 0 skipped), table rows T -> table [T, d] (from zero) and its bound; dt float32: the kernel's own
    arithmetic restated (llrint to 2^-32, exact integer sums, one rounding to fp32)."""
    src, idx, T = p["src"], p["idx"], p["table"]
    d = src.shape[1]
    ii = np.where(idx < 0, 0, idx) if mut == "start_row_scattered" else idx
    keep = ii >= 0
    cnt = np.bincount(ii[keep], minlength=T).astype(F64)
    if dt is F64:
        tab = np.zeros((T, d), F64)
        np.add.at(tab, ii[keep], src[keep].astype(F64))
        return dict(table=tab, b_table=cnt[:, None] * 2.0 ** -33 + 2 * U * A(tab), count=cnt,
                    wraps=bool((A(tab) >= 2.0 ** 31).any()))
    acc = np.zeros((T, d), np.int64)
    np.add.at(acc, ii[keep], np.rint(src[keep].astype(F64) * GRAD_FIX).astype(np.int64))
    return dict(table=(acc.astype(F64) / GRAD_FIX).astype(F32))


def relu_gate(dy, act, mut=None):
    return np.where((act >= 0) if mut == "relu_ge" else (act > 0), dy, F32(0)).astype(F32)


def transposed(bits_or_vals, Rpad, ld, fill, mut=None):
    """[R, C] -> [C, ld]: the transpose in columns < R, zeros up to Rpad, `fill` (the canary) behind."""
    R, C = bits_or_vals.shape
    out = np.full((C, ld), fill, bits_or_vals.dtype)
    out[:, :Rpad] = 0
    out[:, :R] = bits_or_vals.T
    if mut == "pad_from_neighbour" and Rpad > R:
        k = Rpad - R
        out[:, R:Rpad] = np.resize(bits_or_vals.T[:, max(0, R - k):R], (C, k)) if R else 0
    return out


# ---------------------------------------------------------------------------------------------- launches, buffers, expectations
CANARY32 = 0x7FC0BEEF
CANARY16 = 0x7EEF           # a NaN in f16 and in bf16
CANARY64 = 0x7FF8BEEF7FC0BEEF


@dataclass
class Launch:
    op: str
    src: tuple                      # buffer names (None = NULL)
    dst: tuple
    dims: tuple
    f: tuple = ()


@dataclass
class Expect:
    """What a buffer must hold at the end. bound None: bit equality with ref (its dtype the buffer's). written: bool mask of the
    elements the launches own (None = all); every other element keeps the canary."""
    ref: np.ndarray
    bound: Optional[np.ndarray] = None
    written: Optional[np.ndarray] = None
    decode: Optional[Callable] = None      # got (raw buffer) -> float64 values to hold against ref / bound
    flips: Optional[np.ndarray] = None     # rmsnorm_bf16_T: (lo_key, hi_key) admitted neighbours, see check in the GPU file


@dataclass
class Case:
    name: str
    kernel: str                     # the launcher the record files the case under
    bufs: Dict[str, np.ndarray] = field(default_factory=dict)      # inputs and initialised outputs
    outs: Dict[str, tuple] = field(default_factory=dict)           # canary-filled outputs: name -> (shape, dtype)
    launches: List[Launch] = field(default_factory=list)
    expect: Dict[str, Expect] = field(default_factory=dict)
    p: dict = field(default_factory=dict)                          # what the definition takes (the host file)
    define: Optional[Callable] = None                              # the definition (dt, perm, mut) of the bound-checked outputs
    keys: Dict[str, str] = field(default_factory=dict)             # buffer name -> key of the definition's result


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def case_rmsnorm_bwd(rows, d, dres, post_scaled, with_dw, accumulate=0):
    nm = f"rmsnorm_bwd_r{rows}_d{d}" + ("_dres" if dres else "") + ("_post" if post_scaled else "") + ("" if with_dw else "_nodw") + ("_acc" if accumulate else "")
    post = float(F32(d ** -0.5)) if post_scaled else 1.0
    p = dict(x=act_rows(nm + "/x", rows, d), w=weight_row(nm + "/w", d), dh=grad_rows(nm + "/dh", rows, d), eps=EPS, post=post,
             accumulate=accumulate)
    if dres:
        p["dres"] = grad_rows(nm + "/dres", rows, d, 0.25)
    if accumulate:
        p["dw0"] = unif(nm + "/dw0", (d,), 3.0)
    r = rmsnorm_bwd(p)
    nblk = (rows + 15) // 16
    c = Case(nm, "launch_rmsnorm_bwd", p=p, define=rmsnorm_bwd, keys=dict(dx="dx", w_part="w_part", dw="dw"))
    c.bufs = {k: p[k] for k in ("x", "w", "dh") + (("dres",) if dres else ())}
    c.outs = dict(dx=((rows, d), F32), w_part=((nblk, d), F32))
    if with_dw:
        if accumulate:
            c.bufs["dw"] = p["dw0"]
        else:
            c.outs["dw"] = ((d,), F32)
    c.launches = [Launch("RMSNORM_BWD", ("x", "w", "dh", "dres" if dres else None), ("dx", "w_part", "dw" if with_dw else None),
                         (rows, d, accumulate), (EPS, post))]
    c.expect = dict(dx=Expect(r["dx"], r["b_dx"]), w_part=Expect(r["w_part"], r["b_w_part"]))
    if with_dw:
        c.expect["dw"] = Expect(r["dw"], r["b_dw"])
    return c


def case_colsum_multi(d, nparts=(1, 16, 17, 18)):
    nm = f"colsum_multi_d{d}_" + "_".join(str(n) for n in nparts)
    c = Case(nm, "launch_colsum_multi")
    parts = [grad_rows(f"{nm}/part{i}", n, d) for i, n in enumerate(nparts)]
    c.p = dict(parts=parts)
    c.define = lambda p, dt=F64, perm=None, mut=None: _multi(p, dt, perm, mut)
    for i, P in enumerate(parts):
        c.bufs[f"part{i}"] = P
        c.outs[f"out{i}"] = ((d,), F32)
        r = colsum(P)
        c.expect[f"out{i}"] = Expect(r["out"], r["b_out"])
        c.keys[f"out{i}"] = f"out{i}"
    k = len(parts)
    c.launches = [Launch("COLSUM_MULTI", tuple(f"part{i}" for i in range(k)), tuple(f"out{i}" for i in range(k)),
                         (d, k) + tuple(nparts))]
    return c


def _multi(p, dt, perm, mut):
    res = {}
    for i, P in enumerate(p["parts"]):
        r = colsum(P, dt, perm, mut)
        res[f"out{i}"] = r["out"]
        if "b_out" in r:
            res[f"b_out{i}"] = r["b_out"]
    return res


def _codes(name, S, L, V):
    c = synth.randint("train_rows/codes/" + name, (S, L), 0, V).astype(np.int32)
    flat = c.reshape(-1)
    flat[0::5] = -1          # the clamp, both ends
    flat[3::7] = V
    return flat.reshape(S, L)


def _gold_inputs(nm, S, L, d, V, post_scaled):
    rows = S * L
    x = act_rows(nm + "/x", rows, d)
    hi, lo = split_planes(x * F32(X_PLANE_SCALE))
    x = ((hi.astype(F32) + lo.astype(F32)) * F32(1.0 / X_PLANE_SCALE)).astype(F32)      # exactly what the planes hold
    E = unif(nm + "/E", (L, V, d))
    E[:, :, 5::8] = ((np.arange(V) % 31 + 1) / 16.0).astype(F32)[None, :, None]            # the code's signature
    E[:, :, 3::8] += (np.arange(L) + 1).astype(F32)[:, None, None] / 4                     # the position's
    return dict(x=x, hi=hi, lo=lo, ln=weight_row(nm + "/ln", d), E=E, codes=_codes(nm, S, L, V), eps=EPS,
                post=float(F32(d ** -0.5)) if post_scaled else 1.0)


def case_gold_scores(S, L, d, V=64, mode="f32", post_scaled=False):
    nm = f"gold_scores_S{S}_L{L}_d{d}_{mode}" + ("_post" if post_scaled else "")
    p = _gold_inputs(f"gold_S{S}_L{L}_d{d}", S, L, d, V, post_scaled)
    r = gold_scores(p)
    rows = S * L
    c = Case(nm, "launch_gold_scores", p=p, define=gold_scores)
    c.bufs = dict(ln=p["ln"], E=p["E"], codes=p["codes"])
    ps = rows * d + 64
    if mode == "planes":
        planes = np.zeros(2 * ps, np.float16)
        planes[:rows * d] = p["hi"].reshape(-1)
        planes[ps:ps + rows * d] = p["lo"].reshape(-1)
        c.bufs["planes"] = planes
    else:
        c.bufs["x"] = p["x"]
    src = (None if mode == "planes" else "x", "ln", "E", None if mode == "hidden" else "codes", "planes" if mode == "planes" else None)
    if mode == "hidden":
        c.outs = dict(hidden=((rows, d), F32))
        c.expect = dict(hidden=Expect(r["hidden"], r["b_hidden"]))
        c.keys = dict(hidden="hidden")
        dst = (None, "hidden")
    else:
        c.outs = dict(scores=((rows,), F32))
        c.expect = dict(scores=Expect(r["scores"], r["b_scores"]))
        c.keys = dict(scores="scores")
        dst = ("scores",)
    c.launches = [Launch("GOLD_SCORES", src, dst, (S, L, d, V, ps), (EPS, p["post"]))]
    return c


def case_gold_bwd(S, L, d, V=64, rowdot=False):
    nm = f"{'gold_rowdot' if rowdot else 'gold_score_bwd'}_S{S}_L{L}_d{d}"
    p = _gold_inputs(f"gold_S{S}_L{L}_d{d}", S, L, d, V, True)
    rows = S * L
    _, p["out_idx"] = train_indices(p["codes"], V)
    p["dscores"] = grad_rows(nm + "/ds", rows, 8)[:, 0].copy()
    c = Case(nm, "launch_gold_rowdot" if rowdot else "launch_gold_score_bwd", p=p)
    if rowdot:
        p["hd"] = act_rows(nm + "/hd", rows, d)
        r = gold_rowdot(p)
        c.define = gold_rowdot
        c.bufs = dict(hd=p["hd"], E=p["E"], out_idx=p["out_idx"], dscores=p["dscores"])
        c.outs = dict(scores=((rows,), F32), dh=((rows, d), F32), de=((rows, d), F32))
        c.launches = [Launch("GOLD_ROWDOT", ("hd", "E", "out_idx", None), ("scores",), (rows, d)),
                      Launch("GOLD_ROWDOT", ("hd", "E", "out_idx", "dscores"), (None, "dh", "de"), (rows, d))]
        c.expect = {k: Expect(r[k], r["b_" + k]) for k in ("scores", "dh", "de")}
    else:
        r = gold_score_bwd(p)
        c.define = gold_score_bwd
        c.bufs = dict(x=p["x"], ln=p["ln"], E=p["E"], out_idx=p["out_idx"], dscores=p["dscores"])
        c.outs = dict(dh=((rows, d), F32), de=((rows, d), F32))
        c.launches = [Launch("GOLD_SCORE_BWD", ("x", "ln", "E", "out_idx", "dscores"), ("dh", "de"), (rows, d), (EPS, p["post"]))]
        c.expect = {k: Expect(r[k], r["b_" + k]) for k in ("dh", "de")}
    c.keys = {k: k for k in c.expect}
    return c


def _margin_inputs(bz, L, prefixes):
    nm = f"margin_bz{bz}_np{len(prefixes)}"
    sc = grad_rows(nm + "/scores", bz * 2, L, 4.0).reshape(bz, 2, L)
    sc[:, 1] -= F32(1.0)
    npf = len(prefixes)
    return dict(scores=sc, teacher_pos=unif(nm + "/tp", (npf, bz), 8.0), teacher_neg=unif(nm + "/tn", (npf, bz), 8.0),
                prefix_lens=_i32(prefixes), bz=bz, L=L)


def case_margin_mse(bz, prefixes, L=8):
    p = _margin_inputs(bz, L, prefixes)
    r = margin_mse(p)
    npf = len(prefixes)
    c = Case(f"margin_mse_bz{bz}_np{npf}", "launch_margin_mse", p=p, define=margin_mse, keys=dict(losses="losses", margins="margins"))
    c.bufs = {k: p[k] for k in ("scores", "teacher_pos", "teacher_neg", "prefix_lens")}
    c.outs = dict(losses=((npf,), F32), margins=((npf, bz), F32))
    c.launches = [Launch("MARGIN_MSE", ("scores", "teacher_pos", "teacher_neg", "prefix_lens"), ("losses", "margins"), (npf, bz, L))]
    c.expect = dict(losses=Expect(r["losses"], r["b_losses"]), margins=Expect(r["margins"], r["b_margins"]))
    return c


def case_margin_mse_bwd(bz, prefixes, L=8, own=False):
    """own: the margins are the definition's, rounded to fp32; otherwise the forward launch's own output feeds the backward."""
    p = _margin_inputs(bz, L, prefixes)
    npf = len(prefixes)
    fwd = margin_mse(p)
    c = Case(f"margin_mse_bwd_bz{bz}_np{npf}" + ("_def" if own else "_fwd"), "launch_margin_mse_bwd", p=p, define=margin_mse_bwd,
             keys=dict(dscores="dscores"))
    c.bufs = {k: p[k] for k in ("scores", "teacher_pos", "teacher_neg", "prefix_lens")}
    p["margins"] = fwd["margins"].astype(F32)
    c.outs = dict(dscores=((bz, 2, L), F32))
    if own:
        c.bufs["margins"] = p["margins"]
    else:
        c.outs.update(losses=((npf,), F32), margins=((npf, bz), F32))
        c.launches = [Launch("MARGIN_MSE", ("scores", "teacher_pos", "teacher_neg", "prefix_lens"), ("losses", "margins"), (npf, bz, L))]
    c.launches.append(Launch("MARGIN_MSE_BWD", ("margins", "teacher_pos", "teacher_neg", "prefix_lens"), ("dscores",), (npf, bz, L)))
    r = margin_mse_bwd(p)
    b = r["b_dscores"]
    if not own:      # the forward's margins differ from the definition's by up to E_sm: (2 / bz) E_sm per prefix on top
        on = (np.arange(L)[None, :] < np.asarray(prefixes)[:, None]).astype(F64)
        extra = np.einsum("pb,pl->bl", (2.0 / bz) * (1 + 2 * U) * (fwd["b_margins"] + U * A(fwd["margins"])), on)
        b = b + np.stack([extra, extra], 1)
    c.expect = dict(dscores=Expect(r["dscores"], b))
    return c


def case_dense_mse(bz, d):
    nm = f"dense_mse_bz{bz}_d{d}"
    hF = act_rows(nm + "/hF", 3 * bz, d)
    hF[:, 5::8] = ((np.arange(3 * bz) % 61 + 1) / 8.0).astype(F32)[:, None]
    p = dict(hF=hF, teacher_pos=unif(nm + "/tp", (bz,), 8.0), teacher_neg=unif(nm + "/tn", (bz,), 8.0),
             g_in=grad_rows(nm + "/g", bz, 8)[:, 0].copy())
    r = dense_mse(p)
    c = Case(nm, "launch_dense_mse_head", p=p, define=dense_mse, keys={k: k for k in ("scores", "margins", "g", "loss", "dhF")})
    c.bufs = dict(hF=hF, teacher_pos=p["teacher_pos"], teacher_neg=p["teacher_neg"], g_in=p["g_in"])
    c.outs = dict(scores=((bz, 2), F32), margins=((bz,), F32), g=((bz,), F32), loss=((1,), F32), dhF=((3 * bz, d), F32))
    c.launches = [Launch("DENSE_MSE_FWD", ("hF", "teacher_pos", "teacher_neg"), ("scores", "margins", "g", "loss"), (bz, d)),
                  Launch("DENSE_MSE_BWD", ("hF", "g_in"), ("dhF",), (bz, d))]
    c.expect = {k: Expect(r[k], r["b_" + k]) for k in c.keys}
    return c


def case_s2s_head(bz, L, d, V, odd_labels=False):
    nm = f"s2s_head_bz{bz}_L{L}_d{d}_V{V}" + ("_clamp" if odd_labels else "")
    n = bz * L
    hF = unif(nm + "/hF", (n, d))
    E = unif(nm + "/E", (L, V, d))
    E[:, :, 3::8] += (np.arange(L) + 1).astype(F32)[:, None, None] / 8
    pos = np.arange(n) % L
    l64 = np.einsum("nd,nvd->nv", hF.astype(F64), E[pos].astype(F64))
    for r_ in range(1, n, 2):                  # odd rows: a spread of 80 between the largest and the smallest logit
        hF[r_] = (hF[r_].astype(F64) * (80.0 / (l64[r_].max() - l64[r_].min()))).astype(F32)
    for r_ in range(0, n, 4):                  # every fourth: flat (all logits within 1e-3)
        hF[r_] *= F32(1e-4)
    labels = synth.randint("train_rows/labels/" + nm, (n,), 0, V).astype(np.int32)
    labels[0::3] = 0
    labels[1::3] = V - 1
    if odd_labels:
        labels[0::4] = -1
        labels[2::4] = V
    p = dict(hF=hF, E=E, labels=labels)
    p["dl_in"] = np.zeros((n, V), F32)
    p["dl_in"] = s2s_head(p)["dlogits"].astype(F32)
    r = s2s_head(p)
    c = Case(nm, "launch_s2s_head", p=p, define=s2s_head,
             keys={k: k for k in ("dlogits", "row_loss", "label_lp", "loss", "dH", "dE")})
    c.bufs = dict(hF=hF, E=E, labels=labels, dl_in=p["dl_in"])
    c.outs = dict(dlogits=((n, V), F32), row_loss=((n,), F32), label_lp=((n,), F32), loss=((1,), F32), dH=((n, d), F32), dE=((L, V, d), F32))
    c.launches = [Launch("S2S_HEAD_FWD", ("hF", "E", "labels"), ("dlogits", "row_loss", "label_lp", "loss"), (bz, L, d, V)),
                  Launch("S2S_HEAD_BWD", ("hF", "E", "dl_in"), ("dH", "dE"), (bz, L, d, V))]
    c.expect = {k: Expect(r[k], r["b_" + k]) for k in c.keys}
    return c


def _scatter_idx(nm, rows, T, pattern):
    if pattern == "one":
        return np.full(rows, T // 2, np.int32)
    if pattern == "own":
        return np.arange(rows, dtype=np.int32)
    idx = synth.randint("train_rows/idx/" + nm, (rows,), 0, T).astype(np.int32)
    idx[0::3] = -1
    return idx


def case_scatter(rows, d, pattern, mag_exp=0):
    nm = f"scatter_r{rows}_d{d}_{pattern}" + (f"_2e-{mag_exp}" if mag_exp else "")
    T = rows if pattern == "own" else 7
    src = grad_rows(f"scatter_r{rows}_d{d}/src", rows, d)
    src = (src * F32(2.0 ** -mag_exp)).astype(F32)
    p = dict(src=src, idx=_scatter_idx(nm, rows, T, pattern), table=T, mag_exp=mag_exp)
    r = scatter_flush(p)
    assert not r["wraps"]
    c = Case(nm, "launch_scatter_rows_fix+launch_fix_flush", p=p)
    c.bufs = dict(src=src, idx=p["idx"], acc=np.zeros((T, d), np.int64), table=np.zeros((T, d), F32))
    flush = Launch("FIX_FLUSH", (), ("acc", "table"), (T * d,))
    c.launches = [Launch("SCATTER_FIX", ("src", "idx"), ("acc",), (rows, d)), flush, flush]     # the second flush changes nothing
    c.expect = dict(table=Expect(r["table"], r["b_table"]), acc=Expect(np.zeros((T, d), np.int64)))
    return c


def case_sum_selected(rows, d):
    nm = f"sum_selected_r{rows}_d{d}"
    sel = _scatter_idx(nm, rows, 7, "third")
    if rows <= 17:
        sel[-1] = -1            # the last row counts
    p = dict(src=grad_rows(nm + "/src", rows, d), sel=sel, out0=unif(nm + "/out0", (d,), 2.0))
    r = sum_selected(p)
    c = Case(nm, "launch_sum_selected_rows", p=p, define=sum_selected, keys=dict(out="out"))
    c.bufs = dict(src=p["src"], sel=sel, out=p["out0"])
    c.launches = [Launch("SUM_SELECTED", ("src", "sel"), ("out",), (rows, d))]
    c.expect = dict(out=Expect(r["out"], r["b_out"]))
    return c


def case_dec_embed(S, L, d, V=64, planes=False):
    nm = f"dec_embed_S{S}_L{L}_d{d}" + ("_planes" if planes else "")
    rows = S * L
    T = unif(f"dec_embed_d{d}/T", (L, V, d), 2.0)
    T[:, :, 5::8] = ((np.arange(V) % 31 + 1) / 16.0).astype(F32)[None, :, None]
    T[:, :, 3::8] = (np.arange(L) + 1).astype(F32)[:, None, None] / 4
    p = dict(start=unif(f"dec_embed_d{d}/start", (d,), 1.0), in_embeds=T, codes=_codes(nm, S, L, V), V=V)
    r = dec_embed(p)
    in_idx, out_idx = train_indices(p["codes"], V)
    c = Case(nm, "launch_train_dec_embed", p=p)
    c.bufs = dict(start=p["start"], in_embeds=T, codes=p["codes"])
    c.outs = dict(ssq=((rows,), np.uint64))
    if planes:
        ps = rows * d + 64
        c.outs["planes"] = ((2 * ps,), np.float16)
        written = np.zeros(2 * ps, bool)
        written[:rows * d] = True
        written[ps:ps + rows * d] = True
        ref = np.zeros(2 * ps)
        ref[:rows * d] = r["xs"].reshape(-1)
        bound = np.zeros(2 * ps)
        bound[:rows * d] = r["b_planes"].reshape(-1)
        # held as hi + lo against x / 16: the sum is filed under the hi plane's elements, the lo plane's must merely be written
        c.expect = dict(planes=Expect(ref, bound, written, decode=lambda g, n=rows * d, ps=ps: _planes_sum(g, n, ps)),
                        ssq=Expect(r["ssq"], r["b_ssq_planes"], decode=lambda g: g.astype(F64)))
        c.launches = [Launch("DEC_EMBED", ("start", "in_embeds", "codes"), (None, "planes", "ssq"), (S, L, d, V, ps))]
    else:
        c.outs["out"] = ((rows, d), F32)
        c.expect = dict(out=Expect(r["out"]), ssq=Expect(r["ssq"], r["b_ssq_plain"], decode=lambda g: g.astype(F64)))
        c.launches = [Launch("DEC_EMBED", ("start", "in_embeds", "codes"), ("out", None, "ssq"), (S, L, d, V, 0))]
    c2 = Case(f"train_indices_S{S}_L{L}_d{d}", "launch_train_indices", p=p)
    c2.bufs = dict(codes=p["codes"])
    c2.outs = dict(in_idx=((rows,), np.int32), out_idx=((rows,), np.int32))
    c2.launches = [Launch("TRAIN_INDICES", ("codes",), ("in_idx", "out_idx"), (S, L, V))]
    c2.expect = dict(in_idx=Expect(in_idx), out_idx=Expect(out_idx))
    return [c] if planes else [c, c2]


def _planes_sum(g, n, ps):
    """hi + lo of a two-plane buffer, laid over the hi plane's elements (0 elsewhere)."""
    v = np.zeros(g.shape, F64)
    v[:n] = g[:n].astype(F64) + g[ps:ps + n].astype(F64)
    return v


def _conv_x(nm, R, C, ldi):
    x = np.full((R, ldi), np.nan, F32)           # the columns behind C must not be read
    x[:, :C] = grad_rows(nm + "/x", R, C, 3.0)
    x[:, :C][np.arange(R) % 3 == 2] *= F32(2.0 ** -9)
    return x


def case_relu_bwd(n):
    nm = f"relu_bwd_n{n}"
    dy = unif(nm + "/dy", (n,), 2.0)
    act = unif(nm + "/act", (n,), 1.0)
    act[0::4] = 0.0
    act[1::8] = -0.0
    act[2::16] = F32(1e-45)
    dy[np.arange(n) % 4 == 0] += F32(3.0)        # a gate taken at >= 0 lets these through
    c = Case(nm, "launch_relu_bwd", p=dict(dy=dy, act=act))
    c.bufs = dict(act=act, dy=dy.copy())
    c.launches = [Launch("RELU_BWD", ("act",), ("dy",), (n,))]
    c.expect = dict(dy=Expect(relu_gate(dy, act)))
    return c


def case_absmax2(n0, n1):
    nm = f"absmax2_n{n0}" + (f"_n{n1}" if n1 else "")
    x0 = unif(nm + "/x0", (n0,), 4.0)
    x0[-1] = F32(-7.25)                           # the maximum on the last element
    c = Case(nm, "launch_absmax2", p=dict(n0=n0, n1=n1))
    c.bufs = dict(x0=x0, out=np.zeros(2 if n1 else 1, F32))
    ref = [np.abs(x0).max()]
    if n1:
        x1 = unif(nm + "/x1", (n1,), 4.0)
        x1[0] = F32(9.5)
        c.bufs["x1"] = x1
        ref.append(np.abs(x1).max())
    c.launches = [Launch("ABSMAX2", ("x0", "x1" if n1 else None), ("out",), (n0, n1))]
    c.expect = dict(out=Expect(np.array(ref, F32)))
    return c


def case_transpose_pad(R, C, ldi, Rpad):
    nm = f"transpose_pad_R{R}_C{C}_ldi{ldi}_Rpad{Rpad}"
    x = _conv_x(nm, R, C, ldi)
    c = Case(nm, "launch_transpose_pad", p=dict(x=x, R=R, C=C, Rpad=Rpad))
    c.bufs = dict(x=x)
    c.outs = dict(out=((C, Rpad), F32))
    c.launches = [Launch("TRANSPOSE_PAD", ("x",), ("out",), (R, C, ldi, Rpad))]
    c.expect = dict(out=Expect(transposed(x[:, :C], Rpad, Rpad, F32(0))))
    return c


def case_to_bf16(R, C, ldi, Rpad=None, ldt=0, relu=False, plain=True):
    T = Rpad is not None
    nm = (f"to_bf16{'_T' if T else ''}_R{R}_C{C}_ldi{ldi}" + (f"_Rpad{Rpad}_ldt{ldt}" if T else "") + ("_relu" if relu else "") +
          ("" if plain or not T else "_noplain"))
    x = _conv_x(nm, R, C, ldi)
    c = Case(nm, "launch_to_bf16_T" if T else "launch_to_bf16", p=dict(x=x, R=R, C=C, Rpad=Rpad, ldt=ldt, relu=relu))
    c.bufs = dict(x=x)
    v = x[:, :C]
    if relu:
        act = np.full((R, ldi), np.nan, F32)
        act[:, :C] = unif(nm + "/act", (R, C))
        act[:, :C][:, 0::4] = 0.0
        c.bufs["act"] = act
        c.p["act"] = act
        v = relu_gate(v, act[:, :C])
    bits = bf16_bits(v)
    if not T:
        c.outs = dict(out=((R, C), np.uint16))
        c.launches = [Launch("TO_BF16", ("x",), ("out",), (R, C, ldi))]
        c.expect = dict(out=Expect(bits))
        return c
    ld = ldt or Rpad
    c.outs = dict(out_t=((C, ld), np.uint16))
    tr = transposed(bits, Rpad, ld, np.uint16(CANARY16))
    written = np.zeros((C, ld), bool)
    written[:, :Rpad] = True
    c.expect = dict(out_t=Expect(tr, written=written))
    if plain:
        c.outs["out_p"] = ((R, C), np.uint16)
        c.expect["out_p"] = Expect(bits)
    c.launches = [Launch("TO_BF16_T", ("x", "act" if relu else None), ("out_t", "out_p" if plain else None), (R, C, ldi, Rpad, ldt))]
    return c


def case_split_dyn(R, C, ldi, Rpad=None, plain=True, amax_scale=1.0):
    T = Rpad is not None
    nm = f"split_dyn{'_T' if T else ''}_R{R}_C{C}_ldi{ldi}" + (f"_Rpad{Rpad}" if T else "") + ("" if plain or not T else "_noplain") + \
         (f"_x{amax_scale:g}" if amax_scale != 1.0 else "")
    x = _conv_x(nm, R, C, ldi)
    x[:, :C] *= F32(amax_scale)
    amax = np.array([np.abs(x[:, :C]).max()], F32)
    sc = dyn_plane_scale(amax[0])
    xs = (x[:, :C] * sc).astype(F32)
    assert np.abs(xs).max() < 2 ** 14 and np.array_equal(xs.astype(F64), x[:, :C].astype(F64) * float(sc))
    c = Case(nm, "launch_split_dyn_T" if T else "launch_split_dyn", p=dict(xs=xs, R=R, C=C, Rpad=Rpad))
    c.bufs = dict(x=x, amax=amax)

    def two_planes(vals, bound, n):      # [2][n] planes held as hi + lo, filed under the hi plane
        ref, b = np.zeros(2 * n), np.zeros(2 * n)
        ref[:n], b[:n] = vals.reshape(-1), bound.reshape(-1)
        return Expect(ref, b, decode=lambda g, n=n: _planes_sum(g, n, n))
    if plain:
        c.outs["out_p"] = ((2 * R * C,), np.float16)
        c.expect["out_p"] = two_planes(xs.astype(F64), plane_bound(xs), R * C)
    if T:
        c.outs["out_t"] = ((2 * C * Rpad,), np.float16)
        xt = transposed(xs.astype(F64), Rpad, Rpad, 0.0)
        bt = transposed(plane_bound(xs), Rpad, Rpad, 0.0)       # the pad columns: bound 0, exact zeros in both planes
        c.expect["out_t"] = two_planes(xt, bt, C * Rpad)
        c.launches = [Launch("SPLIT_DYN_T", ("x", "amax"), ("out_t", "out_p" if plain else None), (R, C, ldi, Rpad))]
    else:
        c.launches = [Launch("SPLIT_DYN", ("x", "amax"), ("out_p",), (R, C, ldi))]
    return c


def case_rmsnorm_bf16_T(rows, d, ldt_extra=0, post_scaled=False):
    nm = f"rmsnorm_bf16_T_r{rows}_d{d}" + (f"_ldt+{ldt_extra}" if ldt_extra else "") + ("_post" if post_scaled else "")
    Rpad = (rows + 31) // 32 * 32
    ldt = Rpad + ldt_extra
    post = float(F32(d ** -0.5)) if post_scaled else 1.0
    p = dict(x=act_rows(nm + "/x", rows, d), ln=weight_row(nm + "/w", d), eps=EPS, post=post, E=np.zeros((1, 1, d), F32),
             codes=np.zeros((rows, 1), np.int32))
    r = gold_scores(p)
    h, E_h = r["hidden"], r["b_hidden"]
    bits = bf16_bits(h.astype(F32))
    lo, hi = bf16_order(bf16_bits((h - E_h).astype(F32))), bf16_order(bf16_bits((h + E_h).astype(F32)))
    c = Case(nm, "launch_rmsnorm_bf16_T", p=p)
    c.bufs = dict(x=p["x"], ln=p["ln"])
    c.outs = dict(out_p=((rows, d), np.uint16), out_t=((d, ldt), np.uint16))
    c.launches = [Launch("RMSNORM_BF16_T", ("x", "ln"), ("out_p", "out_t"), (rows, d, Rpad, ldt), (EPS, post))]
    written = np.zeros((d, ldt), bool)
    written[:, :Rpad] = True
    big = np.int32(1 << 20)
    c.expect = dict(out_p=Expect(bits, flips=np.stack([lo, hi])),
                    out_t=Expect(transposed(bits, Rpad, ldt, np.uint16(CANARY16)), written=written,
                                 flips=np.stack([transposed(lo, Rpad, ldt, big), transposed(hi, Rpad, ldt, -big)])))
    return c


def case_weights_bf16():
    shapes = [(2, 4), (64, 64), (66, 68), (2, 68), (66, 4)]
    c = Case("weights_bf16_5seg", "launch_weights_bf16", p=dict(shapes=shapes))
    tot = sum(R * C for R, C in shapes)
    plain, tr = np.zeros(tot, np.uint16), np.zeros(tot, np.uint16)
    off = 0
    dims = [len(shapes)]
    for i, (R, C) in enumerate(shapes):
        w = grad_rows(f"weights_bf16/seg{i}", R, C, 2.0)
        c.bufs[f"w{i}"] = w
        b = bf16_bits(w)
        plain[off:off + R * C] = b.reshape(-1)
        tr[off:off + R * C] = b.T.reshape(-1)
        off += R * C
        dims += [R, C]
    c.outs = dict(plain=((tot,), np.uint16), tr=((tot,), np.uint16))
    c.launches = [Launch("WEIGHTS_BF16", tuple(f"w{i}" for i in range(len(shapes))), ("plain", "tr"), tuple(dims))]
    c.expect = dict(plain=Expect(plain), tr=Expect(tr))
    return c


def _build_cases():
    cs: List[Case] = []
    # rmsnorm_bwd / colsum: every row count at d = 260, every width at 37 rows, the corners of both paths
    for rows in (1, 15, 16, 17, 37, 273):
        cs.append(case_rmsnorm_bwd(rows, 260, dres=rows % 2 == 1, post_scaled=rows in (16, 273), with_dw=True, accumulate=int(rows in (17, 273))))
    for d in (32, 1024, 1028, 2048):
        cs.append(case_rmsnorm_bwd(37, d, dres=d in (32, 1028), post_scaled=d in (1024, 1028), with_dw=d != 32, accumulate=int(d == 2048)))
    cs += [case_rmsnorm_bwd(17, 1028, False, False, True), case_rmsnorm_bwd(273, 2048, True, True, True, 1),
           case_rmsnorm_bwd(1, 1028, True, True, False), case_rmsnorm_bwd(16, 1024, True, False, True)]
    cs += [case_colsum_multi(260), case_colsum_multi(32, (18, 1, 16, 17)), case_colsum_multi(1028, (17, 18))]
    # gold scores
    for S, L in ((1, 1), (1, 5), (5, 5)):          # S L = 1, 5, 8 * 3 + 1
        for d in (32, 768, 1028):
            if (S, L) == (5, 5) or d == 32:
                cs.append(case_gold_scores(S, L, d, mode="f32", post_scaled=d == 768))
                cs.append(case_gold_scores(S, L, d, mode="planes", post_scaled=d == 768))
    cs += [case_gold_scores(5, 5, 768, mode="hidden", post_scaled=True), case_gold_scores(1, 5, 1028, mode="hidden")]
    for S, L, d in ((1, 1, 32), (1, 5, 768), (5, 5, 1028), (5, 5, 32)):
        cs += [case_gold_bwd(S, L, d), case_gold_bwd(S, L, d, rowdot=True)]
    # margin-MSE
    for bz in (1, 3, 256, 257, 600):
        pre = (1, 4, 8, 32) if bz != 3 else (32,)
        cs.append(case_margin_mse(bz, pre))
        cs.append(case_margin_mse_bwd(bz, pre, own=bz in (1, 257)))
        if bz == 257:
            cs.append(case_margin_mse_bwd(bz, pre, own=False))
    cs.append(case_margin_mse(257, (4,)))
    for bz, d in ((1, 32), (3, 260), (257, 1028), (3, 1028), (257, 32)):
        cs.append(case_dense_mse(bz, d))
    # embedding gradients
    for rows, d, pat, me in ((1, 40, "one", 0), (15, 100, "third", 0), (17, 256, "own", 0), (273, 40, "third", 0), (273, 100, "one", 0),
                             (273, 100, "one", 12), (273, 100, "one", 24), (17, 100, "third", 12), (17, 100, "third", 24), (273, 256, "own", 12)):
        cs.append(case_scatter(rows, d, pat, me))
    for rows, d in ((1, 40), (15, 100), (17, 256), (273, 40), (273, 100)):
        cs.append(case_sum_selected(rows, d))
    for S, L, d, pl in ((1, 1, 40, False), (3, 5, 100, False), (1, 17, 256, True), (39, 7, 40, True), (3, 5, 100, True), (39, 7, 256, False)):
        cs += case_dec_embed(S, L, d, planes=pl)
    # seq2seq head
    for bz, L, d, V, odd in ((1, 1, 32, 64, False), (15, 3, 96, 256, False), (16, 1, 160, 320, False), (17, 3, 32, 1024, False),
                             (33, 1, 160, 64, True), (33, 3, 96, 320, False), (17, 1, 96, 256, True)):
        cs.append(case_s2s_head(bz, L, d, V, odd))
    # operand conversions
    for R, C in ((1, 4), (63, 60), (64, 64), (65, 68), (130, 132), (63, 132), (130, 4)):
        for ldi in (C, C + 8):
            r2, r64 = (R + 1) // 2 * 2, (R + 63) // 64 * 64
            big = ldi != C
            cs.append(case_transpose_pad(R, C, ldi, r64 if big else r2))
            cs.append(case_to_bf16(R, C, ldi))
            cs.append(case_to_bf16(R, C, ldi, Rpad=r2 if big else r64, ldt=0 if big else r64 + 8, relu=big, plain=not big))
            cs.append(case_to_bf16(R, C, ldi, Rpad=r64 if big else r2, ldt=(r64 + 8) if big else 0, relu=not big, plain=big))
            cs.append(case_split_dyn(R, C, ldi, amax_scale=2.0 ** -20 if big else 1.0))
            cs.append(case_split_dyn(R, C, ldi, Rpad=r2 if big else r64, plain=big, amax_scale=1.0 if big else 2.0 ** 10))
    for rows in (1, 31, 33):
        for d in (64, 1024):
            cs.append(case_rmsnorm_bf16_T(rows, d, ldt_extra=8 if rows == 31 else 0, post_scaled=d == 1024))
    cs.append(case_weights_bf16())
    for n in (4, 1020, 1024, 1028):
        cs.append(case_relu_bwd(n))
    for n0, n1 in ((1, 0), (3, 0), (1023, 0), (1025, 3), (3 * 8192 + 5, 7), (3 * 8192 + 5, 0)):
        cs.append(case_absmax2(n0, n1))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
    """The case table, built once and shared (the references are not recomputed per test)."""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


LAUNCHERS = {"launch_rmsnorm_bwd", "launch_colsum_multi", "launch_gold_scores", "launch_gold_score_bwd", "launch_gold_rowdot",
             "launch_margin_mse", "launch_margin_mse_bwd", "launch_dense_mse_head", "launch_relu_bwd", "launch_train_dec_embed",
             "launch_train_indices", "launch_scatter_rows_fix+launch_fix_flush", "launch_sum_selected_rows", "launch_s2s_head",
             "launch_absmax2", "launch_split_dyn", "launch_split_dyn_T", "launch_to_bf16", "launch_to_bf16_T", "launch_rmsnorm_bf16_T",
             "launch_weights_bf16", "launch_transpose_pad"}
