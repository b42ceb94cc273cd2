"""The attention of the training step from its definition, in numpy fp64, with an a-priori fp32 error bound per output
element; the inputs and the case table of tests/test_gpu_attn_train_direct.py; the mutants of the definition that
tests/test_attn_train_ref_host.py uses to prove that those inputs tell a wrong kernel from a right one. In the style of
tests/attn_ref.py, whose bucket table, u, q-row generator (flat, peaked, near-zero rows) and eps_p it reuses; the dropout
multiplier is tests/dropout_mask.py's. Nothing here follows a kernel's order of operations.

Definition, for one (sequence or query, head); ok marks the attended keys, mul is 0 or fp32(1 / (1 - rate)) (1 without dropout):
    s = Q K^T + bias          p = softmax_ok(s), a masked key exactly 0          pm = p * mul          O = pm V
    dP = (dO V^T) * mul, 0 where the key is masked        c_i = sum_j p_ij dP_ij        dS = p * (dP - c)
    dQ = dS K        dK = dS^T Q        dV = pm^T dO        dbias[b, h] = sum_s sum_{(i, j): bucket(j - i) = b} dS_ij
The bucket table is bidirectional for the encoder; for `causal` it is unidirectional over i - j and key j <= query i. Every row
is a query, attended or not (a padded encoder row still has a gradient); a sequence without an attended key gives zeros.

Bound (first order), u = 2^-24, any summation order, D the head dim, n the attended keys of row i, nk the keys of the launch, nq_j
the rows that meet key j (the rows whose ok_ij is set), eps_p of attn_ref.softmax_eps unchanged:
    E_dP_ij = mul_ij (D + 2) u sum_d |dO_id V_jd| + u |dP_ij|
    E_c_i   = sum_j p_ij (|dP_ij| eps_p_i + E_dP_ij) + (n + 8) u sum_j p_ij |dP_ij|
    E_dS_ij = p_ij (eps_p_i |dP_ij - c_i| + E_dP_ij + E_c_i + 2 u (|dP_ij| + |c_i|)) + 2^-120 ok_ij (|dP_ij| + |c_i|)
    b_dQ    = E_dS |K|   + (nk + 1) u |dS| |K|
    b_dK    = E_dS^T |Q| + (nq_j + 1) u |dS|^T |Q|
    b_dV    = (pm (eps_p + 2 u))^T |dO| + (nq_j + 1) u pm^T |dO| + 2^-120 (ok mul)^T |dO|
    b_O     = (pm (eps_p + 2 u)) |V|    + (nk + 1) u pm |V|      + 2^-120 (ok mul) |V|
    b_dbias = sum of E_dS over the bucket's elements + (count + S + 8) u sum |dS| + u |dbias0 + dbias|
Underflow, which a first-order bound does not see: a product of two fp32 numbers that leaves the normal range is off by at most
UF = 2^-126, whether the hardware flushes it or rounds it to a subnormal. The peaked rows make such products: a losing key of weight
e^-80 against a c_i that is itself the sum of such weights gives p (dP - c) ~ 1e-71, which fp32 returns as 0 (the plain numpy fp32
evaluation does). So every product over attended keys adds UF to the term it enters: D mul UF in E_dP, n UF in E_c, ok UF in E_dS and
n UF / nq_j UF in the four outputs. These terms are 0 for a masked key and 1e-36 or less elsewhere.
count = the attended (sequence, i, j) of the bucket: a term that is exactly 0 adds no rounding error to a sum in any order. A masked
key has p = 0 and ok = 0, so the bounds of its dK and dV rows are 0: exact zeros are what the bound asks there, and of every output
of a sequence without an attended key. The GPU tests assert |got - ref| <= bound with no factor on top.

Inputs (the counter hashes of ripor_amd.utils.synth): K uniform with unit variance; V uniform in [-1, 1) with the key's signature
(position + 1 + sequence / 16) on every eighth column; q rows of attn_ref's three kinds; dO uniform in [-1, 1), its odd rows with the
row's signature (position + 1 + sequence / 16) on every eighth column (column 5 of eight), so that a row taken from the neighbour
shows; masked keys have K rows like any other and V rows of magnitude 100; masks are suffix padding, one case per site has interior
holes; rel_bias as in attn_ref (+-30 on one bucket each per odd head); dbias starts from a nonzero fp32 pattern.

A sequence without an attended key: the training entry points admit it (train_api.hip computes the attended lengths on the device
and raises RPR_STATUS_EMPTY_QUERY, nothing is refused before launch), so one bidirectional case of every kernel has one."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import attn_ref as R
import dropout_mask as DM
from ripor_amd.utils import synth

U = R.U
NB, MAXD = R.NB, R.MAXD
TINY = 2.0 ** -120
UF = 2.0 ** -126          # the smallest normal fp32 number
RATE = 0.1
SEED, STEP = 0x0123456789ABCDEF, 0x0000000100000007      # both halves of the key and of the step are in use
SITE_SELF, SITE_CROSS = DM.site_mid(0, 1, 0), DM.site_mid(1, 1, 1)
LDS_MAX = 160 * 1024

# The mutants of the definition (tests/test_attn_train_ref_host.py), each a mistake a kernel can make:
#   c_over_dropped   c_i summed over the dropped keys too: c = sum_j p_ij (dO V^T)_ij scale, the keep bits forgotten (a key the
#                    mask excludes has p = 0 and cannot enter c either way, so "masked" here can only mean dropped)
#   no_scale_bwd     the backward multiplies dP by the keep bit, not by scale
#   keep_transposed  keep bits indexed (key, query) instead of (query, key)
#   doc_ignored      cross-attention mask drawn with seq = query: every document of a query gets the first one's sequence number
#   philox_word      word (k + 1) & 3 of the Philox block in place of word k & 3
#   dbias_diag       dS_ij lands in the bucket of j - i + 1
#   tables_swapped   the bidirectional and the unidirectional bucket table swapped (bias and dbias)
#   odd_last_row     the last row of an odd number of query rows dropped (the r1 == r0 pairing)
#   drop_key_32      key 32, the first of the second tile, not attended
#   drop_tile5       the query rows of the fifth tile (128 and up) dropped
#   dv_from_p        dV = p^T dO: the multiplier forgotten
#   next_query       K | V of the next sequence / query
MUTANTS = ("c_over_dropped", "no_scale_bwd", "keep_transposed", "doc_ignored", "philox_word", "dbias_diag", "tables_swapped",
           "odd_last_row", "drop_key_32", "drop_tile5", "dv_from_p", "next_query")
DROP_MUTANTS = ("c_over_dropped", "no_scale_bwd", "keep_transposed", "doc_ignored", "philox_word", "dv_from_p")


# ---------------------------------------------------------------------------------------------- the operation itself
@dataclass
class Group:
    """What enters the definition for one (sequence or query, head)."""
    q: np.ndarray                   # [nq, D]
    K: np.ndarray                   # [nk, D]
    V: np.ndarray
    dO: np.ndarray                  # [nq, D]
    bias: Optional[np.ndarray]      # [nq, nk]
    ok: np.ndarray                  # [nq, nk] bool
    mul: np.ndarray                 # [nq, nk] float32: 0 or 1 / (1 - rate); ones without dropout
    bucket: Optional[np.ndarray]    # [nq, nk] the dbias row an element's dS goes to (self-attention)


def define(G: Group, dtype=np.float64, want_bound=True, mut=None, perm=None):
    """{O, dQ, dK, dV, dS} and, in fp64, their bounds {b_O, b_dQ, b_dK, b_dV, E_dS}. dtype float32 is the plain numpy fp32
    evaluation of the same expressions; perm = (rows, keys, columns) evaluates them on permuted operands (another summation
    order) and returns the results in the original order."""
    q, K, V, dO, bias, ok, mul = G.q, G.K, G.V, G.dO, G.bias, G.ok, G.mul
    if perm is not None:
        pr, pk, pc = perm
        q, dO, K, V = q[pr][:, pc], dO[pr][:, pc], K[pk][:, pc], V[pk][:, pc]
        ok, mul = ok[pr][:, pk], mul[pr][:, pk]
        bias = bias[pr][:, pk] if bias is not None else None
    nq, D = q.shape
    nk = K.shape[0]
    K, V, dO = K.astype(dtype), V.astype(dtype), dO.astype(dtype)
    p, eps, cnt = R.softmax_eps(q, K, bias, ok, lambda a, b: a @ b.T, dtype, want_bound)
    q = q.astype(dtype)
    mul = mul.astype(dtype)
    Vok = np.where(ok.any(axis=0)[:, None], V, 0)       # what a key nobody attends holds never enters
    pm = p * mul
    mul_b = mul
    if mut == "no_scale_bwd":
        mul_b = (mul != 0).astype(dtype)
    dP = np.where(ok, (dO @ Vok.T) * mul_b, 0).astype(dtype)
    c_terms = p * dP
    if mut == "c_over_dropped":
        c_terms = p * np.where(ok, dO @ Vok.T, 0) * mul.max(initial=1.0)
    c = c_terms.sum(axis=1)
    dS = (p * (dP - c[:, None])).astype(dtype)
    pv = p if mut == "dv_from_p" else pm
    if mut in ("odd_last_row", "drop_tile5"):
        dead = np.zeros(nq, bool)
        if mut == "odd_last_row" and nq % 2:
            dead[nq - 1] = True
        if mut == "drop_tile5":
            dead[128:] = True
        dS = np.where(dead[:, None], 0, dS)
        pm = np.where(dead[:, None], 0, pm)
        pv = np.where(dead[:, None], 0, pv)
    res = dict(O=pm @ Vok, dQ=dS @ K, dK=dS.T @ q, dV=pv.T @ dO, dS=dS)
    if want_bound:
        e = eps[:, None]
        okf = ok.astype(dtype)
        E_dP = np.where(ok, mul * ((D + 2) * U * (np.abs(dO) @ np.abs(Vok).T) + D * UF) + U * np.abs(dP), 0)
        E_c = (p * (np.abs(dP) * e + E_dP)).sum(axis=1) + (cnt + 8) * U * (p * np.abs(dP)).sum(axis=1) + cnt * UF
        mag = np.abs(dP) + np.abs(c)[:, None]
        E_dS = p * (e * np.abs(dP - c[:, None]) + E_dP + E_c[:, None] + 2 * U * mag) + TINY * okf * mag + UF * okf
        nqj = ok.sum(axis=0)[:, None]
        ni = cnt[:, None]
        aK, aQ, aV, aO = np.abs(K), np.abs(q), np.abs(Vok), np.abs(dO)
        res.update(E_dS=E_dS,
                   b_dQ=E_dS @ aK + (nk + 1) * U * (np.abs(dS) @ aK) + ni * UF,
                   b_dK=E_dS.T @ aQ + (nqj + 1) * U * (np.abs(dS).T @ aQ) + nqj * UF,
                   b_dV=(pm * (e + 2 * U)).T @ aO + (nqj + 1) * U * (pm.T @ aO) + TINY * ((okf * mul).T @ aO) + nqj * UF,
                   b_O=(pm * (e + 2 * U)) @ aV + (nk + 1) * U * (pm @ aV) + TINY * ((okf * mul) @ aV) + ni * UF)
    if perm is not None:
        inv_r, inv_k, inv_c = np.argsort(pr), np.argsort(pk), np.argsort(pc)
        for k, v in res.items():
            rows = inv_k if k in ("dK", "dV", "b_dK", "b_dV") else inv_r
            res[k] = v[rows][:, inv_k if k in ("dS", "E_dS") else inv_c]
    return res


# ---------------------------------------------------------------------------------------------- the case table
@dataclass
class Case:
    name: str
    site: str                       # self | cross
    op: str                         # bwd | fwd (the forward with dropped-out probabilities)
    rate: float                     # 0: no dropout
    kernel: str                     # the AttnKernel the planner must report
    p: dict = field(default_factory=dict)


def _self_shape(Ls, causal=False, dkv=64, big=None, empty=False, holes=(), rate=RATE, lens=None):
    S = 2 if (dkv == 128 or Ls >= 129) else 3
    if lens is None:
        lens = [Ls, max(Ls - 7, 1), 1][:S]
        if empty:
            lens[1] = 0
    name = f"self{dkv if dkv != 64 else ''}_{'causal' if causal else 'bidir'}_L{Ls}" + ("_empty" if empty else "") + (f"_r{rate}" if rate != RATE else "")
    return dict(name=name, site="self", S=S, H=S, Ls=Ls, dkv=dkv, causal=causal, lens=tuple(lens), holes=tuple(holes), drop_rate=rate)


def _cross_shape(docs, L, Lq, dkv=64, empty=False, holes=(), rate=RATE, lens=None):
    n = docs * L
    bz = 2 if (dkv == 128 or n >= 129 or Lq >= 129) else 3
    if lens is None:
        lens = [Lq, max(Lq - 7, 1), 1][:bz]
        if empty:
            lens[1] = 0
    name = f"cross{dkv if dkv != 64 else ''}_{docs}x{L}_Lq{Lq}" + ("_empty" if empty else "") + (f"_r{rate}" if rate != RATE else "")
    return dict(name=name, site="cross", bz=bz, H=bz, docs=docs, L=L, n=n, Lq=Lq, dkv=dkv, lens=tuple(lens), holes=tuple(holes), drop_rate=rate)


def self_carve(Ls):
    """self_attn_bwd_smem (attn_route.h) in bytes, restated."""
    return 4 * (4 * Ls * 65 + 2 * Ls * (Ls + 1) + 64 + 5 * Ls)


def cross_carve(n, Lq):
    """cross_attn_bwd_carve (attn_route.h) in bytes, restated."""
    return 4 * (2 * n * 65 + 2 * Lq * 65 + 2 * n * (Lq + 1) + Lq)


# shape, resident?, (backward, backward with dropout, forward with dropout)
_MFMA = ("TRAIN_BWD_MFMA", "TRAIN_BWD_VALU", "TRAIN_SELF_DROP_FWD")
_VALU = ("TRAIN_BWD_VALU", "TRAIN_BWD_VALU", "TRAIN_SELF_DROP_FWD")
_VALU128 = ("TRAIN_BWD_VALU128", "TRAIN_BWD_VALU128", "TRAIN_SELF_DROP_FWD128")
_STILED = ("TRAIN_SELF_BWD_TILED", "TRAIN_SELF_BWD_TILED", "TRAIN_SELF_DROP_FWD_TILED")
_CROSS = ("TRAIN_CROSS_BWD", "TRAIN_CROSS_BWD", "TRAIN_CROSS_DROP_FWD")
_CROSS128 = ("TRAIN_CROSS_BWD128", "TRAIN_CROSS_BWD128", "TRAIN_CROSS_DROP_FWD128")
_CTILED = ("TRAIN_CROSS_BWD_TILED", "TRAIN_CROSS_BWD_TILED", "TRAIN_CROSS_DROP_FWD_TILED")


def build_shapes():
    sh = []
    # the fp32-MFMA tile (one wave per (sequence, head), S * H odd: the last block's second wave idles); with dropout the VALU kernel
    for Ls in (1, 7, 32):
        sh.append((_self_shape(Ls, causal=True), True, _MFMA))
    sh.append((_self_shape(5), True, _MFMA))
    sh.append((_self_shape(31, empty=True), True, _MFMA))
    sh.append((_self_shape(32), True, _MFMA))
    # the resident VALU kernel: 33 = the first length beyond the tile, odd lengths (r1 == r0), 91 = the last resident length
    for Ls in (33, 64):
        sh.append((_self_shape(Ls, causal=True), True, _VALU))
    sh.append((_self_shape(33), True, _VALU))
    sh.append((_self_shape(65, empty=True, holes=(0,)), True, _VALU))
    sh.append((_self_shape(91), True, _VALU))
    sh.append((_self_shape(1), True, _MFMA))                       # the drop-forward at one position
    # 128-dim heads
    sh.append((_self_shape(9, causal=True, dkv=128), True, _VALU128))
    sh.append((_self_shape(33, dkv=128, empty=True), True, _VALU128))
    sh.append((_self_shape(91, dkv=128), True, _VALU128))
    # the tiles: 92 = the first tiled length, 96 / 97 a whole and a ragged third tile, 129 a fifth query tile (the second round of
    # the wave diagonals), 255 / 256 the longest
    sh.append((_self_shape(92), False, _STILED))
    sh.append((_self_shape(96, empty=True), False, _STILED))
    for Ls in (97, 129, 255, 256):
        sh.append((_self_shape(Ls), False, _STILED))
    # rate 0.9 with 3 keys: rows whose kept keys are all dropped
    sh.append((_self_shape(3, rate=0.9, lens=(3, 3, 3)), True, _MFMA))
    # cross-attention, resident: docs x L rows against Lq keys
    sh.append((_cross_shape(1, 1, 1, lens=(1, 1, 1)), True, _CROSS))
    sh.append((_cross_shape(2, 4, 5), True, _CROSS))
    sh.append((_cross_shape(3, 21, 33, empty=True), True, _CROSS))
    sh.append((_cross_shape(2, 32, 64, holes=(0,)), True, _CROSS))      # the reference's fine-tune shape
    sh.append((_cross_shape(2, 4, 256), True, _CROSS))                  # all eight keep words of a lane
    sh.append((_cross_shape(3, 3, 7, dkv=128, empty=True), True, _CROSS128))
    sh.append((_cross_shape(2, 32, 64, dkv=128), True, _CROSS128))
    # cross-attention, tiled
    sh.append((_cross_shape(2, 8, 256), False, _CTILED))                # one partial query tile, eight key tiles
    sh.append((_cross_shape(3, 32, 92, empty=True), False, _CTILED))
    sh.append((_cross_shape(5, 32, 48), False, _CTILED))
    sh.append((_cross_shape(4, 64, 256), False, _CTILED))
    sh.append((_cross_shape(2, 2, 3, rate=0.9, lens=(3, 3, 3)), True, _CROSS))
    return sh


SHAPES = build_shapes()


def build_cases() -> List[Case]:
    cs = []
    for p, _, (bwd, bwd_drop, fwd) in SHAPES:
        site, rate = p["site"], p["drop_rate"]
        if rate == RATE:
            cs.append(Case(p["name"] + "_bwd", site, "bwd", 0.0, bwd, p))
        cs.append(Case(p["name"] + "_bwd_drop", site, "bwd", rate, bwd_drop, p))
        cs.append(Case(p["name"] + "_fwd_drop", site, "fwd", rate, fwd, p))
    return cs


CASES = build_cases()
KERNELS = {c.kernel for c in CASES}


def planner_query(case: Case) -> Tuple[str, Dict[str, int]]:
    """(site, key=value arguments) of tests/attn_route_driver.cpp for this case."""
    p = case.p
    drop = int(case.rate > 0)
    if case.site == "self":
        return ("train_self_bwd" if case.op == "bwd" else "train_self_drop_fwd",
                dict(S=p["S"], Ls=p["Ls"], H=p["H"], buckets=NB, dkv=p["dkv"], causal=int(p["causal"]), mask=int(not p["causal"]), drop=drop,
                     drop_L=p["Ls"] if drop else 0))
    return ("train_cross_bwd" if case.op == "bwd" else "train_cross_drop_fwd",
            dict(bz=p["bz"], n=p["n"], Lq=p["Lq"], H=p["H"], dkv=p["dkv"], mask=1, drop=drop, drop_L=p["L"] if drop else 0))


# ---------------------------------------------------------------------------------------------- inputs
def _sig_dO(name, pos, seq, D):
    """dO rows: uniform [-1, 1); odd positions carry the row's signature on every eighth column."""
    pos = np.asarray(pos, np.float64)
    g = synth.uniform_f32(name, pos.shape + (D,), 1.0).astype(np.float32)
    sig = (pos + 1.0 + np.asarray(seq, np.float64) / 16.0)[..., None]
    odd = (pos.astype(np.int64) % 2 == 1)[..., None]
    g[..., 5::8] = np.where(odd, sig, g[..., 5::8])
    return g


_INPUTS: Dict[str, dict] = {}


def make_inputs(p: dict) -> dict:
    """numpy inputs of a shape (float32 / int32 arrays as the hooks take them), shared by its cases and left unchanged."""
    if p["name"] in _INPUTS:
        return _INPUTS[p["name"]]
    nm, H, D = p["name"], p["H"], p["dkv"]
    inner = H * D
    inp = dict(p)
    inp.update(D=D, inner=inner)
    if p["site"] == "self":
        S, Ls, causal = p["S"], p["Ls"], p["causal"]
        rows = S * Ls
        mask = None if causal else R.make_mask(S, Ls, p["lens"], p["holes"])
        pos, seq = np.tile(np.arange(Ls), S), np.repeat(np.arange(S), Ls)
        qkv = np.zeros((rows, 3 * inner), np.float32)
        qkv[:, inner:2 * inner] = synth.uniform_f32(nm + "/k", (rows, inner), math.sqrt(3.0))
        qkv[:, 2 * inner:] = R._sig_v(nm + "/v", np.repeat(pos[:, None], H, 1), np.repeat(seq[:, None], H, 1), D).reshape(rows, inner)
        if mask is not None:
            dead = mask.reshape(-1) == 0
            qkv[dead, 2 * inner:] = synth.uniform_f32(nm + "/garbage", (int(dead.sum()), inner), 100.0)
        dO = _sig_dO(nm + "/dO", np.repeat(pos[:, None], H, 1), np.repeat(seq[:, None], H, 1), D).reshape(rows, inner)
        rel_bias = R._rel_bias_table(nm, H, not causal, max(Ls // 2, 1))
        dbias0 = synth.uniform_f32(nm + "/dbias0", (NB, H), 4.0).astype(np.float32)
        inp.update(qkv=qkv, dO=dO, mask=mask, rel_bias=rel_bias, dbias0=dbias0, groups=S, nq=Ls, nk=Ls)
        for s in range(S):          # the crafted q rows need K and the bias of their (sequence, head)
            for h in range(H):
                G = gather(inp, s, h, 0.0)
                ids = np.arange(Ls) + s + h
                qkv[s * Ls:(s + 1) * Ls, h * D:(h + 1) * D] = R._craft_q(f"{nm}/q/{s}/{h}", R.Group(None, G.K[None], None, G.bias, G.ok, None), D, ids)
    else:
        bz, n, Lq, L = p["bz"], p["n"], p["Lq"], p["L"]
        xld = 2 * inner + 8
        mask = R.make_mask(bz, Lq, p["lens"], p["holes"])
        x = np.full((bz * Lq, xld), np.nan, np.float32)            # the gap columns behind K | V are never read
        pos, qid = np.tile(np.arange(Lq), bz), np.repeat(np.arange(bz), Lq)
        x[:, :inner] = synth.uniform_f32(nm + "/k", (bz * Lq, inner), math.sqrt(3.0))
        x[:, inner:2 * inner] = R._sig_v(nm + "/v", np.repeat(pos[:, None], H, 1), np.repeat(qid[:, None], H, 1), D).reshape(bz * Lq, inner)
        dead = mask.reshape(-1) == 0
        x[dead, inner:2 * inner] = synth.uniform_f32(nm + "/garbage", (int(dead.sum()), inner), 100.0)
        rpos, rq = np.tile(np.arange(n), bz), np.repeat(np.arange(bz), n)
        dO = _sig_dO(nm + "/dO", np.repeat(rpos[:, None], H, 1), np.repeat(rq[:, None], H, 1), D).reshape(bz * n, inner)
        q = np.zeros((bz * n, inner), np.float32)
        inp.update(x=x, xld=xld, q=q, dO=dO, mask=mask, groups=bz, nq=n, nk=Lq)
        for g in range(bz):
            for h in range(H):
                G = gather(inp, g, h, 0.0)
                ids = np.arange(n) + g + h
                q[g * n:(g + 1) * n, h * D:(h + 1) * D] = R._craft_q(f"{nm}/q/{g}/{h}", R.Group(None, G.K[None], None, None, G.ok, None), D, ids)
    _INPUTS[p["name"]] = inp
    return inp


def multiplier(inp, g, h, rate):
    """[nq, nk] float32, 0 or 1 / (1 - rate): dropout_mask.attn_mask in the coordinates the step gives its attention sites —
    self-attention: sequence g, query position i; cross-attention: row r of query g is position r % L of sequence g * docs + r // L."""
    nq, nk, H = inp["nq"], inp["nk"], inp["H"]
    if inp["site"] == "self":
        return DM.attn_mask(rate, SEED, STEP, SITE_SELF, [g], H, nq, nk)[0, h]
    docs = nq // inp["L"]
    return DM.attn_mask(rate, SEED, STEP, SITE_CROSS, g * docs + np.arange(docs), H, inp["L"], nk)[:, h].reshape(nq, nk)


def keep_bits(inp, g, h, rate, mut):
    """[nq, nk] uint8, 1 where the probability of (row, key) is kept, as one of the three mask mutants draws it."""
    nq, nk, H = inp["nq"], inp["nk"], inp["H"]
    thr = np.uint64(DM.threshold(rate))
    if inp["site"] == "self":
        seqs, L = [g], nq
    else:
        L = inp["L"]
        docs = nq // L
        seqs = [g] * docs if mut == "doc_ignored" else list(g * docs + np.arange(docs))
    side = max(L, nk) if mut == "keep_transposed" else None
    d = DM.attn_draws(SEED, STEP, SITE_SELF if inp["site"] == "self" else SITE_CROSS, seqs, H, side or L, side or nk)[:, h]
    if mut == "keep_transposed":
        d = d.transpose(0, 2, 1)
    d = d[:, :L, :nk]
    if mut == "philox_word":
        j = np.arange(nk)
        src = (j & ~3) | ((j + 1) & 3)
        wide = DM.attn_draws(SEED, STEP, SITE_SELF if inp["site"] == "self" else SITE_CROSS, seqs, H, L, (nk + 3) // 4 * 4)[:, h]
        d = wide[:, :, src]
    return (d.astype(np.uint64) >= thr).reshape(nq, nk).astype(np.uint8)


def gather(inp, g, h, rate, mut=None) -> Group:
    D, inner, nq, nk = inp["D"], inp["inner"], inp["nq"], inp["nk"]
    c = slice(h * D, (h + 1) * D)
    src = (g + 1) % inp["groups"] if mut == "next_query" else g
    i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
    if inp["site"] == "self":
        rows, kv = g * nq + np.arange(nq), src * nq + np.arange(nq)
        qkv = inp["qkv"]
        q, K, V = qkv[rows, c], qkv[kv, inner + h * D:inner + (h + 1) * D], qkv[kv, 2 * inner + h * D:2 * inner + (h + 1) * D]
        causal = inp["causal"] != (mut == "tables_swapped")     # which table: the mask stays what it is
        if inp["causal"]:
            ok = np.array(j <= i)
        else:
            ok = np.broadcast_to(inp["mask"][g] != 0, (nq, nk)).copy()
        bucket = R.bucket_of(np.minimum(j - i, 0), False) if causal else R.bucket_of(j - i, True)
        bias = inp["rel_bias"][bucket, h]
        if mut == "dbias_diag":
            sh = np.clip(j - i + 1, -(R.MAX_LQ - 1), R.MAX_LQ - 1)
            bucket = R.bucket_of(np.minimum(sh, 0), False) if causal else R.bucket_of(sh, True)
    else:
        rows, kv = g * nq + np.arange(nq), src * nk + np.arange(nk)
        q, K, V = inp["q"][rows, c], inp["x"][kv, c], inp["x"][kv, inner + h * D:inner + (h + 1) * D]
        ok = np.broadcast_to(inp["mask"][g] != 0, (nq, nk)).copy()
        bias = bucket = None
    if mut == "drop_key_32" and nk > 32:
        ok[:, 32] = False
    dO = inp["dO"][rows, c]
    if rate > 0 and mut in ("keep_transposed", "doc_ignored", "philox_word"):
        mul = np.where(keep_bits(inp, g, h, rate, mut) != 0, DM.scale(rate), np.float32(0)).astype(np.float32)
    elif rate > 0:
        mul = multiplier(inp, g, h, rate)
    else:
        mul = np.ones((nq, nk), np.float32)
    return Group(q, K, V, dO, bias, ok, mul, bucket)


def mutant_applies(inp, rate, mut) -> bool:
    """Whether a mutant can mean anything for a (shape, rate): the rest is decided per (group, head) by what it changes."""
    if mut in DROP_MUTANTS and rate == 0:
        return False
    if mut == "doc_ignored":
        return inp["site"] == "cross" and inp["docs"] > 1
    if mut in ("dbias_diag", "tables_swapped"):
        return inp["site"] == "self"
    if mut == "odd_last_row":
        return inp["nq"] % 2 == 1
    if mut == "drop_key_32":
        return inp["nk"] > 32
    if mut == "drop_tile5":
        return inp["nq"] > 128
    if mut == "next_query":
        return inp["groups"] > 1
    return True


_REFS: Dict[Tuple[str, float], dict] = {}


def reference(p: dict, rate: float, mut=None, dtype=np.float64, perm_seed=None) -> dict:
    """The whole launch: {(g, h): define(...)} under "groups", and for self-attention dbias [NB, H] (from dbias0) with its bound.
    The unmutated fp64 reference of a (shape, rate) is computed once and shared."""
    key = (p["name"], float(rate))
    plain = mut is None and dtype == np.float64 and perm_seed is None
    if plain and key in _REFS:
        return _REFS[key]
    inp = make_inputs(p)
    H, nq, nk, D = inp["H"], inp["nq"], inp["nk"], inp["D"]
    groups = {}
    for g in range(inp["groups"]):
        for h in range(H):
            perm = None
            if perm_seed is not None:
                rng = np.random.RandomState(perm_seed + 31 * g + h)
                perm = (rng.permutation(nq), rng.permutation(nk), rng.permutation(D))
            G = gather(inp, g, h, rate, mut)
            r = define(G, dtype, want_bound=dtype == np.float64, mut=mut, perm=perm)
            r["bucket"], r["ok"] = G.bucket, G.ok
            groups[(g, h)] = r
    res = dict(groups=groups)
    if inp["site"] == "self":
        S = inp["groups"]
        acc = np.zeros((NB, H), np.float64)
        e_sum, a_sum, count = np.zeros((NB, H)), np.zeros((NB, H)), np.zeros((NB, H))
        for (g, h), r in groups.items():
            b = r["bucket"].reshape(-1)
            acc[:, h] += np.bincount(b, weights=r["dS"].astype(np.float64).reshape(-1), minlength=NB)
            a_sum[:, h] += np.bincount(b, weights=np.abs(r["dS"]).astype(np.float64).reshape(-1), minlength=NB)
            count[:, h] += np.bincount(b, weights=r["ok"].reshape(-1).astype(np.float64), minlength=NB)
            if "E_dS" in r:
                e_sum[:, h] += np.bincount(b, weights=r["E_dS"].reshape(-1), minlength=NB)
        res["dbias"] = inp["dbias0"].astype(np.float64) + acc
        if dtype == np.float32:     # one fp32 accumulator per entry, element after element (backwards for the permuted order)
            acc32 = inp["dbias0"].copy()
            step = -1 if perm_seed is not None else 1
            for (g, h), r in list(groups.items())[::step]:
                np.add.at(acc32[:, h], r["bucket"].reshape(-1)[::step], r["dS"].astype(np.float32).reshape(-1)[::step])
            res["dbias"] = acc32
        res["b_dbias"] = e_sum + (count + S + 8) * U * a_sum + U * np.abs(res["dbias"])
    if plain:
        _REFS[key] = res
    return res
