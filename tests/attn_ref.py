"""The four attention operations of the search path from their definition, in numpy fp64, with an a-priori fp32 error
bound per output element; the inputs and the case table of tests/test_gpu_attn_direct.py; the mutants of the definition
that tests/test_attn_ref_host.py uses to prove that those inputs tell a wrong kernel from a right one.

Definition (T5, unscaled):  o = softmax_j(q . k_j + bias[bucket(rel_j)]  over the attended keys j) . v.  A masked key has
weight exactly 0; a row without an attended key is zeros. Nothing here follows a kernel's order of operations: an operation
is a `gather` (which q row, which K / V rows, which bias, which keys are attended: the site's addressing) and one `attend`.

Bound, with u = 2^-24, D the head dim, n the attended keys of the row, p the fp64 weights, s the fp64 logits:
    ds      = (D + 2) u max_j(sum_d |q_d k_jd| + |bias_j|)              any-order fp32 dot product + the bias add
    eps_p   = 2 ds + 2 u min(max_j s_j - min_j s_j, 104) + (n + 8) u    argument rounding, 1-ulp exp, the sum, the division
    bound_d = sum_j p_j |v_jd| (eps_p + (n + 1) u) + 2^-120 sum_j |v_jd|   any-order fp32 P.V; weights flushed to 0
The GPU tests assert |got - ref| <= bound with no factor on top.

Inputs (one generator for every case, from the counter hashes of ripor_amd.utils.synth): K uniform with unit variance, V
uniform in [-1, 1) with the key's signature (position + 1 + slot / 16) on every eighth column, and three kinds of q rows by
row index mod 3: flat (logit standard deviation ~ 1), peaked (a multiple of one key's direction, scaled so that the winner
leads by 20 .. 120 with the bias counted; the peaked rows of a (query, head) take the last attended key, the first, then key
i mod n) and near-zero (the bias alone decides). rel_bias is uniform in [-0.5, 0.5); the odd heads also carry +30 on one
bucket and -30 on another, at a distance that depends on the head. Keys a mask excludes have a K row like any other and V rows of magnitude 100: a kernel that lets one in shows it."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from ripor_amd.utils import synth

U = 2.0 ** -24
MAX_LQ, MAX_DEC_LEN = 256, 64
NB, MAXD = 32, 128


# ---------------------------------------------------------------------------------------------- relative-position buckets
def hf_bucket(rel: int, bidirectional: bool, num_buckets: int = NB, max_distance: int = MAXD) -> int:
    """HF T5Attention._relative_position_bucket for one rel = key - query (float32 log, truncation), restated."""
    b = 0
    if bidirectional:
        num_buckets //= 2
        if rel > 0:
            b += num_buckets
        n = abs(rel)
    else:
        n = -min(rel, 0)
    max_exact = num_buckets // 2
    if n < max_exact:
        return b + n
    v = np.log(np.float32(n) / np.float32(max_exact)) / np.float32(math.log(max_distance / max_exact)) * np.float32(num_buckets - max_exact)
    return b + min(max_exact + int(np.float32(v)), num_buckets - 1)


_TABLES: Dict[Tuple[bool, int, int], np.ndarray] = {}


def bucket_of(rel: np.ndarray, bidirectional: bool, num_buckets: int = NB, max_distance: int = MAXD) -> np.ndarray:
    """Bucket of every rel = key - query in the array (|rel| < 256)."""
    key = (bidirectional, num_buckets, max_distance)
    if key not in _TABLES:
        _TABLES[key] = np.array([hf_bucket(r, bidirectional, num_buckets, max_distance) for r in range(-(MAX_LQ - 1), MAX_LQ)], dtype=np.int64)
    return _TABLES[key][np.asarray(rel) + MAX_LQ - 1]


# ---------------------------------------------------------------------------------------------- the operation itself
def softmax_eps(q, K, bias, ok, qk, dtype=np.float64, want_eps=True):
    """The weights of `attend` and their relative error bound: (p [R, n], eps_p [R] or None, attended keys [R]); qk(a, b) is
    the product of q rows with K rows in K's layout. Shared with tests/attn_train_ref.py, whose bound starts from eps_p."""
    D = q.shape[1]
    q = q.astype(dtype)
    s = qk(q, K)
    if bias is not None:
        s = s + bias.astype(dtype)
    has = ok.any(axis=1)
    neg = np.where(ok, s, -np.inf)
    mx = np.where(has, neg.max(axis=1, initial=-np.inf), 0).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.where(ok, np.exp(np.where(ok, s, 0) - mx[:, None]), 0).astype(dtype)
    sm = e.sum(axis=1)
    p = np.where(has[:, None], e / np.where(sm > 0, sm, 1)[:, None], 0).astype(dtype)
    cnt = ok.sum(axis=1)
    if not want_eps:
        return p, None, cnt
    A = qk(np.abs(q), np.abs(K)) + (np.abs(bias) if bias is not None else 0)
    ds = (D + 2) * U * np.where(ok, A, 0).max(axis=1, initial=0)
    spread = np.where(has, mx - np.where(ok, s, np.inf).min(axis=1, initial=np.inf), 0)
    eps = 2 * ds + 2 * U * np.minimum(spread, 104) + (cnt + 8) * U
    return p, eps, cnt


def attend(q, K, V, bias, ok, dtype=np.float64, want_bound=True):
    """q [R, D]; K, V [R or 1, n, D]; bias [R, n] or None; ok [R, n] bool (attended). Returns (out [R, D], bound [R, D]);
    dtype float32 is the plain numpy fp32 evaluation of the same expression (its bound is not meaningful)."""
    R, D = q.shape
    n = ok.shape[1]
    shared = K.shape[0] == 1 and V.shape[0] == 1      # one K / V for all rows: plain matrix products (masked keys hold finite values)
    if shared:
        K, V = K[0].astype(dtype), V[0].astype(dtype)
        qk = lambda a, b: a @ b.T
        pv = lambda a, b: a @ b
    else:
        okb = np.broadcast_to(ok[:, :, None], (R, n, D))
        K = np.where(okb, np.broadcast_to(K, (R, n, D)), 0).astype(dtype)   # what a masked key holds never enters
        V = np.where(okb, np.broadcast_to(V, (R, n, D)), 0).astype(dtype)
        qk = lambda a, b: np.einsum("rd,rnd->rn", a, b)
        pv = lambda a, b: np.einsum("rn,rnd->rd", a, b)
    p, eps, cnt = softmax_eps(q, K, bias, ok, qk, dtype, want_bound)
    out = pv(p, V)
    if not want_bound:
        return out, None
    absV = np.abs(V)
    bound = pv(p, absV) * (eps + (cnt + 1) * U)[:, None] + 2.0 ** -120 * pv(ok.astype(dtype), absV)
    return out, bound


@dataclass
class Group:
    """One (query, head) of a launch: what enters the definition, and where its output rows go."""
    q: np.ndarray                  # [R, D]
    K: np.ndarray                  # [R or 1, n, D]
    V: np.ndarray
    bias: Optional[np.ndarray]     # [R, n]
    ok: np.ndarray                 # [R, n] bool
    rows: np.ndarray               # [R] rows of the q source and of the output; columns h * D .. h * D + D - 1


MUTANTS = ("bias_shift", "bias_head", "drop_last", "drop_16", "mask_ignored", "last_as_count", "anc_ignored", "causal_off",
           "next_query", "padded_offset", "kvq_as_flist")


def _drop_last(ok):
    ok = ok.copy()
    n = ok.shape[1]
    last = n - 1 - np.argmax(ok[:, ::-1], axis=1)
    has = ok.any(axis=1)
    ok[np.nonzero(has)[0], last[has]] = False
    return ok


def _common_mut(ok, mut):
    if mut == "drop_last":
        return _drop_last(ok)
    if mut == "drop_16":
        ok = ok.copy()
        ok[:, ::16] = False
    return ok


def _rel_bias(inp, mut):
    rb = inp["rel_bias"]
    if mut == "bias_shift":
        rb = np.roll(rb, 1, axis=0)
    elif mut == "bias_head":
        rb = np.roll(rb, -1, axis=1)
    return rb


# ---- encoder / causal self-attention over the rows of one sequence: qkv [rows, 3 inner] ----
def gather_enc(inp, qi, h, mut=None) -> Optional[Group]:
    Lq, H, D = inp["Lq"], inp["H"], inp["D"]
    inner = H * D
    packed = inp["offs"] is not None
    nrow = int(inp["lens"][qi]) if packed else Lq
    if nrow == 0:
        return None
    nalloc = inp["qkv"].shape[0]
    row0 = int(inp["offs"][qi]) if packed else qi * Lq
    rows = row0 + np.arange(nrow)
    kv0 = row0
    if mut == "next_query":
        q2 = (qi + 1) % inp["Q"]
        kv0 = int(inp["offs"][q2]) if packed else q2 * Lq
    elif mut == "padded_offset" and packed:
        kv0 = qi * Lq
    kvrows = np.minimum(kv0 + np.arange(nrow), nalloc - 1)
    qkv = inp["qkv"]
    i = np.arange(nrow)[:, None]
    j = np.arange(nrow)[None, :]
    rb = _rel_bias(inp, mut)
    if inp["causal"]:
        ok = j <= (i + 1 if mut == "causal_off" else i)
        bias = rb[bucket_of(np.minimum(j - i, 0), False), h]
    else:
        m = inp["mask"][qi, :nrow] != 0
        ok = np.broadcast_to(np.ones(nrow, bool) if mut == "mask_ignored" else m, (nrow, nrow))
        bias = rb[bucket_of(j - i, True), h]
    ok = _common_mut(np.array(ok), mut)
    c = slice(h * D, (h + 1) * D)
    return Group(qkv[rows, c], qkv[kvrows, inner + h * D:inner + (h + 1) * D][None], qkv[kvrows, 2 * inner + h * D:2 * inner + (h + 1) * D][None],
                 bias, ok, rows)


# ---- KV cache addressing shared by the step and the tail self-attention ----
def _cache_rows(cache, strides, qc, h, pos, slot, D):
    qs, hs, ps, ss = strides
    base = qc * qs + h * hs + np.asarray(pos) * ps + np.asarray(slot) * ss
    return cache[base[..., None] + np.arange(D)]


def gather_self(inp, qi, h, mut=None) -> Optional[Group]:
    B, H, D, t = inp["B"], inp["H"], inp["D"], inp["t"]
    if qi >= inp["nq"]:
        return None
    rows = qi * B + np.arange(B)
    n = t + 1
    pos = np.arange(n)[None, :]
    own = np.arange(B)[:, None]
    slot = np.where(pos == t, own, inp["anc"][rows][:, :n].astype(np.int64) if t > 0 else own)
    if mut == "anc_ignored":
        slot = np.broadcast_to(own, (B, n))
    qc = (qi + 1) % inp["Q"] if mut == "next_query" else qi
    K = _cache_rows(inp["kcache"], inp["strides"], qc, h, np.broadcast_to(pos, (B, n)), slot, D)
    V = _cache_rows(inp["vcache"], inp["strides"], qc, h, np.broadcast_to(pos, (B, n)), slot, D)
    bias = np.broadcast_to(_rel_bias(inp, mut)[bucket_of(-(t - pos), False), h], (B, n))
    ok = _common_mut(np.ones((B, n), bool), mut)
    return Group(inp["q"][rows, h * D:(h + 1) * D], K, V, bias, ok, rows)


# ---- cross-attention: B rows per query against the query's encoder rows ----
def gather_cross(inp, qi, h, mut=None) -> Optional[Group]:
    B, H, D, Lq = inp["B"], inp["H"], inp["D"], inp["Lq"]
    inner = H * D
    if qi >= inp["nq"]:
        return None
    packed = inp["offs"] is not None
    rows = qi * B + np.arange(B)
    m = inp["mask"][qi] != 0
    row0 = int(inp["offs"][qi]) if packed else qi * Lq
    if mut == "next_query":
        q2 = (qi + 1) % inp["Q"]
        row0 = int(inp["offs"][q2]) if packed else q2 * Lq
    elif mut == "padded_offset" and packed:
        row0 = qi * Lq
    okk = m.copy()
    if mut == "mask_ignored":
        okk[:] = True
    elif mut == "last_as_count":
        okk[int(m.sum()):] = False
    xrows = np.minimum(row0 + np.arange(Lq), inp["x"].shape[0] - 1)
    ok = _common_mut(np.broadcast_to(okk, (B, Lq)).copy(), mut)
    x = inp["x"]
    return Group(inp["q"][rows, h * D:(h + 1) * D], x[xrows, h * D:(h + 1) * D][None], x[xrows, inner + h * D:inner + (h + 1) * D][None],
                 None, ok, rows)


# ---- tail self-attention: entry fi (its B sequences), positions < T from the cache, >= T from the own rows ----
def gather_tail_self(inp, fi, h, mut=None) -> Optional[Group]:
    B, H, D, T, L = inp["B"], inp["H"], inp["D"], inp["T"], inp["L"]
    inner, Lt = H * D, L - T
    seqs = [fi * B + b for b in range(B) if fi * B + b < inp["nseq"]]
    if not seqs:
        return None
    qi = int(inp["flist"][fi])
    src = fi
    if mut == "next_query":
        src = (fi + 1) % len(inp["flist"])
    qc = int(inp["flist"][src]) if (mut == "kvq_as_flist" or inp["kvq"] is None) else int(inp["kvq"][src])
    qkv = inp["qkv"]
    Ks, Vs, qs, rows = [], [], [], []
    for s in seqs:
        b = s - fi * B
        slot = np.full(T, b) if mut == "anc_ignored" else inp["anc"][qi * B + b, :T].astype(np.int64)
        own = s * Lt + np.arange(Lt)
        Ks.append(np.concatenate([_cache_rows(inp["kcache"], inp["strides"], qc, h, np.arange(T), slot, D),
                                  qkv[own, inner + h * D:inner + (h + 1) * D]]))
        Vs.append(np.concatenate([_cache_rows(inp["vcache"], inp["strides"], qc, h, np.arange(T), slot, D),
                                  qkv[own, 2 * inner + h * D:2 * inner + (h + 1) * D]]))
        qs.append(qkv[own, h * D:(h + 1) * D])
        rows.append(own)
    K = np.repeat(np.stack(Ks), Lt, axis=0)          # [nseq_g * Lt, L, D]
    V = np.repeat(np.stack(Vs), Lt, axis=0)
    i = np.tile(T + np.arange(Lt), len(seqs))[:, None]
    j = np.arange(L)[None, :]
    ok = _common_mut(np.array(j <= (i + 1 if mut == "causal_off" else i)), mut)
    bias = _rel_bias(inp, mut)[bucket_of(np.minimum(j - i, 0), False), h]
    rows = np.concatenate(rows)
    return Group(np.concatenate(qs), K, V, bias, ok, rows)


GATHER = {"enc": gather_enc, "self": gather_self, "cross": gather_cross, "tail_self": gather_tail_self}


def n_groups(inp) -> int:
    return len(inp["flist"]) if inp["site"] == "tail_self" else inp["Q"]


def all_pairs(inp) -> List[Tuple[int, int]]:
    return [(g, h) for g in range(n_groups(inp)) for h in range(inp["H"])]


def out_shape(inp) -> Tuple[int, int]:
    return inp["out_rows"], inp["H"] * inp["D"]


def reference(inp, pairs=None, mut=None, dtype=np.float64):
    """{(group, head): (rows, out [R, D], bound [R, D] or None)} for the pairs asked for (default: all that are live)."""
    res = {}
    gather = GATHER[inp["site"]]
    for g, h in (pairs if pairs is not None else all_pairs(inp)):
        G = gather(inp, g, h, mut)
        if G is None:
            continue
        o, b = attend(G.q, G.K, G.V, G.bias, G.ok, dtype, want_bound=dtype == np.float64)
        res[(g, h)] = (G.rows, o, b)
    return res


def assemble(inp, res):
    """(out, bound, written) over the whole output buffer: what nobody writes keeps out = 0 and written = False."""
    D = inp["D"]
    out = np.zeros(out_shape(inp), np.float64)
    bound = np.zeros(out_shape(inp), np.float64)
    written = np.zeros(out_shape(inp), bool)
    for (g, h), (rows, o, b) in res.items():
        c = slice(h * D, (h + 1) * D)
        out[rows, c] = o
        if b is not None:
            bound[rows, c] = b
        written[rows, c] = True
    return out, bound, written


def same_definition(a: Optional[Group], b: Optional[Group]) -> bool:
    """True when a mutant leaves everything that enters the definition of this (group, head) as it was: it is then a no-op
    here by construction (a prefix mask has no hole for `last_as_count` to miss, query 0 is packed at the padded offset, a
    single attended key takes weight 1 whatever its bias)."""
    if a is None or b is None:
        return a is None and b is None
    if not np.array_equal(a.ok, b.ok):
        return False
    R, n = a.ok.shape
    okb = a.ok[:, :, None]
    for x, y in ((a.K, b.K), (a.V, b.V)):
        if not np.array_equal(np.where(okb, np.broadcast_to(x, (R, n, x.shape[2])), 0), np.where(okb, np.broadcast_to(y, (R, n, y.shape[2])), 0)):
            return False
    if a.bias is not None:   # a bias that moves by one constant over a row's attended keys leaves the softmax as it is (one key: always)
        db = np.where(a.ok, b.bias.astype(np.float64) - a.bias, np.nan)
        has = a.ok.any(axis=1)
        if has.any() and (np.nanmax(db[has], axis=1) != np.nanmin(db[has], axis=1)).any():
            return False
    return np.array_equal(a.q, b.q)


# ---------------------------------------------------------------------------------------------- inputs
@dataclass
class Case:
    name: str
    site: str                      # enc | self | cross | tail_self
    kernel: str                    # the AttnKernel the planner must report
    p: dict = field(default_factory=dict)
    sample: int = 0                # > 0: the reference is taken on this many hashed (group, head) pairs + the first and the last


def _sig_v(name, pos, extra, D):
    """V rows: uniform [-1, 1) with the key's signature on every eighth column. pos / extra broadcast to the row shape."""
    pos = np.asarray(pos, np.float64)
    v = synth.uniform_f32(name, pos.shape + (D,), 1.0).astype(np.float32)
    v[..., 3::8] = (pos + 1.0 + np.asarray(extra, np.float64) / 16.0)[..., None]
    return v


def _rel_bias_table(name, H, bidirectional, d_uni=None):
    """[NB, H]: uniform [-0.5, 0.5); the odd heads also carry one +30 and one -30 entry (the even heads keep their flat rows
    flat). Bidirectional: +30 on rel = +d (bucket NB / 2 + d), -30 on rel = -d (bucket d), d = 3 .. 6 changing from one odd
    head to the next; a row whose key i + d does not exist or is masked stays flat. Unidirectional (rel = -n): -30 on distance
    2 and +30 on the bucket of distance d_uni — where the rows of a sequence differ in position (causal layouts) the caller
    puts it in the middle of the query positions, so that the rows in front of it stay flat; default 3 .. 6 by head."""
    rb = synth.uniform_f32(name + "/rel_bias", (NB, H), 0.5).astype(np.float32)
    for h in range(1, H, 2):
        d = 3 + (h // 2) % 4
        if bidirectional:
            rb[NB // 2 + d, h], rb[d, h] = 30.0, -30.0
        else:
            rb[2, h] = -30.0
            rb[int(bucket_of(-min(d_uni if d_uni is not None else d, MAX_LQ - 1), False)), h] = 30.0
    return rb


def _craft_q(name, G: Group, D: int, row_ids: np.ndarray) -> np.ndarray:
    """The q rows of one (group, head): kinds by row id mod 3 (flat, peaked, near zero)."""
    R = G.ok.shape[0]
    n = G.ok.shape[1]
    flat = synth.uniform_f32(name, (R, D), math.sqrt(3.0 / D)).astype(np.float64)
    kind = row_ids % 3 if R >= 3 else np.zeros(R, np.int64)   # fewer than three rows: all flat
    q = flat.copy()
    q[kind == 2] *= 1e-3
    pk = np.nonzero((kind == 1) & G.ok.any(axis=1))[0]
    if len(pk):
        ok = G.ok[pk]
        K = np.broadcast_to(G.K, (R, n, D))[pk].astype(np.float64)
        bias = G.bias[pk].astype(np.float64) if G.bias is not None else np.zeros((len(pk), n))
        cnt = ok.sum(axis=1)
        m = np.arange(len(pk))                       # the m-th peaked row of the group: last key, first key, then key i mod n
        first = np.argmax(ok, axis=1)
        last = n - 1 - np.argmax(ok[:, ::-1], axis=1)
        order = np.argsort(~ok, axis=1, kind="stable")   # attended keys first, in order
        kth = order[np.arange(len(pk)), row_ids[pk] % cnt]
        w = np.where(m % 4 == 0, last, np.where(m % 4 == 1, first, kth))
        kw = K[np.arange(len(pk)), w]
        nw = (kw * kw).sum(axis=1)
        c = np.einsum("rnd,rd->rn", K, kw) / nw[:, None]
        lead = 20.0 + 100.0 * ((row_ids[pk] * 37 + 11) % 101) / 100.0
        bw = bias[np.arange(len(pk)), w]
        other = ok.copy()
        other[np.arange(len(pk)), w] = False
        need = np.where(other, (lead[:, None] - bw[:, None] + bias) / np.maximum(1.0 - c, 0.05), -np.inf)
        M = np.maximum(need.max(axis=1, initial=0.0), 0.0)
        M = np.where(other.any(axis=1), M, lead)
        q[pk] = kw * (M / nw)[:, None]
    return q.astype(np.float32)


def _fill_q(case: Case, inp, qbuf, col0, pairs=None):
    """Writes the crafted q rows of every (group, head) (or of `pairs`) into qbuf[:, col0 + h * D ...]."""
    D = inp["D"]
    gather = GATHER[inp["site"]]
    for g, h in (pairs if pairs is not None else all_pairs(inp)):
        G = gather(inp, g, h)
        if G is None:
            continue
        ids = np.arange(len(G.rows)) + g + h      # kinds shift with query and head: every kind meets every row position
        qbuf[G.rows, col0 + h * D:col0 + (h + 1) * D] = _craft_q(f"{case.name}/q/{g}/{h}", G, D, ids)


def make_mask(Q, Lq, lens, holes):
    """lens[q] = index of the last attended key + 1; holes: queries whose mask loses interior positions."""
    mask = np.zeros((Q, Lq), np.int32)
    for q, n in enumerate(lens):
        mask[q, :n] = 1
        if q in holes:
            for j in (1, 4, 15, 16, n - 2):
                if 0 < j < n - 1:
                    mask[q, j] = 0
    return mask


def sample_pairs(case: Case, inp) -> Optional[List[Tuple[int, int]]]:
    if not case.sample:
        return None
    allp = all_pairs(inp)
    idx = synth.randint(case.name + "/sample", (case.sample,), 0, len(allp))
    return sorted({allp[0], allp[-1]} | {allp[int(i)] for i in idx})


def make_inputs(case: Case):
    """numpy inputs of a case (float32 / int32 / uint16 arrays as the hook takes them, plus the scalars of the shape)."""
    p, nm = case.p, case.name
    H, D = p["H"], p.get("dkv", 64)
    inner = H * D
    inp = dict(site=case.site, H=H, D=D, Q=p.get("Q", 0))
    if case.site == "enc":
        Q, Lq = p["Q"], p["Lq"]
        causal = bool(p.get("causal"))
        lens = list(p.get("lens", [Lq] * Q))
        mask = None if causal else make_mask(Q, Lq, lens, p.get("holes", ()))
        packed = bool(p.get("packed"))
        nalloc = Q * Lq
        pos = np.tile(np.arange(Lq), Q)
        qkv = np.zeros((nalloc, 3 * inner), np.float32)
        qkv[:, inner:2 * inner] = synth.uniform_f32(nm + "/k", (nalloc, inner), math.sqrt(3.0))
        qkv[:, 2 * inner:] = _sig_v(nm + "/v", np.repeat(pos[:, None], H, 1), np.repeat(np.arange(Q), Lq)[:, None] * np.ones((1, H)), D).reshape(nalloc, inner)
        offs = plens = None
        if packed:
            plens = np.array(lens, np.int32)
            offs = np.concatenate([[0], np.cumsum(plens)[:-1]]).astype(np.int32)
            packed_pos = np.concatenate([np.arange(n) for n in lens] + [np.zeros(nalloc - int(plens.sum()), np.int64)])
            qkv[:, 2 * inner:] = _sig_v(nm + "/v", np.repeat(packed_pos[:, None], H, 1), np.zeros((nalloc, H)), D).reshape(nalloc, inner)
            keymask = np.concatenate([mask[q, :n] for q, n in enumerate(lens)] + [np.ones(nalloc - int(plens.sum()), np.int32)])
        elif not causal:
            keymask = mask.reshape(-1)
        if not causal:   # keys the mask excludes: K like any other, V of magnitude 100
            dead = keymask == 0
            qkv[dead, 2 * inner:] = synth.uniform_f32(nm + "/garbage", (int(dead.sum()), inner), 100.0)
        inp.update(qkv=qkv, mask=mask, offs=offs, lens=plens, Lq=Lq, causal=causal, mfma=bool(p.get("mfma")),
                   rel_bias=_rel_bias_table(nm, H, not causal, max(Lq // 2, 1)), out_rows=nalloc)
        _fill_q(case, inp, qkv, 0)
    elif case.site in ("self", "tail_self"):
        B = p["B"]
        if case.site == "self":
            Qs, t = p["Q"], p["t"]
            depth, npos = max(p.get("depth", 0), t + 1), t + 1
        else:
            Qs, depth, npos = p["Qs"], p["T"], p["T"]
        ss = D * p.get("slot_mul", 1)
        strides = (H * depth * B * ss, depth * B * ss, B * ss, ss)
        ncache = Qs * strides[0]
        kc = synth.uniform_f32(nm + "/kc", (ncache,), math.sqrt(3.0))
        shp = (Qs, H, depth, B)
        posg = np.broadcast_to(np.arange(depth)[None, None, :, None], shp)
        slotg = np.broadcast_to(np.arange(B)[None, None, None, :], shp)
        vc = synth.uniform_f32(nm + "/vgap", (ncache,), 100.0)
        vc.reshape(Qs, H, depth, B, ss)[..., :D] = _sig_v(nm + "/vc", posg, slotg, D)
        pat = p.get("anc", 0)
        anc_ld = p.get("anc_ld", max(depth, p.get("L", 0)) + 1)
        if pat == 0:
            anc = synth.randint(nm + "/anc", (Qs * B, anc_ld), 0, B)
        elif pat == 1:
            anc = np.zeros((Qs * B, anc_ld), np.int64)
        else:
            anc = np.tile((B - 1 - np.arange(B))[:, None], (Qs, anc_ld))
        d_uni = None if case.site == "self" else p["T"] + (p["L"] - p["T"] + 1) // 2
        inp.update(kcache=kc, vcache=vc, strides=strides, anc=anc.astype(np.uint16), B=B, rel_bias=_rel_bias_table(nm, H, False, d_uni))
        if case.site == "self":
            inp.update(Q=Qs, t=t, nq=p.get("nq", Qs), out_rows=Qs * B + 3)
            q = np.zeros((Qs * B, inner), np.float32)
            inp["q"] = q
            _fill_q(case, inp, q, 0)
        else:
            T, L = p["T"], p["L"]
            Lt = L - T
            nent = p["entries"]
            ncap = nent * B
            flist = np.array(p["flist"], np.int32)
            kvq = np.array(p["kvq"], np.int32) if p.get("kvq") is not None else None
            qkv = np.zeros((ncap * Lt, 3 * inner), np.float32)
            qkv[:, inner:2 * inner] = synth.uniform_f32(nm + "/k", (ncap * Lt, inner), math.sqrt(3.0))
            tpos = np.tile(T + np.arange(Lt), ncap)
            qkv[:, 2 * inner:] = _sig_v(nm + "/v", np.repeat(tpos[:, None], H, 1), np.repeat(np.arange(ncap) % B, Lt)[:, None] * np.ones((1, H)), D).reshape(ncap * Lt, inner)
            inp.update(qkv=qkv, flist=flist, kvq=kvq, nseq=p["live"] * B, ncap=ncap, T=T, L=L, out_rows=ncap * Lt)
            _fill_q(case, inp, qkv, 0)
    elif case.site == "cross":
        Q, B, Lq = p["Q"], p["B"], p["Lq"]
        lens = list(p["lens"])
        mask = make_mask(Q, Lq, lens, p.get("holes", ()))
        packed = bool(p.get("packed"))
        xld = 2 * inner + 8
        nalloc = Q * Lq
        x = np.full((nalloc, xld), np.nan, np.float32)     # the gap columns behind K | V are never read
        x[:, :inner] = synth.uniform_f32(nm + "/k", (nalloc, inner), math.sqrt(3.0))
        offs = None
        if packed:
            plens = np.array(lens, np.int64)
            offs = np.concatenate([[0], np.cumsum(plens)[:-1]]).astype(np.int32)
            pos = np.concatenate([np.arange(n) for n in lens] + [np.zeros(nalloc - int(plens.sum()), np.int64)])
            qid = np.concatenate([np.full(n, q) for q, n in enumerate(lens)] + [np.zeros(nalloc - int(plens.sum()), np.int64)])
            keymask = np.concatenate([mask[q, :n] for q, n in enumerate(lens)] + [np.ones(nalloc - int(plens.sum()), np.int32)])
        else:
            pos, qid, keymask = np.tile(np.arange(Lq), Q), np.repeat(np.arange(Q), Lq), mask.reshape(-1)
        x[:, inner:2 * inner] = _sig_v(nm + "/v", np.repeat(pos[:, None], H, 1), np.repeat(qid[:, None], H, 1), D).reshape(nalloc, inner)
        dead = keymask == 0
        x[dead, inner:2 * inner] = synth.uniform_f32(nm + "/garbage", (int(dead.sum()), inner), 100.0)
        inp.update(x=x, xld=xld, mask=mask, offs=offs, Lq=Lq, B=B, nq=p.get("nq", Q), cross_site=p["cross_site"], out_rows=Q * B + 3)
        pairs = sample_pairs(case, inp)
        q = synth.uniform_f32(nm + "/q", (Q * B, inner), math.sqrt(3.0 / D)) if pairs is not None else np.zeros((Q * B, inner), np.float32)
        inp["q"] = q
        _fill_q(case, inp, q, 0, pairs)
    else:
        raise ValueError(case.site)
    return inp


# ---------------------------------------------------------------------------------------------- the case table
def _self_kernel(nk, d128):
    if d128:
        return ("SELF_FAST4_D128" if nk <= 8 else "SELF_FAST8_D128" if nk <= 16 else "SELF_FAST12_D128" if nk <= 24
                else "SELF_FAST18_D128" if nk <= 36 else "SELF_GENERIC_D128")
    return ("SELF_FAST2" if nk <= 8 else "SELF_FAST4" if nk <= 16 else "SELF_FAST6" if nk <= 24 else "SELF_FAST8" if nk <= 32
            else "SELF_FAST9" if nk <= 36 else "SELF_GENERIC")


def _lens3(Lq):
    return (Lq, max(Lq - 7, 1), 1)


def build_cases() -> List[Case]:
    cs: List[Case] = []
    # encoder, 64-dim heads: the 32 x 32 tile (kk_end steps at 8 / 16 / 24 keys; H 5: a ragged head block), padded and packed
    for packed in (0, 1):
        tag = "packed" if packed else "padded"
        cs.append(Case(f"enc_v2_L32_H12_{tag}", "enc", "ENC_V2", dict(Q=3, Lq=32, H=12, lens=(32, 25, 1), holes=(0,), packed=packed)))
        for Lq in (8, 9, 16, 17, 24, 25, 32):
            cs.append(Case(f"enc_v2_L{Lq}_H5_{tag}", "enc", "ENC_V2", dict(Q=3, Lq=Lq, H=5, lens=_lens3(Lq), holes=(0,), packed=packed)))
        for Lq in (33, 64, 65, 256):
            cs.append(Case(f"enc_valu64_L{Lq}_{tag}", "enc", "ENC_VALU64", dict(Q=3, Lq=Lq, H=4, lens=_lens3(Lq), holes=(0,), packed=packed)))
    # a query of the padded layout whose mask is all zero: zeros from every encoder kernel
    cs.append(Case("enc_v2_L32_empty", "enc", "ENC_V2", dict(Q=3, Lq=32, H=5, lens=(32, 0, 9), holes=(0,))))
    cs.append(Case("enc_valu64_L40_empty", "enc", "ENC_VALU64", dict(Q=3, Lq=40, H=4, lens=(40, 0, 9), holes=(0,))))
    cs.append(Case("enc_valu128_L24_empty", "enc", "ENC_VALU128", dict(Q=3, Lq=24, H=3, dkv=128, lens=(24, 0, 9), holes=(0,))))
    cs.append(Case("enc_valu128vg_L150_empty", "enc", "ENC_VALU128_VG", dict(Q=3, Lq=150, H=3, dkv=128, lens=(150, 0, 9), holes=(0,))))
    # causal (teacher-forced decoder layout)
    for Lq in (1, 31, 32):
        cs.append(Case(f"enc_causal_mfma_L{Lq}", "enc", "TRAIN_SELF_MFMA", dict(Q=3, Lq=Lq, H=5, causal=1, mfma=1)))
    cs.append(Case("enc_causal_mfma_L40", "enc", "ENC_VALU64", dict(Q=3, Lq=40, H=5, causal=1, mfma=1)))
    cs.append(Case("enc_causal_valu_L16", "enc", "ENC_VALU64", dict(Q=3, Lq=16, H=5, causal=1, mfma=0)))
    # 128-dim heads: the LDS switch between 139 and 140 tokens
    cs.append(Case("enc_valu128_L139", "enc", "ENC_VALU128", dict(Q=3, Lq=139, H=3, dkv=128, lens=_lens3(139), holes=(0,))))
    cs.append(Case("enc_valu128vg_L140", "enc", "ENC_VALU128_VG", dict(Q=3, Lq=140, H=3, dkv=128, lens=_lens3(140), holes=(0,))))
    cs.append(Case("enc_valu128vg_L256_packed", "enc", "ENC_VALU128_VG", dict(Q=3, Lq=256, H=3, dkv=128, lens=_lens3(256), holes=(0,), packed=1)))
    # step self-attention: every register-group count, three ancestry patterns, two cache layouts, a dead query
    for k, nk in enumerate((1, 8, 9, 16, 17, 24, 25, 32, 33, 36, 37, 64)):
        cs.append(Case(f"self_nk{nk}", "self", _self_kernel(nk, False),
                       dict(Q=3, B=7, H=12, t=nk - 1, nq=2, anc=k % 3, slot_mul=1 + k % 2, depth=32 if nk <= 32 else 64)))
    for k, nk in enumerate((8, 9, 16, 24, 25, 36, 37)):
        cs.append(Case(f"self128_nk{nk}", "self", _self_kernel(nk, True),
                       dict(Q=3, B=7, H=3, dkv=128, t=nk - 1, nq=2, anc=(k + 1) % 3, slot_mul=1 + (k + 1) % 2, depth=64)))
    # step cross-attention on the 16 x 16 tiles
    for B in (1, 15, 16):
        cs.append(Case(f"step_cross_B{B}", "cross", "STEP_CROSS16_ONE",
                       dict(cross_site=1, Q=3, B=B, H=12, Lq=32, lens=(32, 25, 1), holes=(0,), nq=2 if B == 15 else 3, packed=int(B == 16))))
    for B in (17, 33, 100):
        cs.append(Case(f"step_cross_B{B}", "cross", "STEP_CROSS16_MULTI",
                       dict(cross_site=1, Q=3, B=B, H=12, Lq=32, lens=(32, 25, 1), holes=(0,), packed=int(B == 33))))
    cs.append(Case("step_cross_lens_H5_B7", "cross", "STEP_CROSS16_ONE",
                   dict(cross_site=1, Q=5, B=7, H=5, Lq=32, lens=(1, 16, 17, 32, 0), holes=(3,))))
    cs.append(Case("step_cross_lens_H5_B20_packed", "cross", "STEP_CROSS16_MULTI",
                   dict(cross_site=1, Q=5, B=20, H=5, Lq=32, lens=(1, 16, 0, 17, 32), holes=(4,), packed=1)))
    cs.append(Case("step_cross_many_waves", "cross", "STEP_CROSS16_MULTI",
                   dict(cross_site=1, Q=256, B=130, H=16, Lq=20, lens=tuple(20 - (q % 5) for q in range(256)), holes=(0, 7)), sample=64))
    cs.append(Case("step_cross_L40_block", "cross", "CROSS_BLOCK64", dict(cross_site=1, Q=3, B=7, H=12, Lq=40, lens=_lens3(40), holes=(0,))))
    # block cross-attention: no chunks, a ragged last chunk, chunks of one row; 128-dim heads
    cs.append(Case("block_cross_L33_B10", "cross", "CROSS_BLOCK64", dict(cross_site=0, Q=3, B=10, H=12, Lq=33, lens=_lens3(33), holes=(0,))))
    cs.append(Case("block_cross_L64_B100", "cross", "CROSS_BLOCK64", dict(cross_site=0, Q=3, B=100, H=12, Lq=64, lens=(64, 57, 0), holes=(0,), packed=1)))
    cs.append(Case("block_cross_L256_B5", "cross", "CROSS_BLOCK64", dict(cross_site=0, Q=3, B=5, H=4, Lq=256, lens=_lens3(256), holes=(0,), nq=2)))
    cs.append(Case("block_cross128_L64_B10", "cross", "CROSS_BLOCK128", dict(cross_site=0, Q=3, B=10, H=3, dkv=128, Lq=64, lens=(64, 0, 9), holes=(0,))))
    cs.append(Case("block_cross128_L200_B3", "cross", "CROSS_WAVE128", dict(cross_site=0, Q=3, B=3, H=3, dkv=128, Lq=200, lens=(200, 0, 9), holes=(0,), packed=1)))
    cs.append(Case("step_cross128_L32_B7", "cross", "CROSS_BLOCK128", dict(cross_site=1, Q=3, B=7, H=3, dkv=128, Lq=32, lens=(32, 25, 1), holes=(0,))))
    # tail cross-attention: 32-row tiles (a ragged last tile), every kk_end step of the key count
    for k, rows in enumerate((1, 31, 32, 33, 240)):
        cs.append(Case(f"tail_cross_rows{rows}", "cross", "TAIL_CROSS_V2_TPW1",
                       dict(cross_site=2, Q=7, B=rows, H=12 if rows < 240 else 5, Lq=32, lens=(1, 8, 9, 24, 25, 32, 0), holes=(5,), packed=k % 2, nq=6 if k == 2 else 7)))
    cs.append(Case("tail_cross_many_waves", "cross", "TAIL_CROSS_V2_TPW9",
                   dict(cross_site=2, Q=64, B=1000, H=16, Lq=32, lens=tuple(32 - (q % 9) for q in range(64)), holes=(0, 5), packed=1), sample=64))
    cs.append(Case("tail_cross_L33", "cross", "TAIL_CROSS_G1_NKT2", dict(cross_site=2, Q=3, B=40, H=12, Lq=33, lens=(33, 26, 0), holes=(0,))))
    cs.append(Case("tail_cross_L64", "cross", "TAIL_CROSS_G1_NKT2", dict(cross_site=2, Q=3, B=40, H=5, Lq=64, lens=_lens3(64), holes=(0,), packed=1)))
    cs.append(Case("tail_cross_L65", "cross", "CROSS_BLOCK64", dict(cross_site=2, Q=3, B=40, H=12, Lq=65, lens=_lens3(65), holes=(0,))))
    # tail self-attention: 3 stage queries, 3 entries of which 2 are live, B 7; flist a permutation, kvq different from it
    tail = dict(Qs=3, entries=3, live=2, B=7, flist=(2, 0, 1), kvq=(1, 2, 0))
    for k, (L, T) in enumerate(((32, 1), (32, 8), (9, 3), (16, 5))):
        cs.append(Case(f"tail_self_L{L}_T{T}", "tail_self", "TAIL_SELF_V2", dict(H=12 if k % 2 == 0 else 5, L=L, T=T, anc=k % 3, slot_mul=1 + k % 2, **tail)))
    for k, (L, T) in enumerate(((32, 9), (32, 31))):
        cs.append(Case(f"tail_self_L{L}_T{T}", "tail_self", "TAIL_SELF_G1_NKT1", dict(H=12, L=L, T=T, anc=(k + 2) % 3, slot_mul=1 + k % 2, **tail)))
    for k, (L, T) in enumerate(((33, 2), (64, 40))):
        cs.append(Case(f"tail_self_L{L}_T{T}", "tail_self", "TAIL_SELF_G1_NKT2", dict(H=5, L=L, T=T, anc=k % 3, slot_mul=2 - k % 2, **tail)))
    cs.append(Case("tail_self128_L16_T5", "tail_self", "TAIL_SELF_VALU128", dict(H=3, dkv=128, L=16, T=5, anc=0, slot_mul=2, **tail)))
    return cs


CASES = build_cases()
# every name of RPR_ATTN_KERNELS except: NONE; TAIL_CROSS_G1_NKT1 (reachable only with a development switch); the training
# backward and the forward with dropped-out probabilities, 13 kernels, which tests/test_gpu_attn_train_direct.py takes one by
# one against tests/attn_train_ref.py (and test_gpu_train.py / test_gpu_long_queries.py through whole steps against autograd)
OUT_OF_SCOPE = {"NONE", "TAIL_CROSS_G1_NKT1", "TRAIN_BWD_MFMA", "TRAIN_BWD_VALU", "TRAIN_BWD_VALU128", "TRAIN_SELF_BWD_TILED",
                "TRAIN_CROSS_BWD_TILED", "TRAIN_SELF_DROP_FWD_TILED", "TRAIN_CROSS_DROP_FWD_TILED", "TRAIN_CROSS_BWD", "TRAIN_CROSS_BWD128",
                "TRAIN_SELF_DROP_FWD", "TRAIN_SELF_DROP_FWD128", "TRAIN_CROSS_DROP_FWD", "TRAIN_CROSS_DROP_FWD128"}


def planner_query(case: Case) -> Tuple[str, Dict[str, int]]:
    """(site, key=value arguments) of tests/attn_route_driver.cpp for this case."""
    p = case.p
    dkv = p.get("dkv", 64)
    if case.site == "enc":
        return "enc", dict(Q=p["Q"], Lq=p["Lq"], H=p["H"], buckets=NB, dkv=dkv, causal=int(bool(p.get("causal"))), mask=int(not p.get("causal")),
                           offs=int(bool(p.get("packed"))), out_h=0, mfma=int(bool(p.get("mfma"))))
    if case.site == "self":
        return "dec_self", dict(Q=p["Q"], B=p["B"], H=p["H"], t=p["t"], dkv=dkv)
    if case.site == "cross":
        return ("cross_block", "step_cross", "tail_cross")[p["cross_site"]], dict(Q=p["Q"], B=p["B"], H=p["H"], Lq=p["Lq"], dkv=dkv)
    return "tail_self", dict(nseq_cap=p["entries"] * p["B"], B=p["B"], H=p["H"], T=p["T"], L=p["L"], dkv=dkv)
