"""-m gpu: the gated-GELU feed-forward (T5 v1.1 / Flan-T5 / mT5: wo(gelu_new(wi_0 x) * wi_1 x)) on the device — the two gate
kernels through their operator hooks, then every pass that walks a layer: the search (encoder, decode steps, forced tail),
rpr_embed / rpr_lngknp_forward, and the two training steps in the three arithmetics, with dropout.

Yardsticks: the float64 numpy restatement of the gate (tests/gated_ref.py) for the hooks; the reference's own outputs
(tests/golden/make_golden_gated.py) for the search; the CPU oracles with ONE method overridden (GatedT5Ref, GatedT5RefCached,
GatedDropoutRef — pinned to the reference by tests/test_gated_golden.py) and torch autograd through them for everything else.
Bars are the project's own for these passes, copied: test_gpu_parity.py (ranked smtids, scores 1e-4, encoder output),
test_gpu_forced_tail.py, test_gpu_train.py / test_gpu_heads128.py (losses 1e-4 max(1, |ref|), position scores 1e-3, every
gradient tensor within 2e-4 of its largest entry, global norm 1e-3; bf16: losses and norm 3 %, cosine 0.995),
test_gpu_dropout.py, test_gpu_rq_search.py (embedding logits 5e-4).

GELU is smooth: unlike the ReLU tests no condition on the pre-activations is needed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gated_ref
from conftest import ORDER_TOL, SCORE_TOL, compare_ranked
from test_gated_golden import KIND, SEARCH, gated_golden, mask_fn

pytestmark = pytest.mark.gpu

REL_LOSS_TOL, POS_SCORE_TOL, LP_TOL, GRAD_TOL, NORM_TOL, STEP_LOGIT_TOL = 1e-4, 1e-3, 1e-3, 2e-4, 1e-3, 5e-4
RATE, SEED, STEP = 0.1, 0x1234_5678_9ABC_DEF1, 7   # test_gpu_dropout.py
FFS = 1.0 / 16                                     # FF_PLANE_SCALE (csrc/common.h)
SENTINEL = 12345.0
PLANE_SENTINEL = 1234.0    # (exact in float16)


@pytest.fixture(scope="module")
def E():
    from ripor_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


class _Prec:
    def __init__(self, name):
        from ripor_amd import engine as E
        self.ctx, self.name = E.Context.get(0), name

    def __enter__(self):
        self.ctx.set_precision(self.name)
        return self.ctx

    def __exit__(self, *a):
        self.ctx.set_precision("f16x2")
        self.ctx.lib.rpr_set_train_dropout(self.ctx.handle, 0.0, 0, 0)


# ---- 1. the operator hooks --------------------------------------------------------------------------------------------------
SHAPES = [(3, 32, None), (130, 96, 70), (5, 2816, None)]     # (M, F, live rows): one row group; more than one block with a
                                                             # device-side live count; d_ff of t5-v1.1-large
SPECIAL = [0.0, -0.0, 30.0, -30.0, 29.5, -29.5, 1e-4, -1e-4, 1.25e-4, -0.75e-4, 5.0, -5.0, 8.5, -8.5, 12.0, -12.0]


@functools.lru_cache(maxsize=None)
def hook_inputs(M, F):
    """gu [M, 2F] = (g | u) and dmid [M, F], float32: g ~ 3 N(0, 1) with +-0, |g| up to 30 (tanh saturated) and values around
    +-1e-4 planted four times each at seeded places; u ~ 2 N(0, 1); dmid ~ N(0, 1)."""
    rng = np.random.default_rng(1000 * M + F)
    g = (3.0 * rng.standard_normal((M, F))).astype(np.float32)
    at = rng.choice(M * F, 4 * len(SPECIAL), replace=False)
    g.reshape(-1)[at] = np.tile(np.asarray(SPECIAL, dtype=np.float32), 4)
    u = (2.0 * rng.standard_normal((M, F))).astype(np.float32)
    d = rng.standard_normal((M, F)).astype(np.float32)
    return np.concatenate([g, u], axis=1), d


def fwd_error(y, gu):
    """max |y - float64 y| in units of |u| max(|g|, 1): the size of the product the gate scales (|gelu_new(g)| <= |g|)."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F].astype(np.float64), gu[:, F:].astype(np.float64)
    scale = np.maximum(np.abs(u) * np.maximum(np.abs(g), 1.0), 1e-30)
    return float((np.abs(np.asarray(y, dtype=np.float64) - gated_ref.gate64(gu)) / scale).max())


def bwd_error(dgu, gu, d):
    """dg in units of |dmid u| (|gelu_new'| <= 1.13), du in units of |dmid| max(|g|, 1)."""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].astype(np.float64), gu[:, F:].astype(np.float64), d.astype(np.float64)
    ref = gated_ref.gate_bwd64(gu, d)
    e = np.abs(np.asarray(dgu, dtype=np.float64) - ref)
    sg = np.maximum(np.abs(d * u), 1e-30)
    su = np.maximum(np.abs(d) * np.maximum(np.abs(g), 1.0), 1e-30)
    return float(max((e[:, :F] / sg).max(), (e[:, F:] / su).max()))


@functools.lru_cache(maxsize=None)
def torch_cpu_errors(M, F):
    """The errors of torch's CPU fp32 NewGELUActivation(g) * u and of autograd through it, against float64, on the same inputs."""
    gu, d = hook_inputs(M, F)
    g = torch.from_numpy(gu[:, :F].copy()).requires_grad_(True)
    u = torch.from_numpy(gu[:, F:].copy()).requires_grad_(True)
    y = gated_ref.gelu_new_t(g) * u
    y.backward(torch.from_numpy(d))
    return fwd_error(y.detach().numpy(), gu), bwd_error(torch.cat([g.grad, u.grad], 1).numpy(), gu, d)


def _p(t):
    return t.data_ptr() if t is not None else None


def op_gate(E, gu, m_dev=None, out=None, planes=None):
    ctx = E.Context.get(0)
    M, F2 = gu.shape
    E.check(ctx.lib.rpr_op_gated_gelu(ctx.handle, gu.data_ptr(), M, F2 // 2, _p(m_dev), _p(out), _p(planes), E._stream_ptr(gu.device)),
            "rpr_op_gated_gelu")
    torch.cuda.synchronize()


def op_gate_bwd(E, gu, d):
    ctx = E.Context.get(0)
    M, F2 = gu.shape
    dgu = torch.full((M, F2), SENTINEL, dtype=torch.float32, device=gu.device)
    E.check(ctx.lib.rpr_op_gated_gelu_bwd(ctx.handle, gu.data_ptr(), d.data_ptr(), M, F2 // 2, dgu.data_ptr(), E._stream_ptr(gu.device)),
            "rpr_op_gated_gelu_bwd")
    torch.cuda.synchronize()
    return dgu


@pytest.mark.parametrize("M,F,live", SHAPES)
def test_forward_gate_hook_against_float64(E, M, F, live):
    """Bar: 4 x the error of torch's CPU fp32 NewGELUActivation(g) * u against float64 on the same inputs, in units of
    |u| max(|g|, 1) (the device's exp / division are another implementation than torch's tanh). Measured on the CPU, torch:
    1.09e-7 (3, 32), 1.37e-7 (130, 96), 1.32e-7 (5, 2816); the kernel on an MI355X: 1.00e-7, 1.62e-7, 1.51e-7. It evaluates 0.5 (1 + tanh z) as the logistic of 2 z and has no
    cancellation at g < -4, where torch's fp32 expression keeps one or two bits.
    Rows from *m_dev on keep the sentinel the output was filled with, in the fp32 output and in both planes."""
    gu_np, _ = hook_inputs(M, F)
    bar = 4.0 * torch_cpu_errors(M, F)[0]
    gu = torch.from_numpy(gu_np).cuda()
    m_dev = torch.tensor([live], dtype=torch.int32, device="cuda") if live is not None else None
    out = torch.full((M, F), SENTINEL, dtype=torch.float32, device="cuda")
    ctx = E.Context.get(0)
    ctx.status(clear=True)
    op_gate(E, gu, m_dev, out=out)
    n = M if live is None else live
    err = fwd_error(out[:n].cpu().numpy(), gu_np[:n])
    print(f"[gate] forward ({M}, {F}) live {live}: error {err:.3e}, torch CPU fp32 {bar / 4:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    assert bool((out[n:] == SENTINEL).all()), "rows past the live count were written"
    # +-0 in, +-0 out
    zero = gu[:n, :F] == 0
    assert bool(zero.any()) and bool((out[:n][zero] == 0).all())
    # the planes: (hi + lo) / scale equals the fp32 output to the planes' resolution (test_gpu_gemm_direct_epilogue.py: the
    # quantum of planes at scale 1/16 is 2^-20, 2^-21 relative), nothing flagged
    planes = torch.full((2, M, F), PLANE_SENTINEL, dtype=torch.float16, device="cuda")
    op_gate(E, gu, m_dev, planes=planes)
    dec = (planes[0, :n].double() + planes[1, :n].double()) / FFS
    y = out[:n].double()
    assert bool(((dec - y).abs() <= torch.maximum(torch.full_like(y, 2.0 ** -20), y.abs() * 2.0 ** -21)).all())
    assert bool((planes[:, n:] == PLANE_SENTINEL).all())
    assert ctx.status() == 0
    # both outputs in one call are the same bits
    out2 = torch.full_like(out, SENTINEL); planes2 = torch.full_like(planes, PLANE_SENTINEL)
    op_gate(E, gu, m_dev, out=out2, planes=planes2)
    assert torch.equal(out, out2) and torch.equal(planes, planes2)


def test_forward_gate_planes_saturate_beyond_their_range(E):
    """|y| > 65504 * 16 = 1.05e6 cannot be carried by the planes: clamped and RPR_STATUS_SATURATED, as the ReLU epilogue's."""
    ctx = E.Context.get(0)
    gu = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    gu[:, :32] = 30.0
    gu[:, 32:] = 3.4e4            # y = 30 * 3.4e4 = 1.02e6: inside
    planes = torch.zeros((2, 4, 32), dtype=torch.float16, device="cuda")
    ctx.status(clear=True)
    op_gate(E, gu, planes=planes)
    assert ctx.status() == 0
    gu[2, 32 + 5] = -3.6e4        # 1.08e6: beyond
    op_gate(E, gu, planes=planes)
    assert ctx.status() & E._lib.STATUS_SATURATED
    assert float(planes[0, 2, 5]) == -65504.0 and ctx.status() == 0
    out = torch.zeros((4, 32), dtype=torch.float32, device="cuda")
    op_gate(E, gu, out=out)       # the fp32 output has no such range
    assert ctx.status() == 0 and abs(float(out[2, 5]) + 1.08e6) < 1.0


@pytest.mark.parametrize("M,F,live", SHAPES)
def test_backward_gate_hook_against_float64(E, M, F, live):
    """Bar: 4 x the error of torch autograd (CPU fp32) through NewGELUActivation(g) * u against float64 on the same inputs; dg in
    units of |dmid u|, du in units of |dmid| max(|g|, 1). Measured on the CPU, torch: 4.65e-7 (3, 32), 5.80e-7 (130, 96),
    5.55e-7 (5, 2816); the kernel on an MI355X: 0.94e-7, 2.73e-7, 2.38e-7. Two identical calls give the same bits."""
    gu_np, d_np = hook_inputs(M, F)
    bar = 4.0 * torch_cpu_errors(M, F)[1]
    gu, d = torch.from_numpy(gu_np).cuda(), torch.from_numpy(d_np).cuda()
    dgu = op_gate_bwd(E, gu, d)
    err = bwd_error(dgu.cpu().numpy(), gu_np, d_np)
    print(f"[gate] backward ({M}, {F}): error {err:.3e}, torch CPU fp32 autograd {bar / 4:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    assert torch.equal(dgu, op_gate_bwd(E, gu, d))


# ---- 2. the search ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x2", "f32"])
@pytest.mark.parametrize("name", SEARCH)
def test_search_matches_reference_golden(E, name, precision):
    """The two fixtures of the imported reference (d_ff 96: W_in has 192 rows, one and a half 128-column tiles): ranked smtids,
    scores within 1e-4, the encoder output as test_gpu_parity.py compares it; graph replay, eager launches and the run with taps
    (which never forks) agree."""
    g = gated_golden(name)
    ids, mask = torch.from_numpy(g.input_ids), torch.from_numpy(g.attention_mask)
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, g.state_dict, g.dims)
        assert model.gated_ff
        trie = E.DeviceTrie.from_codes(ctx, g.codes, g.V)
        ctx.status(clear=True)
        res = E.search(model, trie, ids, mask, g.B, g.L)
        torch.cuda.synchronize()
        assert ctx.status() == 0
        stats = compare_ranked(g, res.tokens.cpu().numpy(), res.scores.cpu().numpy(), label=f" (gated {precision})")
        assert stats["boundary_excused"] == 0 and stats["sequences_missing"] == 0 and stats["ranks_checked"] >= 0.9 * g.Q * g.B, stats
        eager = E.search(model, trie, ids, mask, g.B, g.L, use_graph=False)
        assert torch.equal(res.tokens, eager.tokens) and torch.equal(res.scores, eager.scores)
        taps = E.search(model, trie, ids, mask, g.B, g.L, taps=True)
        torch.cuda.synchronize()
        np.testing.assert_allclose(taps.taps["encoder_out"].cpu().numpy(), g.z["encoder_out"], atol=2e-4, rtol=1e-4)
        compare_ranked(g, taps.tokens.cpu().numpy(), taps.scores.cpu().numpy(), label=f" (gated {precision}, step by step)")


def _gated_mini(E, ctx, L, V, seed, Q, **kw):
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=96, **kw)
    sd = synth.make_state_dict(dims, seed=seed, feed_forward_proj=KIND)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=seed, max_len=14)
    return dims, sd, ids, mask, E.DeviceModel(ctx, sd, dims)


def test_forced_tail_pass_equals_the_plain_loop(E):
    """set_forced_tail(1) with an explicit fork at depth 2 against the step-by-step loop (test_gpu_forced_tail.py's bars): the
    forced queries' remaining positions go through the tail pass, whose FF block runs the gate under the pass's device-side row
    count."""
    from ripor_amd.utils import synth
    L, V, B, N, Q = 8, 256, 4, 20_000, 24
    ctx = E.Context.get(0)
    codes = synth.make_codes(N, L, V, seed=11)
    dims, sd, ids, mask, model = _gated_mini(E, ctx, L, V, 3, Q)
    trie = E.DeviceTrie.from_codes(ctx, codes, V)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    try:
        ctx.set_forced_tail(False)
        plain = E.search(model, trie, ti, tm, B, L)
        ctx.set_forced_tail(True)
        ctx.set_fork_depths([2])
        res = E.search(model, trie, ti, tm, B, L)
        torch.cuda.synchronize()
        stats = ctx.last_fork_stats()
    finally:
        ctx.set_fork_depths(None)
        ctx.set_forced_tail(True)
    assert stats[0]["depth"] == 2 and stats[0]["forced"] > 0 and stats[0]["forced"] + stats[0]["left"] == Q, stats
    same = (res.tokens == plain.tokens).all(dim=2)
    close = (res.scores - plain.scores).abs() <= ORDER_TOL
    live = plain.scores > -1e6
    assert bool((same | close | ~live).all()), "sequences differ from the step-by-step loop"
    err = float(((res.scores - plain.scores).abs() * live).max())
    print(f"[gated forced tail] forks {stats}, max score diff {err:.2e}, {int(same.sum())}/{same.numel()} ranks identical")
    assert err <= 0.3 * SCORE_TOL, err
    both = same & live
    assert torch.equal(res.row_lo[both], plain.row_lo[both]) and torch.equal(res.row_hi[both], plain.row_hi[both])


@pytest.mark.parametrize("precision", ["f16x2", "f32"])
def test_search_with_320_decoder_rows_matches_the_cached_oracle(E, precision):
    """32 queries x 10 beams = 320 decoder rows per step (the plain loop): the W_in product of 192 columns leaves the skinny
    kernels. Against GatedT5RefCached: tokens outside score near-ties, scores within 1e-4."""
    from oracle import beam_ref
    from ripor_amd.utils import synth
    L, V, B, N, Q = 4, 256, 10, 3000, 32
    codes = synth.make_codes(N, L, V, seed=5)
    with _Prec(precision) as ctx:
        dims, sd, ids, mask, model = _gated_mini(E, ctx, L, V, 7, Q)
        trie = E.DeviceTrie.from_codes(ctx, codes, V)
        try:
            ctx.set_forced_tail(False)
            res = E.search(model, trie, torch.from_numpy(ids), torch.from_numpy(mask), B, L)
            torch.cuda.synchronize()
        finally:
            ctx.set_forced_tail(True)
    torch.set_num_threads(8)
    pm = beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(codes)), V)
    seqs, sc = beam_ref.beam_search_ref(gated_ref.GatedT5RefCached(sd, dims), pm, ids, mask, B, L, use_kv_cache=True)
    ref_tok, ref_sc = seqs.numpy().reshape(Q, B, L + 1)[:, :, 1:], sc.numpy().reshape(Q, B)
    near = np.zeros((Q, B), dtype=bool)
    near[:, 1:] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
    near[:, :-1] |= (ref_sc[:, :-1] - ref_sc[:, 1:]) <= ORDER_TOL
    assert ((res.tokens.cpu().numpy() == ref_tok).all(axis=2) | near).all() and near.mean() < 0.2
    np.testing.assert_allclose(res.scores.cpu().numpy(), ref_sc, atol=SCORE_TOL, rtol=0)


# ---- 3. the teacher-forced passes: a small gated model, one ragged batch ----------------------------------------------------
class Case:
    """d_model 256, 4 heads of 64, d_ff 96 (W_in 192 rows), 1 + 2 layers; bz 3, queries of 5..13 tokens (Lq 13, odd), L 8.
    The bf16 kernels reduce in tiles of 64 (K % 64 == 0, include/ripor_hip.h: rpr_op_linear_bf16), for either feed-forward
    kind: the bf16 runs take d_ff 192 (W_in 384 rows, W_out's reduction three tiles)."""

    def __init__(self, d_ff=96, shared=False):
        from oracle import train_ref
        from ripor_amd.utils import synth
        self.bz, self.L = 3, 8
        self.dims = synth.mini_dims(L=self.L, V=64, enc_layers=1, d_ff=d_ff, d_model=256, d_kv=64, num_heads=4, num_decoder_layers=2,
                                    shared_output_input_embeds=shared)
        self.sd = synth.make_state_dict(self.dims, seed=92, feed_forward_proj=KIND)
        self.ids, self.mask = synth.make_queries(self.bz, vocab_size=self.dims.vocab_size, seed=17, mean_len=9, std_len=3, min_len=5, max_len=13)
        assert self.ids.shape[1] == 13 and len(set(self.mask.sum(1).tolist())) > 1
        codes = synth.make_codes(2 * self.bz, self.L, 64, seed=23).astype(np.int64)
        self.pos, self.neg = codes[:self.bz], codes[self.bz:]
        self.prefix = train_ref.PREFIX_LENS[self.L]
        self.keys = [("" if k == self.L else train_ref.TEACHER_KEYS[k]) for k in self.prefix]
        self.loss_names = train_ref.LOSS_NAMES[self.L]
        self.teacher = {}
        for k, key in zip(self.prefix, self.keys):
            self.teacher[key + "teacher_pos_scores"] = synth.uniform_f32(f"gated/p{k}", (self.bz,), 30.0)
            self.teacher[key + "teacher_neg_scores"] = synth.uniform_f32(f"gated/n{k}", (self.bz,), 30.0)

    def lngknp_args(self):
        t = torch.from_numpy
        tp = t(np.stack([self.teacher[key + "teacher_pos_scores"] for key in self.keys]))
        tn = t(np.stack([self.teacher[key + "teacher_neg_scores"] for key in self.keys]))
        return t(self.ids), t(self.mask), t(np.stack([self.pos, self.neg], axis=1)), tp, tn, self.prefix

    def s2s_args(self):
        return torch.from_numpy(self.ids), torch.from_numpy(self.mask), torch.from_numpy(self.pos)


@functools.lru_cache(maxsize=None)
def _case(d_ff=96):
    return Case(d_ff)


def _dff(precision):
    return 192 if precision == "bf16" else 96


def _oracle(c, rate):
    return gated_ref.GatedT5Ref(c.sd, c.dims) if rate is None else gated_ref.GatedDropoutRef(c.sd, c.dims, rate, SEED, STEP)


@functools.lru_cache(maxsize=None)
def _lngknp_ref(rate=None, d_ff=96):
    """(losses by name, position scores [bz, 2, L], grads, global norm): autograd through the gated oracle, one thread = one
    summation order; computed once, shared by the precisions."""
    from oracle import train_ref
    c, prev = _case(d_ff), torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = _oracle(c, rate)
        if rate is not None:
            model.begin(2)
        out, _, grads, gn = train_ref.train_step(model, c.ids, c.mask, c.pos, c.neg, c.teacher)
    finally:
        torch.set_num_threads(prev)
    ps = np.stack([out["pos_position_scores"].numpy(), out["neg_position_scores"].numpy()], axis=1)
    return {k: float(out[k]) for k in c.loss_names}, ps, grads, gn


@functools.lru_cache(maxsize=None)
def _s2s_ref(rate=None, d_ff=96):
    from test_seq2seq_host import seq2seq_ce, seq2seq_grads
    c, prev = _case(d_ff), torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = _oracle(c, rate)
        loss, grads, gn = seq2seq_grads(model, c.ids, c.mask, c.pos)
        lp = None
        if rate is None:
            with torch.no_grad():
                lp = seq2seq_ce(model, c.ids, c.mask, c.pos)[1].numpy()
    finally:
        torch.set_num_threads(prev)
    return loss, lp, grads, gn


def _check_losses(tag, got, ref_pairs, tol=REL_LOSS_TOL):
    for g, (name, ref) in zip(got, ref_pairs):
        print(f"[gated] {tag}: loss {name} {float(g):.6f} vs {ref:.6f}")
        assert abs(float(g) - ref) <= tol * max(1.0, abs(ref)), (tag, name, float(g), ref)


def _check_grads(tag, state, og, gn):
    """fp32 level: every tensor, whole, within GRAD_TOL of its largest entry; the global norm within NORM_TOL."""
    grads = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
    assert sum(k.endswith(("wi_0.weight", "wi_1.weight")) for k in grads) == 6 and not any(k.endswith(".wi.weight") for k in grads)
    worst = (0.0, None)
    for k, v in grads.items():
        if k not in og:                      # a table autograd never reached (seq2seq: the last position's input codebook)
            assert not np.any(v), k
            continue
        o = og[k].double().numpy().reshape(v.shape)
        worst = max(worst, (float((np.abs(v - o) / max(np.abs(o).max(), 1e-30)).max()), k))
    hn = float(np.sqrt(sum((v ** 2).sum() for v in grads.values())))
    print(f"[gated] {tag}: worst tensor error {worst[0]:.2e} of its largest entry ({worst[1]}), norm {hn:.6g} vs {gn:.6g}")
    assert worst[0] <= GRAD_TOL, (tag, worst)
    assert abs(hn - gn) <= NORM_TOL * gn, (tag, hn, gn)


def _check_grads_bf16(tag, state, og, gn):
    """bf16 level (test_gpu_train.py / test_gpu_dropout.py): the global norm within 3 %, every tensor that is not noise-level
    (below 1e-4 of the largest entry of any tensor) within cosine 0.995 of the fp32 autograd gradient."""
    got = {k: v.detach().double().cpu() for k, v in state.named_grads().items()}
    hn = float(torch.sqrt(sum((v ** 2).sum() for v in got.values())))
    gmax = max(float(v.abs().max()) for v in og.values())
    cos = {}
    for k, v in got.items():
        if k not in og or float(og[k].abs().max()) < 1e-4 * gmax:
            continue
        r = og[k].double().reshape(v.shape)
        cos[k] = float((v * r).sum() / (v.norm() * r.norm() + 1e-300))
    worst = min((v, k) for k, v in cos.items())
    print(f"[gated] {tag}: norm {hn:.5g} vs {gn:.5g}, worst cosine {worst}")
    assert any(k.endswith("wi_0.weight") for k in cos) and any(k.endswith("wi_1.weight") for k in cos)
    assert abs(hn - gn) <= 3e-2 * hn, (hn, gn)
    assert worst[0] >= 0.995, worst


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_embed_and_lngknp_forward_match_the_oracle(E, precision):
    c = _case()
    oracle = gated_ref.GatedT5Ref(c.sd, c.dims)
    ids, mask = torch.from_numpy(c.ids), torch.from_numpy(c.mask)
    with torch.no_grad():
        want = oracle.last_logits(torch.full((c.bz, 1), -1, dtype=torch.long), oracle.encode(ids.long(), mask.long()), mask.long()).numpy()
    ref_losses, ref_ps, _, _ = _lngknp_ref()
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        ctx.status(clear=True)
        emb = E.embed(model, ids, mask)
        assert emb.shape == (c.bz, c.dims.d_model) and emb.dtype == torch.float32
        got = emb.cpu().double().numpy() @ oracle.out_embed(0).double().numpy().T
        print(f"[gated] embed {precision}: max |logit - oracle| {np.abs(got - want).max():.2e}")
        np.testing.assert_allclose(got, want, atol=STEP_LOGIT_TOL, rtol=0)
        losses, ps = E.lngknp_forward(model, *c.lngknp_args())
        torch.cuda.synchronize()
        assert ctx.status() == 0
        err = np.abs(ps.cpu().numpy() - ref_ps).max()
        print(f"[gated] forward {precision}: max position-score error {err:.2e}")
        assert err <= POS_SCORE_TOL
        _check_losses(f"forward {precision}", losses.cpu().numpy(), [(k, ref_losses[k]) for k in c.loss_names])
        again = E.lngknp_forward(model, *c.lngknp_args())
        assert torch.equal(losses, again[0]) and torch.equal(ps, again[1])


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
def test_lngknp_backward_matches_oracle_autograd(E, precision):
    c = _case(_dff(precision))
    ref_losses, _, og, gn = _lngknp_ref(None, _dff(precision))
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model)
        losses = E.lngknp_backward(model, state, *c.lngknp_args())
        torch.cuda.synchronize()
        tag, pairs = f"lngknp {precision}", [(k, ref_losses[k]) for k in c.loss_names]
        if precision == "bf16":
            _check_losses(tag, losses.cpu().numpy(), pairs, tol=3e-2)
            _check_grads_bf16(tag, state, og, gn)
        else:
            _check_losses(tag, losses.cpu().numpy(), pairs)
            _check_grads(tag, state, og, gn)
        first = state.grads.clone()
        state.grads.zero_()
        E.lngknp_backward(model, state, *c.lngknp_args())
        assert torch.equal(first, state.grads), "two identical calls must give the same bits"


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
def test_seq2seq_forward_and_backward_match_oracle_autograd(E, precision):
    c = _case(_dff(precision))
    ref_loss, ref_lp, og, gn = _s2s_ref(None, _dff(precision))
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        tag = f"seq2seq {precision}"
        tol = 3e-2 if precision == "bf16" else REL_LOSS_TOL
        loss, lp = E.seq2seq_forward(model, *c.s2s_args())
        torch.cuda.synchronize()
        _check_losses(tag + " forward", loss.cpu().numpy(), [("rank", ref_loss)], tol=tol)
        if precision != "bf16":
            assert np.abs(lp.cpu().numpy() - ref_lp).max() <= LP_TOL
        state = E.TrainState(model)
        loss = E.seq2seq_backward(model, state, *c.s2s_args())
        torch.cuda.synchronize()
        _check_losses(tag, loss.cpu().numpy(), [("rank", ref_loss)], tol=tol)
        (_check_grads_bf16 if precision == "bf16" else _check_grads)(tag, state, og, gn)
        first = state.grads.clone()
        E.seq2seq_backward(model, state, *c.s2s_args())
        assert torch.equal(first, state.grads), "two identical calls must give the same bits"


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("step", ["lngknp", "seq2seq"])
def test_steps_at_rate_01_match_autograd_with_the_same_masks(E, step, precision):
    """The inner-activation site masks the product [rows, d_ff] (HF T5DenseGatedActDense): GatedDropoutRef draws the same masks."""
    c = _case()
    if step == "lngknp":
        ref_losses, _, og, gn = _lngknp_ref(RATE)
        plain = _lngknp_ref()[0]
        pairs, plain_vals = [(k, ref_losses[k]) for k in c.loss_names], [plain[k] for k in c.loss_names]
    else:
        ref_loss, _, og, gn = _s2s_ref(RATE)
        pairs, plain_vals = [("rank", ref_loss)], [_s2s_ref()[0]]
    assert all(abs(r - p) > 1e-3 * abs(p) for (_, r), p in zip(pairs, plain_vals)), "dropout must move the losses"

    def run(state, **kw):
        if step == "lngknp":
            out = E.lngknp_backward(state.model, state, *c.lngknp_args(), **kw)
        else:
            out = E.seq2seq_backward(state.model, state, *c.s2s_args(), **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy().copy(), state.grads.clone()

    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        losses, first = run(state, global_step=STEP)
        tag = f"dropout {step} {precision}"
        _check_losses(tag, losses, pairs)
        _check_grads(tag, state, og, gn)
        assert torch.equal(first, run(state, global_step=STEP)[1])       # the masks are a function of (seed, step)


# ---- 4. a ReLU model is what it was ------------------------------------------------------------------------------------------
def test_relu_model_through_the_ext_entry_is_the_plain_entry_bit_for_bit(E):
    """rpr_load_model_ext(ext = {RPR_FF_RELU}) (what the Python side now calls), ext = NULL and rpr_load_model: the same search
    outputs, the same gradients, the same workspace."""
    from ripor_amd.utils import synth
    L, V, B, Q = 8, 256, 4, 6
    ctx = E.Context.get(0)
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=96)
    sd = synth.make_state_dict(dims, seed=21)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=21, max_len=14)
    codes = synth.make_codes(1000, L, V, seed=21)
    trie = E.DeviceTrie.from_codes(ctx, codes, V)
    c = _case()
    tsd = synth.make_state_dict(c.dims, seed=92)

    def reload(model, how):
        """the same weights behind another handle"""
        h = C.c_void_p()
        if how == "plain":
            E.check(ctx.lib.rpr_load_model(ctx.handle, C.byref(model._desc), C.byref(h)), "rpr_load_model")
        else:
            E.check(ctx.lib.rpr_load_model_ext(ctx.handle, C.byref(model._desc), None, C.byref(h)), "rpr_load_model_ext")
        ctx.lib.rpr_free_model(model.handle)
        model.handle = h
        return model

    results = {}
    for how in ("ext_relu", "ext_null", "plain"):
        model = E.DeviceModel(ctx, sd, dims)
        assert not model.gated_ff
        tmodel = E.DeviceModel(ctx, tsd, c.dims)
        if how != "ext_relu":
            model, tmodel = reload(model, how), reload(tmodel, how)
        res = E.search(model, trie, torch.from_numpy(ids), torch.from_numpy(mask), B, L)
        torch.cuda.synchronize()
        ws = ctx.workspace_bytes()
        state = E.TrainState(tmodel)
        losses = E.lngknp_backward(tmodel, state, *c.lngknp_args())
        torch.cuda.synchronize()
        results[how] = (res.tokens.clone(), res.scores.clone(), res.row_lo.clone(), res.row_hi.clone(), losses.clone(), state.grads.clone(), ws)
    for how in ("ext_null", "plain"):
        for a, b in zip(results["ext_relu"][:6], results[how][:6]):
            assert torch.equal(a, b), how
        assert results[how][6] == results["ext_relu"][6], "a ReLU model asked for another workspace"
    # and the entry refuses what it does not know
    h = C.c_void_p()
    model = E.DeviceModel(ctx, sd, dims)
    for ext in (E._lib.ModelExt(size=8, ff_kind=2), E._lib.ModelExt(size=4, ff_kind=0)):
        assert ctx.lib.rpr_load_model_ext(ctx.handle, C.byref(model._desc), C.byref(ext), C.byref(h)) == -1 and not h.value
