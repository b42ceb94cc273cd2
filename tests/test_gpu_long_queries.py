"""-m gpu: queries of 92 .. 256 tokens (64-dim heads) through the six teacher-forced entry points — rpr_lngknp_forward /
_backward, rpr_seq2seq_forward / _backward, both steps with dropout — where the attention backward and the dropped-out attention
forward leave the kernels that hold a whole head in LDS for the 32-row tiles of attn_mfma.hip (attn_bwd_tiled_kernel,
attn_drop_fwd_tiled_kernel; routes: attn_route.h plan_*_tiled, tests/test_attn_route_long.py).

The yardstick, the helpers and the bars are those of tests/test_gpu_heads128.py: torch autograd through the CPU oracle
(oracle.train_ref.train_step, tests/test_seq2seq_host.seq2seq_grads, tests/dropout_ref.DropoutRef at rate 0.1), one oracle
thread, every reference computed once and shared by the precisions; losses 1e-4 max(1, |ref|), position scores and label
log-probabilities 1e-3, every gradient tensor within 2e-4 of its largest entry, the global norm 1e-3.

Models. A64: d_model 256, 3 heads of 64, d_ff 128, 1 + 2 layers. B64: d_model 768, 12 heads of 64, 1 + 1 layers.

Cases (synth.make_queries arguments mean/std/min/max, seed):
  e  A64, bz 2, L 8    85/10/70/92, seed 2      92 and 80 tokens: the first length the resident route refuses; three tiles, the
                                                last of 28 rows; cross-attention still on the resident kernel
  f  A64, bz 2, L 32   115/20/97/129, seed 67   129 and 97: four tiles and one row. The ranking step's cross carve overflows
                                                (2 64 65 + 2 129 65 + 2 64 130 + 129 = 41 859 floats > 40 960): tiled cross; the
                                                seq2seq step's (32 rows) fits: mixed routes
  g  A64, bz 2, L 8    220/40/161/256, seed 52  256 and 196: the maximum; two whole key tiles of the second sequence are masked.
                                                Ranking step: tiled cross (2 16 65 + 2 256 65 + 2 16 257 + 256 = 43 840 floats),
                                                seq2seq (8 rows): the resident kernel
  h  B64, bz 3, L 8    130/30/93/160, seed 13   160, 143, 93: 12 heads, odd batch, exactly five tiles

Condition on the inputs (test_gpu_heads128.py): torch.relu is wrapped while the oracle runs and the smallest |feed-forward
pre-activation| must be >= 2e-5. On the CPU these seeds meet it in all four oracle passes: e 5.2e-5, f 2.6e-5, g 4.4e-5,
h 3.2e-5."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from dropout_ref import DropoutRef

pytestmark = pytest.mark.gpu

REL_LOSS_TOL = 1e-4     # test_gpu_train.py
POS_SCORE_TOL = 1e-3    # test_gpu_train.py
LP_TOL = 1e-3           # test_gpu_seq2seq.py
GRAD_TOL = 2e-4         # test_gpu_train.py::test_lngknp_backward_variants_match_oracle_autograd
NORM_TOL = 1e-3
MIN_PREACT = 2e-5
RATE, SEED, STEP = 0.1, 0x1234_5678_9ABC_DEF1, 7   # test_gpu_dropout.py
ENC_REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"

MODEL_A = dict(V=64, enc_layers=1, d_ff=128, d_model=256, d_kv=64, num_heads=3, num_decoder_layers=2)
MODEL_B = dict(V=64, enc_layers=1, d_ff=128, d_model=768, d_kv=64, num_heads=12, num_decoder_layers=1)
CASES = {"e": (MODEL_A, 2, 8, dict(mean_len=85, std_len=10, min_len=70, max_len=92), 2, [92, 80]),
         "f": (MODEL_A, 2, 32, dict(mean_len=115, std_len=20, min_len=97, max_len=129), 67, [129, 97]),
         "g": (MODEL_A, 2, 8, dict(mean_len=220, std_len=40, min_len=161, max_len=256), 52, [256, 196]),
         "h": (MODEL_B, 3, 8, dict(mean_len=130, std_len=30, min_len=93, max_len=160), 13, [160, 143, 93])}
PRECISIONS = ["f32", "f16x2"]


class Case:
    def __init__(self, name):
        from oracle import train_ref
        from ripor_amd.utils import synth
        kw, self.bz, self.L, q, qseed, lens = CASES[name]
        self.name = name
        self.dims = synth.mini_dims(L=self.L, **kw)
        self.sd = synth.make_state_dict(self.dims, seed=92)
        self.ids, self.mask = synth.make_queries(self.bz, vocab_size=self.dims.vocab_size, seed=qseed, **q)
        assert sorted(self.mask.sum(1).tolist(), reverse=True) == lens and self.ids.shape[1] == lens[0], self.mask.sum(1)
        codes = synth.make_codes(2 * self.bz, self.L, 64, seed=23).astype(np.int64)
        self.pos, self.neg = codes[:self.bz], codes[self.bz:]
        self.prefix = train_ref.PREFIX_LENS[self.L]
        self.keys = [("" if k == self.L else train_ref.TEACHER_KEYS[k]) for k in self.prefix]
        self.loss_names = train_ref.LOSS_NAMES[self.L]
        self.teacher = {}
        for k, key in zip(self.prefix, self.keys):
            self.teacher[key + "teacher_pos_scores"] = synth.uniform_f32(f"long_queries/{name}/p{k}", (self.bz,), 30.0)
            self.teacher[key + "teacher_neg_scores"] = synth.uniform_f32(f"long_queries/{name}/n{k}", (self.bz,), 30.0)

    def lngknp_args(self):
        t = torch.from_numpy
        tp = t(np.stack([self.teacher[key + "teacher_pos_scores"] for key in self.keys]))
        tn = t(np.stack([self.teacher[key + "teacher_neg_scores"] for key in self.keys]))
        return t(self.ids), t(self.mask), t(np.stack([self.pos, self.neg], axis=1)), tp, tn, self.prefix

    def s2s_args(self):
        return torch.from_numpy(self.ids), torch.from_numpy(self.mask), torch.from_numpy(self.pos)


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@contextlib.contextmanager
def _oracle_run(tag):
    """One oracle thread, torch.relu watched: no feed-forward pre-activation within MIN_PREACT of the gate."""
    real, prev, small = torch.relu, torch.get_num_threads(), [np.inf]

    def relu(x):
        small[0] = min(small[0], float(x.detach().abs().min()))
        return real(x)

    torch.set_num_threads(1)
    torch.relu = relu
    try:
        yield
    finally:
        torch.relu = real
        torch.set_num_threads(prev)
    print(f"[long_queries] oracle {tag}: smallest |feed-forward pre-activation| {small[0]:.2e}")
    assert MIN_PREACT <= small[0] < np.inf, (tag, small[0])


def _oracle(c, rate):
    from oracle import t5_ref
    return t5_ref.T5Ref(c.sd, c.dims) if rate is None else DropoutRef(c.sd, c.dims, rate, SEED, STEP)


@functools.lru_cache(maxsize=None)
def _lngknp_ref(name, rate=None):
    """(losses by name, position scores [bz, 2, L], grads, global norm); rate None: the plain oracle, else DropoutRef's masks."""
    from oracle import train_ref
    c = _case(name)
    with _oracle_run(f"lngknp {name} rate {rate}"):
        model = _oracle(c, rate)
        if rate is not None:
            model.begin(2)
        out, _, grads, gn = train_ref.train_step(model, c.ids, c.mask, c.pos, c.neg, c.teacher)
    ps = np.stack([out["pos_position_scores"].numpy(), out["neg_position_scores"].numpy()], axis=1)
    return {k: float(out[k]) for k in c.loss_names}, ps, grads, gn


@functools.lru_cache(maxsize=None)
def _s2s_ref(name, rate=None):
    """(loss, label log-probabilities [bz, L], grads, global norm)."""
    from test_seq2seq_host import seq2seq_ce, seq2seq_grads
    c = _case(name)
    with _oracle_run(f"seq2seq {name} rate {rate}"):
        model = _oracle(c, rate)
        loss, grads, gn = seq2seq_grads(model, c.ids, c.mask, c.pos)
        lp = None
        if rate is None:
            with torch.no_grad():
                lp = seq2seq_ce(model, c.ids, c.mask, c.pos)[1].numpy()
    return loss, lp, grads, gn


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


def _check_losses(tag, got, ref_pairs):
    for g, (name, ref) in zip(got, ref_pairs):
        print(f"[long_queries] {tag}: loss {name} {float(g):.6f} vs {ref:.6f}")
        assert abs(float(g) - ref) <= REL_LOSS_TOL * max(1.0, abs(ref)), (tag, name, float(g), ref)


def _check_grads(tag, state, og, gn):
    """Every tensor, whole, within GRAD_TOL of its largest entry — the encoder's relative-attention-bias table, the tensor most
    exposed to a wrong diagonal, by name as well; the global norm within NORM_TOL."""
    grads = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
    worst = (0.0, None)
    for k, v in grads.items():
        if k not in og:                      # a table autograd never reached (seq2seq: the last position's input codebook)
            assert not np.any(v), k
            continue
        o = og[k].double().numpy().reshape(v.shape)
        err = np.abs(v - o) / max(np.abs(o).max(), 1e-30)
        worst = max(worst, (float(err.max()), k))
        if err.max() > GRAD_TOL and v.ndim == 2:
            print(f"[long_queries] {tag}: {k}: {int((err.max(axis=1) > GRAD_TOL).sum())} of {v.shape[0]} rows beyond {GRAD_TOL}")
    rel, rel_ref = grads[ENC_REL], og[ENC_REL].double().numpy().reshape(grads[ENC_REL].shape)
    rel_err = float(np.abs(rel - rel_ref).max() / np.abs(rel_ref).max())
    hn = float(np.sqrt(sum((v ** 2).sum() for v in grads.values())))
    print(f"[long_queries] {tag}: worst tensor error {worst[0]:.2e} of its largest entry ({worst[1]}), encoder bias table "
          f"{rel_err:.2e} (largest entry {np.abs(rel_ref).max():.3g}), norm {hn:.6g} vs {gn:.6g}")
    assert np.abs(rel_ref).max() > 0 and rel_err <= GRAD_TOL, (tag, "encoder relative-attention bias", rel_err)
    assert worst[0] <= GRAD_TOL, (tag, worst)
    assert abs(hn - gn) <= NORM_TOL * gn, (tag, hn, gn)


# ---- the ranking step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_lngknp_forward_matches_the_oracle(name, precision):
    from ripor_amd import engine as E
    c = _case(name)
    ref_losses, ref_ps, _, _ = _lngknp_ref(name)
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        ctx.status(clear=True)
        losses, ps = E.lngknp_forward(model, *c.lngknp_args())
        torch.cuda.synchronize()
        assert ctx.status() == 0
        err = np.abs(ps.cpu().numpy() - ref_ps).max()
        print(f"[long_queries] forward {name} {precision}: max position-score error {err:.2e}")
        assert err <= POS_SCORE_TOL
        _check_losses(f"forward {name} {precision}", losses.cpu().numpy(), [(k, ref_losses[k]) for k in c.loss_names])
        again = E.lngknp_forward(model, *c.lngknp_args())
        assert torch.equal(losses, again[0]) and torch.equal(ps, again[1])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_lngknp_backward_matches_oracle_autograd(name, precision):
    from ripor_amd import engine as E
    c = _case(name)
    ref_losses, _, og, gn = _lngknp_ref(name)
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model)
        losses = E.lngknp_backward(model, state, *c.lngknp_args())
        torch.cuda.synchronize()
        tag = f"lngknp {name} {precision}"
        _check_losses(tag, losses.cpu().numpy(), [(k, ref_losses[k]) for k in c.loss_names])
        _check_grads(tag, state, og, gn)
        first = state.grads.clone()
        state.grads.zero_()
        E.lngknp_backward(model, state, *c.lngknp_args())
        assert torch.equal(first, state.grads), "two identical calls must give the same bits"


# ---- the seq2seq step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_seq2seq_forward_and_backward_match_oracle_autograd(name, precision):
    from ripor_amd import engine as E
    c = _case(name)
    ref_loss, ref_lp, og, gn = _s2s_ref(name)
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        tag = f"seq2seq {name} {precision}"
        loss, lp = E.seq2seq_forward(model, *c.s2s_args())
        torch.cuda.synchronize()
        _check_losses(tag + " forward", loss.cpu().numpy(), [("rank", ref_loss)])
        err = np.abs(lp.cpu().numpy() - ref_lp).max()
        print(f"[long_queries] {tag}: max label log-probability error {err:.2e}")
        assert err <= LP_TOL
        state = E.TrainState(model)
        loss = E.seq2seq_backward(model, state, *c.s2s_args())
        torch.cuda.synchronize()
        _check_losses(tag, loss.cpu().numpy(), [("rank", ref_loss)])
        _check_grads(tag, state, og, gn)
        first = state.grads.clone()
        E.seq2seq_backward(model, state, *c.s2s_args())
        assert torch.equal(first, state.grads), "two identical calls must give the same bits"


# ---- dropout -------------------------------------------------------------------------------------------------------------------
def _lngknp_step(c, state, **kw):
    from ripor_amd import engine as E
    losses = E.lngknp_backward(state.model, state, *c.lngknp_args(), **kw)
    torch.cuda.synchronize()
    return losses.cpu().numpy().copy(), state.grads.clone()


def _s2s_step(c, state, **kw):
    from ripor_amd import engine as E
    loss = E.seq2seq_backward(state.model, state, *c.s2s_args(), **kw)
    torch.cuda.synchronize()
    return loss.cpu().numpy().copy(), state.grads.clone()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("step", ["lngknp", "seq2seq"])
@pytest.mark.parametrize("name", list(CASES))
def test_steps_at_rate_01_match_autograd_with_the_same_masks(name, step, precision):
    from ripor_amd import engine as E
    c = _case(name)
    if step == "lngknp":
        ref_losses, _, og, gn = _lngknp_ref(name, RATE)
        plain = _lngknp_ref(name)[0]
        pairs, plain_pairs, fn = [(k, ref_losses[k]) for k in c.loss_names], [plain[k] for k in c.loss_names], _lngknp_step
    else:
        ref_loss, _, og, gn = _s2s_ref(name, RATE)
        pairs, plain_pairs, fn = [("rank", ref_loss)], [_s2s_ref(name)[0]], _s2s_step
    assert all(abs(r - p) > 1e-3 * abs(p) for (_, r), p in zip(pairs, plain_pairs)), "dropout must move the losses"
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        losses, first = fn(c, state, global_step=STEP)
        tag = f"dropout {step} {name} {precision}"
        _check_losses(tag, losses, pairs)
        _check_grads(tag, state, og, gn)
        assert torch.equal(first, fn(c, state, global_step=STEP)[1])       # the masks are a function of (seed, step)
        # rate 0 with a seed is bit for bit the step that was never told about dropout
        l0, g0 = fn(c, E.TrainState(model))
        l1, g1 = fn(c, E.TrainState(model, dropout_rate=0.0, dropout_seed=SEED), global_step=STEP)
        assert np.array_equal(l0, l1) and torch.equal(g0, g1)


# ---- beyond 256 tokens ---------------------------------------------------------------------------------------------------------
def test_257_tokens_are_refused_before_anything_runs():
    """Lq = 257 at d_kv 64: RPR_ERR_INVALID with the limit in its message, nothing written, and the context goes on working."""
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    from ripor_amd.utils import synth
    c = _case("e")
    ids, mask = synth.make_queries(c.bz, vocab_size=c.dims.vocab_size, seed=17, fixed_len=257)
    with _Prec("f32") as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model)
        state.grads.fill_(7.0)
        args = c.lngknp_args()
        with pytest.raises(RiporHipError, match=r"status -1\).*at most 256 tokens"):
            E.lngknp_backward(model, state, torch.from_numpy(ids), torch.from_numpy(mask), *args[2:])
        torch.cuda.synchronize()
        assert bool((state.grads == 7.0).all()), "a refused call must not touch the gradient buffer"
        ref_losses, _, og, gn = _lngknp_ref("e")
        losses = E.lngknp_backward(model, state, *args)
        torch.cuda.synchronize()
        _check_losses("after the refusal", losses.cpu().numpy(), [(k, ref_losses[k]) for k in c.loss_names])
        _check_grads("after the refusal", state, og, gn)


# ---- the search after a step ---------------------------------------------------------------------------------------------------
def test_search_after_a_training_step_at_129_tokens_sees_the_new_weights():
    """As test_gpu_seq2seq.py's / test_gpu_train.py's at short queries: after one optimisation step on the 129-token batch a
    search returns the bits of a search on a fresh model loaded with the updated weights, and not those of before."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    c = _case("f")
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, c.sd, c.dims)
    state = E.TrainState(model)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(2000, c.L, 64, seed=5), 64)
    ti, tm, dc, tp, tn, prefix = c.lngknp_args()
    before = E.search(model, trie, ti, tm, 4, c.L)
    E.train_step(model, state, ti.cuda(), tm.cuda(), dc.cuda(), tp, tn, prefix, lr=3e-3)     # a large step: results must move
    after = E.search(model, trie, ti, tm, 4, c.L)
    torch.cuda.synchronize()
    fresh_model = E.DeviceModel(ctx, {k: v.cpu().numpy() for k, v in model.export_state_dict().items()}, c.dims)
    fresh = E.search(fresh_model, trie, ti, tm, 4, c.L)
    torch.cuda.synchronize()
    assert torch.equal(after.tokens, fresh.tokens) and torch.equal(after.scores, fresh.scores)
    assert not torch.equal(after.scores, before.scores), "the step did not change the scores: the test checks nothing"
