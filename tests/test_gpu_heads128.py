"""-m gpu: 128-dim heads (t5-3b: 32 heads of 128) through every teacher-forced entry point — rpr_lngknp_forward, rpr_embed,
rpr_lngknp_backward, rpr_seq2seq_forward / _backward, both steps with dropout, the refusal beyond the LDS carve and a search
after a step.

The yardstick is torch autograd through the CPU oracle, which views [B, T, H, d_kv] and is pinned to the reference at
d_kv = 64 for training (f4_*, s2s_*, drop_*) and at d_kv = 128 for the forward (g7_3b): oracle.train_ref.train_step,
tests/test_seq2seq_host.seq2seq_grads, tests/dropout_ref.DropoutRef. One oracle thread = one summation order; every reference is
computed once and shared by the precisions.

Models. A: d_model 256, 3 heads of 128 (inner 384 != d_model, odd head count), d_ff 128, 1 + 2 layers, 2.6 M parameters.
B: one t5-3b-shaped layer pair, d_model 1024, 32 heads of 128 (inner 4096 = 4 d_model: the wide GEMM routes), d_ff 512, 54 M.

Shapes, the smallest at which the 128-dim attention kernels can go wrong:
  a  A, bz 3, queries of 5..13 tokens (Lq 13, odd), L 8   Ls <= 32, where 64-dim heads take the MFMA tile
  b  A, bz 2, queries of 39 and 64 tokens (Lq 64), L 32   the reference's fine-tune shape: 129-float LDS rows would overflow
                                                           the 160 KB of a CU in both backward kernels
  c  A, bz 2, queries of 77 and 91 tokens (Lq 91), L 8    the last admitted length
  d  B, bz 2, queries of 8 and 13 tokens, L 8             32 heads, inner 4096

Bars: the project's own for these passes (test_gpu_train.py, test_gpu_seq2seq.py, test_gpu_dropout.py, test_gpu_rq_search.py),
unchanged: losses 1e-4 max(1, |ref|), position scores and label log-probabilities 1e-3, every gradient tensor within 2e-4 of
its largest entry, the global norm 1e-3, embedding logits STEP_LOGIT_TOL.

Condition on the inputs: a ReLU gate on the other side of 0 changes one whole row of a wi gradient and would look like a kernel
bug, so torch.relu is wrapped while the oracle runs and the smallest |feed-forward pre-activation| must be >= 2e-5, ten times
the ~2e-6 the f16x2 product can move a sum of this size. Seed 92 meets it on the CPU: a 5.2e-5, b 5.7e-5, c 5.9e-5, d 8.0e-5,
the seq2seq passes 5.2e-5 and 8.7e-5, with the masks of rate 0.1 at least 5.2e-5 (seed 96 does not: 2.5e-6). The query lengths
of b and c were chosen among those the shape allows so that this holds in every oracle pass, the dropped-out ones included."""
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
STEP_LOGIT_TOL = 5e-4   # test_gpu_rq_search.py
MIN_PREACT = 2e-5
RATE, SEED, STEP = 0.1, 0x1234_5678_9ABC_DEF1, 7   # test_gpu_dropout.py

MODEL_A = dict(V=64, enc_layers=1, d_ff=128, d_model=256, d_kv=128, num_heads=3, num_decoder_layers=2)
MODEL_B = dict(V=64, enc_layers=1, d_ff=512, d_model=1024, d_kv=128, num_heads=32, num_decoder_layers=1)
SHORT = dict(mean_len=9, std_len=3, min_len=5, max_len=13)
CASES = {"a": (MODEL_A, 3, 8, SHORT),
         "b": (MODEL_A, 2, 32, dict(mean_len=48.5, std_len=30, min_len=33, max_len=64)),
         "c": (MODEL_A, 2, 8, dict(mean_len=80, std_len=10, min_len=70, max_len=91)),
         "d": (MODEL_B, 2, 8, SHORT)}
LQ = {"a": 13, "b": 64, "c": 91, "d": 13}
PRECISIONS = ["f32", "f16x2"]


class Case:
    def __init__(self, name):
        from oracle import train_ref
        from ripor_amd.utils import synth
        kw, self.bz, self.L, q = CASES[name]
        self.name = name
        self.dims = synth.mini_dims(L=self.L, **kw)
        self.sd = synth.make_state_dict(self.dims, seed=92)
        self.ids, self.mask = synth.make_queries(self.bz, vocab_size=self.dims.vocab_size, seed=17, **q)
        assert self.ids.shape[1] == LQ[name] and len(set(self.mask.sum(1).tolist())) > 1     # ragged, padded to the longest
        codes = synth.make_codes(2 * self.bz, self.L, 64, seed=23).astype(np.int64)
        self.pos, self.neg = codes[:self.bz], codes[self.bz:]
        self.prefix = train_ref.PREFIX_LENS[self.L]
        self.keys = [("" if k == self.L else train_ref.TEACHER_KEYS[k]) for k in self.prefix]
        self.loss_names = train_ref.LOSS_NAMES[self.L]
        self.teacher = {}
        for k, key in zip(self.prefix, self.keys):
            self.teacher[key + "teacher_pos_scores"] = synth.uniform_f32(f"heads128/{name}/p{k}", (self.bz,), 30.0)
            self.teacher[key + "teacher_neg_scores"] = synth.uniform_f32(f"heads128/{name}/n{k}", (self.bz,), 30.0)

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
    print(f"[heads128] oracle {tag}: smallest |feed-forward pre-activation| {small[0]:.2e}")
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
        print(f"[heads128] {tag}: loss {name} {float(g):.6f} vs {ref:.6f}")
        assert abs(float(g) - ref) <= REL_LOSS_TOL * max(1.0, abs(ref)), (tag, name, float(g), ref)


def _check_grads(tag, state, og, gn):
    """Every tensor, whole, within GRAD_TOL of its largest entry; the global norm within NORM_TOL."""
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
            print(f"[heads128] {tag}: {k}: {int((err.max(axis=1) > GRAD_TOL).sum())} of {v.shape[0]} rows beyond {GRAD_TOL}")
    hn = float(np.sqrt(sum((v ** 2).sum() for v in grads.values())))
    print(f"[heads128] {tag}: worst tensor error {worst[0]:.2e} of its largest entry ({worst[1]}), norm {hn:.6g} vs {gn:.6g}")
    assert worst[0] <= GRAD_TOL, (tag, worst)
    assert abs(hn - gn) <= NORM_TOL * gn, (tag, hn, gn)


# ---- 1. / 2. the ranking step -----------------------------------------------------------------------------------------------
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
        print(f"[heads128] forward {name} {precision}: max position-score error {err:.2e}")
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


# ---- 3. the seq2seq step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["a", "b"])
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
        print(f"[heads128] {tag}: max label log-probability error {err:.2e}")
        assert err <= LP_TOL
        state = E.TrainState(model)
        loss = E.seq2seq_backward(model, state, *c.s2s_args())
        torch.cuda.synchronize()
        _check_losses(tag, loss.cpu().numpy(), [("rank", ref_loss)])
        _check_grads(tag, state, og, gn)
        first = state.grads.clone()
        E.seq2seq_backward(model, state, *c.s2s_args())
        assert torch.equal(first, state.grads)


# ---- 4. dense embeddings -----------------------------------------------------------------------------------------------------
def _mirror(cls, c):
    """The modeling mirror of a checkpoint class around the case's weights. T5ForDocIDGeneration's constructor admits only the
    reference's (decoder layers, heads) pairs, (24, 32) for t5-3b; the test models are smaller, so the object is put together by
    hand."""
    from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig, T5ForDocIDGeneration
    m = cls.__new__(cls)
    m.config = T5forDocIDConfig.from_dims(c.dims)
    bm = T5ForDocIDGeneration.__new__(T5ForDocIDGeneration)
    bm.config, bm._sd, bm._device, bm._engine_model = m.config, {}, torch.device("cpu"), None
    bm.load_state_dict(c.sd)
    m.base_model = bm.to(0)
    m.model_args, m.multi_vocab_sizes = None, False
    return m


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_embed_matches_the_oracle_the_forward_and_query_encode(name, precision):
    from oracle import t5_ref
    from ripor_amd import engine as E
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder
    c = _case(name)
    oracle = t5_ref.T5Ref(c.sd, c.dims)
    ids, mask = torch.from_numpy(c.ids), torch.from_numpy(c.mask)
    with torch.no_grad():
        want = oracle.last_logits(torch.full((c.bz, 1), -1, dtype=torch.long), oracle.encode(ids.long(), mask.long()), mask.long()).numpy()
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        emb = E.embed(model, ids, mask)
        assert emb.shape == (c.bz, c.dims.d_model) and emb.dtype == torch.float32
        e0 = oracle.out_embed(0).double()
        got = emb.cpu().double().numpy() @ e0.numpy().T
        print(f"[heads128] embed {name} {precision}: max |logit - oracle| {np.abs(got - want).max():.2e}")
        np.testing.assert_allclose(got, want, atol=STEP_LOGIT_TOL, rtol=0)
        dc = c.lngknp_args()[2]
        _, ps = E.lngknp_forward(model, ids, mask, dc)
        at0 = torch.einsum("bd,bnd->bn", emb.cpu().double(), e0[dc[:, :, 0].long()]).numpy()
        np.testing.assert_allclose(at0, ps[:, :, 0].cpu().numpy(), atol=POS_SCORE_TOL, rtol=0)
        rep = _mirror(T5SeqAQEncoder, c).query_encode(input_ids=ids, attention_mask=mask, decoder_input_ids=torch.full((c.bz, 1), -1))
        assert torch.equal(rep, emb)


# ---- 5. dropout --------------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("name", ["a", "b"])
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


# ---- 6. beyond the carve ----------------------------------------------------------------------------------------------------
def test_a_length_beyond_the_lds_carve_is_refused_before_anything_runs():
    """Lq = 92: self_attn_bwd_smem(92) is past the 160 KB of a CU (tests/test_attn_route.py: 91 -> 163 692 bytes). The call
    returns RPR_ERR_INVALID with the limit in its message, writes nothing, and the context goes on working."""
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    from ripor_amd.utils import synth
    c = _case("a")
    ids, mask = synth.make_queries(c.bz, vocab_size=c.dims.vocab_size, seed=17, fixed_len=92)
    with _Prec("f32") as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model)
        state.grads.fill_(7.0)
        args = c.lngknp_args()
        with pytest.raises(RiporHipError, match=r"status -1\).*160 KB"):
            E.lngknp_backward(model, state, torch.from_numpy(ids), torch.from_numpy(mask), *args[2:])
        torch.cuda.synchronize()
        assert bool((state.grads == 7.0).all()), "a refused call must not touch the gradient buffer"
        ref_losses, _, og, gn = _lngknp_ref("a")
        losses = E.lngknp_backward(model, state, *args)
        torch.cuda.synchronize()
        _check_losses("after the refusal", losses.cpu().numpy(), [(k, ref_losses[k]) for k in c.loss_names])
        _check_grads("after the refusal", state, og, gn)


# ---- 7. the model classes and the search after a step ------------------------------------------------------------------------
def test_model_classes_run_a_128_head_checkpoint():
    """T5SeqAQEncoderForLngKnpMarginMSE / ForSeq2Seq: forward and training_step on model A return the oracle's losses."""
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE, T5SeqAQEncoderForSeq2Seq
    c = _case("a")
    t = torch.from_numpy
    start = np.full((c.bz, 1), -1, dtype=np.int64)

    def tq(codes):
        return {"input_ids": t(c.ids), "attention_mask": t(c.mask), "decoder_input_ids": t(np.concatenate([start, codes[:, :-1]], axis=1))}

    with _Prec("f32"):
        m = _mirror(T5SeqAQEncoderForLngKnpMarginMSE, c)
        inputs = {"pos_tokenized_query": tq(c.pos), "neg_tokenized_query": tq(c.neg), "pos_doc_encoding": t(c.pos), "neg_doc_encoding": t(c.neg)}
        inputs.update({k: t(v) for k, v in c.teacher.items()})
        ref = _lngknp_ref("a")[0]
        for out in (m(**inputs), m.training_step(lr=1e-4, **inputs)):
            _check_losses("model class", [out[k] for k in c.loss_names], [(k, ref[k]) for k in c.loss_names])
        s = _mirror(T5SeqAQEncoderForSeq2Seq, c)
        s_in = {"tokenized_query": tq(c.pos), "labels": t(c.pos)}
        for out in (s(**s_in), s.training_step(lr=1e-4, **s_in)):
            _check_losses("seq2seq model class", [out["rank"]], [("rank", _s2s_ref("a")[0])])


def test_search_after_a_training_step_sees_the_new_weights():
    """As test_gpu_train.py's at 64: after one optimisation step a search returns the bits of a search on a fresh model loaded
    with the updated weights, and not those of before."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    c = _case("a")
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
