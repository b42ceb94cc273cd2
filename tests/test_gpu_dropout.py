"""-m gpu: dropout in the two device training steps (rpr_set_train_dropout, DESIGN.md "Dropout in the training step").

The device mask against its numpy restatement bit for bit (rpr_op_dropout), rate 0 inert in every precision, rate 0.1 against
torch autograd through the CPU oracle with the SAME masks multiplied in (tests/dropout_ref.py) at the bounds the dropout-free
step is held to (test_gpu_train.py::test_lngknp_backward_variants_match_oracle_autograd: losses 1e-4 max(1, |ref|), every
gradient tensor within 2e-4 of its largest entry, global norm 1e-3; bf16: test_bf16_training_mode_is_the_references_autocast_
arithmetic's 3 % / cosine 0.995), determinism in (seed, step), the loop with a resume in the middle, and the search after a step.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import dropout_mask as dm
from dropout_ref import DropoutRef

pytestmark = pytest.mark.gpu

RATE, SEED, STEP = 0.1, 0x1234_5678_9ABC_DEF1, 7


# ---- 1. the mask itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seq,n_pos,n_feat", [(1, 1, 1), (3, 7, 63), (2, 5, 257), (4, 3, 6), (2, 9, 64), (300, 17, 128)])
def test_op_dropout_is_the_numpy_mask_bit_for_bit(n_seq, n_pos, n_feat):
    """Same zeros, kept values x * fp32(1 / (1 - p)) to the bit; widths 1, 63, 257, one that is no multiple of 4 (6), the
    vector path (64, 128) and more than one block. Also in place, and another site / step / seed gives another mask."""
    from ripor_amd import engine as E
    from ripor_amd._lib import check
    ctx = E.Context.get(0)
    rng = np.random.default_rng(n_seq * 1000 + n_feat)
    x = rng.standard_normal((n_seq, n_pos, n_feat)).astype(np.float32)
    x[x == 0] = 1.0
    xd = torch.from_numpy(x).cuda()

    def run(rate, seed, step, site, src, dst):
        check(ctx.lib.rpr_op_dropout(ctx.handle, src.data_ptr(), dst.data_ptr(), n_seq, n_pos, n_feat, rate, seed, step, site, None),
              "rpr_op_dropout")
        torch.cuda.synchronize()
        return dst.cpu().numpy()

    site = dm.site_sub_out(1, 3, 2)
    got = run(RATE, SEED, STEP, site, xd, torch.empty_like(xd))
    def masked(m):      # a dropped element is +0 on the device, whatever its sign was
        return np.where(m == 0, np.float32(0), x * m).astype(np.float32)

    want = masked(dm.act_mask(RATE, SEED, STEP, site, np.arange(n_seq), n_pos, n_feat))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    inplace = xd.clone()
    assert np.array_equal(run(RATE, SEED, STEP, site, inplace, inplace).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(run(0.0, SEED, STEP, site, xd, torch.empty_like(xd)), x)       # rate 0: the identity
    if x.size >= 1000:
        for other in ((SEED, STEP, site + 1), (SEED, STEP + 1, site), (SEED + 1, STEP, site), (SEED, STEP + (1 << 32), site)):
            o = run(RATE, other[0], other[1], other[2], xd, torch.empty_like(xd))
            assert np.array_equal(o, masked(dm.act_mask(RATE, other[0], other[1], other[2], np.arange(n_seq), n_pos, n_feat)))
            assert not np.array_equal(o == 0, got == 0)


def test_setter_refuses_rates_outside_the_unit_interval():
    from ripor_amd import engine as E
    ctx = E.Context.get(0)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert ctx.lib.rpr_set_train_dropout(ctx.handle, bad, 1, 1) == -1   # RPR_ERR_INVALID
    assert ctx.lib.rpr_set_train_dropout(ctx.handle, 0.0, 0, 0) == 0


# ---- the cases: the inputs of the drop_* reference fixtures (tests/golden/make_golden_dropout.py; the CPU suite pins the
# autograd restatement to the reference on exactly these): bz 3, ragged queries (padding), L 8 and 16, shared codebooks --------
CASES = {"f4_l8": "drop_f4_bz3_l8", "f4_l16": "drop_f4_bz3_l16", "f4_l8_shared": "drop_f4_bz3_l8_shared", "s2s_l8": "drop_s2s_bz3_l8"}


class Case:
    def __init__(self, name):
        import json
        from conftest import GOLDEN_DIR
        from oracle import train_ref
        from ripor_amd.utils import synth
        z = np.load(os.path.join(GOLDEN_DIR, CASES[name] + ".npz"), allow_pickle=False)
        spec = json.loads(str(z["spec"]))
        assert (float(z["rate"]), int(z["mask_seed"]), int(z["mask_step"])) == (RATE, SEED, STEP)
        self.name, self.L, self.bz = name, spec["L"], spec["bz"]
        self.dims = synth.ModelDims(**spec["dims"])
        self.sd = synth.make_state_dict(self.dims, seed=spec["seed"])
        self.ids, self.mask = z["input_ids"], z["attention_mask"]
        assert len(set(self.mask.sum(1).tolist())) > 1, "the queries must have unequal lengths"
        if "labels" in z.files:                 # the seq2seq fixture: labels only
            self.pos = z["labels"]
            return
        self.pos, self.neg = z["pos_doc_encoding"], z["neg_doc_encoding"]
        self.prefix = train_ref.PREFIX_LENS[self.L]
        self.keys = [("" if k == self.L else train_ref.TEACHER_KEYS[k]) for k in self.prefix]
        self.teacher = {k: z[k] for k in z.files if k.endswith("_scores") and "teacher" in k}
        self.loss_names = train_ref.LOSS_NAMES[self.L]

    def device_args(self):
        t = torch.from_numpy
        tp = t(np.stack([self.teacher[key + "teacher_pos_scores"] for key in self.keys]))
        tn = t(np.stack([self.teacher[key + "teacher_neg_scores"] for key in self.keys]))
        return t(self.ids), t(self.mask), t(np.stack([self.pos, self.neg], axis=1)), tp, tn, self.prefix


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def _lngknp_ref(name, rate):
    """(losses by name, grads, global norm) by autograd through the oracle with the masks of (rate, SEED, STEP); one oracle
    thread = one summation order. Computed once per case, shared by the precisions."""
    from oracle import train_ref
    c = _case(name)
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = DropoutRef(c.sd, c.dims, rate, SEED, STEP)
        model.begin(2)
        losses, _, grads, gn = train_ref.train_step(model, c.ids, c.mask, c.pos, c.neg, c.teacher)
    finally:
        torch.set_num_threads(prev)
    return {k: float(losses[k]) for k in c.loss_names}, grads, gn


@functools.lru_cache(maxsize=None)
def _s2s_ref(name, rate):
    from test_seq2seq_host import seq2seq_grads
    c = _case(name)
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = DropoutRef(c.sd, c.dims, rate, SEED, STEP)
        model.begin(1)
        return seq2seq_grads(model, c.ids, c.mask, c.pos)
    finally:
        torch.set_num_threads(prev)


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


def _lngknp(c, state, **kw):
    from ripor_amd import engine as E
    losses = E.lngknp_backward(state.model, state, *c.device_args(), **kw)
    torch.cuda.synchronize()
    return losses.cpu().numpy().copy(), state.grads.clone()


def _s2s(c, state, **kw):
    from ripor_amd import engine as E
    loss = E.seq2seq_backward(state.model, state, torch.from_numpy(c.ids), torch.from_numpy(c.mask), torch.from_numpy(c.pos), **kw)
    torch.cuda.synchronize()
    return loss.cpu().numpy().copy(), state.grads.clone()


# ---- 2. rate 0 is inert --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
@pytest.mark.parametrize("step_fn", [_lngknp, _s2s], ids=["lngknp", "seq2seq"])
def test_rate_zero_with_a_seed_is_bit_for_bit_no_dropout(step_fn, precision):
    from ripor_amd import engine as E
    c = _case("f4_l8")
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        plain = E.TrainState(model)            # never told anything about dropout
        l0, g0 = step_fn(c, plain)
        seeded = E.TrainState(model, dropout_rate=0.0, dropout_seed=SEED)
        l1, g1 = step_fn(c, seeded, global_step=STEP)
        assert np.array_equal(l0, l1) and torch.equal(g0, g1)
        # and a state at rate 0 switches off what another state of the same context had set
        step_fn(c, E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED), global_step=STEP)
        l2, g2 = step_fn(c, plain)
        assert np.array_equal(l0, l2) and torch.equal(g0, g2)


# ---- 3. / 4. rate 0.1 against autograd with the same masks ---------------------------------------------------------------------
def _check_fp32_level(tag, losses, ref_losses, grads, og, gn):
    for got, (name, ref) in zip(losses, ref_losses):
        print(f"[dropout] {tag}: loss {name} {float(got):.6f} vs {ref:.6f}")
        assert abs(float(got) - ref) <= 1e-4 * max(1.0, abs(ref)), (tag, name, float(got), ref)
    worst = (0.0, None)
    for k, v in grads.items():
        if k not in og:                      # a table autograd never reached (seq2seq: the last position's input codebook)
            assert not np.any(v), k
            continue
        o = og[k].double().numpy().reshape(v.shape)
        err = np.abs(v - o) / max(np.abs(o).max(), 1e-30)
        worst = max(worst, (float(err.max()), k))
        if err.max() > 2e-4 and v.ndim == 2:     # the signature of a ReLU gate on the other side of 0 is ONE row of a wi gradient
            print(f"[dropout] {tag}: {k}: {int((err.max(axis=1) > 2e-4).sum())} of {v.shape[0]} rows beyond 2e-4")
    hn = float(np.sqrt(sum((v ** 2).sum() for v in grads.values())))
    print(f"[dropout] {tag}: worst tensor error {worst[0]:.2e} of its largest entry ({worst[1]}), norm {hn:.6g} vs {gn:.6g}")
    assert worst[0] <= 2e-4, (tag, worst)
    assert abs(hn - gn) <= 1e-3 * gn, (tag, hn, gn)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["f4_l8", "f4_l16", "f4_l8_shared"])
def test_lngknp_step_at_rate_01_matches_autograd_with_the_same_masks(name, precision):
    from ripor_amd import engine as E
    c = _case(name)
    ref_losses, og, gn = _lngknp_ref(name, RATE)
    ref0, _, _ = _lngknp_ref(name, 0.0)
    assert all(abs(ref_losses[k] - ref0[k]) > 1e-3 * abs(ref0[k]) for k in c.loss_names), "dropout must move the losses"
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        losses, _ = _lngknp(c, state, global_step=STEP)
        grads = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
        _check_fp32_level(f"lngknp {name} {precision}", losses, [(k, ref_losses[k]) for k in c.loss_names], grads, og, gn)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["s2s_l8", "f4_l8_shared"])
def test_seq2seq_step_at_rate_01_matches_autograd_with_the_same_masks(name, precision):
    from ripor_amd import engine as E
    c = _case(name)
    ref_loss, og, gn = _s2s_ref(name, RATE)
    assert abs(ref_loss - _s2s_ref(name, 0.0)[0]) > 1e-3 * ref_loss
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        loss, _ = _s2s(c, state, global_step=STEP)
        grads = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
        _check_fp32_level(f"seq2seq {name} {precision}", loss, [("rank", ref_loss)], grads, og, gn)


def _bf16_run(c, step, rate, ref):
    """(losses, global norm, {tensor: cosine with the fp32 autograd gradient}) of one bf16 step; tensors whose reference
    gradient is noise-level (below 1e-4 of the largest entry of any tensor) carry no direction and are left out."""
    from ripor_amd import engine as E
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, c.sd, c.dims)
    state = E.TrainState(model, dropout_rate=rate, dropout_seed=SEED)
    losses, _ = (_lngknp if step == "lngknp" else _s2s)(c, state, global_step=STEP)
    got = {k: v.detach().double().cpu() for k, v in state.named_grads().items()}
    hn = float(torch.sqrt(sum((v ** 2).sum() for v in got.values())))
    og = ref[1]
    gmax = max(float(v.abs().max()) for v in og.values())
    cos = {}
    for k, v in got.items():
        if k not in og or float(og[k].abs().max()) < 1e-4 * gmax:
            continue
        r = og[k].double().reshape(v.shape)
        cos[k] = float((v * r).sum() / (v.norm() * r.norm() + 1e-300))
    return [float(x) for x in losses], hn, cos


@pytest.mark.parametrize("step,name", [("lngknp", "f4_l8"), ("lngknp", "f4_l16"), ("lngknp", "f4_l8_shared"), ("seq2seq", "s2s_l8")])
def test_bf16_step_at_rate_01_is_autocast_arithmetic_on_the_same_masks(step, name):
    """bf16 GEMM operands against the fp32 autograd with the same masks, on the shapes of the drop_* fixtures and at the bounds
    of the dropout-free bf16 test (test_gpu_train.py::test_bf16_training_mode_is_the_references_autocast_arithmetic): losses
    and global norm within 3 %, every gradient tensor that is not noise-level within cosine 0.995."""
    c = _case(name)
    ref = _lngknp_ref(name, RATE) if step == "lngknp" else _s2s_ref(name, RATE)
    with _Prec("bf16"):
        losses, hn, cos = _bf16_run(c, step, RATE, ref)
    rl, _, gn = ref
    ref_losses = [rl[k] for k in c.loss_names] if step == "lngknp" else [rl]
    worst = min((v, k) for k, v in cos.items())
    print(f"[dropout] bf16 {step} {name}: losses {losses} vs {ref_losses}, norm {hn:.5g} vs {gn:.5g}, worst cosine {worst}")
    for got, r in zip(losses, ref_losses):
        assert abs(got - r) <= 3e-2 * max(1.0, abs(r)), (step, got, r)
    assert abs(hn - gn) <= 3e-2 * hn, (hn, gn)
    assert worst[0] >= 0.995, worst


# ---- 6. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x2", "bf16"])
def test_masks_are_a_function_of_seed_and_step_only(precision):
    from ripor_amd import engine as E
    c = _case("f4_l8")
    with _Prec(precision) as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        l0, g0 = _lngknp(c, state, global_step=STEP)
        l1, g1 = _lngknp(c, state, global_step=STEP)
        assert np.array_equal(l0, l1) and torch.equal(g0, g1)
        l2, g2 = _lngknp(c, state, global_step=STEP + 1)
        assert not torch.equal(g0, g2) and not np.array_equal(l0, l2)
        ex = E.GradExchange(state.grads, dry_run=True)        # the bucketed entry point
        state.grads.fill_(float("nan"))
        l3, _ = _lngknp(c, state, global_step=STEP, exchange=ex)
        ex.finish()
        torch.cuda.synchronize()
        assert np.array_equal(l0, l3) and torch.equal(g0, state.grads)
        s0, h0 = _s2s(c, state, global_step=STEP)
        ex = E.GradExchange(state.grads, dry_run=True)
        s1, _ = _s2s(c, state, global_step=STEP, exchange=ex)
        ex.finish()
        torch.cuda.synchronize()
        assert np.array_equal(s0, s1) and torch.equal(h0, state.grads)


def test_forward_entry_points_stay_in_evaluation_mode():
    """rpr_lngknp_forward and rpr_seq2seq_forward ignore the setter."""
    from ripor_amd import engine as E
    c = _case("f4_l8")
    with _Prec("f16x2") as ctx:
        model = E.DeviceModel(ctx, c.sd, c.dims)
        ids, mask, codes, tp, tn, prefix = c.device_args()
        a = [x.clone() for x in E.lngknp_forward(model, ids, mask, codes, tp, tn, prefix)]
        b = [x.clone() for x in E.seq2seq_forward(model, ids, mask, torch.from_numpy(c.pos))]
        ctx.lib.rpr_set_train_dropout(ctx.handle, 0.5, SEED, STEP)
        a2 = E.lngknp_forward(model, ids, mask, codes, tp, tn, prefix)
        b2 = E.seq2seq_forward(model, ids, mask, torch.from_numpy(c.pos))
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a + b, list(a2) + list(b2)))


# ---- 7. the loop, and a resume in the middle of it -----------------------------------------------------------------------------
def test_four_steps_equal_two_steps_checkpoint_resume_two_steps(tmp_path):
    """LngKnpTrainer at rate 0.1: the masks are a function of (seed, rank, global step), so a run resumed from checkpoint-2
    ends bit for bit where the uninterrupted run ends. No RNG state of the masks exists anywhere."""
    from test_trainer_plumbing import CASES as PLUMB, WordTokenizer, _write
    from ripor_amd.dataset.lng_knp import LngKnpMarginMSEforT5SeqAQCollator, LngKnpMarginMSEforT5SeqAQDataset
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE
    from ripor_amd.tasks import trainer as T
    from ripor_amd.utils import synth
    _write(tmp_path, PLUMB["L8_smtid"]["files"])
    dims = synth.mini_dims(L=8, V=256, enc_layers=1, d_ff=128)

    def run(out, resume=None, max_steps=4, model=None, rate=RATE):
        ds = LngKnpMarginMSEforT5SeqAQDataset(str(tmp_path / "examples.jsonl"), None, str(tmp_path / "queries"), None, True)
        coll = LngKnpMarginMSEforT5SeqAQCollator(WordTokenizer(), 16)
        if model is None:
            model = T5SeqAQEncoderForLngKnpMarginMSE.from_synthetic(dims, seed=9)
        model.to(0)
        args = T.LngKnpTrainingArgs(output_dir=str(tmp_path / out), learning_rate=1e-3, warmup_ratio=0.25, per_device_train_batch_size=3,
                                    max_steps=max_steps, logging_steps=1, save_steps=2, bf16=False, dropout_rate=rate)
        os.makedirs(args.output_dir, exist_ok=True)
        tr = T.LngKnpTrainer(model, ds, coll, args, log=lambda s: None)
        hist = tr.train(resume_from_checkpoint=resume)
        torch.cuda.synchronize()
        return {k: v.cpu().clone() for k, v in model.base_model.engine_model().export_state_dict().items()}, hist

    try:
        whole, hist = run("a")
        ck = os.path.join(str(tmp_path / "a"), "checkpoint-2")
        resumed_model = T5SeqAQEncoderForLngKnpMarginMSE.from_pretrained(ck)
        resumed, hist2 = run("b", resume=ck, model=resumed_model)
        assert [h["step"] for h in hist2][-2:] == [3, 4]
        assert [h["loss"] for h in hist[-2:]] == [h["loss"] for h in hist2[-2:]]
        for k in whole:
            assert torch.equal(whole[k], resumed[k]), k
        plain, _ = run("c", rate=0.0)
        assert any(not torch.equal(whole[k], plain[k]) for k in whole), "dropout changed nothing: the test checks nothing"
        assert "dropout" not in " ".join(os.listdir(ck)) and not any("drop" in k for k in torch.load(os.path.join(ck, "optimizer.pt")))
    finally:
        from ripor_amd import engine as E
        ctx = E.Context.get(0)
        ctx.lib.rpr_set_train_dropout(ctx.handle, 0.0, 0, 0)


# ---- 8. the search after a dropout step ----------------------------------------------------------------------------------
def test_search_after_a_dropout_step_sees_the_new_weights_and_no_dropout():
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    L, bz, V = 8, 4, 256
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=31)
    ctx = E.Context.get(0)
    try:
        model = E.DeviceModel(ctx, sd, dims)
        state = E.TrainState(model, dropout_rate=RATE, dropout_seed=SEED)
        trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(2000, L, V, seed=5), V)
        ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=9, max_len=12)
        ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
        before = E.search(model, trie, ti, tm, 4, L)
        doc = torch.from_numpy(synth.make_codes(2 * bz, L, V, seed=6).astype(np.int64).reshape(2, bz, L).transpose(1, 0, 2).copy())
        prefix = [L, 4]
        tp = torch.from_numpy(np.stack([synth.uniform_f32(f"sd/p{k}", (bz,), 30.0) for k in prefix]))
        tn = torch.from_numpy(np.stack([synth.uniform_f32(f"sd/n{k}", (bz,), 30.0) for k in prefix]))
        E.train_step(model, state, ti.cuda(), tm.cuda(), doc.cuda(), tp, tn, prefix, lr=3e-3)
        after = E.search(model, trie, ti, tm, 4, L)      # the dropout setting is still in force on the context
        torch.cuda.synchronize()
        fresh_model = E.DeviceModel(ctx, {k: v.cpu().numpy() for k, v in model.export_state_dict().items()}, dims)
        ctx.lib.rpr_set_train_dropout(ctx.handle, 0.0, 0, 0)
        fresh = E.search(fresh_model, trie, ti, tm, 4, L)
        torch.cuda.synchronize()
        assert torch.equal(after.tokens, fresh.tokens) and torch.equal(after.scores, fresh.scores)
        assert not torch.equal(after.scores, before.scores)
    finally:
        ctx.lib.rpr_set_train_dropout(ctx.handle, 0.0, 0, 0)
