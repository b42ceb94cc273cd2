"""-m gpu: what one training step leaves for the next. Both steps (prefix-ranking fine-tune, seq2seq docid) in all three
precisions: after rpr_adamw_step, and after the caller has written weights through the device tensors, the next backward
pass must be, bit for bit, the pass of a fresh model loaded with the weights as they now are. Both passes are deterministic
and read the same fp32 weights, so anything derived from the weights that lagged behind — the bf16 copies and transposed
copies of the weight cache (refresh_weight_cache), an f16 plane, a dynamic plane scale, the layer-0 table — shows as a
difference. The smallest training shape of the suite: mini dims with one encoder layer, d_ff 128, L 8, V 256, three ragged
queries of at most 13 tokens."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L, V, BZ = 8, 256, 3
PREFIX = [L, 4]


@functools.lru_cache(maxsize=None)
def _world():
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=57)
    ids, mask = synth.make_queries(BZ, vocab_size=dims.vocab_size, seed=17, mean_len=9, std_len=3, min_len=5, max_len=13)
    assert ids.shape[1] <= 13 and len(set(mask.sum(1).tolist())) > 1
    codes = synth.make_codes(2 * BZ, L, V, seed=23).astype(np.int64)
    tp = np.stack([synth.uniform_f32(f"state/p{k}", (BZ,), 30.0) for k in PREFIX])
    tn = np.stack([synth.uniform_f32(f"state/n{k}", (BZ,), 30.0) for k in PREFIX])
    return dims, sd, ids, mask, codes, tp, tn


def _backward(step, model, state):
    """One backward pass of `step` -> (losses, a copy of the flat gradient buffer)."""
    from ripor_amd import engine as E
    dims, sd, ids, mask, codes, tp, tn = _world()
    t = torch.from_numpy
    if step == "lngknp":
        doc = t(np.stack([codes[:BZ], codes[BZ:]], axis=1))
        losses = E.lngknp_backward(model, state, t(ids), t(mask), doc, t(tp), t(tn), PREFIX)
    else:
        losses = E.seq2seq_backward(model, state, t(ids), t(mask), t(codes[:BZ]))
    torch.cuda.synchronize()
    return losses.clone(), state.grads.clone()


def _fresh_copy(model):
    """A new DeviceModel + TrainState holding the weights `model` has on the device now."""
    from ripor_amd import engine as E
    fresh = E.DeviceModel(model.ctx, {k: v.cpu().numpy() for k, v in model.export_state_dict().items()}, model.cfg)
    return fresh, E.TrainState(fresh)


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
@pytest.mark.parametrize("step", ["lngknp", "seq2seq"])
def test_the_pass_after_an_optimizer_step_reads_the_new_weights(step, precision):
    """backward, adamw_step (lr 1e-2: every weight moves by about its own size, nothing hides in rounding), backward — against
    one backward of a fresh model built from the weights exported after the optimizer step."""
    from ripor_amd import engine as E
    dims, sd = _world()[:2]
    ctx = E.Context.get(0)
    ctx.set_precision(precision)
    try:
        a = E.DeviceModel(ctx, sd, dims)
        sa = E.TrainState(a)
        l1, g1 = _backward(step, a, sa)
        E.adamw_step(a, sa, 1e-2)
        l2, g2 = _backward(step, a, sa)
        b, sb = _fresh_copy(a)
        lb, gb = _backward(step, b, sb)
        assert torch.isfinite(g2).all() and torch.isfinite(l2).all()
        assert torch.equal(l2, lb), (step, precision, l2.tolist(), lb.tolist())
        assert torch.equal(g2, gb), (step, precision, float((g2 - gb).abs().max()))
        assert not torch.equal(g2, g1) and not torch.equal(l2, l1), "the optimizer step changed nothing: the test checks nothing"
    finally:
        ctx.set_precision("f16x2")


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
@pytest.mark.parametrize("step", ["lngknp", "seq2seq"])
def test_the_pass_after_the_caller_wrote_weights_reads_them(step, precision):
    """The weights are caller-owned: between two passes one encoder wi and one decoder cross-attention k tensor are doubled in
    place through the device tensors the engine exposes (the cross k/v of all layers are one packed tensor: a slice of it)."""
    from ripor_amd import engine as E
    dims, sd = _world()[:2]
    ctx = E.Context.get(0)
    ctx.set_precision(precision)
    try:
        a = E.DeviceModel(ctx, sd, dims)
        sa = E.TrainState(a)
        l1, g1 = _backward(step, a, sa)
        wanted = {"encoder.block.0.layer.1.DenseReluDense.wi.weight", "decoder.block.3.layer.1.EncDecAttention.k.weight"}
        hit = 0
        for name, t, sl in a.named_device_params():
            if name in wanted:
                (t if sl is None else t[sl]).mul_(2.0)
                hit += 1
        assert hit == 2
        torch.cuda.synchronize()
        l2, g2 = _backward(step, a, sa)
        b, sb = _fresh_copy(a)
        assert torch.equal(b.export_state_dict()["decoder.block.3.layer.1.EncDecAttention.k.weight"],
                           torch.from_numpy(sd["decoder.block.3.layer.1.EncDecAttention.k.weight"]).to(ctx.device) * 2.0)
        lb, gb = _backward(step, b, sb)
        assert torch.equal(l2, lb), (step, precision, l2.tolist(), lb.tolist())
        assert torch.equal(g2, gb), (step, precision, float((g2 - gb).abs().max()))
        assert not torch.equal(g2, g1) and not torch.equal(l2, l1), "doubling two tensors changed nothing: the test checks nothing"
    finally:
        ctx.set_precision("f16x2")


def test_search_after_two_bf16_training_steps_sees_the_new_weights():
    """test_search_after_a_training_step_sees_the_new_weights (tests/test_gpu_train.py) for two consecutive steps in bf16: the
    second rpr_adamw_step marks stale the planes and the layer-0 table the first search has just rebuilt. Every search must
    return the bits of a search on a fresh model loaded with the weights of that moment."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    dims, sd, ids, mask, codes, tp, tn = _world()
    ctx = E.Context.get(0)
    t = torch.from_numpy
    ti, tm = t(ids), t(mask)
    doc = t(np.stack([codes[:BZ], codes[BZ:]], axis=1))
    ctx.set_precision("bf16")
    try:
        model = E.DeviceModel(ctx, sd, dims)
        state = E.TrainState(model)
        trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(2000, L, V, seed=5), V)
        seen = [E.search(model, trie, ti, tm, 4, L).scores.clone()]
        for _ in range(2):
            E.train_step(model, state, ti, tm, doc, t(tp), t(tn), PREFIX, lr=3e-3)
            after = E.search(model, trie, ti, tm, 4, L)
            torch.cuda.synchronize()
            fresh_model = _fresh_copy(model)[0]
            fresh = E.search(fresh_model, trie, ti, tm, 4, L)
            torch.cuda.synchronize()
            assert torch.equal(after.tokens, fresh.tokens) and torch.equal(after.scores, fresh.scores)
            assert not torch.equal(after.scores, seen[-1]), "the step did not change the scores: the test checks nothing"
            seen.append(after.scores.clone())
        assert state.step == 2
    finally:
        ctx.set_precision("f16x2")
