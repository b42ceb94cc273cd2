"""-m gpu: the dense first-stage step (loss_type t5seq_pretrain_margin_mse) on the device — rpr_dense_mse_forward / _backward /
_backward_buckets against the reference's own T5SeqPretrainEncoder run in float64 (tests/golden/pre_*.npz,
make_golden_pretrain.py), determinism, bucket coverage, the optimizer step, refusals, dropout against autograd with the same
masks, and the command line end to end. Bars as the other two steps' (tests/test_gpu_train.py, test_gpu_seq2seq.py): losses 1e-4
relative, scores and representations 1e-3 absolute (the position scores' bar), gradients 1e-3 of each tensor's scale."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dense_ref import PRE_CASES, PreGolden, dense_grads, dense_margin_mse_stacked
from test_seq2seq_host import check_grads

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_LOSS_TOL = 1e-4
POS_SCORE_TOL = 1e-3          # tests/test_gpu_train.py: the bar of the ranking step's position scores
# bf16 GEMM operands (the reference's autocast): no bar existed for these scores. Measured on an MI355X over the three fixtures the
# bf16 kernels take (profiles/r26_dense_stage_summary.txt): worst |score - fixture| 0.4798 (pre_mini_bz3_q9_d24; scores of up to
# 640, so 8e-4 of the scale), worst relative loss error 2.0844e-3 (pre_mini_bz1_q5_d12). The bars are twice the worst measured
# value: the factor allows for another box's clocks and summation order.
BF16_SCORE_MEASURED, BF16_LOSS_MEASURED = 0.4798, 2.0844e-3
BF16_SCORE_TOL, BF16_LOSS_TOL = 2 * BF16_SCORE_MEASURED, 2 * BF16_LOSS_MEASURED


@functools.lru_cache(maxsize=None)
def _golden(name):
    return PreGolden(name)


def _model(g):
    from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig, T5ForDocIDGeneration, T5SeqPretrainEncoder
    m = T5SeqPretrainEncoder.__new__(T5SeqPretrainEncoder)
    m.config = T5forDocIDConfig.from_dims(g.dims)
    m.config.feed_forward_proj = g.kind
    m.base_model = T5ForDocIDGeneration(m.config, g.state_dict).to(0)
    m.model_args = None
    return m


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


def _embed_scores(m, g):
    """The dot products of engine.embed's outputs for the same texts (each group at its own padded length)."""
    reps = [m.query_encode(**{k: v for k, v in g.tok(grp).items() if k != "decoder_input_ids"}) for grp in ("q", "pd", "nd")]
    return torch.stack([(reps[0] * reps[1]).sum(-1), (reps[0] * reps[2]).sum(-1)], 1).cpu().numpy()


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", PRE_CASES)
def test_dense_forward_matches_reference(name, precision):
    g = _golden(name)
    m = _model(g)
    with _Prec(precision):
        out = m(**g.inputs())
        torch.cuda.synchronize()
        ref = float(g.z["loss"])
        scores, reps = m.last_scores.cpu().numpy(), m.last_reps.cpu().numpy()
        es = _embed_scores(m, g)
        print(f"[dense-fwd] {name} {precision}: loss {float(out['rank']):.6f} vs {ref:.6f} (rel {abs(float(out['rank']) - ref) / ref:.2e}); "
              f"scores max err {np.abs(scores - g.z['scores']).max():.2e} of {np.abs(g.z['scores']).max():.4g}; reps max err "
              f"{np.abs(reps - g.z['reps']).max():.2e}; scores vs embed dot products {np.abs(scores - es).max():.2e}")
        assert set(out) == {"rank"} and out["rank"].dtype == torch.float32
        assert abs(float(out["rank"]) - ref) <= REL_LOSS_TOL * abs(ref), (name, precision, float(out["rank"]), ref)
        assert scores.shape == (g.bz, 2) and reps.shape == (3 * g.bz, g.dims.d_model)
        np.testing.assert_allclose(scores, g.z["scores"], atol=POS_SCORE_TOL, rtol=0)
        np.testing.assert_allclose(reps, g.z["reps"], atol=POS_SCORE_TOL, rtol=0)
        np.testing.assert_allclose(scores, es, atol=POS_SCORE_TOL, rtol=0)
        out2 = m(**g.inputs())
        assert torch.equal(out["rank"], out2["rank"]) and torch.equal(m.last_scores.cpu(), torch.from_numpy(scores))


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", PRE_CASES)
def test_dense_backward_matches_reference_gradients(name, precision):
    """Every gradient tensor (norm and seeded samples) of the reference's loss.backward(), the 96-token documents (tiled attention
    backward) and the gated feed-forward included; the codebooks get exactly zero, the start embedding does not; two identical
    backward calls give the same bits, and so does the bucket variant, whose buckets cover the flat buffer exactly once."""
    from ripor_amd import engine as E
    g = _golden(name)
    m = _model(g)
    with _Prec(precision):
        loss = m.backward(**g.inputs())["rank"]
        torch.cuda.synchronize()
        assert abs(float(loss) - float(g.z["loss"])) <= REL_LOSS_TOL * abs(float(g.z["loss"]))
        st = m.train_state()
        grads = {k: v.detach().cpu().numpy() for k, v in st.named_grads().items()}
        worst = check_grads(g, grads, rel=1e-3, label=" (HIP)")
        gnorm = float(torch.sqrt((st.grads.double() ** 2).sum()))
        print(f"[dense-bwd] {name} {precision}: worst sampled error {worst[0]:.2e} ({worst[1]}), global norm {gnorm:.6g} vs "
              f"{float(g.z['grad_global_norm']):.6g}")
        assert abs(gnorm - float(g.z["grad_global_norm"])) <= 1e-3 * gnorm
        books = [k for k in grads if k.startswith("list_")]
        assert len(books) == 2 * len(g.dims.decoder_vocab_sizes) and not any(np.any(grads[k]) for k in books)
        assert np.abs(grads["start_token_embed"]).max() > 0
        first, first_loss = st.grads.clone(), loss.clone()
        again = m.backward(**g.inputs())["rank"]
        assert torch.equal(first, st.grads) and torch.equal(first_loss, again)
        ids, mask, tp, tn = m._batch(g.inputs())
        ex = E.GradExchange(st.grads, dry_run=True)
        E.dense_mse_backward(m.base_model.engine_model(), st, ids, mask, tp, tn, exchange=ex)
        ex.finish()
        torch.cuda.synchronize()
        assert torch.equal(first, st.grads)                 # the hand-over changes no gradient
        pos = 0
        for off, n in sorted(ex.history):
            assert off == pos
            pos += n
        assert pos == st.total


# the bf16 kernels reduce in tiles of 64 (test_gpu_gated_ff.py): the gated fixture's d_ff of 96 is outside them, in every step
BF16_CASES = [n for n in PRE_CASES if PreGolden(n).dims.d_ff % 64 == 0]


@pytest.mark.parametrize("name", BF16_CASES)
def test_dense_bf16_stays_within_twice_the_measured_error(name):
    g = _golden(name)
    m = _model(g)
    with _Prec("bf16"):
        out = m(**g.inputs())
        torch.cuda.synchronize()
        ref = float(g.z["loss"])
        err = float(np.abs(m.last_scores.cpu().numpy() - g.z["scores"]).max())
        rel = abs(float(out["rank"]) - ref) / abs(ref)
        print(f"[dense-bf16] {name}: max |score - fixture| {err:.4f} of {np.abs(g.z['scores']).max():.4g}, relative loss error {rel:.4e}")
        assert err <= BF16_SCORE_TOL and rel <= BF16_LOSS_TOL, (name, err, rel)
        out2 = m(**g.inputs())
        assert torch.equal(out["rank"], out2["rank"])


def test_dense_training_step_matches_reference_adamw_update():
    from test_oracle_golden import grad_sample_indices
    g = _golden("pre_mini_bz3_q9_d24")
    m = _model(g)
    em = m.base_model.engine_model()
    before = {k: v.clone() for k, v in em.export_state_dict().items()}
    lr = float(g.z["step_lr"])
    loss = m.training_step(lr=lr, **g.inputs())["rank"]
    torch.cuda.synchronize()
    assert abs(float(loss) - float(g.z["loss"])) <= REL_LOSS_TOL * abs(float(g.z["loss"]))
    after = em.export_state_dict()
    off = 0
    for n, c in zip([str(x) for x in g.z["grad_names"]], g.z["grad_sample_counts"]):
        ref = g.z["param_delta_samples"][off:off + c]
        off += c
        key = "shared.weight" if n == "encoder.embed_tokens.weight" else n
        d = (after[key] - before[key]).reshape(-1).cpu().numpy()[grad_sample_indices(n, tuple(before[key].shape))]
        err = np.abs(d - ref)     # same bound as the seq2seq step's test (noise-level gradients may flip an entry's update)
        assert (err <= 3e-2 * lr).mean() >= 0.9 and err.max() <= 2.0 * lr * 1.001, f"update of {n}: {err.max() / lr:.3f} lr"
    for k in before:                       # zero gradient, weight_decay 0: the codebooks leave AdamW bit-identical
        if k.startswith("list_"):
            assert torch.equal(before[k], after[k]), k
    out = m(**g.inputs())
    torch.cuda.synchronize()
    ref_after = float(g.z["loss_after_step"])
    print(f"[dense-step] loss {float(loss):.4f} -> {float(out['rank']):.4f} (reference {ref_after:.4f})")
    assert abs(float(out["rank"]) - ref_after) <= 5e-3 * abs(ref_after), (float(out["rank"]), ref_after)


def test_dense_refusals_enqueue_nothing():
    """128-dim heads beyond the carve, more than 256 tokens and an empty batch return the invalid-argument error before anything is
    enqueued (the flat gradient buffer keeps its bits); the Python surface refuses differing query tensors and decoder inputs of
    length 2. The device is fine afterwards."""
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    from ripor_amd.utils import synth
    ctx = E.Context.get(0)
    dims = synth.mini_dims(L=2, V=64, enc_layers=1, d_ff=128, d_model=256, d_kv=128, num_heads=3, num_decoder_layers=2)   # as test_gpu_heads128
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=11), dims)
    st = E.TrainState(model)
    tp, tn = torch.zeros(2), torch.zeros(2)

    def batch(Lt):
        return torch.randint(3, 60, (3, 2, Lt)), torch.ones((3, 2, Lt), dtype=torch.long)

    E.dense_mse_backward(model, st, *batch(91), tp, tn)            # 128-dim heads up to the carve run
    torch.cuda.synchronize()
    assert float(st.grads.abs().max()) > 0
    st.grads.fill_(7.0)
    with pytest.raises(RiporHipError, match="LDS"):
        E.dense_mse_backward(model, st, *batch(92), tp, tn)
    with pytest.raises(RiporHipError, match="LDS"):
        E.dense_mse_forward(model, *batch(92), tp, tn)
    ids, mask = batch(8)
    dev = dict(device=ctx.device, dtype=torch.int32)
    i257, m257 = torch.ones((3, 2, 257), **dev), torch.ones((3, 2, 257), **dev)
    t2 = torch.zeros(2, device=ctx.device)
    loss = torch.zeros(1, device=ctx.device)
    assert ctx.lib.rpr_dense_mse_backward(ctx.handle, model.handle, i257.data_ptr(), m257.data_ptr(), 2, 257, t2.data_ptr(), t2.data_ptr(),
                                          loss.data_ptr(), st.grads.data_ptr(), None) == -1
    assert b"256" in ctx.lib.rpr_last_error()
    assert ctx.lib.rpr_dense_mse_backward(ctx.handle, model.handle, i257.data_ptr(), m257.data_ptr(), 0, 8, t2.data_ptr(), t2.data_ptr(),
                                          loss.data_ptr(), st.grads.data_ptr(), None) == -1
    with pytest.raises(ValueError, match="at most 256"):
        E.dense_mse_backward(model, st, i257, m257, tp, tn)
    torch.cuda.synchronize()
    assert bool((st.grads == 7.0).all())                               # nothing was enqueued: not even the memset
    g = _golden("pre_mini_bz1_q5_d12")
    m = _model(g)
    bad = g.inputs()
    bad["tokenized_neg_query"]["input_ids"] = bad["tokenized_neg_query"]["input_ids"] + 1
    with pytest.raises(ValueError, match="same query tokens"):
        m(**bad)
    bad = g.inputs()
    bad["tokenized_pos_doc"]["decoder_input_ids"] = torch.tensor([[-1, 5]])
    with pytest.raises(ValueError, match="commit-loss"):
        m.backward(**bad)
    empty = g.inputs()
    empty["tokenized_neg_doc"]["attention_mask"] = torch.zeros_like(empty["tokenized_neg_doc"]["attention_mask"])
    with pytest.raises(ValueError, match="all-zero attention_mask"):
        m(**empty)
    out = m(**g.inputs())
    assert abs(float(out["rank"]) - float(g.z["loss"])) <= 1e-3 * abs(float(g.z["loss"]))


# ---- dropout -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dropout_ref(rate):
    """(loss, grads, global norm) by autograd through the float32 oracle with the masks of (rate, SEED, STEP) over ONE pass of the
    3 bz sequences, as the device step runs them; one oracle thread = one summation order. Shared by the precisions."""
    from dropout_ref import DropoutRef
    from test_gpu_dropout import SEED, STEP
    g = _golden("pre_mini_bz3_q9_d24")
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        model = DropoutRef(g.state_dict, g.dims, rate, SEED, STEP)
        model.begin(1)
        return dense_grads(model, dense_margin_mse_stacked, *g.stacked(), g.z["teacher_pos"], g.z["teacher_neg"])
    finally:
        torch.set_num_threads(prev)


def _step(m, g, state, **kw):
    from ripor_amd import engine as E
    ids, mask, tp, tn = m._batch(g.inputs())
    loss = E.dense_mse_backward(m.base_model.engine_model(), state, ids, mask, tp, tn, **kw)
    torch.cuda.synchronize()
    return loss.cpu().numpy().copy(), state.grads.clone()


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
def test_dense_rate_zero_with_a_seed_is_bit_for_bit_no_dropout(precision):
    from ripor_amd import engine as E
    from test_gpu_dropout import RATE, SEED, STEP
    g = _golden("pre_mini_bz3_q9_d24")
    m = _model(g)
    with _Prec(precision):
        em = m.base_model.engine_model()
        plain = E.TrainState(em)
        l0, g0 = _step(m, g, plain)
        l1, g1 = _step(m, g, E.TrainState(em, dropout_rate=0.0, dropout_seed=SEED), global_step=STEP)
        assert np.array_equal(l0, l1) and torch.equal(g0, g1)
        l2, g2 = _step(m, g, E.TrainState(em, dropout_rate=RATE, dropout_seed=SEED), global_step=STEP)
        assert not np.array_equal(l0, l2)
        fwd = m(**g.inputs())["rank"]                       # the forward entry point stays in evaluation mode
        torch.cuda.synchronize()
        assert float(fwd) == float(l0[0])
        l3, g3 = _step(m, g, plain)
        assert np.array_equal(l0, l3) and torch.equal(g0, g3)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_dense_step_at_rate_01_matches_autograd_with_the_same_masks(precision):
    from ripor_amd import engine as E
    from test_gpu_dropout import RATE, SEED, STEP, _check_fp32_level
    g = _golden("pre_mini_bz3_q9_d24")
    ref_loss, og, gn = _dropout_ref(RATE)
    assert abs(ref_loss - _dropout_ref(0.0)[0]) > 1e-3 * ref_loss, "dropout must move the loss"
    m = _model(g)
    with _Prec(precision):
        state = E.TrainState(m.base_model.engine_model(), dropout_rate=RATE, dropout_seed=SEED)
        loss, _ = _step(m, g, state, global_step=STEP)
        grads = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
        _check_fp32_level(f"dense {precision}", loss, [("rank", ref_loss)], grads, og, gn)


def test_main_dense_trains_end_to_end(tmp_path):
    """python -m t5_pretrainer.main_dense on a synthetic checkpoint directory and seeded files, two steps; the checkpoint loads
    with T5SeqPretrainEncoder.from_pretrained and embeds a text."""
    from test_gpu_cli import _make_world
    ckpt, _d2s, qdir, _codes, queries, dims = _make_world(str(tmp_path))
    rng = np.random.RandomState(5)
    coll = tmp_path / "collection"
    coll.mkdir()
    with open(coll / "raw.tsv", "w") as f:
        for d in range(40):
            f.write(f"{500 + d}\t{' '.join('w%d' % x for x in rng.randint(0, 200, 6 + d % 9))}\n")
    with open(tmp_path / "teacher.jsonl", "w") as f:
        for j in range(24):
            docs = [str(500 + int(x)) for x in rng.permutation(40)[:4]]
            f.write(json.dumps({"qid": list(queries)[j % len(queries)], "docids": docs,
                                "scores": [float(x) for x in rng.uniform(-4, 9, 4)]}) + "\n")
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [sys.executable, "-m", "t5_pretrainer.main_dense", "--loss_type=t5seq_pretrain_margin_mse", "--model_name_or_path", ckpt,
            "--model_type=t5_docid_gen_encoder", "--pretrained_path", ckpt, "--teacher_score_path", str(tmp_path / "teacher.jsonl"),
            "--collection_path", str(coll), "--queries_path", qdir, "--output_dir", str(out), "--max_length", "32",
            "--per_device_train_batch_size", "8", "--learning_rate", "1e-4", "--max_steps", "2", "--logging_steps", "1",
            "--save_steps", "0", '--task_names=["rank"]', "--use_fp16"]
    p = subprocess.run(["timeout", "-k", "10", "300"] + args, cwd=REPO, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    assert "t5seq_pretrain_margin_mse (dense first stage)" in p.stdout
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert [r["step"] for r in recs] == [1, 2] and all(np.isfinite(r["rank"]) and r["rank"] > 0 for r in recs)
    from transformers import AutoTokenizer
    from ripor_amd.modeling.t5_generative_retriever import T5SeqPretrainEncoder
    model = T5SeqPretrainEncoder.from_pretrained(str(out / "checkpoint")).to(0)
    tok = AutoTokenizer.from_pretrained(str(out / "checkpoint"))(["document: w3 w5 what is"], return_tensors="pt")
    rep = model.doc_encode(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"])
    torch.cuda.synchronize()
    assert tuple(rep.shape) == (1, dims.d_model) and bool(torch.isfinite(rep).all()) and float(rep.abs().max()) > 0
    before = T5SeqPretrainEncoder.from_pretrained(ckpt).base_model.state_dict()
    after = model.base_model.state_dict()
    assert not torch.equal(before["shared.weight"], after["shared.weight"])
    assert torch.equal(before["list_decoder_embeds.0.weight"], after["list_decoder_embeds.0.weight"])
