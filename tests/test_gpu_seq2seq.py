"""-m gpu: the seq2seq docid step (loss_type t5seq_aq_encoder_seq2seq) on the device — rpr_seq2seq_forward / _backward /
_backward_buckets against the reference's own T5SeqAQEncoderForSeq2Seq (tests/golden/s2s_*.npz, make_golden_seq2seq.py) and
against the autograd restatement of tests/test_seq2seq_host.py at t5-base dims, determinism, bucket coverage, label checks,
the command line end to end and the search after a step. Bars as the ranking step's (tests/test_gpu_train.py): losses 1e-4
relative, gradients 1e-3 of each tensor's scale; label log-probabilities 1e-3 absolute (logits are O(10) here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from test_seq2seq_host import S2S_CASES, S2SGolden, check_grads, seq2seq_grads

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_LOSS_TOL = 1e-4
LP_TOL = 1e-3


def _model(g):
    from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig, T5ForDocIDGeneration, T5SeqAQEncoderForSeq2Seq
    m = T5SeqAQEncoderForSeq2Seq.__new__(T5SeqAQEncoderForSeq2Seq)
    m.config = T5forDocIDConfig.from_dims(g.dims)
    m.base_model = T5ForDocIDGeneration(m.config, g.state_dict).to(0)
    m.model_args, m.multi_vocab_sizes = None, False
    return m


class _Prec:
    def __init__(self, name):
        from ripor_amd import engine as E
        self.ctx, self.name = E.Context.get(0), name

    def __enter__(self):
        self.ctx.set_precision(self.name)

    def __exit__(self, *a):
        self.ctx.set_precision("f16x2")


@pytest.mark.parametrize("precision", ["f32", "f16x2", "bf16"])
@pytest.mark.parametrize("name", S2S_CASES)
def test_seq2seq_forward_matches_reference(name, precision):
    g = S2SGolden(name)
    m = _model(g)
    with _Prec(precision):
        out = m(**g.inputs())
        torch.cuda.synchronize()
        ref = float(g.z["loss"])
        # bf16 GEMM operands in the encoder / decoder (the reference's autocast): the loss moves by the rounding of 24 layers
        tol = REL_LOSS_TOL if precision != "bf16" else 3e-2
        assert set(out) == {"rank"} and out["rank"].dtype == torch.float32
        assert abs(float(out["rank"]) - ref) <= tol * max(1.0, abs(ref)), (name, precision, float(out["rank"]), ref)
        lp = m.last_label_logprobs.cpu().numpy()
        if precision != "bf16":
            np.testing.assert_allclose(lp, g.z["label_logprobs"], atol=LP_TOL * max(1.0, np.abs(g.z["label_logprobs"]).max() / 10),
                                       rtol=0)
        assert abs(-lp.mean() - float(out["rank"])) <= 1e-4 * abs(float(out["rank"]))   # the loss is the mean of -log p(label)
        out2 = m(**g.inputs())
        assert torch.equal(out["rank"], out2["rank"])


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", S2S_CASES)
def test_seq2seq_backward_matches_reference_gradients(name, precision):
    """Every gradient tensor (norm and seeded samples) of the reference's loss.backward(), shared codebooks and V = 1024
    included; two identical backward calls give the same bits."""
    g = S2SGolden(name)
    m = _model(g)
    with _Prec(precision):
        loss = m.backward(**g.inputs())["rank"]
        torch.cuda.synchronize()
        assert abs(float(loss) - float(g.z["loss"])) <= REL_LOSS_TOL * abs(float(g.z["loss"]))
        st = m.train_state()
        grads = {k: v.detach().cpu().numpy() for k, v in st.named_grads().items()}
        worst = check_grads(g, grads, rel=1e-3, label=" (HIP)")
        gnorm = float(torch.sqrt((st.grads.double() ** 2).sum()))
        assert abs(gnorm - float(g.z["grad_global_norm"])) <= 1e-3 * gnorm
        if g.dims.shared_output_input_embeds:
            assert not any(k.startswith("list_output_embeds") for k in grads)
        print(f"[s2s-bwd] {name} {precision}: worst sampled error {worst[0]:.2e} ({worst[1]}), global norm {gnorm:.6g}")
        first = st.grads.clone()
        m.backward(**g.inputs())
        assert torch.equal(first, st.grads)


def test_seq2seq_training_step_matches_reference_adamw_update():
    from test_oracle_golden import grad_sample_indices
    g = S2SGolden("s2s_mini_bz4_l16")
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
        err = np.abs(d - ref)     # same bound as the ranking step's test (noise-level gradients may flip an entry's update)
        assert (err <= 3e-2 * lr).mean() >= 0.9 and err.max() <= 2.0 * lr * 1.001, f"update of {n}: {err.max() / lr:.3f} lr"
    out = m(**g.inputs())
    torch.cuda.synchronize()
    ref_after = float(g.z["loss_after_step"])
    assert abs(float(out["rank"]) - ref_after) <= 5e-3 * abs(ref_after), (float(out["rank"]), ref_after)


def _robust_compare(hip, og, gn):
    """As the ranking step's whole-tensor comparison (test_gpu_train._robust_grad_compare: a ReLU pre-activation within fp32
    noise of 0 may take different sides in two summation orders and perturb everything upstream): here 64 queries of up to
    88 tokens put 16x more feed-forward units near that edge, so the 99.9th percentile bound per tensor is 5e-3 of its
    largest entry (measured 2.0e-3 at worst); the median tensor within 2e-4, no entry off by more than 10 %, the global norm
    within 1e-3."""
    worst, rels = (0.0, ""), []
    for k, v in hip.items():
        if k not in og:           # a table autograd never reached (the input codebook of the last position): zero here
            assert not np.any(v), k
            continue
        o = og[k].double().numpy().reshape(v.shape)
        e = np.abs(v - o).reshape(-1)
        scale = max(np.abs(o).max(), 1e-30)
        q = float((np.partition(e, int(0.999 * (e.size - 1)))[int(0.999 * (e.size - 1))] if e.size > 1000 else np.median(e)) / scale)
        rels.append(q)
        worst = max(worst, (q, k))
        assert q <= 5e-3, (k, q)
        assert e.max() / scale <= 0.1, (k, e.max() / scale)
    assert np.median(rels) <= 2e-4, np.median(rels)
    hn = float(np.sqrt(sum((v ** 2).sum() for v in hip.values())))
    assert abs(hn - gn) <= 1e-3 * gn
    return worst, float(np.median(rels)), hn


def test_seq2seq_backward_matches_autograd_at_t5_base_dims_bz64():
    """t5-base dims (12 + 12 layers, d_ff 3072), bz 64, L 32, ragged queries up to 88 tokens (the longest the LDS-resident
    encoder self-attention backward holds, as for the ranking step): larger than the fixtures; every gradient tensor against
    autograd through the CPU oracle."""
    from oracle import t5_ref
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    L, bz = 32, 64
    dims = synth.t5_base_dims(L=L, V=256, vocab_size=2048)
    sd = synth.make_state_dict(dims, seed=808)
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=809, mean_len=40, std_len=30, min_len=4, max_len=88)
    labels = synth.make_codes(bz, L, 256, seed=810).astype(np.int64)
    ctx = E.Context.get(0)
    with _Prec("f32"):
        model = E.DeviceModel(ctx, sd, dims)
        state = E.TrainState(model)
        loss = E.seq2seq_backward(model, state, torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(labels))
        torch.cuda.synchronize()
        hip = {k: v.detach().cpu().double().numpy() for k, v in state.named_grads().items()}
    torch.set_num_threads(16)
    ref_loss, og, gn = seq2seq_grads(t5_ref.T5Ref(sd, dims), ids, mask, labels)
    assert abs(float(loss) - ref_loss) <= REL_LOSS_TOL * abs(ref_loss)
    worst, med, hn = _robust_compare(hip, og, gn)
    print(f"[s2s-bwd] t5-base bz {bz} L {L} Lq {ids.shape[1]}: worst p99.9 {worst[0]:.2e} ({worst[1]}), median {med:.2e}")


def test_seq2seq_buckets_cover_the_flat_buffer_in_lngknp_order():
    from ripor_amd import engine as E
    g = S2SGolden("s2s_mini_bz4_l8")
    m = _model(g)
    em = m.base_model.engine_model()
    st = m.train_state()
    inp = g.inputs()
    ids, mask, labels = inp["tokenized_query"]["input_ids"], inp["tokenized_query"]["attention_mask"], inp["labels"]
    ex = E.GradExchange(st.grads, dry_run=True)
    E.seq2seq_backward(em, st, ids, mask, labels, exchange=ex)
    ex.finish()
    torch.cuda.synchronize()
    s2s_buckets = list(ex.history)
    with_buckets = st.grads.clone()
    E.seq2seq_backward(em, st, ids, mask, labels)
    torch.cuda.synchronize()
    assert torch.equal(with_buckets, st.grads)          # the hand-over changes no gradient
    covered = sorted(s2s_buckets)
    pos = 0
    for off, n in covered:
        assert off == pos
        pos += n
    assert pos == st.total
    # the ranking step's order and layout on the same model
    codes = torch.stack([labels, labels], dim=1)
    tp = torch.zeros((2, g.bz)); tn = torch.zeros((2, g.bz))
    ex2 = E.GradExchange(st.grads, dry_run=True)
    E.lngknp_backward(em, st, ids, mask, codes, tp, tn, [8, 4], exchange=ex2)
    ex2.finish()
    torch.cuda.synchronize()
    assert ex2.history == s2s_buckets


def test_seq2seq_refuses_labels_outside_the_codebooks():
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    g = S2SGolden("s2s_mini_bz4_l8")
    m = _model(g)
    inp = g.inputs()
    em = m.base_model.engine_model()
    ids, mask = inp["tokenized_query"]["input_ids"], inp["tokenized_query"]["attention_mask"]
    for bad in (256, -1, 100000):
        lab = inp["labels"].clone()
        lab[1, 3] = bad
        with pytest.raises(RiporHipError, match="outside"):
            E.seq2seq_forward(em, ids, mask, lab)
        with pytest.raises(RiporHipError, match="outside"):
            E.seq2seq_backward(em, m.train_state(), ids, mask, lab)
        bad_inp = {"tokenized_query": dict(inp["tokenized_query"]), "labels": lab}
        bad_inp["tokenized_query"]["decoder_input_ids"] = torch.cat([torch.full((g.bz, 1), -1), lab[:, :-1]], 1)
        with pytest.raises(ValueError, match="outside"):
            m(**bad_inp)
    bad_inp = {"tokenized_query": dict(inp["tokenized_query"]), "labels": inp["labels"]}
    bad_inp["tokenized_query"]["decoder_input_ids"] = inp["tokenized_query"]["decoder_input_ids"].clone()
    bad_inp["tokenized_query"]["decoder_input_ids"][0, 2] += 1
    with pytest.raises(ValueError, match="decoder_input_ids"):
        m(**bad_inp)
    # the device is still fine afterwards
    out = m(**inp)
    assert abs(float(out["rank"]) - float(g.z["loss"])) <= 1e-3 * abs(float(g.z["loss"]))


def test_search_after_a_seq2seq_step_sees_the_new_weights():
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    g = S2SGolden("s2s_mini_bz4_l8")
    m = _model(g)
    em = m.base_model.engine_model()
    trie = E.DeviceTrie.from_codes(em.ctx, synth.make_codes(500, g.L, g.V, seed=3), g.V)
    ids, mask = torch.from_numpy(g.z["input_ids"]), torch.from_numpy(g.z["attention_mask"])
    before = E.search(em, trie, ids, mask, 4, g.L)
    sc0 = before.scores.cpu().clone()
    m.training_step(lr=1e-3, **g.inputs())
    after = E.search(em, trie, ids, mask, 4, g.L)
    sc1 = after.scores.cpu()
    # what a fresh model built from the updated weights finds
    fresh = E.DeviceModel(em.ctx, {k: v.cpu().numpy() for k, v in em.export_state_dict().items()}, g.dims)
    ref = E.search(fresh, trie, ids, mask, 4, g.L)
    torch.cuda.synchronize()
    assert not torch.equal(sc0, sc1)
    assert torch.equal(after.tokens.cpu(), ref.tokens.cpu())
    assert torch.allclose(sc1, ref.scores.cpu(), atol=1e-5, rtol=0)


def test_main_trains_seq2seq_end_to_end(tmp_path):
    """python -m t5_pretrainer.main --loss_type=t5seq_aq_encoder_seq2seq on a synthetic checkpoint directory: the logged loss
    falls, the checkpoint loads with T5SeqAQEncoder.from_pretrained, and a constrained search on it returns valid smtids."""
    from test_gpu_cli import _make_world
    ckpt, d2s_path, _qdir, codes, queries, dims = _make_world(str(tmp_path))
    rng = np.random.RandomState(3)
    docs = [str(100 + i) for i in range(16)]               # a small set of docids, many queries each: learnable in 20 steps
    with open(tmp_path / "q2d.jsonl", "w") as f:
        for j in range(64):
            d = docs[j % len(docs)]
            f.write(json.dumps({"docid": d, "query": f"what is w{int(d) % 50} {' '.join('w%d' % x for x in rng.randint(0, 200, 3))}"}) + "\n")
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [sys.executable, "-m", "t5_pretrainer.main", "--loss_type=t5seq_aq_encoder_seq2seq", "--model_name_or_path", ckpt,
            "--pretrained_path", ckpt, "--query_to_docid_path", str(tmp_path / "q2d.jsonl"), "--docid_to_smtid_path", d2s_path,
            "--output_dir", str(out), "--max_length", "64", "--per_device_train_batch_size", "16", "--learning_rate", "1e-3",
            "--warmup_ratio", "0.1", "--max_steps", "20", "--logging_steps", "5", "--save_steps", "0", "--multi_vocab_sizes"]
    p = subprocess.run(["timeout", "-k", "10", "600"] + args, cwd=REPO, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    assert "t5seq_aq_encoder_seq2seq (seq2seq docid step)" in p.stdout      # the start-up line names the loss type
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert [r["step"] for r in recs] == [5, 10, 15, 20]
    assert recs[-1]["rank"] < 0.8 * recs[0]["rank"], [r["rank"] for r in recs]
    from ripor_amd import engine as E
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder
    model = T5SeqAQEncoder.from_pretrained(str(out / "checkpoint")).to(0)
    em = model.base_model.engine_model()
    trie = E.DeviceTrie.from_codes(em.ctx, codes, 256)
    ids, mask = torch.randint(3, 200, (3, 7)), torch.ones((3, 7), dtype=torch.long)
    res = E.search(em, trie, ids, mask, 4, len(dims.decoder_vocab_sizes))
    tok = res.tokens.cpu().numpy().reshape(-1, codes.shape[1])
    valid = {tuple(int(x) for x in r) for r in codes}
    assert all(tuple(int(x) for x in t) in valid for t in tok)
