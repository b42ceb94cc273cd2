"""-m gpu: the rank-oriented stage (loss_type t5seq_aq_encoder_margin_mse) on the device — T5SeqAQEncoderForMarginMSE and
T5SeqAQEncoder.rerank_forward through rpr_lngknp_forward / rpr_lngknp_backward with ONE prefix (and none), at the shapes this
stage adds: a single loss, and 4 codes on a model of 8 positions. References: the rk_ fixtures of the imported reference class in
float64 (tests/golden/make_golden_rank.py), the lng_knp class on the same batch, engine.train_step, the CPU oracle.

Bars (restated from the tests that hold the f4_ fixtures to them, tests/test_gpu_train.py):
  f32, f16x2 — loss 1e-4 relative (REL_LOSS_TOL), position scores 1e-3 (POS_SCORE_TOL), every gradient tensor at rel = 1e-3 of
               check_grads_against_fixture, the global norm 1e-3 (test_lngknp_backward_matches_reference_gradients);
  bf16       — loss and global norm 3 %, every gradient tensor's cosine with the f16x2 gradient >= 0.995 where the tensor is
               not noise-level (test_bf16_training_mode_is_the_references_autocast_arithmetic)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_rank_stage_host import RK_CASES, RankGolden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_LOSS_TOL = 1e-4      # test_gpu_train.py
POS_SCORE_TOL = 1e-3     # test_gpu_train.py, test_gpu_heads128.py
GRAD_REL = 1e-3          # test_gpu_train.py::_backward_checks
NORM_TOL = 1e-3
BF16_TOL = 3e-2          # test_gpu_train.py::test_bf16_training_mode_is_the_references_autocast_arithmetic
BF16_COS = 0.995


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


def _unused_codebooks(g):
    """Names of the codebooks of the positions past the smtid."""
    tabs = ["list_decoder_embeds"] + ([] if g.dims.shared_output_input_embeds else ["list_output_embeds"])
    return [f"{t}.{i}.weight" for t in tabs for i in range(g.L, len(g.dims.decoder_vocab_sizes))]


def _check_unreached_are_zero(g, grads):
    """A tensor the reference's autograd never reached has an exactly zero gradient on the device."""
    names = {("shared.weight" if str(n) == "encoder.embed_tokens.weight" else str(n)) for n in g.z["grad_names"]}
    for k, v in grads.items():
        if k not in names:
            assert not np.any(v), k
    for k in _unused_codebooks(g):
        assert k in grads and not np.any(grads[k]), k


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", RK_CASES)
def test_forward_and_backward_match_the_reference_fixture(name, precision):
    from test_oracle_golden import check_grads_against_fixture
    g = RankGolden(name)
    m = g.model(device=0)
    ref = float(g.z["loss"])
    with _Prec(precision) as ctx:
        ctx.status(clear=True)
        out = m(**g.inputs())
        torch.cuda.synchronize()
        assert ctx.status() == 0 and set(out) == {"rank"} and out["rank"].dtype == torch.float32
        ps = m.last_position_scores.cpu().numpy().astype(np.float64)
        assert ps.shape == (g.bz, 2, g.L)
        err = max(np.abs(ps[:, 0] - g.z["pos_position_scores"]).max(), np.abs(ps[:, 1] - g.z["neg_position_scores"]).max())
        print(f"[rank] {name} {precision}: forward loss {float(out['rank']):.6f} vs {ref:.6f}, max position-score error {err:.2e}")
        assert err <= POS_SCORE_TOL
        assert abs(float(out["rank"]) - ref) <= REL_LOSS_TOL * max(1.0, abs(ref))
        assert torch.equal(m(**g.inputs())["rank"], out["rank"])                      # deterministic
        st = m.train_state()
        st.grads.fill_(float("nan"))                                                  # the backward overwrites all of it
        losses = m.backward(**g.inputs())
        torch.cuda.synchronize()
        assert set(losses) == {"rank"}
        total = float(losses["rank"])
        grads = {k: v.detach().cpu().numpy() for k, v in st.named_grads().items()}
        gnorm = float(torch.sqrt((st.grads.double() ** 2).sum()))
        print(f"[rank] {name} {precision}: backward loss {total:.6f} vs {ref:.6f}, global norm {gnorm:.6g} vs {float(g.z['grad_global_norm']):.6g}")
        assert abs(total - ref) <= 1e-4 * abs(total)
        worst = check_grads_against_fixture(g, grads, rel=GRAD_REL, label=f" (HIP {precision})")
        print(f"[rank] {name} {precision}: worst sampled-gradient error {worst[0]:.2e} of scale ({worst[1]})")
        assert abs(gnorm - float(g.z["grad_global_norm"])) <= NORM_TOL * gnorm
        _check_unreached_are_zero(g, grads)
        first = st.grads.clone()
        m.backward(**g.inputs())
        assert torch.equal(first, st.grads)                                          # deterministic


@pytest.mark.parametrize("name", RK_CASES)
def test_bf16_step_is_the_references_autocast_arithmetic(name):
    g = RankGolden(name)
    m = g.model(device=0)
    ref = float(g.z["loss"])
    with _Prec("f16x2"):
        m.backward(**g.inputs())
        split = {k: v.detach().double().cpu() for k, v in m.train_state().named_grads().items()}
    with _Prec("bf16") as ctx:
        assert ctx.get_precision() == "bf16"
        st = m.train_state()
        st.grads.fill_(float("nan"))
        losses = m.backward(**g.inputs())
        torch.cuda.synchronize()
        got = {k: v.detach().double().cpu() for k, v in st.named_grads().items()}
        gn = float(torch.sqrt((st.grads.double() ** 2).sum()))
        gmax = max(float(v.abs().max()) for v in split.values())
        worst = (1.0, None)
        for k, v in got.items():
            r = split[k]
            if float(r.abs().max()) < 1e-4 * gmax:      # tensors whose gradient is noise-level carry no direction
                continue
            cos = float((v * r).sum() / (v.norm() * r.norm() + 1e-300))
            worst = min(worst, (cos, k))
        print(f"[rank-bf16] {name}: loss {float(losses['rank']):.6f} vs {ref:.6f}, global norm {gn:.6g} vs "
              f"{float(g.z['grad_global_norm']):.6g}, worst gradient cosine {worst[0]:.5f} ({worst[1]})")
        assert abs(float(losses["rank"]) - ref) <= BF16_TOL * max(1.0, abs(ref))
        assert abs(gn - float(g.z["grad_global_norm"])) <= BF16_TOL * gn
        assert worst[0] >= BF16_COS, worst
        _check_unreached_are_zero(g, {k: v.numpy() for k, v in got.items()})
        first = st.grads.clone()
        m.backward(**g.inputs())
        assert torch.equal(first, st.grads), "bf16 backward is not deterministic"
        # the forward keeps fp32-equivalent arithmetic under this setting
        out = m(**g.inputs())
        assert abs(float(out["rank"]) - ref) <= REL_LOSS_TOL * max(1.0, abs(ref))


def test_rank_loss_is_the_lngknp_rank_loss_bit_for_bit():
    """The two classes enqueue the same pass, and a prefix's loss does not depend on the other prefixes."""
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE
    from ripor_amd.utils import synth
    g = RankGolden("rk_mini_bz4_l8")
    one, knp = g.model(device=0), g.model(T5SeqAQEncoderForLngKnpMarginMSE, device=0)
    inputs = g.inputs()
    with_4 = dict(inputs)
    with_4["smtid_4_teacher_pos_scores"] = torch.from_numpy(synth.uniform_f32("rk/knp/p4", (g.bz,), 30.0))
    with_4["smtid_4_teacher_neg_scores"] = torch.from_numpy(synth.uniform_f32("rk/knp/n4", (g.bz,), 30.0))
    a = one(**inputs)
    b = knp(**with_4)
    torch.cuda.synchronize()
    assert set(a) == {"rank"} and set(b) == {"rank", "rank_4"}
    assert torch.equal(a["rank"], b["rank"]) and float(a["rank"]) != float(b["rank_4"])
    assert torch.equal(one.last_position_scores, knp.last_position_scores)


@pytest.mark.parametrize("dropout", [None, 0.1])
def test_training_step_is_engine_train_step_with_one_prefix(dropout):
    """Two optimisation steps of the class against engine.train_step(prefix_lens=[L]) on a twin: the same weights and AdamW
    moments, bit for bit; without dropout and at rate 0.1 under a fixed seed. 4 codes on a model of 8 positions."""
    from ripor_amd import engine as E
    g = RankGolden("rk_mini_bz3_l4of8")
    m, twin = g.model(device=0), g.model(device=0)
    inputs = g.inputs()
    em = twin.base_model.engine_model()
    st2 = E.TrainState(em)
    codes = torch.stack([inputs["pos_doc_encoding"], inputs["neg_doc_encoding"]], dim=1)
    tp, tn = inputs["teacher_pos_scores"][None].float(), inputs["teacher_neg_scores"][None].float()
    q = inputs["pos_tokenized_query"]
    before = {k: v.clone() for k, v in em.export_state_dict().items()}
    with _Prec("f16x2"):
        for step in range(2):
            drop = dict(dropout_rate=dropout, dropout_seed=0x5EED_1234_ABCD, global_step=step) if dropout else {}
            la = m.training_step(lr=1e-4, **drop, **inputs)
            lb = E.train_step(em, st2, q["input_ids"], q["attention_mask"], codes, tp, tn, [g.L], 1e-4, **drop)
            torch.cuda.synchronize()
            assert set(la) == {"rank"} and torch.equal(la["rank"], lb[0])
            first = float(la["rank"]) if step == 0 else first
    st1 = m.train_state()
    assert st1.step == st2.step == 2
    assert torch.equal(st1.exp_avg, st2.exp_avg) and torch.equal(st1.exp_avg_sq, st2.exp_avg_sq) and torch.equal(st1.grads, st2.grads)
    a, b = m.base_model.engine_model().export_state_dict(), em.export_state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["shared.weight"], before["shared.weight"]), "the weights did not move"
    for k in _unused_codebooks(g):                                                   # never read, never updated
        assert torch.equal(a[k], before[k]), k
    ref = float(g.z["loss"])
    if dropout:
        assert abs(first - ref) > 1e-3 * ref, "dropout changed nothing"
    else:
        assert abs(first - ref) <= REL_LOSS_TOL * max(1.0, ref)


@pytest.mark.parametrize("name", ["rk_mini_bz4_l8", "rk_mini_bz3_l4of8"])
def test_rerank_forward_is_the_positive_row_sum(name):
    """Bit for bit the row sums of forward's position scores, at 12 decoder rows per document slot (bz 3, L 4) and at 32 (bz 4,
    L 8): the split-precision GEMM changes its kernel past 32 rows, and a pass over ONE slot missed the second shape in the last
    digit of two scores of four (profiles/r27_rank_stage_summary.txt) — rerank_forward fills both slots of forward's pass."""
    from oracle import t5_ref, train_ref
    g = RankGolden(name)
    m = g.model(device=0)
    inputs = g.inputs()
    m(**inputs)
    rows = m.last_position_scores[:, 0].clone()
    got = m.rerank_forward(tokenized_query=inputs["pos_tokenized_query"], doc_encoding=inputs["pos_doc_encoding"])
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (g.bz,)
    assert torch.equal(got, rows.sum(dim=-1))
    prev = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        with torch.no_grad():
            ref = train_ref.position_scores(t5_ref.T5Ref(g.state_dict, g.dims), g.z["q_ids"], g.z["q_mask"], g.z["pos_doc_encoding"])
    finally:
        torch.set_num_threads(prev)
    ref = ref.double().numpy()
    assert np.abs(ref - g.z["pos_position_scores"]).max() <= 1e-4       # the oracle itself, against the reference's float64
    err_rows = np.abs(rows.cpu().double().numpy() - ref).max()
    err = np.abs(got.cpu().double().numpy() - ref.sum(-1)).max()
    print(f"[rank] {name}: rerank_forward max error {err:.2e}, per position {err_rows:.2e}")
    assert err_rows <= POS_SCORE_TOL and err <= POS_SCORE_TOL
    # the base class has it too (the reference defines it on T5SeqAQEncoder), for the negative as well
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder
    base = g.model(T5SeqAQEncoder, device=0)
    neg = base.rerank_forward(tokenized_query=inputs["neg_tokenized_query"], doc_encoding=inputs["neg_doc_encoding"])
    assert torch.equal(neg, m.last_position_scores[:, 1].sum(dim=-1))


def _state(path):
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForMarginMSE
    return T5SeqAQEncoderForMarginMSE.from_pretrained(path).base_model.state_dict()


@pytest.mark.parametrize("form", ["docid", "smtid"])
def test_main_rank_trains_resumes_and_writes_a_checkpoint(tmp_path, form):
    """python -m t5_pretrainer.main_rank --max_steps=3 in a fresh process on a mini checkpoint and a six-line example file; the
    final checkpoint loads and differs from the initial one; a second process resumed from checkpoint-2 leaves step 3's weights
    bit for bit. docid: full-length docids looked up in docid_to_smtid.json, bf16 like the reference's scripts; smtid:
    --smtid_as_docid with smtids of 4 codes on the model of 8 positions."""
    from test_gpu_cli import _make_world
    ckpt, d2s_path, qdir, codes, queries, dims = _make_world(str(tmp_path))
    rng = np.random.RandomState(11)
    qids = list(queries)
    with open(tmp_path / "examples.jsonl", "w") as f:
        for j in range(6):
            rows = [int(x) for x in rng.permutation(len(codes))[:4]]
            ex = {"qid": qids[j], "scores": [float(x) for x in rng.uniform(-4, 9, 4)]}
            if form == "docid":
                ex["docids"] = [str(100 + r) for r in rows]
            else:
                ex["smtids"] = ["_".join(str(int(c)) for c in codes[r][:4]) for r in rows]
            f.write(json.dumps(ex) + "\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(out, *more):
        args = [sys.executable, "-m", "t5_pretrainer.main_rank", "--loss_type=t5seq_aq_encoder_margin_mse", "--model_name_or_path", ckpt,
                "--model_type=t5_docid_gen_encoder", "--pretrained_path", ckpt, "--teacher_score_path", str(tmp_path / "examples.jsonl"),
                "--queries_path", qdir, "--output_dir", str(out), "--max_length", "32", "--per_device_train_batch_size", "4",
                "--learning_rate", "1e-4", "--max_steps=3", "--logging_steps", "1", "--save_steps", "2", '--task_names=["rank"]',
                "--wandb_project_name=unused", "--epochs=150"]
        args += ["--docid_to_smtid_path", d2s_path, "--use_fp16"] if form == "docid" else ["--smtid_as_docid"]
        p = subprocess.run(["timeout", "-k", "10", "300"] + args + list(more), cwd=REPO, env=env, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
        return p.stdout

    out = tmp_path / "out"
    stdout = run(out)
    assert "t5seq_aq_encoder_margin_mse (rank-oriented stage): 6 examples" in stdout
    recs = [json.loads(l) for l in stdout.splitlines() if l.startswith("{")]
    assert [r["step"] for r in recs] == [1, 2, 3] and all(np.isfinite(r["rank"]) and r["rank"] > 0 for r in recs)
    assert sorted(os.listdir(out)) == ["checkpoint", "checkpoint-2"]
    before, after = _state(ckpt), _state(str(out / "checkpoint"))
    assert set(before) == set(after) and all(bool(torch.isfinite(v).all()) for v in after.values())
    assert not torch.equal(before["shared.weight"], after["shared.weight"])
    assert not torch.equal(before["list_decoder_embeds.0.weight"], after["list_decoder_embeds.0.weight"])
    if form == "smtid":   # 4 codes: the codebooks of positions 4 .. 7 are as they were
        assert all(torch.equal(before[f"list_decoder_embeds.{i}.weight"], after[f"list_decoder_embeds.{i}.weight"]) for i in range(4, 8))
    out2 = tmp_path / "out_resumed"
    stdout2 = run(out2, "--resume_from_checkpoint", str(out / "checkpoint-2"))
    assert [json.loads(l)["step"] for l in stdout2.splitlines() if l.startswith("{")] == [3]
    resumed = _state(str(out2 / "checkpoint"))
    assert all(torch.equal(after[k], resumed[k]) for k in after)


def test_rerank_for_create_trainset_end_to_end(tmp_path, monkeypatch):
    """A run of 3 queries x 5 passages -> task 1 -> task 2: the merged file holds, per query, the passages sorted by the teacher's
    score with exactly the scores CrossEncoder gives the same pairs."""
    import xenc_ref as ref
    from transformers import AutoTokenizer
    from ripor_amd import rerank as R
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    fx = ref.load_fixture("x1")
    ckpt = ref.write_checkpoint(fx, str(tmp_path / "teacher"))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(5, 200)]
    with open(os.path.join(ckpt, "vocab.txt"), "w") as f:
        f.write("\n".join(words) + "\n")
    rng = np.random.default_rng(9)
    text = lambda n: " ".join(f"w{int(i)}" for i in rng.integers(5, 200, size=n))  # noqa: E731
    docs = {f"{100 + i}": text(int(rng.integers(3, 40))) for i in range(9)}
    queries = {f"{i}": text(int(rng.integers(2, 9))) for i in range(3)}
    for d, rows in (("collection", docs), ("queries", queries)):
        (tmp_path / d).mkdir()
        with open(tmp_path / d / "raw.tsv", "w") as f:
            f.writelines(f"{k}\t{v}\n" for k, v in rows.items())
    dk = list(docs)
    run = {q: {dk[(3 * int(q) + t) % 9]: float(t) for t in range(5)} for q in queries}
    with open(tmp_path / "run.json", "w") as f:
        json.dump(run, f)
    out = tmp_path / "out"
    R.main(["--task=rerank_for_create_trainset", f"--model_name_or_path={ckpt}", f"--collection_path={tmp_path / 'collection'}",
            f"--q_collection_path={tmp_path / 'queries'}", f"--run_json_path={tmp_path / 'run.json'}", "--json_type=json",
            f"--out_dir={out}", "--batch_size=16", "--max_length=32", "--local_rank=0"])
    assert os.listdir(out) == ["rerank_0.json"]
    shard = json.load(open(out / "rerank_0.json"))
    assert {q: list(v) for q, v in shard.items()} == {q: list(v) for q, v in run.items()}
    R.main(["--task=rerank_for_create_trainset_2", f"--out_dir={out}"])
    assert os.listdir(out) == [R.TRAINSET_NAME]
    lines = [json.loads(l) for l in open(out / R.TRAINSET_NAME).read().splitlines()]
    assert [ex["qid"] for ex in lines] == list(run) and all(set(ex) == {"qid", "docids", "scores"} for ex in lines)
    pairs = [(q, d) for q, by in run.items() for d in by]
    tok = AutoTokenizer.from_pretrained(ckpt)
    kw = tok([queries[q] for q, _ in pairs], [docs[d] for _, d in pairs], padding=True, truncation="longest_first",
             return_attention_mask=True, return_tensors="pt", max_length=32)
    direct = dict(zip(pairs, CrossEncoder(ckpt).to(0).rerank_forward(kw)["scores"].cpu().tolist()))
    assert np.std(list(direct.values())) > 0.01
    for ex in lines:
        assert sorted(ex["docids"]) == sorted(run[ex["qid"]]) and len(ex["docids"]) == 5
        assert ex["scores"] == sorted(ex["scores"], reverse=True)
        assert ex["scores"] == [direct[(ex["qid"], d)] for d in ex["docids"]]     # one batch of the same 15 pairs: the same bits
