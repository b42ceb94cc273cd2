"""-m gpu: the f16 mode of the cross-encoder teacher (``rpr_xenc_set_precision(RPR_XENC_F16)``).

The mode replaces the reference's fp16 autocast, so it must be at least as close to the truth: per model the bar is
max |HF fp16 autocast - HF fp64| over the model's recorded pairs (tests/golden/xh_xenc.npz: x1 1.37e-3, x2 1.17e-3,
x3 1.38e-3), and max |ours - fp64| must not exceed it. No margin is added; the torch restatement of the data flow
(tests/xenc_half_ref.py) sits at 5.3e-4 / 6.9e-4 / 4.5e-4."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xenc_half_ref as href  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(m, k) for m, keys in href.ref.FIXTURES.items() for k in keys] + [("x3", "a")]


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


def _model(ctx, name, precision):
    from ripor_amd import engine as E
    fx = href.load(name)
    m = E.XencModel(ctx, fx["weights"], fx["cfg"])
    m.set_precision(precision)
    return m


@pytest.fixture(scope="module")
def half(ctx):
    return {m: _model(ctx, m, "f16") for m in href.MODELS}


@pytest.fixture(scope="module")
def full(ctx):
    return {m: _model(ctx, m, "f32") for m in href.MODELS}


def _score(model, b, rows=slice(None)):
    from ripor_amd import engine as E
    return E.xenc_score(model, torch.from_numpy(b["ids"][rows]), torch.from_numpy(b["types"][rows]),
                        torch.from_numpy(b["mask"][rows])).cpu().numpy()


@pytest.mark.parametrize("model,key", CASES)
def test_f16_mode_within_the_references_own_error(half, model, key):
    fx = href.load(model)
    b = fx["batches"][key]
    assert half[model].precision == "f16"
    got = _score(half[model], b)
    err = np.abs(got.astype(np.float64) - b["fp64"]).max()
    print(f"[xenc f16] {model}/{key}: bz {len(got)}, max |hip f16 - fp64| {err:.3e}, bar {fx['bar']:.3e}")
    assert got.shape == b["fp64"].shape and got.dtype == np.float32 and np.isfinite(got).all()
    assert err <= fx["bar"]


@pytest.mark.parametrize("model,key", [("x1", "b"), ("x3", "a")])
def test_f16_mode_is_not_the_fp32_path(half, full, model, key):
    b = href.load(model)["batches"][key]
    diff = np.abs(_score(half[model], b).astype(np.float64) - _score(full[model], b)).max()
    print(f"[xenc f16] {model}/{key}: max |f16 mode - f32 mode| {diff:.3e}")
    assert diff > 1e-5   # the restatement differs from fp32 by more than 4e-4 here; fp32 itself sits at 5e-7


@pytest.mark.parametrize("model,key", [("x1", "b"), ("x2", "c"), ("x1", "e"), ("x3", "a")])
def test_same_call_twice_same_bits(half, model, key):
    b = href.load(model)["batches"][key]
    one, two = _score(half[model], b), _score(half[model], b)
    assert one.tobytes() == two.tobytes()


@pytest.mark.parametrize("model,key,cut", [("x1", "b", 6), ("x2", "b", 9), ("x1", "d", 33), ("x2", "f", 1), ("x3", "a", 4)])
def test_whole_batch_against_two_halves(half, model, key, cut):
    fx = href.load(model)
    b = fx["batches"][key]
    whole = _score(half[model], b)
    halves = np.concatenate([_score(half[model], b, slice(0, cut)), _score(half[model], b, slice(cut, None))])
    assert np.abs(whole.astype(np.float64) - halves).max() <= fx["bar"]   # a wrong sequence offset costs about 0.1


def test_every_x3_pair_alone(half):
    fx = href.load("x3")
    b = fx["batches"]["a"]
    whole = _score(half["x3"], b)
    alone = np.concatenate([_score(half["x3"], b, slice(i, i + 1)) for i in range(len(whole))])
    assert np.abs(whole.astype(np.float64) - alone).max() <= fx["bar"]
    assert np.abs(alone.astype(np.float64) - b["fp64"]).max() <= fx["bar"]


def test_round_trip_restores_the_fp32_bits(ctx, full):
    b = href.load("x1")["batches"]["b"]
    never = _score(full["x1"], b)
    m = _model(ctx, "x1", "f32")
    before = _score(m, b)
    m.set_precision("f16")
    assert m.precision == "f16"
    in_half = _score(m, b)
    m.set_precision("f32")
    assert m.precision == "f32"
    after = _score(m, b)
    assert before.tobytes() == never.tobytes() and after.tobytes() == never.tobytes()
    assert in_half.tobytes() != never.tobytes()


def test_two_models_in_different_modes_do_not_disturb_each_other(half, full):
    b1, b2 = href.load("x1")["batches"]["c"], href.load("x2")["batches"]["b"]
    h1, f2 = _score(half["x1"], b1), _score(full["x2"], b2)
    for _ in range(2):   # interleaved on one ctx: the same workspace serves both modes
        assert _score(full["x2"], b2).tobytes() == f2.tobytes()
        assert _score(half["x1"], b1).tobytes() == h1.tobytes()
    assert half["x1"].precision == "f16" and full["x2"].precision == "f32" and full["x1"].precision == "f32"


def test_invalid_precision_changes_nothing(ctx, half):
    lib = ctx.lib
    b = href.load("x2")["batches"]["b"]
    before = _score(half["x2"], b)
    assert lib.rpr_xenc_set_precision(ctx.handle, half["x2"].handle, 7, None) == -1   # RPR_ERR_INVALID
    assert b"precision" in lib.rpr_last_error()
    assert lib.rpr_xenc_get_precision(half["x2"].handle) == 1
    with pytest.raises(ValueError):
        half["x2"].set_precision("bf16")
    assert _score(half["x2"], b).tobytes() == before.tobytes()


def test_cross_encoder_class_and_cli_in_f16(tmp_path):
    """CrossEncoder(ckpt, precision="f16") and rerank.py --teacher_precision=fp16 as a child process: the filed scores are
    the class's f16 scores on the same tokenised pairs, and not those of an fp32 run."""
    from transformers import AutoTokenizer
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    import xenc_ref as ref
    fx = href.load("x1")
    ckpt = ref.write_checkpoint(fx, str(tmp_path / "teacher"))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(5, 200)]
    with open(os.path.join(ckpt, "vocab.txt"), "w") as f:
        f.write("\n".join(words) + "\n")
    rng = np.random.default_rng(5)
    text = lambda n: " ".join(f"w{int(i)}" for i in rng.integers(5, 200, size=n))  # noqa: E731
    coll = tmp_path / "collection"; coll.mkdir()
    docs = {f"{100 + i}": text(int(rng.integers(3, 40))) for i in range(12)}
    queries = {f"{i}": text(int(rng.integers(2, 9))) for i in range(5)}
    with open(coll / "raw.tsv", "w") as f:
        f.writelines(f"{k}\t{v}\n" for k, v in docs.items())
    with open(tmp_path / "queries.tsv", "w") as f:
        f.writelines(f"{k}\t{v}\n" for k, v in queries.items())
    out = tmp_path / "out"; out.mkdir()
    dk = list(docs)
    data = {q: {f"{3 * j}_{int(q) + j}": [dk[(int(q) * 5 + 3 * j + t) % 12] for t in range(1 + (int(q) + j) % 3)]
                for j in range(3)} for q in queries}
    with open(out / "qid_smtid_docids.train.json", "w") as f:
        json.dump(data, f)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "t5_pretrainer.rerank", "--task=cross_encoder_rerank_for_qid_smtid_docids",
                        f"--model_name_or_path={ckpt}", f"--collection_path={coll}", f"--train_queries_path={tmp_path / 'queries.tsv'}",
                        f"--qid_smtid_docids_path={out / 'qid_smtid_docids.train.json'}", "--batch_size=7", "--max_length=32",
                        "--local_rank=0", "--teacher_precision=fp16"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("teacher precision:  fp16") == 1
    with open(out / "qid_smtid_docids_teacher_score_0.train.json") as f:
        filed = {(q, s, d): sc for q, by in json.load(f).items() for s, rows in by.items() for d, sc in rows}
    trip = sorted((q, s, d) for q, by in data.items() for s, dd in by.items() for d in dd)
    assert len(trip) > 10 and set(filed) == set(trip)
    tok = AutoTokenizer.from_pretrained(ckpt)
    kw = tok([queries[q] for q, _, _ in trip], [docs[d] for _, _, d in trip], padding=True, truncation="longest_first",
             return_attention_mask=True, return_tensors="pt", max_length=32)
    ce = CrossEncoder(ckpt, precision="f16").to(0)
    assert ce.precision == "f16" and ce._model.precision == "f16"
    in_half = ce.rerank_forward(kw)["scores"].cpu().numpy()
    in_full = ce.set_precision("f32").rerank_forward(kw)["scores"].cpu().numpy()
    assert ce._model.precision == "f32"
    got = np.array([filed[t] for t in trip])
    # the child scored batches of 7, here all pairs are one batch: rows do not mix, but the GEMM tile may follow T
    assert np.abs(in_half - got).max() <= 1e-6
    assert np.abs(in_full - got).max() > 1e-5
    assert np.std(in_half) > 0.01
