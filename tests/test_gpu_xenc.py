"""-m gpu: the cross-encoder teacher on the device. ``engine.xenc_score`` and ``CrossEncoder.rerank_forward`` against the HF
fp64 logits of the fixtures (tests/golden/make_golden_xenc.py) within 1e-5 absolute — the per-value bar of
tests/test_callers_golden.py; CPU fp32 itself sits at <= 5.5e-7 on these shapes — run-to-run bits, batch composition, the
refusals of rpr_xenc_score, and preprocess -> rerank task 1 (a child process) -> task 2 end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xenc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
CASES = [(m, k) for m, keys in ref.FIXTURES.items() for k in keys]


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


@pytest.fixture(scope="module")
def models(ctx):
    from ripor_amd import engine as E
    return {m: E.XencModel(ctx, ref.load_fixture(m)["weights"], ref.load_fixture(m)["cfg"]) for m in ref.FIXTURES}


def _score(model, b, rows=slice(None)):
    from ripor_amd import engine as E
    return E.xenc_score(model, torch.from_numpy(b["ids"][rows]), torch.from_numpy(b["types"][rows]),
                        torch.from_numpy(b["mask"][rows])).cpu().numpy()


@pytest.mark.parametrize("model,key", CASES)
def test_engine_matches_hf_fp64(models, model, key):
    b = ref.load_fixture(model)["batches"][key]
    got = _score(models[model], b)
    err = np.abs(got.astype(np.float64) - b["fp64"]).max()
    print(f"[xenc] {model}/{key}: bz {len(got)}, max |hip - fp64| {err:.3e}")
    assert got.shape == b["fp64"].shape and np.isfinite(got).all()
    assert err <= TOL


@pytest.mark.parametrize("model", list(ref.FIXTURES))
def test_cross_encoder_class_matches_hf_fp64(tmp_path, model):
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    fx = ref.load_fixture(model)
    ce = CrossEncoder.from_pretrained(ref.write_checkpoint(fx, str(tmp_path / model), with_position_ids=True)).to(0).eval()
    for key, b in fx["batches"].items():
        kw = {"input_ids": torch.from_numpy(b["ids"]).long(), "token_type_ids": torch.from_numpy(b["types"]).long(),
              "attention_mask": torch.from_numpy(b["mask"]).long()}
        if key in ("b", "f"):   # device tensors, as the reference's kwargs_to_cuda hands them over
            kw = {k: v.cuda() for k, v in kw.items()}
        got = ce.rerank_forward(kw)["scores"]
        assert got.is_cuda and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - b["fp64"]).max()
        print(f"[xenc] CrossEncoder {model}/{key}: max |hip - fp64| {err:.3e}")
        assert err <= TOL
        assert torch.equal(ce(qd_kwargs=kw), got)
    with pytest.raises(ValueError, match="column 0"):
        bad = fx["batches"]["f"]["mask"].copy(); bad[2, 0] = 0
        ce.rerank_forward({"input_ids": torch.from_numpy(fx["batches"]["f"]["ids"]), "attention_mask": torch.from_numpy(bad)})


@pytest.mark.parametrize("model,key", [("x1", "b"), ("x2", "c"), ("x1", "e")])
def test_same_call_twice_same_bits(models, model, key):
    b = ref.load_fixture(model)["batches"][key]
    one, two = _score(models[model], b), _score(models[model], b)
    assert one.tobytes() == two.tobytes()


@pytest.mark.parametrize("model,key,cut", [("x1", "b", 6), ("x2", "b", 9), ("x1", "d", 33), ("x2", "f", 1)])
def test_whole_batch_equals_two_halves(models, model, key, cut):
    b = ref.load_fixture(model)["batches"][key]
    whole = _score(models[model], b)
    halves = np.concatenate([_score(models[model], b, slice(0, cut)), _score(models[model], b, slice(cut, None))])
    assert np.abs(whole.astype(np.float64) - halves).max() <= TOL   # the GEMM tile follows T: the bits may differ


def test_refusals_leave_the_ctx_usable(ctx, models):
    from ripor_amd import engine as E
    from ripor_amd import _lib
    lib = ctx.lib
    dev = ctx.device
    out = torch.zeros(4, dtype=torch.float32, device=dev)
    z = torch.zeros(600, dtype=torch.int32, device=dev)

    def call(model, seq_off):
        off = np.asarray(seq_off, dtype=np.int32)
        return lib.rpr_xenc_score(ctx.handle, model.handle, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                  off.ctypes.data_as(C.POINTER(C.c_int32)), len(off) - 1, out.data_ptr(), None)

    cfg48 = E.XencConfig(vocab_size=10, hidden=96, layers=1, heads=2, d_ff=96, max_pos=16, type_vocab=2)
    g = torch.Generator().manual_seed(0)
    m48 = E.XencModel(ctx, {k: torch.randn(s, generator=g) for k, s in E.xenc_weight_shapes(cfg48).items()}, cfg48)
    assert call(m48, [0, 4]) == -1 and b"32 or 64" in lib.rpr_last_error()          # RPR_ERR_INVALID: a 48-dim head
    assert call(models["x1"], [0, 513]) == -1 and b"longer" in lib.rpr_last_error()  # 513 tokens
    assert call(models["x2"], [0, 193]) == -1                                        # beyond max_pos = 192
    assert call(models["x1"], [0, 3, 3, 5]) == -1 and b"empty" in lib.rpr_last_error()
    assert call(models["x1"], [0, 3, 5]) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.RiporHipError):
        E.xenc_score_packed(models["x1"], z[:5], z[:5], z[:5], np.array([0, 5, 5], dtype=np.int32))
    with pytest.raises(ValueError, match="vocabulary"):
        E.xenc_score(models["x1"], torch.full((1, 3), 200), None, torch.ones((1, 3), dtype=torch.long))
    b = ref.load_fixture("x1")["batches"]["b"]
    assert np.abs(_score(models["x1"], b).astype(np.float64) - b["fp64"]).max() <= TOL


def test_end_to_end_preprocess_rerank_merge(tmp_path):
    """rank data -> preprocess -> task 1 as a child process on one rank -> task 2; every (qid, smtid, docid) once, scores equal
    the class on the same tokenised pairs."""
    from transformers import AutoTokenizer
    from ripor_amd import rerank as R
    from ripor_amd.aq_preprocess.argparse_from_qid_smtid_rank_to_qid_smtid_docids import main as preprocess
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    fx = ref.load_fixture("x1")
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
    rankdata = {q: {f"{3 * j}_{int(q) + j}": {dk[(int(q) * 5 + 3 * j + t) % 12]: float(10 - t) for t in range((int(q) + j) % 4)}
                    for j in range(3)} for q in queries}
    with open(out / "qid_smtid_rankdata.json", "w") as f:
        json.dump(rankdata, f)
    preprocess(["--root_dir", str(out)])
    want = {(q, s, d) for q, by in rankdata.items() for s, dd in by.items() for d in dd}
    assert len(want) > 10
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "t5_pretrainer.rerank", "--task=cross_encoder_rerank_for_qid_smtid_docids",
                        f"--model_name_or_path={ckpt}", f"--collection_path={coll}", f"--train_queries_path={tmp_path / 'queries.tsv'}",
                        f"--qid_smtid_docids_path={out / 'qid_smtid_docids.train.json'}", "--batch_size=7", "--max_length=32",
                        "--local_rank=0"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(out / "qid_smtid_docids_teacher_score_0.train.json")
    R.main(["--task=cross_encoder_rerank_for_qid_smtid_docids_2", f"--out_dir={out}"])
    assert sorted(os.listdir(out)) == sorted(["qid_smtid_rankdata.json", "qid_smtid_docids.train.json", R.MERGED_NAME])
    with open(out / R.MERGED_NAME) as f:
        merged = json.load(f)
    got = [(q, s, d) for q, by in merged.items() for s, rows in by.items() for d, _ in rows]
    assert len(got) == len(set(got)) and set(got) == want
    tok = AutoTokenizer.from_pretrained(ckpt)
    ce = CrossEncoder(ckpt).to(0)
    trip = sorted(want)
    kw = tok([queries[q] for q, _, _ in trip], [docs[d] for _, _, d in trip], padding=True, truncation="longest_first",
             return_attention_mask=True, return_tensors="pt", max_length=32)
    direct = ce.rerank_forward(kw)["scores"].cpu().numpy()
    filed = {(q, s, d): sc for q, by in merged.items() for s, rows in by.items() for d, sc in rows}
    assert np.abs(direct - np.array([filed[t] for t in trip])).max() <= TOL
    assert np.std(direct) > 0.01
