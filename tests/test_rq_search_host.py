"""Host side of the residual-quantizer search (aq_evaluate): the numpy restatement itself, the ABI surface, the CLI flags,
the run.json writer over a stubbed engine, and the errors for a missing or mismatched index. No GPU."""
import json
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_search_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_small_case_by_hand():
    q = np.zeros((1, 8), dtype=np.float32); q[0, :2] = [1, 2]
    books = np.zeros((2, 4, 8), dtype=np.float32)
    books[0, :, 0] = [0, 1, 2, 3]          # LUT level 0 = 0 1 2 3
    books[1, :, 1] = [0, -1, 1, 0]         # LUT level 1 = 0 -2 2 0
    for dt in (np.float32, np.float64):
        np.testing.assert_array_equal(ref.lut(q, books, dt)[0], [[0, 1, 2, 3], [0, -2, 2, 0]])
    codes = np.array([[3, 1], [1, 0], [0, 3], [1, 3], [2, 2]])           # scores 1 1 0 1 4
    idx, sc = ref.search(q, books, codes, 7)
    np.testing.assert_array_equal(idx[0], [4, 0, 1, 3, 2, -1, -1])       # ties to the smaller row, -1 past N
    np.testing.assert_array_equal(sc[0], [4, 1, 1, 1, 0, -np.inf, -np.inf])
    assert idx.dtype == np.int64 and sc.dtype == np.float32


def test_restatement_f32_chain_is_fp32_and_close_to_fp64():
    rng = np.random.default_rng(0)
    q, books = rng.standard_normal((3, 64)).astype(np.float32), rng.standard_normal((2, 8, 64)).astype(np.float32)
    codes = rng.integers(0, 8, size=(50, 2))
    a, b = ref.lut(q, books, np.float32), ref.lut(q, books, np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64
    s32, s64 = ref.scores(a, codes), ref.scores(b, codes)
    assert (np.abs(s32 - s64) <= ref.rounding_bound(q, books, codes)).all()


def test_negative_zero_ties_with_zero():
    sc = np.array([[-0.0, 0.0, -0.0, 1.0]], dtype=np.float32)
    idx, _ = ref.topk(sc, 4)
    np.testing.assert_array_equal(idx[0], [3, 0, 1, 2])


def test_signatures_in_header_and_binding():
    from ripor_amd import _lib
    header = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    for name, nargs in (("rpr_embed", 8), ("rpr_rq_search", 13)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and m.group(1).count(",") + 1 == nargs
    assert _lib.ABI_VERSION == 5


def test_cli_accepts_the_aq_evaluate_flags():
    from ripor_amd import evaluate as ev
    a = ev.get_args(["--task=aq_evaluate", "--pretrained_path=/m", "--mmap_dir=/x/mmap", "--index_dir=/x/aq_index", "--out_dir=/x/out",
                     "--q_collection_paths=" + json.dumps(["/q/dev"]), "--eval_qrel_path=" + json.dumps(["/q/dev_qrel.json"]),
                     "--eval_metric=" + json.dumps([["mrr_10", "recall"]])])
    assert (a.task, a.mmap_dir, a.index_dir, a.out_dir) == ("aq_evaluate", "/x/mmap", "/x/aq_index", "/x/out")
    assert ev._list_flag(a.q_collection_paths) == ["/q/dev"]
    assert (ev.AQ_EVALUATE_TOPK, ev.AQ_EVALUATE_BATCH) == (200, 128)
    assert callable(ev.aq_evaluate)


def _index(tmp_path, N=7, d=32, M=2, K=64):
    mmap_dir, index_dir = str(tmp_path / "mmap"), str(tmp_path / "aq_index")
    os.makedirs(mmap_dir); os.makedirs(index_dir)
    X = np.arange(N * d, dtype=np.float32).reshape(N, d)
    X.tofile(os.path.join(mmap_dir, "doc_embeds.mmap"))
    with open(os.path.join(mmap_dir, "text_ids.tsv"), "w") as f:
        for i in range(N):
            f.write(f"{1000 + i}\n")
    pickle.dump({"num_embeddings": N}, open(os.path.join(mmap_dir, "meta.pkl"), "wb"))
    np.save(os.path.join(index_dir, "rq_codebooks.npy"), np.zeros((M, K, d), dtype=np.float32))
    json.dump(dict(M=M, K=K, d=d), open(os.path.join(index_dir, "rq.json"), "w"))
    return mmap_dir, index_dir


class _StubModel:
    """What search_index touches of a T5SeqAQEncoder on a device."""

    def __init__(self, d):
        em = types.SimpleNamespace(d_model=d, ctx=types.SimpleNamespace(device=torch.device("cpu")))
        self.base_model = types.SimpleNamespace(engine_model=lambda: em)


def test_search_index_writes_the_reference_run_layout(tmp_path, monkeypatch):
    from ripor_amd import engine as E
    from ripor_amd.tasks import rq_indexer
    mmap_dir, index_dir = _index(tmp_path)
    seen = {}

    def fake_encode(ctx, x, books, chunk_rows=0):
        seen["encoded"] = x.shape
        return np.zeros((x.shape[0], books.shape[0]), dtype=np.uint16), np.zeros(books.shape[0])

    def fake_embed(model, ids, mask):
        return torch.zeros((ids.shape[0], 32))

    def fake_search(ctx, q, books, codes, topk):
        seen["topk"] = topk
        assert codes.shape == (7, 2)
        idx = torch.tensor([[2, 0, -1]] * q.shape[0])
        return idx, torch.tensor([[1.5, 0.25, float("-inf")]] * q.shape[0])

    monkeypatch.setattr(E, "rq_encode", fake_encode)
    monkeypatch.setattr(E, "embed", fake_embed)
    monkeypatch.setattr(E, "rq_search", fake_search)
    loader = [{"input_ids": torch.zeros((2, 4), dtype=torch.long), "attention_mask": torch.ones((2, 4), dtype=torch.long),
               "id": torch.tensor([900, 901])},
              {"input_ids": torch.zeros((1, 4), dtype=torch.long), "attention_mask": torch.ones((1, 4), dtype=torch.long),
               "id": torch.tensor([902])}]
    out_dir = str(tmp_path / "out" / "MSMARCO")
    rq_indexer.search_index(_StubModel(32), loader, mmap_dir, index_dir, out_dir, topk=3)
    run = json.load(open(os.path.join(out_dir, "run.json")))
    assert run == {q: {"1002": 1.5, "1000": 0.25} for q in ("900", "901", "902")}
    assert seen == {"encoded": (7, 32), "topk": 3}


@pytest.mark.parametrize("missing", ["rq.json", "rq_codebooks.npy", "text_ids.tsv"])
def test_missing_index_files_are_a_clear_error(tmp_path, missing):
    from ripor_amd.tasks import rq_indexer
    mmap_dir, index_dir = _index(tmp_path)
    os.remove(os.path.join(mmap_dir if missing == "text_ids.tsv" else index_dir, missing))
    with pytest.raises(ValueError, match=re.escape(missing)):
        rq_indexer.search_index(_StubModel(32), [], mmap_dir, index_dir, str(tmp_path / "out"))


def test_dimension_mismatch_is_a_clear_error(tmp_path):
    from ripor_amd.tasks import rq_indexer
    mmap_dir, index_dir = _index(tmp_path)
    with pytest.raises(ValueError, match="d_model is 64"):
        rq_indexer.search_index(_StubModel(64), [], mmap_dir, index_dir, str(tmp_path / "out"))


def test_main_dispatches_aq_evaluate(tmp_path):
    from ripor_amd import evaluate as ev
    with pytest.raises(ValueError, match="rq.json"):   # refused for the missing index, not as an unknown task
        ev.main(["--task=aq_evaluate", f"--pretrained_path={tmp_path}", f"--mmap_dir={tmp_path}", f"--index_dir={tmp_path}",
                 f"--out_dir={tmp_path}/out"])
    with pytest.raises(ValueError, match="--mmap_dir, --index_dir"):
        ev.main(["--task=aq_evaluate", f"--pretrained_path={tmp_path}", f"--out_dir={tmp_path}/out"])
