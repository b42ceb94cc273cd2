"""Docid creation (residual quantization) without a GPU: the numpy restatement of the algorithm, the C ABI surface, the
mmap_2 layout, the docid_to_smtid.json writer and the embed-layer change."""
import ctypes as C
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ref_level_mse_does_not_increase():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3000, 32)).astype(np.float32)
    books, mse, S, init = rq_ref.train(X, M=4, K=8, niter=3)
    assert books.shape == (4, 8, 32) and books.dtype == np.float32
    assert len(S) == min(3000, 256 * 8) and (np.diff(S) > 0).all()
    total = float((X[S].astype(np.float64) ** 2).sum(1).mean())
    assert mse[0] < total
    assert (np.diff(mse) <= 1e-9 * mse[0]).all(), mse
    codes, enc_mse = rq_ref.encode(X[S], books)
    np.testing.assert_allclose(enc_mse, mse, rtol=1e-9)


def test_ref_tie_rule_and_empty_cluster():
    C0 = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [50.0, 50.0]], dtype=np.float32)   # 0 == 1, 3 is never chosen
    R = np.array([[1.0, 0.1], [0.9, 0.0], [0.0, 2.0]], dtype=np.float32)
    code = rq_ref.assign(R, C0)
    assert code.tolist() == [0, 0, 2]
    C1 = rq_ref.update(R, code, C0)
    np.testing.assert_array_equal(C1[1], C0[1])   # no rows: keeps its value
    np.testing.assert_array_equal(C1[3], C0[3])
    np.testing.assert_allclose(C1[0], [0.95, 0.05], rtol=1e-6)
    assert C1.dtype == np.float32


def test_ref_plan_is_the_engines():
    from ripor_amd import engine as E
    S, init = E.rq_training_plan(5000, 3, 64)
    S2, init2 = rq_ref.plan(5000, 3, 64)
    np.testing.assert_array_equal(S, S2)
    np.testing.assert_array_equal(init, init2)
    assert init.dtype == np.int32 and init.shape == (3, 64)


def test_rq_symbols_exported_and_declared():
    import __graft_entry__ as ge
    from ripor_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    for name in ("rpr_rq_train", "rpr_rq_encode"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint " + name + r"\(", hdr), name
    lib = C.CDLL(ge.LIB)
    assert hasattr(lib, "rpr_rq_train") and hasattr(lib, "rpr_rq_encode")
    assert _lib.ABI_VERSION == 5


def test_rq_entry_points_fail_cleanly_without_a_context():
    from ripor_amd import _lib
    lib = _lib.load()
    init = (C.c_int32 * 64)()
    mse = (C.c_double * 1)()
    assert lib.rpr_rq_train(None, None, 100, 32, 1, 64, 1, init, None, mse, None) == -1
    assert lib.rpr_rq_encode(None, None, 100, 32, None, 1, 64, None, None, None) == -1
    assert b"NULL" in lib.rpr_last_error()


def _write_chunks(d, nranks=2, num_chunks=3, dim=32, seed=0):
    rng = np.random.default_rng(seed)
    embs, ids = [], []
    nid = 0
    for r in range(nranks):
        for c in range(num_chunks):
            n = 5 + 3 * r + c
            e = rng.standard_normal((n, dim)).astype(np.float16 if (r + c) % 2 else np.float32)
            i = np.arange(nid, nid + n, dtype=np.int64) * 7
            nid += n
            np.save(os.path.join(d, f"embs_{r}_{c}.npy"), e)
            np.save(os.path.join(d, f"ids_{r}_{c}.npy"), i)
            embs.append(e.astype(np.float32))
            ids.append(i)
    with open(os.path.join(d, "plan.json"), "w") as f:
        json.dump({"nranks": nranks, "num_chunks": num_chunks, "index_path": os.path.join(d, "model.index")}, f)
    return np.concatenate(embs), np.concatenate(ids)


def test_mmap_2_layout(tmp_path):
    from ripor_amd import evaluate
    from ripor_amd.tasks.rq_indexer import load_doc_embeds
    d = str(tmp_path / "mmap")
    os.makedirs(d)
    embs, ids = _write_chunks(d)
    evaluate.main(["--task=mmap_2", f"--index_dir={d}", f"--mmap_dir={d}"])
    raw = np.fromfile(os.path.join(d, "doc_embeds.mmap"), dtype=np.float32)
    np.testing.assert_array_equal(raw.reshape(embs.shape), embs)
    with open(os.path.join(d, "text_ids.tsv")) as f:
        assert [int(x) for x in f.read().split()] == ids.tolist()
    with open(os.path.join(d, "meta.pkl"), "rb") as f:
        meta = pickle.load(f)
    assert meta["num_embeddings"] == len(ids)
    np.testing.assert_array_equal(meta["text_ids"], ids)
    assert sorted(os.listdir(d)) == ["doc_embeds.mmap", "meta.pkl", "plan.json", "text_ids.tsv"]
    np.testing.assert_array_equal(load_doc_embeds(d), embs)


def test_other_dense_tasks_stay_refused():
    from ripor_amd import evaluate
    for task in ("mmap", "index", "aq_evaluate", "retrieve", "aq_to_flat_index_search_evaluate"):
        with pytest.raises(ValueError, match="is not valid"):
            evaluate.main([f"--task={task}"])


def test_docid_to_smtid_writer_reads_back(tmp_path):
    from ripor_amd import engine as E
    from ripor_amd.aq_preprocess.create_customized_smtid_file import smtid_stats, write_docid_to_smtid
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 256, size=(50, 6)).astype(np.uint16)
    codes[7] = codes[3]
    docids = [f"d{i}" for i in range(50)]
    path = str(tmp_path / "docid_to_smtid.json")
    write_docid_to_smtid(path, docids, codes)
    with open(path) as f:
        obj = json.load(f)
    assert list(obj.keys()) == docids
    assert obj["d0"] == [-1] + codes[0].tolist()
    got_ids, got = E.read_docid_to_smtid(path)
    assert got_ids == docids
    np.testing.assert_array_equal(got, codes)
    st = smtid_stats(codes)
    assert st["total_smtid"] == 49 and st["unique_smtid_num"] == 48


def test_change_customized_embed_layer(tmp_path):
    from ripor_amd.aq_preprocess import change_customized_embed_layer as ch
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=4, V=64, enc_layers=1, d_ff=64, vocab_size=64)
    model_dir = str(tmp_path / "model")
    T5SeqAQEncoder.from_synthetic(dims).save_pretrained(os.path.join(model_dir, "checkpoint"))
    with open(os.path.join(model_dir, "checkpoint", "spiece.model"), "wb") as f:
        f.write(b"tok")
    M, K, d = 6, 128, dims.d_model
    books = np.random.default_rng(2).standard_normal((M, K, d)).astype(np.float32)
    os.makedirs(os.path.join(model_dir, "aq_index"))
    np.save(os.path.join(model_dir, "aq_index", "rq_codebooks.npy"), books)
    with open(os.path.join(model_dir, "aq_index", "rq.json"), "w") as f:
        json.dump(dict(M=M, K=K, d=d), f)
    out = ch.main([f"--model_dir={model_dir}", f"--K={K}"])
    assert out == os.path.join(model_dir, "no_share_checkpoint")
    with open(os.path.join(out, "config.json")) as f:
        cfg = json.load(f)
    assert cfg["decoder_vocab_sizes"] == [K] * M and cfg["shared_output_input_embeds"] is False
    assert open(os.path.join(out, "spiece.model"), "rb").read() == b"tok"
    sd = torch.load(os.path.join(out, "pytorch_model.bin"), weights_only=True)
    for i in range(M):
        assert tuple(sd[f"list_decoder_embeds.{i}.weight"].shape) == (K, d)
        np.testing.assert_array_equal(sd[f"list_output_embeds.{i}.weight"].numpy(), books[i])
    assert f"list_output_embeds.{M}.weight" not in sd
    emb = sd["list_decoder_embeds.0.weight"]
    assert abs(float(emb.mean())) < 0.02 and abs(float(emb.std()) - 1.0) < 0.02
    m = T5SeqAQEncoder.from_pretrained(out)
    assert m.config.decoder_vocab_sizes == [K] * M and m.config.max_decoder_length == M
    np.testing.assert_array_equal(m.base_model.state_dict()["list_output_embeds.2.weight"].numpy(), books[2])
    with pytest.raises(ValueError):
        ch.main([f"--model_dir={model_dir}", "--K=256"])


def test_aliases_and_file_path_entry():
    import importlib
    for m in ("create_customized_smtid_file", "change_customized_embed_layer", "change_embed_layer"):
        mod = importlib.import_module(f"t5_pretrainer.aq_preprocess.{m}")
        assert callable(mod.main)
    src = open(os.path.join(REPO, "t5_pretrainer", "aq_preprocess", "create_customized_smtid_file.py")).read()
    assert '__name__ == "__main__"' in src
