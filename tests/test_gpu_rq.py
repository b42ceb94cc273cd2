"""-m gpu: docid creation on the device (rpr_rq_train / rpr_rq_encode) against the numpy restatement tests/rq_ref.py, its
determinism and edge cases, and the reference's all_aq_pipline steps from mmap_2 to the embed-layer change, followed by a
retrieval over the docids they produced."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


def _train(ctx, X, M, K, niter=rq_ref.NITER):
    from ripor_amd import engine as E
    S, init = E.rq_training_plan(X.shape[0], M, K)
    books, mse = E.rq_train(ctx, torch.from_numpy(np.ascontiguousarray(X[S])).cuda(), M, K, init, niter=niter)
    return books, mse, S, init


def _hierarchy(N, d, M, K, seed, scales):
    """Every level a mixture of K well separated centres, each level on a much smaller scale than the one before."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, d), dtype=np.float64)
    for m in range(M):
        centres = rng.standard_normal((K, d)) * scales[m]
        X += centres[rng.integers(0, K, size=N)]
    X += rng.standard_normal((N, d)) * scales[-1] * 0.01
    return X.astype(np.float32)


def test_separable_mixture_equals_reference(ctx):
    M, K, d = 3, 64, 64
    X = _hierarchy(6000, d, M, K, seed=11, scales=[100.0, 10.0, 1.0])
    books, mse, S, init = _train(ctx, X, M, K, niter=10)
    ref_books, ref_mse = rq_ref.train_on(X[S], init, K, niter=10)
    b = books.cpu().numpy()
    for m in range(M):
        err = np.abs(b[m] - ref_books[m]).max() / np.abs(ref_books[m]).max()
        assert err < 1e-5, (m, err)
    np.testing.assert_allclose(mse, ref_mse, rtol=1e-5)
    from ripor_amd import engine as E
    codes, _ = E.rq_encode(ctx, X, books)
    ref_codes, _ = rq_ref.encode(X, ref_books)
    np.testing.assert_array_equal(codes.astype(np.int64), ref_codes)


def test_gaussian_level0_and_mse(ctx):
    from ripor_amd import engine as E
    M, K, d, N = 4, 256, 768, 20011
    X = np.random.default_rng(5).standard_normal((N, d)).astype(np.float32)
    books, mse, S, init = _train(ctx, X, M, K)
    assert len(S) == N
    b = books.cpu().numpy()
    codes, enc_mse = E.rq_encode(ctx, X[S], books)
    # level 0: the fp64 argmin over the device's own codebook wherever the top-2 gap is clear
    sc = rq_ref.scores(X[S], b[0])
    top2 = np.sort(sc, axis=1)[:, :2]
    scale = float((X[S].astype(np.float64) ** 2).sum(1).mean())
    ok = (top2[:, 1] - top2[:, 0]) > 1e-4 * scale
    assert ok.mean() >= 0.99, ok.mean()
    np.testing.assert_array_equal(codes[ok, 0].astype(np.int64), np.argmin(sc, axis=1)[ok])
    assert (np.diff(mse) <= 0).all(), mse
    assert mse[0] < scale
    # the training's level sums are those of the encoder over the training rows (same kernel, same fixed order)
    np.testing.assert_allclose(mse, enc_mse, rtol=1e-12)
    _, ref_mse = rq_ref.encode(X[S], b)
    np.testing.assert_allclose(mse, ref_mse, rtol=1e-5)


def test_determinism_and_chunking(ctx):
    from ripor_amd import engine as E
    M, K, d, N = 3, 128, 256, 9001
    X = np.random.default_rng(9).standard_normal((N, d)).astype(np.float32)
    b1, m1, _, _ = _train(ctx, X, M, K, niter=8)
    b2, m2, _, _ = _train(ctx, X, M, K, niter=8)
    assert torch.equal(b1, b2) and (m1 == m2).all()
    whole, mw = E.rq_encode(ctx, torch.from_numpy(X).cuda(), b1)
    chunked, mc = E.rq_encode(ctx, X, b1, chunk_rows=2000)
    np.testing.assert_array_equal(whole, chunked)
    np.testing.assert_allclose(mw, mc, rtol=1e-12)
    again, _ = E.rq_encode(ctx, torch.from_numpy(X).cuda(), b1, chunk_rows=777)
    np.testing.assert_array_equal(whole, again)


@pytest.mark.parametrize("K,d", [(64, 64), (1024, 64), (192, 96)])
def test_codebook_sizes(ctx, K, d):
    M, N = 2, 5000
    X = np.random.default_rng(K + d).standard_normal((N, d)).astype(np.float32)
    books, mse, S, init = _train(ctx, X, M, K, niter=4)
    assert books.shape == (M, K, d) and np.isfinite(mse).all() and mse[1] <= mse[0]
    from ripor_amd import engine as E
    codes, enc = E.rq_encode(ctx, X[S], books)
    assert int(codes.max()) < K
    np.testing.assert_allclose(mse, enc, rtol=1e-12)
    sc = rq_ref.scores(X[S], books[0].cpu().numpy())
    top2 = np.sort(sc, axis=1)[:, :2]
    ok = (top2[:, 1] - top2[:, 0]) > 1e-4 * float((X[S].astype(np.float64) ** 2).sum(1).mean())
    np.testing.assert_array_equal(codes[ok, 0].astype(np.int64), np.argmin(sc, axis=1)[ok])


def test_duplicate_rows_empty_clusters(ctx):
    M, K, d = 2, 64, 64
    base = np.random.default_rng(4).standard_normal((10, d)).astype(np.float32) * 5
    X = np.repeat(base, 64, axis=0)     # 640 rows, 10 distinct: most centroids start as copies and lose every row
    books, mse, S, init = _train(ctx, X, M, K, niter=5)
    ref_books, ref_mse = rq_ref.train_on(X[S], init, K, niter=5)
    np.testing.assert_array_equal(books.cpu().numpy(), ref_books)
    assert mse[0] == 0.0
    from ripor_amd import engine as E
    codes, _ = E.rq_encode(ctx, X, books)
    ref_codes, _ = rq_ref.encode(X, ref_books)
    np.testing.assert_array_equal(codes.astype(np.int64), ref_codes)


def test_invalid_shapes_refused(ctx):
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    x = torch.zeros((2048, 96), device="cuda")
    init = np.zeros((1, 64), dtype=np.int32)
    with pytest.raises(RiporHipError, match="multiple of 32"):
        E.rq_train(ctx, x[:, :48].contiguous(), 1, 64, init)
    with pytest.raises(RiporHipError, match="multiple of 64"):
        E.rq_train(ctx, x, 1, 96, np.zeros((1, 96), dtype=np.int32))
    with pytest.raises(RiporHipError, match="at most 1024"):
        E.rq_train(ctx, x, 1, 2048, np.zeros((1, 2048), dtype=np.int32))
    with pytest.raises(RiporHipError, match="fewer training rows"):
        E.rq_train(ctx, x[:32].contiguous(), 1, 64, init)
    with pytest.raises(RiporHipError, match="init_idx"):
        E.rq_train(ctx, x, 1, 64, np.full((1, 64), 5000, dtype=np.int32))
    with pytest.raises(RiporHipError, match="multiple of 64"):
        E.rq_encode(ctx, x, torch.zeros((1, 100, 96), device="cuda"))


def test_pipeline_mmap_2_to_embed_layer_then_retrieve(tmp_path):
    from test_gpu_cli import _make_world, _run
    from ripor_amd import engine as E
    root = str(tmp_path / "model")
    ckpt, _, qdir, _, queries, dims = _make_world(root)
    M, bits, N, d = len(dims.decoder_vocab_sizes), 8, 3000, dims.d_model
    mmap_dir, index_dir = os.path.join(root, "mmap"), os.path.join(root, "aq_index")
    os.makedirs(mmap_dir)
    X = _hierarchy(N, d, 3, 16, seed=3, scales=[4.0, 2.0, 1.0])
    lo = 0
    for r in range(2):
        for c in range(2):
            n = [700, 800, 650, 850][2 * r + c]
            np.save(os.path.join(mmap_dir, f"embs_{r}_{c}.npy"), X[lo:lo + n])
            np.save(os.path.join(mmap_dir, f"ids_{r}_{c}.npy"), np.arange(lo, lo + n) + 5000)
            lo += n
    json.dump({"nranks": 2, "num_chunks": 2, "index_path": ""}, open(os.path.join(mmap_dir, "plan.json"), "w"))
    _run(["-m", "t5_pretrainer.evaluate", "--task=mmap_2", f"--index_dir={mmap_dir}", f"--mmap_dir={mmap_dir}"])
    out = _run(["-m", "t5_pretrainer.evaluate", "--task=aq_index", f"--num_subvectors_for_pq={M}", f"--codebook_bits={bits}",
                f"--index_dir={index_dir}", f"--mmap_dir={mmap_dir}"])
    assert "[level 0]" in out
    info = json.load(open(os.path.join(index_dir, "rq.json")))
    assert (info["M"], info["K"], info["d"], info["n_train"]) == (M, 256, d, N)
    assert not os.path.exists(os.path.join(index_dir, "model.index"))
    out = _run([os.path.join("t5_pretrainer", "aq_preprocess", "create_customized_smtid_file.py"), f"--model_dir={root}",
                f"--M={M}", f"--bits={bits}"])
    assert "percentage of smtid is unique" in out
    d2s_path = os.path.join(root, "aq_smtid", "docid_to_smtid.json")
    d2s = json.load(open(d2s_path))
    assert list(d2s) == [str(i + 5000) for i in range(N)]
    assert all(len(v) == M + 1 and v[0] == -1 for v in d2s.values())
    assert os.path.exists(os.path.join(root, "aq_smtid", "list_smtid_to_nextids.rprtrie"))
    books = np.load(os.path.join(index_dir, "rq_codebooks.npy"))
    ref_codes, _ = rq_ref.encode(X, books)
    got = np.asarray([v[1:] for v in d2s.values()])
    assert (got == ref_codes).mean() > 0.999
    _run(["-m", "t5_pretrainer.aq_preprocess.change_customized_embed_layer", f"--model_dir={root}", "--K=256"])
    new_ckpt = os.path.join(root, "no_share_checkpoint")
    for f in ("spiece.model", "tokenizer_config.json", "config.json", "pytorch_model.bin"):
        assert os.path.exists(os.path.join(new_ckpt, f)), f
    out_dir = os.path.join(root, "out")
    txt = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                "--master-port", "29547", "-m", "t5_pretrainer.evaluate", f"--pretrained_path={new_ckpt}", f"--out_dir={out_dir}",
                "--task=t5seq_aq_retrieve_docids", f"--docid_to_smtid_path={d2s_path}",
                "--q_collection_paths=" + json.dumps([qdir]), "--batch_size=4", f"--max_new_token_for_docid={M}", "--topk=5"])
    assert "trie cache:" in txt
    run = json.load(open(os.path.join(out_dir, "MSMARCO", "run_0.json")))
    assert set(run) == set(queries)
    returned = {docid for docs in run.values() for docid in docs}
    assert returned and returned <= set(d2s)


def test_one_million_rows_32_levels(ctx):
    from ripor_amd import engine as E
    M, K, d, N = 32, 256, 768, 1 << 20
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((N, d), generator=g, device="cuda") * torch.linspace(0.5, 2.0, d, device="cuda")
    S, init = E.rq_training_plan(N, M, K)
    books, mse = E.rq_train(ctx, X[torch.from_numpy(S).cuda()].contiguous(), M, K, init)
    assert books.shape == (M, K, d) and torch.isfinite(books).all()
    assert (np.diff(mse) <= 0).all(), mse
    codes, enc = E.rq_encode(ctx, X, books, chunk_rows=1 << 19)
    assert codes.shape == (N, M) and int(codes.max()) < K
    assert (np.diff(enc) <= 0).all() and enc[-1] < enc[0]
    # all rows (mostly held out of the training sample) are quantised about as well as the training rows
    assert 0.9 * mse[-1] <= enc[-1] <= 1.2 * mse[-1], (enc[-1], mse[-1])
