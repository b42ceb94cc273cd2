"""-m gpu: beam encoding of the residual quantizer on the device (rpr_rq_encode_beam) against the numpy restatement
tests/rq_beam_ref.py: bit for bit on integer-valued input (exact arithmetic, frequent exact ties), the greedy chain at
beam 1, float input, determinism and chunking, refusals, and create_customized_smtid_file --max_beam_size."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_beam_ref  # noqa: E402
import rq_ref  # noqa: E402
from test_rq_beam_host import gaussian_rows, integer_input  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


def _call(ctx, x, books, beam, entry="rpr_rq_encode_beam", fill=None):
    """One raw call of the C entry on device tensors -> (status, codes uint16 [n, M], level_sse float64 [M])."""
    n, d = x.shape
    M, K, _ = books.shape
    codes = torch.zeros((n, M), dtype=torch.int16, device=x.device)
    if fill is not None:
        codes.fill_(fill)
    sse = (C.c_double * M)()
    stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    if entry == "rpr_rq_encode":
        st = ctx.lib.rpr_rq_encode(ctx.handle, x.data_ptr(), n, d, books.data_ptr(), M, K, codes.data_ptr(), sse, stream)
    else:
        st = ctx.lib.rpr_rq_encode_beam(ctx.handle, x.data_ptr(), n, d, books.data_ptr(), M, K, beam, codes.data_ptr(), sse, stream)
    torch.cuda.synchronize()
    return st, codes.cpu().numpy().view(np.uint16), np.asarray(list(sse), dtype=np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# K 64: one 64-wide codeword tile; K 192, d 96: three of them, three k-tiles; K 1024: eight 128-wide tiles. 1000 rows are
# 7 full row tiles and a partial one at level 0 and, from level 1 on, beam * 1000 entries (a multiple of 128 at beam 8).
@pytest.mark.parametrize("K,d,M", [(64, 64, 6), (192, 96, 6), (1024, 64, 2)])
def test_integer_input_bit_for_bit(ctx, K, d, M):
    X, books = integer_input(K=K, d=d, M=M)
    greedy, _ = rq_ref.encode(X, books)
    xd, bd = _dev(X), _dev(books)
    for beam in (2, 5, 8):
        ref_codes, ref_sse = rq_beam_ref.encode(X, books, beam=beam)
        st, codes, sse = _call(ctx, xd, bd, beam)
        assert st == 0
        differ = (codes.astype(np.int64) != ref_codes).any(1)
        print(f"K {K} d {d} M {M} beam {beam}: rows differing from the reference {int(differ.sum())}, from greedy "
              f"{float((ref_codes != greedy).any(1).mean()):.3f}, level_sse {sse.tolist()} reference {ref_sse.tolist()}")
        np.testing.assert_array_equal(codes.astype(np.int64), ref_codes)
        np.testing.assert_array_equal(sse, ref_sse)
        assert (ref_codes != greedy).any(1).mean() > 0.25   # a beam that degrades to greedy cannot pass


@pytest.fixture(scope="module")
def gaussian(ctx):
    from ripor_amd import engine as E
    X = gaussian_rows()
    S, init = E.rq_training_plan(X.shape[0], 8, 64)
    books, _ = E.rq_train(ctx, _dev(X[S]), 8, 64, init, niter=10)
    return X, books


def test_beam_1_is_rpr_rq_encode(ctx, gaussian):
    X, books = gaussian
    xd = _dev(X)
    st0, greedy, greedy_sse = _call(ctx, xd, books, 1, entry="rpr_rq_encode")
    st1, codes, sse = _call(ctx, xd, books, 1)
    assert st0 == 0 and st1 == 0
    np.testing.assert_array_equal(codes, greedy)
    assert (sse == greedy_sse).all(), (sse, greedy_sse)


def test_float_input_beam_5(ctx, gaussian):
    X, books = gaussian
    b = books.cpu().numpy()
    xd = _dev(X)
    st, codes, sse = _call(ctx, xd, books, 5)
    assert st == 0
    ref_codes, ref_sse = rq_beam_ref.encode(X, b, beam=5)
    differ = float((codes.astype(np.int64) != ref_codes).any(1).mean())
    rec = sum(b[m][codes[:, m]].astype(np.float64) for m in range(b.shape[0]))
    final = float(((X.astype(np.float64) - rec) ** 2).sum())
    _, _, greedy_sse = _call(ctx, xd, books, 1, entry="rpr_rq_encode")
    print(f"rows differing from the reference {differ:.5f}; final level_sse {sse[-1]!r}, from the codes {final!r}, "
          f"reference {ref_sse[-1]!r}, greedy {greedy_sse[-1]!r}, ratio to greedy {sse[-1] / greedy_sse[-1]:.4f}")
    assert differ <= 0.01, differ
    np.testing.assert_allclose(sse[-1], final, rtol=1e-5)
    assert sse[-1] < greedy_sse[-1]


def test_determinism_and_chunking(ctx):
    from ripor_amd import engine as E
    M, K, d, N = 3, 128, 256, 9001
    X = np.random.default_rng(9).standard_normal((N, d)).astype(np.float32)
    S, init = E.rq_training_plan(N, M, K)
    books, _ = E.rq_train(ctx, _dev(X[S]), M, K, init, niter=8)
    xd = _dev(X)
    st1, c1, s1 = _call(ctx, xd, books, 5)
    st2, c2, s2 = _call(ctx, xd, books, 5)
    assert st1 == 0 and st2 == 0
    np.testing.assert_array_equal(c1, c2)
    assert (s1 == s2).all()
    chunked, mse = E.rq_encode(ctx, X, books, chunk_rows=777, beam=5)
    np.testing.assert_array_equal(chunked, c1)
    np.testing.assert_allclose(mse * N, s1, rtol=1e-12)
    greedy, _ = E.rq_encode(ctx, xd, books)
    assert (greedy != c1).any()


@pytest.mark.parametrize("beam", [0, 9])
def test_beam_out_of_range_is_refused(ctx, beam):
    x = torch.zeros((256, 64), device="cuda")
    books = torch.zeros((2, 64, 64), device="cuda")
    st, codes, _ = _call(ctx, x, books, beam, fill=-1)
    assert st == -1   # RPR_ERR_INVALID
    msg = ctx.lib.rpr_last_error().decode()
    assert "beam" in msg and "1 .. 8" in msg, msg
    assert (codes == 0xFFFF).all()   # nothing ran
    from ripor_amd import engine as E
    with pytest.raises(ValueError, match="beam"):
        E.rq_encode(ctx, x, books, beam=beam)


def test_create_customized_smtid_file_max_beam_size(ctx, tmp_path, capsys):
    from ripor_amd import engine as E
    from ripor_amd import evaluate
    from ripor_amd.aq_preprocess import create_customized_smtid_file as cc
    from test_gpu_rq import _hierarchy
    root = str(tmp_path / "model")
    M, bits, N, d = 4, 6, 1500, 64
    mmap_dir, index_dir = os.path.join(root, "mmap"), os.path.join(root, "aq_index")
    os.makedirs(mmap_dir)
    X = _hierarchy(N, d, 3, 16, seed=3, scales=[4.0, 2.0, 1.0])
    lo = 0
    for r in range(2):
        for c in range(2):
            n = [350, 400, 325, 425][2 * r + c]
            np.save(os.path.join(mmap_dir, f"embs_{r}_{c}.npy"), X[lo:lo + n])
            np.save(os.path.join(mmap_dir, f"ids_{r}_{c}.npy"), np.arange(lo, lo + n) + 5000)
            lo += n
    with open(os.path.join(mmap_dir, "plan.json"), "w") as f:
        json.dump({"nranks": 2, "num_chunks": 2, "index_path": ""}, f)
    evaluate.main(["--task=mmap_2", f"--index_dir={mmap_dir}", f"--mmap_dir={mmap_dir}"])
    evaluate.main(["--task=aq_index", f"--num_subvectors_for_pq={M}", f"--codebook_bits={bits}", f"--index_dir={index_dir}",
                   f"--mmap_dir={mmap_dir}"])
    capsys.readouterr()
    cc.main([f"--model_dir={root}", f"--M={M}", f"--bits={bits}", "--max_beam_size=5"])
    out = capsys.readouterr().out
    assert f"[level {M - 1}] encoding MSE after the level" in out and "percentage of smtid is unique" in out
    d2s_path = os.path.join(root, "aq_smtid", "docid_to_smtid.json")
    docids, got = E.read_docid_to_smtid(d2s_path)
    assert docids == [str(i + 5000) for i in range(N)]
    books = torch.from_numpy(np.load(os.path.join(index_dir, "rq_codebooks.npy"))).cuda()
    want, _ = E.rq_encode(ctx, X, books, beam=5)
    np.testing.assert_array_equal(got, want)
    greedy, _ = E.rq_encode(ctx, X, books)
    assert (want != greedy).any()
    trie = E.DeviceTrie.load(ctx, os.path.join(root, "aq_smtid", "list_smtid_to_nextids.rprtrie"))
    assert (trie.N, trie.L, trie.V) == (N, M, 1 << bits)
    assert trie.docids() == docids
