"""Beam encoding of the residual quantizer without a GPU: the C ABI surface of rpr_rq_encode_beam, the numpy restatement
tests/rq_beam_ref.py against the greedy one (beam 1) and its gain at beam 5, and the --max_beam_size flag."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_beam_ref  # noqa: E402
import rq_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def integer_input(K=64, d=64, M=6, n=1000):
    """Integer-valued rows and codewords: every order of summation is exact and exact ties are frequent."""
    rng = np.random.default_rng(22)
    X = rng.integers(-8, 9, (n, d)).astype(np.float32)
    books = rng.integers(-4, 5, (M, K, d)).astype(np.float32)
    return X, books


def gaussian_rows():
    return np.random.default_rng(21).standard_normal((3001, 64)).astype(np.float32)


@pytest.fixture(scope="module")
def gaussian_input():
    X = gaussian_rows()
    S, init = rq_ref.plan(X.shape[0], 8, 64)
    books, _ = rq_ref.train_on(X[S], init, 64, niter=10)
    return X, books


def test_symbol_exported_and_declared():
    import __graft_entry__ as ge
    from ripor_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    assert "rpr_rq_encode_beam" in _lib.SIGNATURES
    assert re.search(r"\bint rpr_rq_encode_beam\(", hdr)
    assert hasattr(C.CDLL(ge.LIB), "rpr_rq_encode_beam")
    assert _lib.ABI_VERSION == 5


def test_entry_point_fails_cleanly_without_a_context():
    from ripor_amd import _lib
    lib = _lib.load()
    assert lib.rpr_rq_encode_beam(None, None, 100, 32, None, 1, 64, 5, None, None, None) == -1
    assert b"NULL" in lib.rpr_last_error()


def test_beam_1_is_the_greedy_chain_integer():
    X, books = integer_input()
    codes, sse = rq_beam_ref.encode(X, books, beam=1)
    ref_codes, ref_mse = rq_ref.encode(X, books)
    np.testing.assert_array_equal(codes, ref_codes)
    np.testing.assert_array_equal(sse, ref_mse * X.shape[0])   # integer sums: exact


def test_beam_1_is_the_greedy_chain_gaussian(gaussian_input):
    X, books = gaussian_input
    codes, sse = rq_beam_ref.encode(X, books, beam=1, rows_per_step=1000)   # the rows are independent of the stepping
    ref_codes, ref_mse = rq_ref.encode(X, books)
    np.testing.assert_array_equal(codes, ref_codes)
    np.testing.assert_allclose(sse / X.shape[0], ref_mse, rtol=1e-12)


def test_beam_5_beats_greedy_on_the_integer_input():
    X, books = integer_input()
    codes, sse = rq_beam_ref.encode(X, books, beam=5)
    _, greedy_mse = rq_ref.encode(X, books)
    assert codes.shape == (1000, 6) and codes.min() >= 0 and codes.max() < 64
    assert (np.diff(sse) <= 0).all(), sse
    assert sse[-1] / X.shape[0] < 0.95 * greedy_mse[-1], (sse[-1] / X.shape[0], greedy_mse[-1])
    # the returned history reconstructs the row to the reported error
    rec = sum(books[m][codes[:, m]].astype(np.float64) for m in range(6))
    assert ((X.astype(np.float64) - rec) ** 2).sum() == sse[-1]


def test_tie_rule_smaller_parent_then_smaller_code():
    d = 32
    e = np.eye(d, dtype=np.float32)
    C0 = np.stack([2 * e[0], 2 * e[1]] + [50 * e[2]] * 62)          # two equally good codewords for x = e0 + e1
    C1 = np.stack([e[0] - e[1], -e[0] + e[1]] + [50 * e[3]] * 62)   # parent 0 reaches zero with k = 1, parent 1 with k = 0
    x = (e[0] + e[1])[None, :]
    codes, sse = rq_beam_ref.encode(x, np.stack([C0, C1]), beam=2)
    assert codes.tolist() == [[0, 1]] and sse[-1] == 0.0            # equal totals: the parent slot decides before the code


def test_max_beam_size_flag():
    from ripor_amd.aq_preprocess.create_customized_smtid_file import get_args
    assert get_args(["--model_dir=x"]).max_beam_size == 1
    assert get_args(["--model_dir=x", "--max_beam_size", "5"]).max_beam_size == 5
    assert get_args(["--max_beam_size=8", "--M=4"]).max_beam_size == 8
