"""not-gpu: bench.py --dump-outputs (the arrays a caller of the timed search receives, written as .npy) and the
--steps / --warmup guard."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _result(Q, B, L):
    from ripor_amd.engine import SearchResult
    g = torch.Generator().manual_seed(3)
    lo = torch.randint(0, 8_841_823, (Q, B), generator=g, dtype=torch.int64)
    return SearchResult(tokens=torch.randint(0, 256, (Q, B, L), generator=g, dtype=torch.int32),
                        scores=-torch.rand((Q, B), generator=g, dtype=torch.float32),
                        row_lo=lo, row_hi=lo + torch.randint(1, 3, (Q, B), generator=g, dtype=torch.int64))


def test_dump_writes_every_result_array_exactly(tmp_path):
    bench = _bench()
    res = _result(5, 3, 4)
    shapes = bench.dump_outputs(str(tmp_path), res)
    assert shapes == {"tokens": [5, 3, 4], "scores": [5, 3], "row_lo": [5, 3], "row_hi": [5, 3]}
    assert sorted(os.listdir(tmp_path)) == ["row_hi.npy", "row_lo.npy", "scores.npy", "tokens.npy"]
    for name, dt in (("tokens", np.float32), ("scores", np.float32), ("row_lo", np.float64), ("row_hi", np.float64)):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == dt
        assert (a == getattr(res, name).numpy()).all(), name      # integers below 2^24 / 2^53: exact


def test_dump_samples_the_same_queries_under_the_size_limit(tmp_path):
    bench = _bench()
    Q, B, L = 64, 2, 8
    res = _result(Q, B, L)
    per_query = B * L * 4 + B * 4 + 2 * B * 8
    limit = 10 * per_query + per_query // 2                      # room for 10 queries
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), res, limit=limit)
    bench.dump_outputs(str(b), res, limit=limit)
    total = sum(os.path.getsize(a / f) - 128 for f in os.listdir(a))   # .npy header of 128 bytes
    assert total <= limit
    tok = np.load(a / "tokens.npy")
    assert tok.shape == (10, B, L)
    assert (tok == np.load(b / "tokens.npy")).all()              # fixed seed: same sample every run
    rows = [int(np.flatnonzero((res.tokens.numpy() == t).all(axis=(1, 2)))[0]) for t in tok.astype(np.int32)]
    assert rows == sorted(rows) and len(set(rows)) == 10
    assert (np.load(a / "scores.npy") == res.scores.numpy()[rows]).all()   # every array carries the same queries
    assert (np.load(a / "row_lo.npy") == res.row_lo.numpy()[rows]).all()


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_an_empty_timed_region(flags):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_bench_secondary_legs_need_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--secondary", "latency"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--secondary needs --full" in r.stderr
