"""-m gpu: the cross-encoder teacher keeps its bits. ``engine.xenc_score`` in both precisions against
tests/golden/xenc_bits.npz, the scores the MI355X gave at the commit named in that file, compared as bytes.

A refactoring of the teacher must leave this green. Re-record (tests/golden/make_golden_xenc_bits.py, by hand, on the GPU)
only from a commit whose scores are trusted by other means (the accuracy tests of test_gpu_xenc.py and
test_gpu_xenc_half.py), for instance after a toolchain change (the file holds the ``hipcc --version`` it was built with),
or with a change that is meant to move the arithmetic — never to make a restructuring pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_xenc_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scores():
    from ripor_amd import engine as E
    return rec.score_all(E.Context.get(0))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(rec.HERE, "xenc_bits.npz"))


@pytest.mark.parametrize("precision", rec.PRECISIONS)
@pytest.mark.parametrize("model,key", rec.CASES)
def test_scores_keep_their_bits(scores, golden, model, key, precision):
    name = f"{model}_{key}_{precision}"
    got, want = scores[name], golden[name]
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    diff = np.abs(got.astype(np.float64) - want).max()
    print(f"[xenc bits] {name}: {len(got)} scores, max |now - recorded| {diff:.3e} (recorded at {str(golden['commit'])[:12]})")
    assert got.tobytes() == want.tobytes()
