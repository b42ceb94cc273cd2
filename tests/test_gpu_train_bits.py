"""-m gpu: the training step keeps its bits. The ranking step and the seq2seq step on the batches of
tests/golden/make_golden_train_bits.py against tests/golden/train_bits.json, what the MI355X gave at the commit named in
that file: the sha256 of the flat gradient buffer, the losses as float32 bit patterns, the gradient buckets in hand-over
order and the launch count per kernel class, all compared exactly. The cases added later (one per route of the training attention,
csrc/attn_route.h) name the commit they were recorded at in a "commit" key of their own; it is printed and not compared.

A restructuring of the step (csrc/train_api.hip, train_layout.h, the launchers of train_kernels.hip) must leave this green.
Re-record (the script, by hand, on the GPU) only with a change that is meant to move the arithmetic or the launch sequence,
from a commit whose gradients are trusted by other means (test_gpu_train.py, test_gpu_seq2seq.py) — never to make a
restructuring pass."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


@pytest.fixture(scope="module")
def records(ctx):
    return rec.record_all(ctx, [p for p in rec.PRECISIONS if p != "bf16" or ctx.has_bf16()])


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(rec.HERE, "train_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case,precision", rec.CASES)
def test_training_step_keeps_its_bits(ctx, records, golden, case, precision):
    if precision == "bf16" and not ctx.has_bf16():
        pytest.skip("the library was built without the bf16 training GEMMs")
    got, want = records[case], golden["cases"][case]
    print(f"[train bits] {case}: grads {got['grads_sha256'][:16]} (recorded {want['grads_sha256'][:16]} at "
          f"{want.get('commit', golden['commit'])[:12]}), "
          f"loss bits {got['loss_bits']}, {len(got['buckets'])} buckets, launches {got['launches']}")
    assert got["launches"] == want["launches"]
    assert got["buckets"] == want["buckets"]
    assert got["loss_bits"] == want["loss_bits"]
    assert got["grads_sha256"] == want["grads_sha256"]

