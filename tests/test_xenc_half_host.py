"""No GPU: the fixture, the restatement and the surface of the cross-encoder's f16 mode."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xenc_half_ref as href  # noqa: E402
import xenc_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _packed(b):
    from ripor_amd import engine as E
    return E.xenc_pack(torch.from_numpy(b["ids"]), torch.from_numpy(b["types"]), torch.from_numpy(b["mask"]))


def test_regenerated_x3_is_the_recorded_model():
    z = np.load(os.path.join(ref.GOLDEN, "xh_xenc.npz"))
    fx = href.load("x3")   # (asserts the checksum)
    assert abs(href.checksum(fx["state_dict"]) - float(z["x3_checksum"])) <= 1e-9 * abs(float(z["x3_checksum"]))
    b = fx["batches"]["a"]
    assert b["mask"].sum(axis=1).tolist() == href.X3_LENGTHS and int(b["mask"].sum()) == 766
    got = ref.forward_padded(fx["weights"], fx["cfg"], b["ids"], b["types"], b["mask"], dtype=torch.float64).numpy()
    assert np.abs(got - b["fp64"]).max() <= 1e-9
    assert b["fp64"].std() > 0.05   # the pairs score differently


def test_bars_are_the_references_own_error():
    # (what the generator printed when it wrote the fixture)
    for name, bar in (("x1", 1.37e-3), ("x2", 1.17e-3), ("x3", 1.38e-3)):
        assert abs(href.load(name)["bar"] - bar) <= 0.01e-3, (name, href.load(name)["bar"])


@pytest.mark.parametrize("name", href.MODELS)
def test_restatement_meets_the_bar(name):
    fx = href.load(name)
    worst = 0.0
    for key, b in fx["batches"].items():
        got = href.forward_packed_half(fx["weights"], fx["cfg"], *_packed(b)).double().numpy()
        worst = max(worst, float(np.abs(got - b["fp64"]).max()))
    print(f"[xenc f16] {name}: restatement max |f16 flow - fp64| {worst:.3e}, bar {fx['bar']:.3e}")
    assert worst <= fx["bar"]
    assert worst > 1e-5   # it does round: fp32 sits at 5e-7


def test_new_symbols_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    for name in ("rpr_xenc_set_precision", "rpr_xenc_get_precision"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+RPR_XENC_F32\s+0\b", hdr) and re.search(r"#define\s+RPR_XENC_F16\s+1\b", hdr)
    assert lib.rpr_abi_version() == 5 and _lib.ABI_VERSION == 5
    from ripor_amd import engine as E
    assert E.XENC_PRECISIONS == {"f32": 0, "f16": 1}
    assert "xenc_half.hip" in ge.SOURCES


def test_rerank_accepts_teacher_precision():
    from ripor_amd import rerank as R
    assert R.get_args([]).teacher_precision == "fp32"
    assert R.get_args(["--teacher_precision=fp16"]).teacher_precision == "fp16"
    assert R.get_args(["--teacher_precision", "fp32"]).teacher_precision == "fp32"
    for bad in ("f16", "bf16", "half", ""):
        with pytest.raises(SystemExit):
            R.get_args([f"--teacher_precision={bad}"])
    assert R.TEACHER_PRECISIONS == {"fp32": "f32", "fp16": "f16"}


def test_fp16_teacher_stops_at_a_non_finite_score():
    from ripor_amd import rerank as R

    class Tok:
        def __call__(self, q, d, **kw):
            return {"n": len(q)}

    triples = [("q1", "d1", "s"), ("q1", "d2", "s"), ("q2", "d1", "s")]
    fn = lambda kw: torch.tensor([0.5, float("inf")][:kw["n"]])  # noqa: E731
    q, d = {"q1": "a", "q2": "b"}, {"d1": "x", "d2": "y"}
    with pytest.raises(FloatingPointError, match="teacher_precision=fp32"):
        R.score_triples(triples, q, d, Tok(), fn, 2, 8, require_finite=True)
    assert R.score_triples(triples, q, d, Tok(), fn, 2, 8)[1] == float("inf")   # the fp32 task is as before


def test_cross_encoder_refuses_an_unknown_precision(tmp_path):
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    ckpt = ref.write_checkpoint(ref.load_fixture("x1"), str(tmp_path / "t"))
    with pytest.raises(ValueError, match="precision"):
        CrossEncoder(ckpt, precision="fp16")
    ce = CrossEncoder(ckpt, precision="f16")
    assert ce.precision == "f16" and ce.set_precision("f32").precision == "f32"
    with pytest.raises(ValueError, match="precision"):
        ce.set_precision("half")


def _scratch_by_kernel(source):
    """{mangled kernel name: scratch bytes per lane} of a cross-compile of ripor_amd/csrc/<source> for gfx950."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(REPO, "ripor_amd", "csrc", source)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    return seen


def test_f16_kernels_use_no_scratch():
    """Every f16 GEMM and attention instantiation of xenc_half.hip compiles without scratch (cross-compile for gfx950, no
    GPU needed; the pattern of test_abi.py::test_hot_gemm_kernels_use_no_scratch), and so do the two fp32 instantiations of
    the shared attention kernel and the row kernels in xenc_kernels.hip."""
    seen = _scratch_by_kernel("xenc_half.hip")
    gemm = {k: v for k, v in seen.items() if "xenc_gemm_h_kernel" in k}
    attn = {k: v for k, v in seen.items() if "xenc_attn_kernel" in k and "XencAttnF16" in k}
    assert len(gemm) == 3 and len(attn) == 2, sorted(seen)   # three epilogues; heads of 32 and 64
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
    seen = _scratch_by_kernel("xenc_kernels.hip")   # (the row kernels with the f16 copy live there too)
    full = {k: v for k, v in seen.items() if "xenc_attn_kernel" in k and "XencAttnF32" in k}
    assert len(full) == 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
