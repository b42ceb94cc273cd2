"""synth.make_state_dict(stream_scale=s): a model whose residual stream is s times the unscaled model's (host only).

The split-precision search path carries the un-normalised stream in f16 planes at a fixed scale and its row sums of squares in
fixed point (csrc/common.h: X_PLANE_SCALE, SSQ_FIX); tests/test_gpu_magnitude.py walks that path down the magnitudes with the
models made here. This file pins what those tests rely on: the default is the state dict it always was, the embedding really
has RMS s, and the fp32 oracle computes the same function at every s up to the effect of the norms' eps (1e-6 against a
mean square of s^2: a relative change of the norm scale of eps / (2 s^2), i.e. 16 x per two octaves)."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import t5_ref
from ripor_amd.utils import synth

DIMS = dict(L=8, V=256, enc_layers=2, d_ff=128, vocab_size=512)
SCALED = ("shared.weight", "start_token_embed")
# sha256 over (name, dtype, shape, bytes) of every tensor, names sorted, as the generator wrote them before it had the argument
DIGESTS = {
    (): "9558e25b7e9c85ef567b42a096bc4af62b68f0b7c958269ad012585f8993ed9f",
    (("logit_scale", 3.0), ("outliers", 1e4)): "1c2bd7c91b66f9077eb24ba1783300541b6ad7fcf819e7f7ebca8ad0d25dbdfb",
}


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode()); h.update(str(sd[k].dtype).encode()); h.update(str(sd[k].shape).encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def _is_scaled(name):
    return name in SCALED or name.startswith("list_decoder_embeds.") or name.endswith(".o.weight") or name.endswith(".wo.weight")


@pytest.mark.parametrize("kw", list(DIGESTS))
def test_default_stream_scale_leaves_every_array_as_it_was(kw):
    dims = synth.mini_dims(**DIMS)
    assert _digest(synth.make_state_dict(dims, seed=91, **dict(kw))) == DIGESTS[kw]
    assert _digest(synth.make_state_dict(dims, seed=91, stream_scale=1.0, **dict(kw))) == DIGESTS[kw]


@pytest.mark.parametrize("s", [4.0, 2.0 ** -3, 2.0 ** -7])
def test_stream_scale_multiplies_the_tensors_that_write_the_stream_and_no_other(s):
    dims = synth.mini_dims(**DIMS)
    base, sd = synth.make_state_dict(dims, seed=91), synth.make_state_dict(dims, seed=91, stream_scale=s)
    assert base.keys() == sd.keys()
    n_scaled = 0
    for k in base:
        assert sd[k].dtype == np.float32 and sd[k].shape == base[k].shape
        if _is_scaled(k):
            n_scaled += 1
            assert np.array_equal(sd[k], base[k] * np.float32(s)), k          # a power of two: exact
        else:
            assert np.array_equal(sd[k], base[k]), k
    # 3 embeddings' worth (shared, start, L tables) + o of every attention (2 encoder, 12 x 2 decoder) + wo of every block
    assert n_scaled == 2 + DIMS["L"] + (2 + 24) + (2 + 12)
    rms = float(np.sqrt((sd["shared.weight"].astype(np.float64) ** 2).mean()))
    assert abs(rms / s - 1.0) < 5e-3, rms                                      # uniform with unit variance x s
    for i in range(DIMS["L"]):
        rms = float(np.sqrt((sd[f"list_decoder_embeds.{i}.weight"].astype(np.float64) ** 2).mean()))
        assert abs(rms / s - 1.0) < 1e-2, (i, rms)


def test_stream_scale_must_be_a_power_of_two():
    with pytest.raises(AssertionError):
        synth.make_state_dict(synth.mini_dims(**DIMS), seed=91, stream_scale=0.3)


def test_oracle_encoder_is_the_same_function_up_to_the_eps_effect():
    """max |enc(s) - enc(1)| over five queries, measured with the fp32 oracle on a CPU: 1.4e-4 at 2^-3, 2.3e-3 at 2^-5, 3.6e-2
    at 2^-7 against max |enc| = 4.56. The bound is twice those figures; the growth is 16 x per two octaves (eps / s^2)."""
    dims = synth.mini_dims(**DIMS)
    ids, mask = synth.make_queries(5, vocab_size=512, seed=92, max_len=12)
    ti, tm = torch.from_numpy(ids).long(), torch.from_numpy(mask).long()
    enc = {s: t5_ref.T5Ref(synth.make_state_dict(dims, seed=91, stream_scale=s), dims).encode(ti, tm).double()
           for s in (1.0, 2.0 ** -3, 2.0 ** -5, 2.0 ** -7)}
    assert abs(float(enc[1.0].abs().max()) - 4.56) < 0.01
    live = tm.bool()
    delta = {s: float((enc[s] - enc[1.0])[live].abs().max()) for s in enc}
    print("[stream_scale] max |enc(s) - enc(1)|:", {f"2^{int(np.log2(s))}": f"{d:.3g}" for s, d in delta.items()})
    for s, seen in ((2.0 ** -3, 1.4e-4), (2.0 ** -5, 2.3e-3), (2.0 ** -7, 3.6e-2)):
        assert 0.0 < delta[s] < 2.0 * seen, (s, delta[s])
    for hi, lo in ((2.0 ** -3, 2.0 ** -5), (2.0 ** -5, 2.0 ** -7)):
        assert 11.0 < delta[lo] / delta[hi] < 23.0, (hi, lo, delta[lo] / delta[hi])   # 16 x, within sqrt(2)
