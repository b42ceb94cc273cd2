"""Golden vectors of the gated-GELU feed-forward (T5 v1.1 / Flan-T5 / mT5: ``feed_forward_proj="gated-gelu"``) from the
*imported* reference on CPU.

Same rules as make_golden.py, whose case builders this runs unchanged: the reference's own model, processor, beam loop,
training forwards and ``save_pretrained`` run unmodified; what is stored is data. The only difference to the ReLU fixtures is
the model under them — for the duration of a case the three helpers the builders call are swapped (``gated()`` below):
``build_reference_model`` builds the reference with ``feed_forward_proj="gated-gelu"``, ``synth.make_state_dict`` makes the
``wi_0`` / ``wi_1`` weights, ``synth.mini_dims`` defaults to d_ff 96 (W_in then has 192 rows: one and a half 128-column tiles).
Every spec records ``feed_forward_proj`` beside the dims (the kind is not a field of ``synth.ModelDims``).

Fixture names start with ``v11_`` (never ``g``, ``f4_``, ``s2s_`` or ``drop_``: conftest, test_seq2seq_host and
test_dropout_host feed those prefixes to the tests of the ReLU model). Search fixtures must keep every pruning margin above
MARGIN_BAR: asserted here, seeds were picked for which the reference alone satisfies it.

Usage:  python tests/golden/make_golden_gated.py [--only NAME]
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
import make_golden_seq2seq  # noqa: E402
from make_golden import load_reference, synth  # noqa: E402

KIND = "gated-gelu"
D_FF = 96
MARGIN_BAR = 2e-3     # tests/test_oracle_golden.py::test_fixture_margins_are_comfortable asks 1e-3 (PRUNE_TOL); twice that here

SEARCH_CASES = {
    "v11_g8_mini_b4_l8": dict(kind="mini", N=1000, Q=6, B=4, L=8, V=256, seed=801),
    "v11_g8_mini_b10_l8_shared": dict(kind="mini", N=1000, Q=6, B=10, L=8, V=256, seed=802, shared=True),
}
TRAIN_CASES = {"v11_f5_mini_bz3_l8": dict(kind="mini", bz=3, L=8, V=256, seed=811)}
S2S_CASES = {"v11_s2s_mini_bz3_l8": dict(kind="mini", bz=3, L=8, V=256, seed=821)}
CHECKPOINT = "c11_ref_checkpoint_gated"


def build_gated_reference_model(mod, dims, sd_np, which="t5-base"):
    """make_golden.build_reference_model with the gated feed-forward (HF then builds T5DenseGatedActDense, gelu_new)."""
    cfg = mod.T5forDocIDConfig(
        vocab_size=dims.vocab_size, d_model=dims.d_model, d_kv=dims.d_kv, d_ff=dims.d_ff,
        num_layers=dims.num_layers, num_decoder_layers=dims.num_decoder_layers, num_heads=dims.num_heads,
        relative_attention_num_buckets=dims.relative_attention_num_buckets,
        relative_attention_max_distance=dims.relative_attention_max_distance,
        decoder_vocab_sizes=list(dims.decoder_vocab_sizes), decoding=True,
        shared_output_input_embeds=dims.shared_output_input_embeds,
        scaleup_output_hidden=dims.scaleup_output_hidden,
        decoder_start_token_path=f"./t5_decoder_start_token_embeds/{which}.npy",
        feed_forward_proj=KIND, dropout_rate=0.0, use_cache=False,
        decoder_start_token_id=0, pad_token_id=0, eos_token_id=1,
    )
    cfg._attn_implementation = "eager"
    assert cfg.dense_act_fn == "gelu_new" and cfg.is_gated_act
    model = mod.T5ForDocIDGeneration(cfg)
    assert type(model.encoder.block[0].layer[1].DenseReluDense).__name__ == "T5DenseGatedActDense"
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [m for m in missing if "decoder.embed_tokens" not in m]
    assert not missing and not unexpected, (missing, unexpected)
    model.eval()
    return model


@contextlib.contextmanager
def gated():
    """The case builders of make_golden / make_golden_seq2seq see a gated model: see the module docstring."""
    make_sd, mini, patterned = synth.make_state_dict, synth.mini_dims, synth.patterned_state_dict
    saved = (make_golden.build_reference_model, make_golden_seq2seq.build_reference_model)
    synth.make_state_dict = lambda dims, **kw: make_sd(dims, **dict(kw, feed_forward_proj=KIND))
    synth.mini_dims = lambda **kw: mini(**dict(dict(d_ff=D_FF), **kw))
    synth.patterned_state_dict = lambda dims: patterned(dims, feed_forward_proj=KIND)
    make_golden.build_reference_model = make_golden_seq2seq.build_reference_model = build_gated_reference_model
    try:
        yield
    finally:
        synth.make_state_dict, synth.mini_dims, synth.patterned_state_dict = make_sd, mini, patterned
        make_golden.build_reference_model, make_golden_seq2seq.build_reference_model = saved


def stamp(name):
    """Record the feed-forward kind in the fixture's spec; returns the arrays."""
    path = os.path.join(HERE, name + ".npz")
    z = dict(np.load(path, allow_pickle=False))
    spec = json.loads(str(z["spec"]))
    assert spec["dims"]["d_ff"] == D_FF, spec["dims"]
    spec["feed_forward_proj"] = KIND
    z["spec"] = np.array(json.dumps(spec))
    np.savez_compressed(path, **z)
    return z, spec


def margins(z, B):
    """conftest.prune_margins on the stored candidates."""
    ts = z["top_scores"]
    gap = np.where(ts[:, :, B] > -1e8, ts[:, :, B - 1] - ts[:, :, B], np.inf)
    return gap.min(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    gen, mod, utils, shim = load_reference()
    want = lambda name: not args.only or args.only == name   # noqa: E731
    with gated():
        for name, spec in SEARCH_CASES.items():
            if want(name):
                make_golden.make_case(name, spec, gen, mod, utils, shim)
                z, s = stamp(name)
                m = margins(z, s["B"])
                print(f"[golden] {name}: pruning margins {np.array2string(m, precision=4)}")
                assert (m > MARGIN_BAR).all(), f"{name}: a pruning margin under {MARGIN_BAR}: pick another seed"
        for name, spec in TRAIN_CASES.items():
            if want(name):
                make_golden.make_train_case(name, spec, gen, mod, utils, shim)
                stamp(name)
        for name, spec in S2S_CASES.items():
            if want(name):
                make_golden_seq2seq.make_s2s_case(name, spec, mod)
                stamp(name)
        if want(CHECKPOINT):
            make_golden.make_checkpoint_case(mod, name=CHECKPOINT)


if __name__ == "__main__":
    main()
