"""not-gpu: the gated-GELU feed-forward (T5 v1.1 / Flan-T5 / mT5, feed_forward_proj="gated-gelu") on the host side. The CPU
oracles of tests/gated_ref.py (T5Ref & co. with ONE method overridden) are pinned to the fixtures the imported reference
produced with that config (tests/golden/make_golden_gated.py): a search, a search with shared codebooks, the ranking step and
the seq2seq step with their gradients, and a checkpoint directory written by the reference's own save_pretrained. Then the
config, the key list and the C ABI. Bars are those of test_oracle_golden.py / test_seq2seq_host.py / test_host_logic.py."""
import ctypes as C
import json
import os
import zipfile

import numpy as np
import pytest
import torch

import gated_ref
from conftest import GOLDEN_DIR, Golden, compare_ranked, prune_margins
from oracle import beam_ref, train_ref
from ripor_amd.modeling.t5_generative_retriever import (FEED_FORWARD_KINDS, T5forDocIDConfig, T5ForDocIDGeneration,
                                                        T5SeqAQEncoder, expected_keys)
from ripor_amd.utils import synth

KIND = "gated-gelu"
SEARCH = ["v11_g8_mini_b4_l8", "v11_g8_mini_b10_l8_shared"]
MARGIN_BAR = 2e-3


class GatedGolden(Golden):
    """conftest.Golden whose weights are the gated variant of the same seed."""

    def __init__(self, name):
        super().__init__(name)
        assert self.spec["feed_forward_proj"] == KIND and self.dims.d_ff == 96

    @property
    def state_dict(self):
        if self._sd is None:
            self._sd = synth.make_state_dict(self.dims, seed=self.seed, feed_forward_proj=KIND)
        return self._sd


_CACHE = {}


def gated_golden(name):
    if name not in _CACHE:
        _CACHE[name] = GatedGolden(name)
    return _CACHE[name]


def mask_fn(g):
    return beam_ref.PrefixMaskRef(beam_ref.build_list_smtid_to_nextids(synth.codes_to_docid_to_smtid(g.codes)), g.V)


def test_gated_state_dict_differs_from_relu_only_in_wi():
    dims = synth.mini_dims(L=2, enc_layers=1, d_ff=32, vocab_size=64)
    relu, gate = synth.make_state_dict(dims, seed=3), synth.make_state_dict(dims, seed=3, feed_forward_proj=KIND)
    assert {k for k in relu if k not in gate} == {k for k in relu if k.endswith("DenseReluDense.wi.weight")}
    new = {k for k in gate if k not in relu}
    assert len(new) == 2 * 13 and all(k.endswith(("wi_0.weight", "wi_1.weight")) for k in new)
    assert all(np.array_equal(relu[k], gate[k]) for k in relu if k in gate)
    assert all(gate[k].shape == (32, 768) for k in new)
    assert not np.array_equal(gate["encoder.block.0.layer.1.DenseReluDense.wi_0.weight"],
                              gate["encoder.block.0.layer.1.DenseReluDense.wi_1.weight"])
    d = synth.t5_v11_base_dims()
    assert (d.d_ff, d.d_model, d.num_heads, d.num_layers, d.num_decoder_layers) == (2048, 768, 12, 12, 12)
    with pytest.raises(ValueError):
        synth.make_state_dict(dims, feed_forward_proj="gated-silu")


@pytest.mark.parametrize("name", SEARCH)
def test_fixture_margins(name):
    """Every pruning margin of the reference's own search is above 2e-3 (the generator asserts the same)."""
    g = gated_golden(name)
    m, near = prune_margins(g)
    assert g.Q == 6 and (m > MARGIN_BAR).all() and (near == 0).all(), m


@pytest.mark.parametrize("name", SEARCH)
def test_gated_oracle_reproduces_reference_search(name):
    g = gated_golden(name)
    torch.set_num_threads(8)
    rec = {}
    seqs, scores = beam_ref.beam_search_ref(gated_ref.GatedT5Ref(g.state_dict, g.dims), mask_fn(g), g.input_ids, g.attention_mask,
                                            g.B, g.L, g.log_softmax, record=rec)
    np.testing.assert_allclose(rec["encoder_out"], g.z["encoder_out"], atol=1e-5, rtol=1e-5)
    assert (seqs.numpy() == g.sequences).all(), "oracle smtid sequences differ from the reference"
    np.testing.assert_allclose(scores.numpy(), g.sequences_scores, atol=1e-6, rtol=0)
    ss = g.z["step_scores"]
    for t in range(g.L):
        valid = ss[t] > -1e8
        np.testing.assert_allclose(rec["steps"][t]["logits"][valid], ss[t][valid], atol=1e-5, rtol=1e-6)
    # the ReLU oracle on the same weights is NOT this model (the fixture pins the gate, not only the plumbing)
    assert "encoder.block.0.layer.1.DenseReluDense.wi.weight" not in g.state_dict


@pytest.mark.parametrize("name", SEARCH)
def test_gated_kv_cached_oracle_equals_full_prefix(name):
    g = gated_golden(name)
    torch.set_num_threads(8)
    seqs, scores = beam_ref.beam_search_ref(gated_ref.GatedT5RefCached(g.state_dict, g.dims), mask_fn(g), g.input_ids,
                                            g.attention_mask, g.B, g.L, g.log_softmax, use_kv_cache=True)
    got = seqs.numpy().reshape(g.Q, g.B, g.L + 1)
    stats = compare_ranked(g, got[:, :, 1:], scores.numpy().reshape(g.Q, g.B), label=" (gated KV-cached oracle)")
    assert stats["boundary_excused"] == 0 and stats["sequences_missing"] == 0


class GatedTrainGolden:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.spec = json.loads(str(self.z["spec"]))
        assert self.spec["feed_forward_proj"] == KIND
        self.dims = synth.ModelDims(**self.spec["dims"])
        self.bz, self.L, self.V, self.seed = self.spec["bz"], self.spec["L"], self.spec["V"], self.spec["seed"]
        self.state_dict = synth.make_state_dict(self.dims, seed=self.seed, feed_forward_proj=KIND)
        self.teacher = {k: self.z[k] for k in self.z.files if k.endswith("_scores") and "teacher" in k}
        if "loss_names" in self.z.files:
            self.losses = dict(zip([str(x) for x in self.z["loss_names"]], self.z["losses"].tolist()))


def test_gated_train_step_oracle_reproduces_reference():
    """Losses, position scores, gradients, the clipped AdamW update and the losses after it: the existing train-golden bars."""
    from test_oracle_golden import check_grads_against_fixture, grad_sample_indices
    g = GatedTrainGolden("v11_f5_mini_bz3_l8")
    torch.set_num_threads(8)
    args = (g.z["input_ids"], g.z["attention_mask"], g.z["pos_doc_encoding"], g.z["neg_doc_encoding"], g.teacher)
    with torch.no_grad():
        out = train_ref.lng_knp_margin_mse(gated_ref.GatedT5Ref(g.state_dict, g.dims), *args)
    assert set(g.losses) == set(train_ref.LOSS_NAMES[g.L])
    np.testing.assert_allclose(out["pos_position_scores"].numpy(), g.z["pos_position_scores"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(out["neg_position_scores"].numpy(), g.z["neg_position_scores"], atol=2e-5, rtol=1e-5)
    for k, v in g.losses.items():
        assert abs(float(out[k]) - v) <= 1e-5 * max(1.0, abs(v)), (k, float(out[k]), v)
    model = gated_ref.GatedT5Ref(g.state_dict, g.dims)
    before = {k: v.clone() for k, v in model.sd.items()}
    lr = float(g.z["step_lr"])
    losses, total, grads, gnorm = train_ref.train_step(model, *args, lr=lr)
    assert abs(total - float(g.z["total_loss"])) <= 1e-5 * abs(total)
    assert abs(gnorm - float(g.z["grad_global_norm"])) <= 1e-4 * gnorm
    names = [str(x) for x in g.z["grad_names"]]
    assert sum(n.endswith(("wi_0.weight", "wi_1.weight")) for n in names) == 2 * (g.dims.num_layers + g.dims.num_decoder_layers)
    check_grads_against_fixture(g, {k: v.numpy() for k, v in grads.items()}, label=" (gated oracle)")
    off = 0
    for n, c in zip(names, g.z["grad_sample_counts"]):
        ref = g.z["param_delta_samples"][off:off + c]
        off += c
        key = "shared.weight" if n == "encoder.embed_tokens.weight" else n
        d = (model.sd[key] - before[key]).numpy().reshape(-1)[grad_sample_indices(n, before[key].shape)]
        np.testing.assert_allclose(d, ref, atol=2e-2 * lr, rtol=0, err_msg=f"update of {n}")
    with torch.no_grad():
        after = train_ref.lng_knp_margin_mse(model, *args)
    for k, v in zip(sorted(g.losses), g.z["losses_after_step"]):
        assert abs(float(after[k]) - v) <= 2e-3 * max(1.0, abs(v)), (k, float(after[k]), v)


def test_gated_seq2seq_oracle_reproduces_reference():
    from test_seq2seq_host import check_grads, seq2seq_ce, seq2seq_grads
    g = GatedTrainGolden("v11_s2s_mini_bz3_l8")
    torch.set_num_threads(8)
    model = gated_ref.GatedT5Ref(g.state_dict, g.dims)
    with torch.no_grad():
        loss, lp = seq2seq_ce(model, g.z["input_ids"], g.z["attention_mask"], g.z["labels"])
    assert abs(float(loss) - float(g.z["loss"])) <= 1e-5 * max(1.0, abs(float(g.z["loss"])))
    np.testing.assert_allclose(lp.numpy(), g.z["label_logprobs"], atol=1e-5 * max(1.0, np.abs(g.z["label_logprobs"]).max()), rtol=0)
    _, grads, gn = seq2seq_grads(model, g.z["input_ids"], g.z["attention_mask"], g.z["labels"])
    assert abs(gn - float(g.z["grad_global_norm"])) <= 1e-4 * gn
    check_grads(g, {k: v.numpy() for k, v in grads.items()}, label=" (gated seq2seq oracle)")


def test_gelu_new_restatements_agree():
    """The float64 numpy gate, HF's expression in torch float64, and the derivative against a central difference."""
    g = np.concatenate([np.linspace(-30, 30, 2001), [0.0, -0.0, 1e-4, -1e-4]])
    # (numpy's and torch's tanh differ by an ulp of 1 + tanh, 2.2e-16, which 0.5 |g| <= 15 scales: four of those)
    np.testing.assert_allclose(gated_ref.gelu_new64(g), gated_ref.gelu_new_t(torch.from_numpy(g)).numpy(), rtol=1e-13, atol=1.4e-14)
    x = np.linspace(-6, 6, 241)
    num = (gated_ref.gelu_new64(x + 1e-6) - gated_ref.gelu_new64(x - 1e-6)) / 2e-6
    np.testing.assert_allclose(gated_ref.gelu_new_grad64(x), num, atol=1e-8)
    t = torch.from_numpy(x).requires_grad_(True)
    gated_ref.gelu_new_t(t).sum().backward()
    # (both cancel 1 + t and 1 - t^2 in the negative tail: absolute errors of 1.1e-16 that |g| c (1 + 0.134 g^2) <= 28 scales)
    np.testing.assert_allclose(gated_ref.gelu_new_grad64(x), t.grad.numpy(), rtol=1e-12, atol=2e-14)


def test_reference_gated_checkpoint_directory_loads(tmp_path):
    """tests/golden/c11_ref_checkpoint_gated.zip: what the reference's own save_pretrained wrote for a gated config at the
    sizes of c9. from_pretrained reads it as it is, every tensor bit for bit; this repo's save_pretrained writes wi_0 / wi_1
    back as two tensors and the round trip is exact."""
    with zipfile.ZipFile(os.path.join(GOLDEN_DIR, "c11_ref_checkpoint_gated.zip")) as z:
        assert sorted(z.namelist()) == ["config.json", "model.safetensors"]
        z.extractall(str(tmp_path))
    enc = T5SeqAQEncoder.from_pretrained(str(tmp_path))
    cfg = enc.config
    assert (cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_decoder_layers, cfg.num_heads, cfg.vocab_size) == (768, 2, 4, 1, 12, 12, 16)
    assert cfg.feed_forward_proj == KIND and cfg.is_gated_ff and cfg.decoder_vocab_sizes == [64, 64]
    dims = synth.ModelDims(vocab_size=16, d_model=768, d_kv=2, d_ff=4, num_layers=1, num_decoder_layers=12, num_heads=12,
                           decoder_vocab_sizes=[64, 64])
    want = synth.patterned_state_dict(dims, feed_forward_proj=KIND)
    got = enc.base_model.state_dict()
    assert set(got) == set(expected_keys(cfg)) == set(want)
    assert sum(k.endswith(("wi_0.weight", "wi_1.weight")) for k in got) == 26 and not any(k.endswith(".wi.weight") for k in got)
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and torch.equal(got[k], torch.from_numpy(v)), k
    enc.save_pretrained(str(tmp_path / "again"))
    assert json.load(open(tmp_path / "again" / "config.json"))["feed_forward_proj"] == KIND
    again = T5SeqAQEncoder.from_pretrained(str(tmp_path / "again")).base_model.state_dict()
    assert set(again) == set(got) and all(torch.equal(again[k], got[k]) for k in got)
    # a ReLU state dict does not load into a gated model, nor the other way round
    with pytest.raises(RuntimeError):
        T5ForDocIDGeneration(cfg, synth.patterned_state_dict(dims))


def test_config_accepts_the_two_kinds_and_refuses_the_rest():
    assert FEED_FORWARD_KINDS == ("relu", "gated-gelu")
    assert not T5forDocIDConfig().is_gated_ff and T5forDocIDConfig(feed_forward_proj="relu").feed_forward_proj == "relu"
    assert T5forDocIDConfig(feed_forward_proj=KIND).is_gated_ff
    for bad in ("gated-silu", "gelu"):
        with pytest.raises(ValueError) as e:
            T5forDocIDConfig(feed_forward_proj=bad)
        assert "'relu'" in str(e.value) and "'gated-gelu'" in str(e.value) and bad in str(e.value)
    relu_keys, gate_keys = expected_keys(T5forDocIDConfig(num_layers=1, num_decoder_layers=12)), expected_keys(T5forDocIDConfig(num_layers=1, num_decoder_layers=12, feed_forward_proj=KIND))
    assert len(gate_keys) == len(relu_keys) + 13
    assert "decoder.block.11.layer.2.DenseReluDense.wi_1.weight" in gate_keys and "encoder.block.0.layer.1.DenseReluDense.wi_0.weight" in gate_keys


def test_abi_exports_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "ripor_hip.h")).read()
    for name, nargs in (("rpr_load_model_ext", 4), ("rpr_op_gated_gelu", 8), ("rpr_op_gated_gelu_bwd", 7)):
        assert hasattr(lib, name) and name in hdr and len(_lib.SIGNATURES[name][1]) == nargs
    assert lib.rpr_abi_version() == 5 == _lib.ABI_VERSION
    assert C.sizeof(_lib.ModelExt) == 8 and (_lib.FF_RELU, _lib.FF_GATED_GELU) == (0, 1)
    assert "#define RPR_FF_RELU 0" in hdr and "#define RPR_FF_GATED_GELU 1" in hdr
    assert C.sizeof(_lib.ModelDesc) == 56 + 24 * 8   # unchanged
