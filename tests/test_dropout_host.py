"""not-gpu: dropout of the training steps on the host side — the numpy restatement of the device mask (tests/dropout_mask.py),
the torch autograd restatement with the masks as constants (tests/dropout_ref.py) pinned to the reference classes in train()
mode with the same masks injected (tests/golden/drop_*.npz, make_golden_dropout.py), and the plumbing from the command line
and the trainer down to the engine call, through a stub engine."""
import json
import os
import types

import numpy as np
import pytest
import torch

import dropout_mask as dm
from conftest import GOLDEN_DIR
from dropout_ref import DropoutRef

DROP_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("drop_") and f.endswith(".npz"))


def test_philox_known_answers():
    """Vectors produced by the numpy restatement itself (no published copy ships with the toolchain to cite): counter and key
    all zero, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in dm.philox4x32_10(*ctr, *key)) == want


def test_drop_fraction_is_binomial():
    """10^6 draws at each of three sites, rate 0.1: the dropped fraction within six binomial standard deviations."""
    n, p = 10 ** 6, 0.1
    sd = np.sqrt(p * (1 - p) / n)
    for site in (dm.site_input(0), dm.site_mid(1, 5, 2), dm.site_sub_out(0, 11, 1)):
        m = dm.act_mask(p, 2024, 3, site, np.arange(10), 100, 1000)
        assert m.size == n and set(np.unique(m).tolist()) == {0.0, float(dm.scale(p))}
        assert abs(float((m == 0).mean()) - p) <= 6 * sd, (site, float((m == 0).mean()))
    a = dm.attn_mask(p, 2024, 3, dm.site_mid(0, 0, 0), np.arange(10), 10, 100, 100)
    assert abs(float((a == 0).mean()) - p) <= 6 * sd
    assert dm.threshold(0.1) == 429496736 and dm.scale(0.1) == np.float32(1.0) / np.float32(0.9)


def test_masks_depend_on_site_step_seed_and_nothing_else():
    args = dict(rate=0.1, seed=5, step=9, site=dm.site_sub_out(1, 2, 0), seqs=np.arange(4), n_pos=8, n_feat=64)
    base = dm.act_mask(**args)
    assert np.array_equal(base, dm.act_mask(**args))
    for k, v in (("site", dm.site_sub_out(1, 2, 1)), ("step", 10), ("seed", 6), ("step", 9 + (1 << 32)), ("seed", 5 + (1 << 32))):
        assert not np.array_equal(base, dm.act_mask(**dict(args, **{k: v}))), k
    # logical coordinates only: a sequence's mask does not depend on which other sequences are in the call, nor a feature's on
    # the width of the row
    assert np.array_equal(base[2:3], dm.act_mask(**dict(args, seqs=[2])))
    assert np.array_equal(base[:, :, :30], dm.act_mask(**dict(args, n_feat=30)))
    at = dm.attn_mask(0.1, 5, 9, dm.site_mid(1, 2, 1), np.arange(4), 4, 8, 13)
    assert np.array_equal(at[:, :, :, :6], dm.attn_mask(0.1, 5, 9, dm.site_mid(1, 2, 1), np.arange(4), 4, 8, 6))
    sites = {dm.site_input(d) for d in (0, 1)} | {dm.site_output(d) for d in (0, 1)}
    sites |= {f(d, i, j) for f in (dm.site_mid, dm.site_sub_out) for d in (0, 1) for i in range(24) for j in range(3)}
    assert len(sites) == 4 + 2 * 2 * 24 * 3 and max(sites) < 1 << 16


class _Golden:
    def __init__(self, name):
        from ripor_amd.utils import synth
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.spec = json.loads(str(self.z["spec"]))
        self.dims = synth.ModelDims(**self.spec["dims"])
        self.sd = synth.make_state_dict(self.dims, seed=self.spec["seed"])
        self.rate, self.seed, self.step = float(self.z["rate"]), int(self.z["mask_seed"]), int(self.z["mask_step"])


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.mark.parametrize("name", DROP_CASES)
def test_autograd_restatement_reproduces_the_reference_in_train_mode(name):
    """CPU float32 against CPU float32, the same masks on both sides: losses within 1e-6 relative, per-position scores /
    label log-probabilities within 1e-5 of their scale, every sampled gradient within 1e-5 of its tensor's scale."""
    from oracle import train_ref
    from test_seq2seq_host import check_grads, seq2seq_ce, seq2seq_grads
    assert len(DROP_CASES) == 4
    g = _Golden(name)
    assert g.rate == 0.1
    torch.set_num_threads(1)
    model = DropoutRef(g.sd, g.dims, g.rate, g.seed, g.step)
    z = g.z
    if g.spec["step"] == "lngknp":
        teacher = {k: z[k] for k in z.files if k.endswith("_scores") and "teacher" in k}
        model.begin(2)
        out, total, grads, gn = train_ref.train_step(model, z["input_ids"], z["attention_mask"], z["pos_doc_encoding"],
                                                     z["neg_doc_encoding"], teacher)
        for k, v in zip([str(x) for x in z["loss_names"]], z["losses"].tolist()):
            assert _rel(float(out[k]), v) <= 1e-6, (k, float(out[k]), v)
        for side in ("pos", "neg"):
            ref = z[side + "_position_scores"]
            assert np.abs(out[side + "_position_scores"].numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
        assert _rel(total, float(z["total_loss"])) <= 1e-6
    else:
        model.begin(1)
        loss, grads, gn = seq2seq_grads(model, z["input_ids"], z["attention_mask"], z["labels"])
        assert _rel(loss, float(z["losses"][0])) <= 1e-6, (loss, float(z["losses"][0]))
        model.begin(1)
        with torch.no_grad():
            _, lp = seq2seq_ce(model, z["input_ids"], z["attention_mask"], z["labels"])
        assert np.abs(lp.numpy() - z["label_logprobs"]).max() <= 1e-5 * max(1.0, np.abs(z["label_logprobs"]).max())
    assert _rel(gn, float(z["grad_global_norm"])) <= 1e-5
    # (check_grads holds the tensor norms to rel and the sampled entries to 10 rel: the sampled entries are held to 1e-5 here)
    worst = check_grads(g, {k: v.numpy() for k, v in grads.items()}, rel=1e-5, label=" (dropout oracle)")
    print(f"[dropout-oracle] {name}: worst sampled-gradient error {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 1e-5, worst


def test_restatement_at_rate_zero_is_the_oracle():
    from oracle import t5_ref, train_ref
    g = _Golden("drop_f4_bz3_l8")
    z = g.z
    teacher = {k: z[k] for k in z.files if k.endswith("_scores") and "teacher" in k}
    args = (z["input_ids"], z["attention_mask"], z["pos_doc_encoding"], z["neg_doc_encoding"], teacher)
    with torch.no_grad():
        a = train_ref.lng_knp_margin_mse(t5_ref.T5Ref(g.sd, g.dims), *args)
        m = DropoutRef(g.sd, g.dims, 0.0, 1, 1)
        m.begin(2)
        b = train_ref.lng_knp_margin_mse(m, *args)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- plumbing: command line -> trainer -> model -> engine, without a GPU ----------------------------------------------------
def test_config_reads_and_writes_dropout_rate(tmp_path):
    from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig
    cfg = T5forDocIDConfig(decoder_vocab_sizes=[256] * 8, dropout_rate=0.25)
    cfg.save_pretrained(str(tmp_path))
    assert json.load(open(tmp_path / "config.json"))["dropout_rate"] == 0.25
    assert T5forDocIDConfig.from_pretrained(str(tmp_path)).dropout_rate == 0.25
    assert T5forDocIDConfig(decoder_vocab_sizes=[256] * 8).dropout_rate == 0.1      # T5Config's default


def test_dropout_config_takes_the_rate_of_the_loaded_checkpoint(tmp_path):
    """--dropout=config through the objects main() uses: a checkpoint directory whose config.json says 0.25, read back by
    from_pretrained, resolved against model.config as main() does."""
    from ripor_amd import main as M
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE
    from ripor_amd.utils import synth
    model = T5SeqAQEncoderForLngKnpMarginMSE.from_synthetic(synth.mini_dims(L=8, V=256, enc_layers=1, d_ff=128), seed=9)
    model.base_model.config.dropout_rate = 0.25
    model.base_model.save_pretrained(str(tmp_path))
    assert json.load(open(tmp_path / "config.json"))["dropout_rate"] == 0.25
    back = T5SeqAQEncoderForLngKnpMarginMSE.from_pretrained(str(tmp_path))
    said = []
    assert M.resolve_dropout("config", float(getattr(back.config, "dropout_rate", 0.0)), said.append) == 0.25 and not said
    assert M.resolve_dropout("off", float(getattr(back.config, "dropout_rate", 0.0)), said.append) == 0.0 and "0.25" in said[0]


def test_dropout_flag_default_off_config_and_float():
    from ripor_amd import main as M
    base = ["--pretrained_path", "p", "--output_dir", "o"]
    assert M.get_args(base).dropout == "off"
    said = []
    assert M.resolve_dropout("off", 0.1, said.append) == 0.0
    assert len(said) == 1 and "0.1" in said[0] and "reference trains with it" in said[0]
    said = []
    assert M.resolve_dropout("off", 0.0, said.append) == 0.0 and not said
    assert M.resolve_dropout("config", 0.1, said.append) == 0.1 and M.resolve_dropout("0.05", 0.1, said.append) == 0.05
    assert not said
    assert M.get_args(base + ["--dropout=config"]).dropout == "config"
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit):
            M.resolve_dropout(bad, 0.1, said.append)


class _StubEngine:
    """What engine.train_step touches below the Python layer: a lib whose setter and steps record their arguments."""

    def __init__(self):
        self.calls = []
        lib = types.SimpleNamespace()
        lib.rpr_set_train_dropout = lambda h, rate, seed, step: (self.calls.append(("drop", rate, seed, step)), 0)[1]
        lib.rpr_param_total = lambda h: 8
        lib.rpr_param_count = lambda h: 0
        lib.rpr_lngknp_backward = lambda *a: (self.calls.append(("bwd",)), 0)[1]
        lib.rpr_adamw_step = lambda *a: (self.calls.append(("adamw", a[5])), 0)[1]
        self.ctx = types.SimpleNamespace(lib=lib, handle=None, device=torch.device("cpu"))
        self.model = types.SimpleNamespace(ctx=self.ctx, handle=None)


def test_step_and_rank_key_reach_the_engine(tmp_path, monkeypatch):
    """LngKnpTrainer -> model.training_step -> engine.train_step -> rpr_set_train_dropout(rate, key(seed, rank), global step)
    in front of every backward; a resumed trainer goes on at the recorded step; rate 0 (the default) passes nothing new."""
    from test_trainer_plumbing import CASES, WordTokenizer, _write
    from ripor_amd import engine as E
    from ripor_amd.dataset.lng_knp import LngKnpMarginMSEforT5SeqAQCollator, LngKnpMarginMSEforT5SeqAQDataset
    from ripor_amd.tasks import trainer as T
    monkeypatch.setenv("RPR_GRAD_OVERLAP", "0")
    monkeypatch.setattr(E, "_stream_ptr", lambda dev: None)
    _write(tmp_path, CASES["L8_smtid"]["files"])
    ds = LngKnpMarginMSEforT5SeqAQDataset(str(tmp_path / "examples.jsonl"), None, str(tmp_path / "queries"), None, True)
    coll = LngKnpMarginMSEforT5SeqAQCollator(WordTokenizer(), 16)

    class Model:
        def __init__(self):
            self.eng = _StubEngine()
            self.state = E.TrainState(self.eng.model)
            self.base_model = types.SimpleNamespace(engine_model=lambda: self.eng.model)
            self.eng.ctx.get_precision = lambda: "f16x2"
            self.eng.ctx.set_precision = lambda p: None
            self.kwargs = []

        def training_step(self, lr, **kw):
            self.kwargs.append({k: kw[k] for k in ("dropout_rate", "dropout_seed", "global_step") if k in kw})
            b = kw["pos_doc_encoding"].shape[0]
            E.train_step(self.eng.model, self.state, kw["pos_tokenized_query"]["input_ids"], kw["pos_tokenized_query"]["attention_mask"],
                         torch.zeros((b, 2, 8), dtype=torch.long), torch.zeros((2, b)), torch.zeros((2, b)), [8, 4], lr,
                         dropout_rate=kw.get("dropout_rate"), dropout_seed=kw.get("dropout_seed"), global_step=kw.get("global_step"))
            return {"rank": torch.tensor(1.0)}

    def run(rate, rank=0, start=0):
        m = Model()
        args = T.LngKnpTrainingArgs(output_dir=str(tmp_path / "o"), max_steps=3, per_device_train_batch_size=2, save_steps=0,
                                    logging_steps=10, seed=11, **({} if rate is None else dict(dropout_rate=rate)))
        tr = T.LngKnpTrainer(m, ds, coll, args, log=lambda s: None)
        tr.rank, tr.world, tr.global_step = rank, max(tr.world, rank + 1), start
        tr.train()
        return m

    m = run(0.1)
    key0 = T.dropout_key(11, 0)
    drops = [c for c in m.eng.calls if c[0] == "drop"]
    assert [(round(c[1], 6), c[2], c[3]) for c in drops] == [(0.1, key0, 0), (0.1, key0, 1), (0.1, key0, 2)]
    order = [c[0] for c in m.eng.calls]
    assert order == ["drop", "bwd", "adamw"] * 3                       # the setter in front of every backward
    m1 = run(0.1, rank=1)
    key1 = T.dropout_key(11, 1)
    assert key1 != key0 and 0 <= key1 < 2 ** 64 and {c[2] for c in m1.eng.calls if c[0] == "drop"} == {key1}
    resumed = run(0.1, start=2)                                         # what load_checkpoint_state leaves: global_step 2
    assert [c[3] for c in resumed.eng.calls if c[0] == "drop"] == [2]
    off = run(None)                                                     # the default
    assert T.LngKnpTrainingArgs(output_dir="x").dropout_rate == 0.0
    assert off.kwargs == [{}, {}, {}] and all(c[1] == 0.0 for c in off.eng.calls if c[0] == "drop")
