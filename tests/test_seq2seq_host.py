"""not-gpu: the seq2seq docid step (loss_type t5seq_aq_encoder_seq2seq) on the host side — a torch autograd restatement of
the reference's T5SeqAQEncoderForSeq2Seq pinned to the s2s_* fixtures (tests/golden/make_golden_seq2seq.py), the dataset and
collator against the reference's own on seeded files, the command line, and the C ABI of the device step."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

S2S_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("s2s_") and f.endswith(".npz") and f != "s2s_data.npz")


class S2SGolden:
    def __init__(self, name):
        from ripor_amd.utils import synth
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.spec = json.loads(str(self.z["spec"]))
        self.dims = synth.ModelDims(**self.spec["dims"])
        self.bz, self.L, self.V, self.seed = self.spec["bz"], self.spec["L"], self.spec["V"], self.spec["seed"]
        self.state_dict = synth.make_state_dict(self.dims, seed=self.seed)

    def inputs(self):
        t = torch.from_numpy
        labels = self.z["labels"]
        dec_in = np.concatenate([np.full((self.bz, 1), -1, dtype=np.int64), labels[:, :-1]], axis=1)
        return {"tokenized_query": {"input_ids": t(self.z["input_ids"]), "attention_mask": t(self.z["attention_mask"]),
                                    "decoder_input_ids": t(dec_in)}, "labels": t(labels)}


def seq2seq_ce(model, input_ids, attention_mask, labels):
    """Restatement of T5SeqAQEncoderForSeq2Seq.forward (reference :968-1019) on the CPU oracle: h = decoder_last_hidden_state
    of the teacher-forced pass over [-1, labels[:, :-1]], logits[:, i] = h[:, i] E_i^T (output codebook, or the input one when
    shared), nn.CrossEntropyLoss over the bz * L rows. Returns (loss, label log-probabilities [bz, L])."""
    ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    mask = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    bz, L = lab.shape
    enc = model.encode(ids, mask)
    dec_in = torch.cat([torch.full((bz, 1), -1, dtype=torch.long), lab[:, :-1]], dim=1)
    h = model.decode_full(dec_in, enc, mask)                                          # [bz, L, d]
    logits = torch.stack([h[:, i] @ model.out_embed(i).t() for i in range(L)], dim=1)   # [bz, L, V]
    loss = torch.nn.functional.cross_entropy(logits.reshape(bz * L, -1), lab.reshape(-1))
    lp = torch.log_softmax(logits, -1).gather(-1, lab[..., None])[..., 0]
    return loss, lp


def seq2seq_grads(model, input_ids, attention_mask, labels):
    """Autograd of seq2seq_ce: (loss, grads: state-dict name -> tensor, global norm)."""
    for t in model.sd.values():
        t.requires_grad_(True)
        t.grad = None
    loss, _ = seq2seq_ce(model, input_ids, attention_mask, labels)
    loss.backward()
    grads = {k: t.grad.detach().clone() for k, t in model.sd.items() if t.grad is not None}
    for t in model.sd.values():
        t.requires_grad_(False)
        t.grad = None
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    return float(loss.detach()), grads, gn


def check_grads(g, grads, rel=2e-4, label=""):
    """grads: state-dict name -> numpy array. Every gradient tensor of the fixture must match in Frobenius norm and at the
    sampled positions (tests/golden/make_golden.py::grad_samples); the tolerance is relative to the tensor's scale.
    Returns (worst sampled error, tensor name)."""
    from test_oracle_golden import grad_sample_indices
    names = [str(x) for x in g.z["grad_names"]]
    norms, counts, samples = g.z["grad_norms"], g.z["grad_sample_counts"], g.z["grad_samples"]
    off, worst = 0, (0.0, "")
    for n, nr, c in zip(names, norms, counts):
        ref = samples[off:off + c]
        off += c
        key = "shared.weight" if n == "encoder.embed_tokens.weight" else n
        arr = np.asarray(grads[key], dtype=np.float64)
        got = arr.reshape(-1)[grad_sample_indices(n, arr.shape)]
        scale = max(np.abs(ref).max(), nr / np.sqrt(arr.size), 1e-12)
        err = float(np.abs(got - ref).max() / scale)
        worst = max(worst, (err, n))
        assert err <= rel * 10, f"{g.name}{label} gradient of {n}: sampled entries differ by {err:.2e} of its scale"
        gnr = np.sqrt((arr ** 2).sum())
        assert abs(gnr - nr) <= rel * max(nr, 1e-12), f"{g.name}{label} gradient norm of {n}: {gnr} vs {nr}"
    return worst


def test_fixtures_exist_and_are_small():
    names = set(S2S_CASES)
    assert {"s2s_mini_bz4_l8", "s2s_mini_bz4_l16", "s2s_mini_bz4_l32", "s2s_mini_bz3_l16_v1024", "s2s_mini_bz4_l8_shared",
            "s2s_base_bz4_l32"} <= names
    for n in names | {"s2s_data"}:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, n + ".npz")) < 1 << 20


@pytest.mark.parametrize("name", [n for n in S2S_CASES if "mini" in n])
def test_autograd_restatement_matches_reference_fixture(name):
    from oracle import t5_ref
    g = S2SGolden(name)
    torch.set_num_threads(8)
    model = t5_ref.T5Ref(g.state_dict, g.dims)
    with torch.no_grad():
        loss, lp = seq2seq_ce(model, g.z["input_ids"], g.z["attention_mask"], g.z["labels"])
    assert abs(float(loss) - float(g.z["loss"])) <= 1e-5 * max(1.0, abs(float(g.z["loss"])))
    # multi_vocab_sizes: the per-position mean / L is the same value when every position has the same V
    assert abs(float(g.z["loss_multi_vocab"]) - float(g.z["loss"])) <= 1e-5 * abs(float(g.z["loss"]))
    np.testing.assert_allclose(lp.numpy(), g.z["label_logprobs"], atol=1e-5 * max(1.0, np.abs(g.z["label_logprobs"]).max()), rtol=0)
    total, grads, gn = seq2seq_grads(model, g.z["input_ids"], g.z["attention_mask"], g.z["labels"])
    assert abs(gn - float(g.z["grad_global_norm"])) <= 1e-4 * gn
    check_grads(g, {k: v.numpy() for k, v in grads.items()}, label=" (seq2seq oracle)")
    if g.dims.shared_output_input_embeds:
        assert not any(k.startswith("list_output_embeds") for k in grads)


def _write(root, files):
    with open(os.path.join(root, "query_to_docid.jsonl"), "w") as f:
        f.write(files["examples"])
    with open(os.path.join(root, "docid_to_smtid.json"), "w") as f:
        f.write(files["docid_to_smtid"])


def test_dataset_and_collator_reproduce_the_reference():
    import sys
    sys.path.insert(0, GOLDEN_DIR)
    from make_golden import WordTokenizer
    from ripor_amd.dataset.seq2seq import Seq2SeqForT5SeqAQCollator, Seq2SeqForT5SeqAQDataset
    from t5_pretrainer.dataset.data_collator import Seq2SeqForT5SeqAQCollator as C2
    from t5_pretrainer.dataset.dataset import Seq2SeqForT5SeqAQDataset as D2
    assert C2 is Seq2SeqForT5SeqAQCollator and D2 is Seq2SeqForT5SeqAQDataset
    cases = json.loads(str(np.load(os.path.join(GOLDEN_DIR, "s2s_data.npz"))["cases"]))
    assert set(cases) == {"L4", "L8", "L32"}
    import tempfile
    for key, c in cases.items():
        with tempfile.TemporaryDirectory() as root:
            _write(root, c["files"])
            ds = Seq2SeqForT5SeqAQDataset(os.path.join(root, "query_to_docid.jsonl"), os.path.join(root, "docid_to_smtid.json"))
            assert len(ds) == c["length"]
            items = [ds[i] for i in c["order"]]
            assert [list(it) for it in items] == c["items"], key
            batch = Seq2SeqForT5SeqAQCollator(WordTokenizer(), max_length=c["max_length"])(items[:4])
            flat = {f"tokenized_query.{k}": v.tolist() for k, v in batch["tokenized_query"].items()}
            flat["labels"] = batch["labels"].tolist()
            assert flat == c["batch"], key
            assert batch["labels"].dtype == torch.long and batch["tokenized_query"]["decoder_input_ids"].dtype == torch.long


def test_command_line_accepts_seq2seq_and_refuses_other_losses(tmp_path):
    from ripor_amd import main as M
    a = M.get_args(["--loss_type", "t5seq_aq_encoder_seq2seq", "--pretrained_path", "p", "--output_dir", "o",
                    "--query_to_docid_path", "q.jsonl", "--docid_to_smtid_path", "d.json", "--multi_vocab_sizes"])
    assert a.loss_type == "t5seq_aq_encoder_seq2seq" and a.query_to_docid_path == "q.jsonl" and a.multi_vocab_sizes
    assert not M.get_args(["--pretrained_path", "p", "--output_dir", "o"]).multi_vocab_sizes
    for lt in ("t5seq_aq_encoder_margin_mse", "t5seq_pretrain_margin_mse"):
        with pytest.raises(NotImplementedError, match="outside this repository"):
            M.main(["--loss_type", lt, "--pretrained_path", "p", "--output_dir", str(tmp_path), "--query_to_docid_path", "q"])
    with pytest.raises(SystemExit, match="query_to_docid_path"):
        M.main(["--loss_type", "t5seq_aq_encoder_seq2seq", "--pretrained_path", "p", "--output_dir", str(tmp_path),
                "--docid_to_smtid_path", "d.json"])


def test_abi_exports_the_seq2seq_step():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    lib = _lib.load()
    assert lib.rpr_abi_version() == _lib.ABI_VERSION == 5
    for name in ("rpr_seq2seq_forward", "rpr_seq2seq_backward", "rpr_seq2seq_backward_buckets"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "ripor_hip.h")).read()
    assert "int rpr_seq2seq_backward_buckets(" in hdr
    # NULL arguments are refused without a device
    assert lib.rpr_seq2seq_forward(None, None, None, None, 1, 1, None, 1, None, None, None) == -1
