"""not-gpu: the host side of the cross-encoder teacher. The plain-torch restatement tests/xenc_ref.py against the HF fp64
logits of the fixtures (padded and packed form), the packing, the checkpoint reader, rerank.py's sharding / triple order /
output structure / merge and the preprocess script against the reference's own output (c10_rerank_callers.json), and the ABI."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xenc_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(m, k) for m, keys in ref.FIXTURES.items() for k in keys]


@pytest.fixture(scope="module")
def c10():
    with open(os.path.join(ref.GOLDEN, "c10_rerank_callers.json")) as f:
        return json.load(f)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,key", CASES)
def test_restatement_reproduces_hf_fp64(model, key):
    from ripor_amd import engine as E
    fx = ref.load_fixture(model)
    b = fx["batches"][key]
    padded = ref.forward_padded(fx["weights"], fx["cfg"], b["ids"], b["types"], b["mask"]).numpy()
    assert np.abs(padded - b["fp64"]).max() <= 1e-9
    pk = E.xenc_pack(torch.from_numpy(b["ids"]), torch.from_numpy(b["types"]), torch.from_numpy(b["mask"]))
    packed = ref.forward_packed(fx["weights"], fx["cfg"], *pk).numpy()
    assert np.abs(packed - b["fp64"]).max() <= 1e-9
    assert np.abs(b["fp32"].astype(np.float64) - b["fp64"]).max() <= 6e-7   # what CPU fp32 itself does on these shapes (5.5e-7 at most)


def test_fixture_batches_are_what_they_claim():
    x1, x2 = ref.load_fixture("x1"), ref.load_fixture("x2")
    assert (x1["cfg"].hidden, x1["cfg"].heads, x1["cfg"].d_ff, x1["cfg"].max_pos) == (64, 2, 96, 512)
    assert (x2["cfg"].hidden, x2["cfg"].heads, x2["cfg"].d_ff, x2["cfg"].max_pos) == (128, 2, 160, 192)
    for fx in (x1, x2):
        lens = {k: b["mask"].sum(1).tolist() for k, b in fx["batches"].items()}
        assert lens["a"] == [1] and lens["c"] == [127, 128, 129] and len(lens["d"]) == 70 and set(lens["d"]) == {1, 2, 3, 4, 5}
        assert lens["b"] == [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 40]
        f = fx["batches"]["f"]
        assert f["mask"].shape == (4, 24) and f["mask"][0, 11] == 0 and f["mask"][1, 5] == 0 and set(np.unique(f["types"])) == {0, 1}
        assert len(f["fp64"]) > 1 and f["fp64"].std() > 0.05   # the pairs do not all score the same
    assert x1["batches"]["e"]["mask"].sum(1).tolist() == [512, 7]


# ---- packing -----------------------------------------------------------------------------------------------------------
def test_pack_maps_masks_with_holes_exactly():
    from ripor_amd import engine as E
    ids = torch.tensor([[5, 6, 7, 8, 9], [1, 2, 3, 4, 0], [11, 0, 0, 0, 0]])
    types = torch.tensor([[0, 0, 1, 1, 1], [0, 1, 1, 1, 0], [1, 0, 0, 0, 0]])
    mask = torch.tensor([[1, 1, 0, 1, 1], [1, 1, 1, 0, 0], [1, 0, 0, 0, 0]])
    pi, pt, pp, off = E.xenc_pack(ids, types, mask)
    assert pi.tolist() == [5, 6, 8, 9, 1, 2, 3, 11] and pi.dtype == torch.int32
    assert pt.tolist() == [0, 0, 1, 1, 0, 1, 1, 1]
    assert pp.tolist() == [0, 1, 3, 4, 0, 1, 2, 0]      # the original columns: the hole does not shift what follows
    assert off.tolist() == [0, 4, 7, 8] and off.dtype == np.int32
    pi2, pt2, _, _ = E.xenc_pack(ids, None, mask)
    assert pi2.tolist() == pi.tolist() and pt2.tolist() == [0] * 8   # missing token types are zeros


def test_pack_refuses_masked_first_column():
    from ripor_amd import engine as E
    ids = torch.ones((2, 3), dtype=torch.long)
    with pytest.raises(ValueError, match="column 0"):
        E.xenc_pack(ids, None, torch.tensor([[1, 1, 0], [0, 1, 1]]))


# ---- checkpoints -------------------------------------------------------------------------------------------------------
def _hf_dir(tmp_path, name="hf", **over):
    from transformers import BertConfig, BertForSequenceClassification
    torch.manual_seed(3)
    cfg = BertConfig(vocab_size=50, hidden_size=32, num_hidden_layers=2, num_attention_heads=1, intermediate_size=64,
                     max_position_embeddings=40, type_vocab_size=2, num_labels=1)
    model = BertForSequenceClassification(cfg).eval()
    d = str(tmp_path / name)
    model.save_pretrained(d)
    if over:
        with open(os.path.join(d, "config.json")) as f:
            c = json.load(f)
        c.update(over)
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(c, f)
    return d, model


@pytest.mark.parametrize("with_position_ids,fmt", [(False, "safetensors"), (True, "safetensors"), (True, "bin")])
def test_checkpoint_round_trip(tmp_path, with_position_ids, fmt):
    from safetensors.torch import load_file, save_file
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    d, model = _hf_dir(tmp_path)
    st = os.path.join(d, "model.safetensors")
    sd = load_file(st)
    sd.pop("bert.embeddings.position_ids", None)
    if with_position_ids:
        sd["bert.embeddings.position_ids"] = torch.arange(40)[None]   # the buffer old checkpoints carry
    if fmt == "bin":   # the older layout: pytorch_model.bin under the same BERT tensor names
        os.remove(st)
        torch.save(sd, os.path.join(d, "pytorch_model.bin"))
    else:
        save_file(sd, st)
    ce = CrossEncoder.from_pretrained(d)
    assert (ce.cfg.hidden, ce.cfg.layers, ce.cfg.heads, ce.cfg.d_ff, ce.cfg.max_pos, ce.cfg.vocab_size) == (32, 2, 1, 64, 40, 50)
    hf = model.state_dict()
    w = ce._weights
    assert torch.equal(w["qkv_w"][1], torch.cat([hf[f"bert.encoder.layer.1.attention.self.{x}.weight"] for x in ("query", "key", "value")]))
    assert torch.equal(w["ff2_w"][0], hf["bert.encoder.layer.0.output.dense.weight"])
    assert torch.equal(w["cls_w"], hf["classifier.weight"][0]) and torch.equal(w["pool_b"], hf["bert.pooler.dense.bias"])
    # the loaded weights compute what HF computes
    ids = torch.randint(0, 50, (3, 9)); mask = torch.ones_like(ids); mask[1, 6:] = 0
    types = torch.zeros_like(ids); types[:, 4:] = 1
    with torch.no_grad():
        want = model.double()(input_ids=ids, token_type_ids=types, attention_mask=mask).logits.view(-1)
    got = ref.forward_padded(w, ce.cfg, ids, types, mask)
    assert (got - want).abs().max() <= 1e-9
    with pytest.raises(NotImplementedError):
        ce.forward(qd_kwargs={"input_ids": ids, "attention_mask": mask}, labels=torch.zeros(3))


@pytest.mark.parametrize("over,word", [({"hidden_act": "relu"}, "hidden_act"), ({"model_type": "roberta"}, "model_type"),
                                       ({"position_embedding_type": "relative_key"}, "position_embedding_type")])
def test_unbuilt_configs_are_refused(tmp_path, over, word):
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    d, _ = _hf_dir(tmp_path, **over)
    with pytest.raises(ValueError, match=word):
        CrossEncoder(d)


def test_two_label_classifier_is_refused(tmp_path):
    from safetensors.torch import load_file, save_file
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    d, _ = _hf_dir(tmp_path)
    st = os.path.join(d, "model.safetensors")
    sd = load_file(st)
    sd["classifier.weight"] = torch.zeros(2, 32); sd["classifier.bias"] = torch.zeros(2)
    save_file(sd, st)
    with pytest.raises(ValueError, match="classifier"):
        CrossEncoder(d)


# ---- rerank.py and the preprocess script against the reference's output ----------------------------------------------------
def test_preprocess_equals_reference(tmp_path, c10):
    from t5_pretrainer.aq_preprocess.argparse_from_qid_smtid_rank_to_qid_smtid_docids import main
    with open(tmp_path / "qid_smtid_rankdata.json", "w") as f:
        json.dump(c10["rankdata"], f)
    main(["--root_dir", str(tmp_path)])
    with open(tmp_path / "qid_smtid_docids.train.json") as f:
        got = json.load(f)
    assert got == c10["qid_smtid_docids"]
    assert list(got) == list(c10["qid_smtid_docids"]) and "3_2" not in got["q7"]   # file order kept, the empty smtid dropped


def test_sharding_triples_and_output_equal_reference(c10):
    from ripor_amd import rerank as R
    seen = []
    for shard in c10["shards"]:
        sampled = R.shard_qids(c10["qid_smtid_docids"], c10["world"], shard["rank"])
        triples = R.build_triples(sampled)
        assert [list(t) for t in triples] == shard["triples"]
        out = R.triple_ids_to_json_output(shard["scores"], triples)
        assert json.loads(json.dumps(out)) == shard["output"]
        assert [list(v) for v in out.values()] == [list(v) for v in shard["output"].values()]   # smtid order too
        seen += list(sampled)
    assert sorted(seen) == sorted(c10["qid_smtid_docids"])


def test_score_triples_batches_in_order():
    from ripor_amd import rerank as R
    triples = [("q1", "d1", "s"), ("q1", "d2", "s"), ("q2", "d1", "t")]
    calls = []

    def tok(queries, docs, **kw):
        calls.append((list(queries), list(docs), kw))
        return {"n": len(queries)}
    scores = R.score_triples(triples, {"q1": "a", "q2": "b"}, {"d1": "x", "d2": "y"}, tok,
                             lambda kw: torch.arange(kw["n"], dtype=torch.float32) + 10 * len(calls), batch_size=2, max_length=17)
    assert scores == [10.0, 11.0, 20.0]
    assert [(c[0], c[1]) for c in calls] == [(["a", "a"], ["x", "y"]), (["b"], ["x"])]
    assert calls[0][2] == dict(padding=True, truncation="longest_first", return_attention_mask=True, return_tensors="pt", max_length=17)


def test_shard_path():
    from ripor_amd import rerank as R
    assert R.teacher_score_path("./out/x/qid_smtid_docids.train.json", 3) == "./out/x/qid_smtid_docids_teacher_score_3.train.json"
    assert R.teacher_score_path("/a/b.c/qid_smtid_docids.train.json", 0) == "/a/b.c/qid_smtid_docids_teacher_score_0.train.json"


def test_merge_equals_reference_and_removes_shards(tmp_path, c10):
    from ripor_amd import rerank as R
    for name, shard in zip(c10["shard_files"], c10["shards"]):
        with open(tmp_path / name, "w") as f:
            json.dump(shard["output"], f)
    with open(tmp_path / R.MERGED_NAME, "w") as f:
        f.write("{\"stale\": {}}")   # an old merged file goes first
    R.main(["--task", "cross_encoder_rerank_for_qid_smtid_docids_2", "--out_dir", str(tmp_path)])
    assert sorted(os.listdir(tmp_path)) == c10["after_merge_files"]
    with open(tmp_path / R.MERGED_NAME) as f:
        assert json.load(f) == c10["merged"]


def test_merge_concatenates_lists(tmp_path):
    from ripor_amd import rerank as R
    for r, rows in enumerate(([["d1", 1.0]], [["d2", 2.0]])):
        with open(tmp_path / f"qid_smtid_docids_teacher_score_{r}.train.json", "w") as f:
            json.dump({"q": {"s": rows}}, f)
    got = R.merge_shards(str(tmp_path))
    assert sorted(got["q"]["s"]) == [["d1", 1.0], ["d2", 2.0]]


def test_unbuilt_task_raises():
    from ripor_amd import rerank as R
    for task in R.UNBUILT_TASKS[:3] + ("nonsense",):
        with pytest.raises(NotImplementedError, match="cross_encoder_rerank_for_qid_smtid_docids_2"):
            R.main(["--task", task])
    import t5_pretrainer.rerank as alias
    import t5_pretrainer.modeling.cross_encoder as alias_ce
    from ripor_amd.modeling.cross_encoder import CrossEncoder
    assert alias.main is R.main and alias_ce.CrossEncoder is CrossEncoder


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_desc_layout():
    from ripor_amd import _lib
    lib = _lib.load()
    for name in ("rpr_xenc_load", "rpr_xenc_free", "rpr_xenc_score"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.rpr_abi_version() == 5
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    body = re.search(r"typedef struct rpr_xenc_desc \{(.*?)\} rpr_xenc_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"(int32_t|float|const float)\s*(.*)", decl, re.S).groups()
        for n in names.split(","):
            n = n.strip()
            fields.append((n.lstrip("*").strip(), "ptr" if n.startswith("*") else ctype))
    want = {"int32_t": C.c_int32, "float": C.c_float, "ptr": C.c_void_p}
    assert [(n, want[t]) for n, t in fields] == list(_lib.XencDesc._fields_)
    assert C.sizeof(_lib.XencDesc) == 8 * 4 + 21 * C.sizeof(C.c_void_p)
