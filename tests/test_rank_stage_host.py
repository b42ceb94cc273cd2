"""not-gpu: the rank-oriented stage (loss_type t5seq_aq_encoder_margin_mse) on the host side — the dataset and the collator
against the reference's own on seeded files (tests/golden/make_golden_rank.py), the command line of main_rank, what the model
class refuses before it touches a device, the merge of the teacher's shards, add_qrel_to_rerank_run, and the aliases."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK_CASES = ["rk_mini_bz3_l4of8", "rk_mini_bz3_l8_shared", "rk_mini_bz4_l8", "rk_v11_mini_bz3_l8"]

# the literal flag lists of the reference's two invocations of this stage (shell variables expanded):
# full_scripts/full_train_t5seq_seq2seq_0_1_pipeline.sh:55-72 and full_scripts/full_lng_knp_train_pipline.sh:28-45
SCRIPT_FLAGS = {
    "seq2seq_1": ["--epochs=150", "--run_name=t5seq_aq_encoder_seq2seq_1", "--learning_rate=1e-4", "--loss_type=t5seq_aq_encoder_margin_mse",
                  "--model_name_or_path=t5-base", "--model_type=t5_docid_gen_encoder",
                  "--teacher_score_path=./experiments-full-t5seq-aq/t5_docid_gen_encoder_1/out/MSMARCO_TRAIN/"
                  "qrel_added_qid_docids_teacher_scores.train.json",
                  "--output_dir=./experiments-full-t5seq-aq/", '--task_names=["rank"]', "--wandb_project_name=full_t5seq_encoder",
                  "--use_fp16", "--collection_path=./data/msmarco-full/full_collection/", "--max_length=64",
                  "--per_device_train_batch_size=128", "--queries_path=./data/msmarco-full/all_train_queries/train_queries",
                  "--pretrained_path=./experiments-full-t5seq-aq/t5seq_aq_encoder_seq2seq_0/checkpoint",
                  "--docid_to_smtid_path=./experiments-full-t5seq-aq/t5_docid_gen_encoder_1/aq_smtid/docid_to_smtid.json"],
    "sub_smtid_4": ["--epochs=120", "--run_name=t5seq_aq_encoder_seq2seq_1_lng_knp_mnt_4_dcy_2", "--learning_rate=1e-4",
                    "--loss_type=t5seq_aq_encoder_margin_mse", "--model_name_or_path=t5-base", "--model_type=t5_docid_gen_encoder",
                    "--teacher_score_path=./experiments-full-t5seq-aq/t5seq_aq_encoder_seq2seq_1//sub_smtid_train_decay2/"
                    "qid_smtids_scores_4.train.json",
                    "--output_dir=./experiments-full-t5seq-aq/", '--task_names=["rank"]', "--wandb_project_name=full_t5seq_encoder",
                    "--use_fp16", "--collection_path=./data/msmarco-full/full_collection/", "--max_length=64",
                    "--per_device_train_batch_size=128", "--queries_path=./data/msmarco-full/all_train_queries/train_queries",
                    "--pretrained_path=./experiments-full-t5seq-aq/t5seq_aq_encoder_seq2seq_1/checkpoint", "--smtid_as_docid"],
}


class RankGolden:
    """A committed rk_ fixture: the weights are regenerated from the stored seed and dims."""

    def __init__(self, name):
        from ripor_amd.utils import synth
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.spec = json.loads(str(self.z["spec"]))
        self.dims = synth.ModelDims(**self.spec["dims"])
        self.bz, self.L, self.seed = self.spec["bz"], self.spec["L"], self.spec["seed"]
        self.kind = self.spec.get("feed_forward_proj", "relu")
        self._sd = None

    @property
    def state_dict(self):
        from ripor_amd.utils import synth
        if self._sd is None:
            self._sd = synth.make_state_dict(self.dims, seed=self.seed, feed_forward_proj=self.kind)
        return self._sd

    def inputs(self):
        t = torch.from_numpy
        start = np.full((self.bz, 1), -1, dtype=np.int64)
        pos, neg = self.z["pos_doc_encoding"], self.z["neg_doc_encoding"]

        def tq(codes):
            return {"input_ids": t(self.z["q_ids"]), "attention_mask": t(self.z["q_mask"]),
                    "decoder_input_ids": t(np.concatenate([start, codes[:, :-1]], axis=1))}

        return {"pos_tokenized_query": tq(pos), "neg_tokenized_query": tq(neg), "pos_doc_encoding": t(pos), "neg_doc_encoding": t(neg),
                "teacher_pos_scores": t(self.z["teacher_pos_scores"]), "teacher_neg_scores": t(self.z["teacher_neg_scores"])}

    def model(self, cls=None, device=None):
        """The class under test on this fixture's weights (on the CPU unless a device is given)."""
        from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig, T5ForDocIDGeneration, T5SeqAQEncoderForMarginMSE
        cls = cls or T5SeqAQEncoderForMarginMSE
        m = cls.__new__(cls)
        m.config = T5forDocIDConfig.from_dims(self.dims)
        m.config.feed_forward_proj = self.kind
        m.base_model = T5ForDocIDGeneration(m.config, self.state_dict)
        m.model_args = None
        if device is not None:
            m.base_model.to(device)
        return m


def test_fixtures_exist_are_small_and_hold_the_cases_they_name():
    for n in RK_CASES + ["rk_data"]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, n + ".npz")) < 1 << 20
    assert sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("rk_") and f.endswith(".npz")) == sorted(RK_CASES + ["rk_data"])
    g = RankGolden("rk_mini_bz4_l8")
    lens = g.z["q_mask"].sum(1).tolist()
    assert len(set(lens)) == 4 and 1 in lens and g.L == 8 == len(g.dims.decoder_vocab_sizes)
    assert g.z["q_ids"][lens.index(1)].tolist() == [1] + [0] * (g.z["q_ids"].shape[1] - 1)      # the single token </s>
    g = RankGolden("rk_mini_bz3_l4of8")
    assert g.L == 4 and len(g.dims.decoder_vocab_sizes) == 8 and g.z["pos_doc_encoding"].shape == (3, 4)
    names = [str(x) for x in g.z["grad_names"]]
    assert not any(n.startswith(f"list_{tab}_embeds.{i}.") for n in names for tab in ("decoder", "output") for i in range(4, 8))
    assert "list_output_embeds.3.weight" in names and "list_decoder_embeds.2.weight" in names
    g = RankGolden("rk_mini_bz3_l8_shared")
    assert g.dims.shared_output_input_embeds and not any("list_output_embeds" in str(x) for x in g.z["grad_names"])
    assert RankGolden("rk_v11_mini_bz3_l8").kind == "gated-gelu"


@pytest.mark.parametrize("name", RK_CASES)
def test_teacher_margins_are_away_from_the_student(name):
    """What the generator asserts: |margin - teacher margin| >= 1 % of the largest |score| for every example; and the stored loss
    is the MSE of exactly these numbers."""
    z = RankGolden(name).z
    scores = np.stack([z["pos_position_scores"].sum(-1), z["neg_position_scores"].sum(-1)], 1)
    margin = scores[:, 0] - scores[:, 1]
    teacher = z["teacher_pos_scores"].astype(np.float64) - z["teacher_neg_scores"].astype(np.float64)
    assert (np.abs(margin - teacher) >= 0.01 * np.abs(scores).max()).all()
    assert abs(np.mean((margin - teacher) ** 2) - float(z["loss"])) <= 1e-9 * float(z["loss"])


def _flat(batch):
    flat = {}
    for name, val in batch.items():
        if isinstance(val, torch.Tensor):
            flat[name] = val.tolist()
        else:
            flat.update({f"{name}.{k}": v.tolist() for k, v in val.items()})
    return flat


def _write_rk_files(root, files):
    os.makedirs(os.path.join(root, "queries"), exist_ok=True)
    for rel, key in (("queries/raw.tsv", "queries"), ("docid_to_smtid.json", "docid_to_smtid"),
                     ("examples_docid.jsonl", "examples_docid"), ("examples_smtid.jsonl", "examples_smtid")):
        with open(os.path.join(root, rel), "w") as f:
            f.write(files[key])


def test_dataset_and_collator_reproduce_the_reference(tmp_path):
    sys.path.insert(0, GOLDEN_DIR)
    from make_golden import WordTokenizer
    from ripor_amd.dataset.margin_mse import MarginMSEforT5SeqAQCollator, MarginMSEforT5SeqAQDataset
    z = np.load(os.path.join(GOLDEN_DIR, "rk_data.npz"))
    files, cases = json.loads(str(z["files"])), json.loads(str(z["cases"]))
    assert set(cases) == {"docid", "smtid"} and len(files["examples_docid"].splitlines()) == 6
    root = str(tmp_path)
    _write_rk_files(root, files)
    for form, c in cases.items():
        # document_dir names a directory that does not exist: the passages are never loaded
        ds = MarginMSEforT5SeqAQDataset(dataset_path=os.path.join(root, f"examples_{form}.jsonl"), document_dir=os.path.join(root, "absent"),
                                        query_dir=os.path.join(root, "queries"),
                                        docid_to_smtid_path=os.path.join(root, "docid_to_smtid.json") if form == "docid" else None,
                                        smtid_as_docid=form == "smtid")
        assert len(ds) == c["length"] == 6
        random.seed(c["random_seed"])                                # the negative is drawn with random.sample
        items = [ds[i] for i in c["order"]]
        assert [list(it) for it in items] == c["items"], form
        assert all(it[0].startswith("query: ") and it[0] == it[1] and it[6][0] == -1 and it[6][1:] == it[2][:-1] for it in items)
        assert len(items[0][2]) == (8 if form == "docid" else 4)
        batch = MarginMSEforT5SeqAQCollator(WordTokenizer(), max_length=c["max_length"])(items[:5])
        assert _flat(batch) == c["batch"], form
        assert batch["teacher_pos_scores"].dtype == torch.float32 and batch["pos_doc_encoding"].dtype == torch.long
        assert set(batch) == {"pos_tokenized_query", "neg_tokenized_query", "pos_doc_encoding", "neg_doc_encoding", "teacher_pos_scores",
                              "teacher_neg_scores"}
    with pytest.raises(AssertionError):     # the reference's assertion (dataset.py:565-567)
        MarginMSEforT5SeqAQDataset(os.path.join(root, "examples_smtid.jsonl"), None, os.path.join(root, "queries"),
                                   os.path.join(root, "docid_to_smtid.json"), smtid_as_docid=True)


def test_command_line_parses_the_reference_scripts_and_refuses_other_losses(tmp_path):
    from ripor_amd import main_rank as M
    for which, flags in SCRIPT_FLAGS.items():
        a = M.get_args(flags)
        assert a.loss_type == "t5seq_aq_encoder_margin_mse" and a.model_type == "t5_docid_gen_encoder" and a.use_fp16
        assert (a.learning_rate, a.max_length, a.per_device_train_batch_size) == (1e-4, 64, 128)
        assert json.loads(a.task_names) == ["rank"] and a.wandb_project_name == "full_t5seq_encoder"
        assert a.queries_path.endswith("train_queries") and a.pretrained_path.endswith("/checkpoint")
    a, b = M.get_args(SCRIPT_FLAGS["seq2seq_1"]), M.get_args(SCRIPT_FLAGS["sub_smtid_4"])
    assert a.epochs == 150 and not a.smtid_as_docid and a.docid_to_smtid_path.endswith("aq_smtid/docid_to_smtid.json")
    assert b.epochs == 120 and b.smtid_as_docid and b.docid_to_smtid_path is None
    a = M.get_args(["--pretrained_path", "p", "--output_dir", "o", "--max_steps", "7", "--save_steps", "0", "--logging_steps", "1",
                    "--resume_from_checkpoint", "c", "--dropout", "config", "--local_rank", "0"])
    assert (a.max_steps, a.save_steps, a.logging_steps, a.dropout, a.local_rank) == (7, 0, 1, "config", 0)
    assert a.loss_type == "t5seq_aq_encoder_margin_mse"
    base = ["--pretrained_path", "p", "--output_dir", str(tmp_path), "--teacher_score_path", "t", "--queries_path", "q"]
    for lt in ("t5seq_pretrain_margin_mse", "t5seq_aq_encoder_seq2seq", "t5seq_aq_encoder_lng_knp_margin_mse"):
        with pytest.raises(NotImplementedError, match="t5seq_aq_encoder_margin_mse only"):
            M.main(base + ["--smtid_as_docid", "--loss_type", lt])
    with pytest.raises(SystemExit, match="--max_length 257: the training passes take at most 256"):
        M.main(base + ["--smtid_as_docid", "--max_length", "257"])
    with pytest.raises(SystemExit, match="queries_path"):
        M.main(base[:-2] + ["--smtid_as_docid"])
    with pytest.raises(SystemExit, match="docid_to_smtid_path or --smtid_as_docid"):
        M.main(base)
    with pytest.raises(SystemExit, match="must not be given"):
        M.main(base + ["--smtid_as_docid", "--docid_to_smtid_path", "d.json"])


def test_main_still_refuses_this_loss_type_and_names_main_rank(tmp_path):
    from ripor_amd import main as M
    with pytest.raises(NotImplementedError, match=r"outside this repository.*t5seq_aq_encoder_margin_mse: python -m t5_pretrainer\.main_rank"):
        M.main(["--loss_type", "t5seq_aq_encoder_margin_mse", "--pretrained_path", "p", "--output_dir", str(tmp_path)])


def test_model_refuses_inconsistent_batches_before_it_touches_a_device():
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE, T5SeqAQEncoderForMarginMSE
    g = RankGolden("rk_mini_bz4_l8")
    m = g.model()                                        # on the CPU: anything that got as far as the engine would raise RiporHipError
    pos_q, codes, tp, tn, prefix_lens, names = m._batch(g.inputs(), check_shift=True)
    assert prefix_lens == [8] and names == ["rank"] and tuple(codes.shape) == (4, 2, 8) and tuple(tp.shape) == (1, 4) == tuple(tn.shape)
    assert tp.dtype == torch.float32
    for call in (m.forward, m.backward, lambda **kw: m.training_step(lr=1e-4, **kw)):
        bad = g.inputs()
        bad["neg_tokenized_query"]["input_ids"] = bad["neg_tokenized_query"]["input_ids"].clone()
        bad["neg_tokenized_query"]["input_ids"][0, 1] += 1
        with pytest.raises(ValueError, match="same query tokens"):
            call(**bad)
    for side in ("pos", "neg"):
        bad = g.inputs()
        bad[f"{side}_tokenized_query"]["decoder_input_ids"] = bad[f"{side}_tokenized_query"]["decoder_input_ids"].clone()
        bad[f"{side}_tokenized_query"]["decoder_input_ids"][1, 3] += 1
        with pytest.raises(ValueError, match=f"{side}: decoder_input_ids must be the doc encoding shifted right"):
            m(**bad)
    unshifted = g.inputs()
    unshifted["pos_tokenized_query"]["decoder_input_ids"] = unshifted["pos_doc_encoding"].clone()
    with pytest.raises(ValueError, match="shifted right"):
        m(**unshifted)

    def cut(inputs, L):
        out = dict(inputs)
        for side in ("pos", "neg"):
            out[f"{side}_doc_encoding"] = inputs[f"{side}_doc_encoding"][:, :L]
            out[f"{side}_tokenized_query"] = dict(inputs[f"{side}_tokenized_query"],
                                                  decoder_input_ids=inputs[f"{side}_tokenized_query"]["decoder_input_ids"][:, :L])
        return out

    with pytest.raises(ValueError, match="smtid length 1 is not built"):
        m(**cut(g.inputs(), 1))
    long = g.inputs()
    for side in ("pos", "neg"):
        long[f"{side}_doc_encoding"] = torch.cat([long[f"{side}_doc_encoding"], long[f"{side}_doc_encoding"][:, :1]], 1)
    with pytest.raises(ValueError, match=r"not valid length: 9 \(the model decodes 8 positions\)"):
        m(**long)
    # every length from 2 to the model's 8 is a batch of this class (no table of lengths) ...
    for L in range(2, 9):
        assert m._batch(cut(g.inputs(), L), check_shift=True)[4] == [L]
    # ... and the lng_knp class keeps its table and its guards: the two share them
    k = g.model(T5SeqAQEncoderForLngKnpMarginMSE)
    with pytest.raises(ValueError, match="not valid length: 6"):
        k(**cut(g.inputs(), 6))
    assert T5SeqAQEncoderForLngKnpMarginMSE._batch is T5SeqAQEncoderForMarginMSE._batch
    assert T5SeqAQEncoderForLngKnpMarginMSE.forward is T5SeqAQEncoderForMarginMSE.forward
    # rerank_forward: the same two guards
    with pytest.raises(ValueError, match="tokenized_query: decoder_input_ids must be the doc encoding shifted right"):
        m.rerank_forward(tokenized_query=unshifted["pos_tokenized_query"], doc_encoding=unshifted["pos_doc_encoding"])
    with pytest.raises(ValueError, match="smtid length 1"):
        c1 = cut(g.inputs(), 1)
        m.rerank_forward(tokenized_query=c1["pos_tokenized_query"], doc_encoding=c1["pos_doc_encoding"])


def test_merge_of_rerank_shards_sorts_cuts_and_cleans_up(tmp_path):
    from ripor_amd import rerank as R
    out = tmp_path / "out"
    out.mkdir()
    # q1: 250 passages over two shards, scores descending in steps with runs of equal scores; q2 in one shard; q3 in the other
    q1 = {f"d{i}": float(1000 - i // 3) for i in range(250)}
    first, second = dict(list(q1.items())[:120]), dict(list(q1.items())[120:])
    with open(out / "rerank_0.json", "w") as f:
        json.dump({"q1": first, "q2": {"a": 0.5, "b": 2.5, "c": 2.5, "d": -1.0}}, f)
    with open(out / "rerank_1.json", "w") as f:
        json.dump({"q3": {"x": 3.0}, "q1": second}, f)
    (out / R.TRAINSET_NAME).write_text("stale\n")
    (out / "rerank_perf.json").write_text("{}")                      # not a shard: left alone
    R.main(["--task=rerank_for_create_trainset_2", f"--out_dir={out}"])
    assert sorted(os.listdir(out)) == sorted([R.TRAINSET_NAME, "rerank_perf.json"])      # the shards are deleted
    assert R.TRAINSET_NAME == "qid_docids_teacher_scores.train.json"
    lines = [json.loads(l) for l in (out / R.TRAINSET_NAME).read_text().splitlines()]
    assert [set(ex) for ex in lines] == [{"qid", "docids", "scores"}] * 3
    by = {ex["qid"]: ex for ex in lines}
    assert set(by) == {"q1", "q2", "q3"}
    assert by["q1"]["docids"] == [f"d{i}" for i in range(200)]          # cut at 200; equal scores in the order they were read
    assert by["q1"]["scores"] == [float(1000 - i // 3) for i in range(200)]
    assert by["q2"]["docids"] == ["b", "c", "a", "d"] and by["q2"]["scores"] == [2.5, 2.5, 0.5, -1.0]
    assert by["q3"] == {"qid": "q3", "docids": ["x"], "scores": [3.0]}
    assert {"rerank_for_create_trainset", "rerank_for_create_trainset_2"} <= set(R.BUILT_TASKS)
    assert not {"rerank_for_create_trainset", "rerank_for_create_trainset_2"} & set(R.UNBUILT_TASKS) and len(R.UNBUILT_TASKS) >= 3


def test_run_file_is_read_in_both_forms(tmp_path):
    from ripor_amd import rerank as R
    (tmp_path / "run.json").write_text(json.dumps({"7": {"d2": 1.0, "d1": 3.0}, "8": {"d3": 0.0}}))
    (tmp_path / "run.jsonl").write_text(json.dumps({"qid": 7, "docids": ["d2", "d1"]}) + "\n" + json.dumps({"qid": "8", "docids": ["d3"]}) + "\n")
    want = {"7": ["d2", "d1"], "8": ["d3"]}
    assert R.read_run(str(tmp_path / "run.json"), "json") == want and R.read_run(str(tmp_path / "run.jsonl"), "jsonl") == want
    assert list(R.shard_qids(want, 2, 1)) == ["8"]
    assert R.pair_ids_to_json_output([0.5, 1.5, 2.0], [("7", "d2", ""), ("7", "d1", ""), ("8", "d3", "")]) == \
        {"7": {"d2": 0.5, "d1": 1.5}, "8": {"d3": 2.0}}
    assert R.get_args(["--task=rerank_for_create_trainset", "--json_type=json"]).json_type == "json"


def test_add_qrel_to_rerank_run(tmp_path):
    from ripor_amd.aq_preprocess import add_qrel_to_rerank_run as A
    run = [{"qid": "1", "docids": ["a", "b", "c"], "scores": [9.0, 5.0, 1.0]},
           {"qid": "2", "docids": ["d", "e"], "scores": [4.0, 3.0]}]
    qrels = {"1": {"b": 7.5, "z": 8.25}, "2": {"y": -2.0}, "3": {"unused": 1.0}}
    (tmp_path / "run.jsonl").write_text("".join(json.dumps(ex) + "\n" for ex in run))
    (tmp_path / "qrels.json").write_text(json.dumps(qrels))
    A.main(["--qid_to_reldocid_to_score_path", str(tmp_path / "qrels.json"), "--teacher_score_path", str(tmp_path / "run.jsonl"),
            "--out_path", str(tmp_path / "out.jsonl")])
    got = [json.loads(l) for l in (tmp_path / "out.jsonl").read_text().splitlines()]
    assert got == [
        run[0],                                                                    # "b" is among the docids: unchanged
        {"qid": "1", "docids": ["z", "a", "b", "c"], "scores": [8.25, 9.0, 5.0, 1.0]},    # "z" is not: put in front with its score
        {"qid": "2", "docids": ["y", "d", "e"], "scores": [-2.0, 4.0, 3.0]}]
    assert A.add_qrels(run, qrels)[1] == 2


def test_aliases_resolve_to_the_same_objects():
    import t5_pretrainer.aq_preprocess.add_qrel_to_rerank_run as alias_add
    import t5_pretrainer.main_rank as alias_main
    import t5_pretrainer.rerank as alias_rerank
    from ripor_amd import main_rank, rerank
    from ripor_amd.aq_preprocess import add_qrel_to_rerank_run
    from ripor_amd.dataset.margin_mse import MarginMSEforT5SeqAQCollator, MarginMSEforT5SeqAQDataset
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder, T5SeqAQEncoderForMarginMSE
    from t5_pretrainer.dataset.data_collator import MarginMSEforT5SeqAQCollator as C2
    from t5_pretrainer.dataset.dataset import MarginMSEforT5SeqAQDataset as D2
    from t5_pretrainer.modeling.t5_generative_retriever import T5SeqAQEncoder as E2
    from t5_pretrainer.modeling.t5_generative_retriever import T5SeqAQEncoderForMarginMSE as M2
    assert C2 is MarginMSEforT5SeqAQCollator and D2 is MarginMSEforT5SeqAQDataset and M2 is T5SeqAQEncoderForMarginMSE
    assert E2 is T5SeqAQEncoder and callable(E2.rerank_forward) and issubclass(M2, T5SeqAQEncoder)
    assert alias_main.main is main_rank.main and alias_main.get_args is main_rank.get_args
    assert alias_add.main is add_qrel_to_rerank_run.main
    assert alias_rerank.main is rerank.main and alias_rerank.rerank_for_create_trainset_2 is rerank.rerank_for_create_trainset_2
