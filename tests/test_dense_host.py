"""not-gpu: the dense first-stage step (loss_type t5seq_pretrain_margin_mse) on the host side — the float64 restatement of the
reference's T5SeqPretrainEncoder (tests/dense_ref.py) pinned to the pre_* fixtures (tests/golden/make_golden_pretrain.py), the
dataset and collator against the reference's own on seeded files, the command line, loading a plain T5 checkpoint, the
attention plans of a one-position decoder, and the C ABI of the device step."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from dense_ref import PRE_CASES, PreGolden, dense_grads, dense_margin_mse, dense_margin_mse_stacked, golden_groups

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = 1e-9

# the literal flag lists of the reference's full_scripts/full_train_t5seq_encoder_0.sh and _1.sh (shell variables expanded)
SCRIPT_FLAGS = {
    "0": ["--epochs=50", "--run_name=t5_docid_gen_encoder_0", "--learning_rate=1e-4", "--loss_type=t5seq_pretrain_margin_mse",
          "--model_name_or_path=t5-base", "--model_type=t5_docid_gen_encoder",
          "--teacher_score_path=./data/msmarco-full/bm25_run/qrel_added_qid_docids_teacher_scores.train.json",
          "--output_dir=./experiments-full-t5seq-aq/", '--task_names=["rank"]', "--wandb_project_name=full_t5seq_encoder", "--use_fp16",
          "--collection_path=./data/msmarco-full/full_collection/", "--max_length=128", "--per_device_train_batch_size=64",
          "--queries_path=./data/msmarco-full/all_train_queries/train_queries", "--pretrained_path=t5-base"],
    "1": ["--epochs=50", "--run_name=t5_docid_gen_encoder_1", "--learning_rate=1e-4", "--loss_type=t5seq_pretrain_margin_mse",
          "--model_name_or_path=t5-base", "--model_type=t5_docid_gen_encoder",
          "--teacher_score_path=./experiments-full-t5seq-aq/t5_docid_gen_encoder_0/all_train/MSMARCO_TRAIN/"
          "qrel_added_qid_docids_teacher_scores.train.json",
          "--output_dir=./experiments-full-t5seq-aq/", '--task_names=["rank"]', "--wandb_project_name=full_t5seq_encoder", "--use_fp16",
          "--collection_path=./data/msmarco-full/full_collection/", "--max_length=128", "--per_device_train_batch_size=64",
          "--queries_path=./data/msmarco-full/all_train_queries/train_queries",
          "--pretrained_path=./experiments-full-t5seq-aq/t5_docid_gen_encoder_0/checkpoint/"],
}


def test_fixtures_exist_and_are_small():
    assert set(PRE_CASES) == {"pre_mini_bz3_q9_d24", "pre_mini_bz1_q5_d12", "pre_mini_bz2_q8_d96", "pre_v11_mini_bz3_q7_d20"}
    for n in PRE_CASES + ["pre_data"]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, n + ".npz")) < 1 << 20
    g = PreGolden("pre_mini_bz3_q9_d24")
    lens = {k: g.z[k + "_mask"].sum(1).tolist() for k in ("q", "pd", "nd")}
    assert all(len(set(v)) == 3 for v in lens.values()) and g.z["q_ids"].shape[1] == 9 and g.z["pd_ids"].shape[1] == 24
    assert g.z["pd_ids"][1].tolist() == [1] + [0] * 23          # a document that is the single token </s>
    assert PreGolden("pre_mini_bz2_q8_d96").z["pd_ids"].shape[1] == 96
    assert PreGolden("pre_v11_mini_bz3_q7_d20").kind == "gated-gelu"


@pytest.mark.parametrize("name", PRE_CASES)
def test_teacher_margins_are_away_from_the_student(name):
    """What the generator asserts: |margin - teacher margin| >= 1 % of the largest |score| for every example."""
    z = PreGolden(name).z
    margin = z["scores"][:, 0] - z["scores"][:, 1]
    teacher = z["teacher_pos"].astype(np.float64) - z["teacher_neg"].astype(np.float64)
    assert (np.abs(margin - teacher) >= 0.01 * np.abs(z["scores"]).max()).all()


@pytest.mark.parametrize("name", PRE_CASES)
def test_float64_restatement_matches_reference_fixture(name):
    from test_oracle_golden import grad_sample_indices
    g = PreGolden(name)
    torch.set_num_threads(8)
    model = g.ref_model()
    groups = golden_groups(g)
    with torch.no_grad():
        loss, scores, reps = dense_margin_mse(model, groups, g.z["teacher_pos"], g.z["teacher_neg"])
    assert scores.dtype == torch.float64
    assert abs(float(loss) - float(g.z["loss"])) <= TOL64 * abs(float(g.z["loss"]))
    assert np.abs(scores.numpy() - g.z["scores"]).max() <= TOL64 * np.abs(g.z["scores"]).max()
    assert np.abs(reps.numpy() - g.z["reps"]).max() <= TOL64 * np.abs(g.z["reps"]).max()
    # the device step's layout, all three groups padded to one length: the same values
    with torch.no_grad():
        loss1, scores1, _ = dense_margin_mse_stacked(model, *g.stacked(), g.z["teacher_pos"], g.z["teacher_neg"])
    assert abs(float(loss1) - float(g.z["loss"])) <= TOL64 * abs(float(g.z["loss"]))
    assert np.abs(scores1.numpy() - g.z["scores"]).max() <= TOL64 * np.abs(g.z["scores"]).max()
    total, grads, gn = dense_grads(model, dense_margin_mse, groups, g.z["teacher_pos"], g.z["teacher_neg"])
    assert abs(gn - float(g.z["grad_global_norm"])) <= TOL64 * gn
    assert not any(k.startswith("list_") for k in grads)            # no codebook is reached
    assert float(grads["start_token_embed"].abs().max()) > 0
    off = 0
    for n, nr, c in zip([str(x) for x in g.z["grad_names"]], g.z["grad_norms"], g.z["grad_sample_counts"]):
        ref = g.z["grad_samples"][off:off + c]
        off += c
        arr = grads["shared.weight" if n == "encoder.embed_tokens.weight" else n].numpy()
        got = arr.reshape(-1)[grad_sample_indices(n, arr.shape)]
        scale = max(np.abs(ref).max(), nr / np.sqrt(arr.size), 1e-300)
        assert np.abs(got - ref).max() <= TOL64 * scale, (n, np.abs(got - ref).max() / scale)
        assert abs(np.sqrt((arr ** 2).sum()) - nr) <= TOL64 * max(nr, 1e-300), n


def test_dataset_and_collator_reproduce_the_reference(tmp_path):
    import sys
    sys.path.insert(0, GOLDEN_DIR)
    from make_golden import WordTokenizer
    from ripor_amd.dataset.pretrain import MarginMSEforPretrainCollator, MarginMSEforPretrainDataset
    from t5_pretrainer.dataset.data_collator import MarginMSEforPretrainCollator as C2
    from t5_pretrainer.dataset.dataset import MarginMSEforPretrainDataset as D2
    assert C2 is MarginMSEforPretrainCollator and D2 is MarginMSEforPretrainDataset
    cases = json.loads(str(np.load(os.path.join(GOLDEN_DIR, "pre_data.npz"))["cases"]))
    assert set(cases) == {"ml4", "ml16"}
    for key, c in cases.items():
        root = tmp_path / key
        for rel, k in (("collection/raw.tsv", "collection"), ("queries/raw.tsv", "queries"), ("teacher_scores.jsonl", "examples")):
            (root / rel).parent.mkdir(parents=True, exist_ok=True)
            (root / rel).write_text(c["files"][k])
        ds = MarginMSEforPretrainDataset(dataset_path=str(root / "teacher_scores.jsonl"), document_dir=str(root / "collection"),
                                         query_dir=str(root / "queries"), qrels_path=None, docid_to_smtid_path=None)
        assert len(ds) == c["length"]
        random.seed(c["random_seed"])                                # the negative is drawn with random.sample
        items = [ds[i] for i in c["order"]]
        assert [list(it) for it in items] == c["items"], key
        assert all(it[0].startswith("query: ") and it[2].startswith("document: ") and it[3].startswith("document: ") for it in items)
        batch = MarginMSEforPretrainCollator(WordTokenizer(), max_length=c["max_length"])(items[:4])
        flat = {}
        for name, val in batch.items():
            if isinstance(val, torch.Tensor):
                flat[name] = val.tolist()
            else:
                flat.update({f"{name}.{k}": v.tolist() for k, v in val.items()})
        assert flat == c["batch"], key
        assert batch["teacher_pos_score"].dtype == torch.float32 and batch["tokenized_pos_doc"]["decoder_input_ids"].tolist() == [[-1]] * 4
    with pytest.raises(NotImplementedError, match="commit loss"):
        MarginMSEforPretrainDataset("x", "y", "z", None, docid_to_smtid_path="d.json")


def test_command_line_parses_the_reference_scripts_and_refuses_other_losses(tmp_path):
    from ripor_amd import main_dense as M
    from t5_pretrainer import main_dense as alias
    assert alias.main is M.main
    for which, flags in SCRIPT_FLAGS.items():
        a = M.get_args(flags)
        assert a.loss_type == "t5seq_pretrain_margin_mse" and a.model_type == "t5_docid_gen_encoder" and a.use_fp16
        assert (a.epochs, a.learning_rate, a.max_length, a.per_device_train_batch_size) == (50, 1e-4, 128, 64)
        assert json.loads(a.task_names) == ["rank"] and a.run_name == "t5_docid_gen_encoder_" + which
        assert a.pretrained_path == flags[-1].split("=", 1)[1] and a.queries_path.endswith("train_queries")
    a = M.get_args(["--pretrained_path", "p", "--output_dir", "o", "--qrels_path", "q", "--max_steps", "7", "--save_steps", "0",
                    "--logging_steps", "1", "--resume_from_checkpoint", "c", "--dropout", "config", "--local_rank", "0",
                    "--decoder_start_token_path", "s.npy"])
    assert (a.max_steps, a.save_steps, a.logging_steps, a.dropout, a.local_rank) == (7, 0, 1, "config", 0)
    assert a.loss_type == "t5seq_pretrain_margin_mse" and a.max_length == 128 and a.per_device_train_batch_size == 64
    base = ["--pretrained_path", "p", "--output_dir", str(tmp_path), "--teacher_score_path", "t", "--collection_path", "c",
            "--queries_path", "q"]
    for lt in ("t5seq_aq_encoder_margin_mse", "t5seq_aq_encoder_seq2seq", "t5seq_aq_encoder_lng_knp_margin_mse"):
        with pytest.raises(NotImplementedError, match="t5seq_pretrain_margin_mse only"):
            M.main(base + ["--loss_type", lt])
    with pytest.raises(SystemExit, match="at most 256"):
        M.main(base + ["--max_length", "257"])
    with pytest.raises(SystemExit, match="queries_path"):
        M.main(base[:-2])


def _plain_t5(root, cfg_extra=None):
    """A synthetic plain-T5 directory: config.json of a T5 and shared / encoder.* / decoder.* / lm_head tensors."""
    from ripor_amd.modeling.t5_generative_retriever import T5forDocIDConfig, expected_keys
    from ripor_amd.utils import synth
    dims = synth.mini_dims(L=2, V=256, enc_layers=1, d_ff=64, vocab_size=64)
    sd = synth.make_state_dict(dims, seed=5)
    t5 = {k: torch.from_numpy(v) for k, v in sd.items() if k.split(".")[0] in ("shared", "encoder", "decoder")}
    t5["lm_head.weight"] = torch.zeros((dims.vocab_size, dims.d_model))
    t5["encoder.embed_tokens.weight"] = t5["decoder.embed_tokens.weight"] = t5["shared.weight"]
    os.makedirs(root, exist_ok=True)
    torch.save(t5, os.path.join(root, "pytorch_model.bin"))
    cfg = dict(architectures=["T5ForConditionalGeneration"], model_type="t5", vocab_size=dims.vocab_size, d_model=dims.d_model,
               d_kv=dims.d_kv, d_ff=dims.d_ff, num_layers=dims.num_layers, num_decoder_layers=dims.num_decoder_layers,
               num_heads=dims.num_heads, relative_attention_num_buckets=32, layer_norm_epsilon=1e-6, feed_forward_proj="relu",
               dropout_rate=0.1, n_positions=512, is_encoder_decoder=True, **(cfg_extra or {}))
    json.dump(cfg, open(os.path.join(root, "config.json"), "w"))
    return dims, sd, t5


def test_plain_t5_checkpoint_loads_with_a_start_embedding_file(tmp_path):
    from ripor_amd.modeling.t5_generative_retriever import T5SeqPretrainEncoder
    root = str(tmp_path / "t5")
    dims, sd, t5 = _plain_t5(root)
    start = np.arange(dims.d_model, dtype=np.float32).reshape(1, 1, -1) / 100
    np.save(tmp_path / "start.npy", start)
    m = T5SeqPretrainEncoder.from_pretrained(root, decoder_start_token_path=str(tmp_path / "start.npy"))
    got = m.base_model.state_dict()
    for k, v in t5.items():                                                   # all T5 tensors arrive; lm_head is ignored
        if k.startswith(("lm_head", "encoder.embed_tokens", "decoder.embed_tokens")):
            assert k not in got
        else:
            assert torch.equal(got[k], v), k
    assert torch.equal(got["start_token_embed"], torch.from_numpy(start))
    assert m.config.decoder_vocab_sizes == [256] * 32 and m.config.shared_output_input_embeds and m.config.dropout_rate == 0.1
    assert len([k for k in got if k.startswith("list_decoder_embeds")]) == 32 and got["list_decoder_embeds.31.weight"].shape == (256, dims.d_model)
    # the codebook seed reproduces, and another seed gives other codebooks
    again = T5SeqPretrainEncoder.from_pretrained(root, decoder_start_token_path=str(tmp_path / "start.npy")).base_model.state_dict()
    other = T5SeqPretrainEncoder.from_pretrained(root, decoder_start_token_path=str(tmp_path / "start.npy"), codebook_seed=1)
    assert all(torch.equal(again[k], got[k]) for k in got)
    assert not torch.equal(other.base_model.state_dict()["list_decoder_embeds.0.weight"], got["list_decoder_embeds.0.weight"])
    assert 0.9 < float(got["list_decoder_embeds.0.weight"].std()) < 1.1
    # a missing start file: a clear error, whether named by the argument or by the config field
    with pytest.raises(FileNotFoundError, match="decoder_start_token_path"):
        T5SeqPretrainEncoder.from_pretrained(root, decoder_start_token_path=str(tmp_path / "absent.npy"))
    with pytest.raises(FileNotFoundError, match="decoder_start_token_path"):
        T5SeqPretrainEncoder.from_pretrained(root)
    root2 = str(tmp_path / "t5_cfg")
    _plain_t5(root2, dict(decoder_start_token_path=str(tmp_path / "start.npy"), decoder_vocab_sizes=[64, 64]))
    m2 = T5SeqPretrainEncoder.from_pretrained(root2)
    assert torch.equal(m2.base_model.state_dict()["start_token_embed"], torch.from_numpy(start)) and m2.config.decoder_vocab_sizes == [64, 64]
    # a checkpoint of this project's format still loads as before, and a saved plain-T5 model comes back as one
    m.save_pretrained(str(tmp_path / "saved"))
    back = T5SeqPretrainEncoder.from_pretrained(str(tmp_path / "saved")).base_model.state_dict()
    assert all(torch.equal(back[k], got[k]) for k in got)


def test_model_refuses_what_the_step_does_not_build():
    from ripor_amd.modeling.t5_generative_retriever import T5SeqPretrainEncoder
    g = PreGolden("pre_mini_bz1_q5_d12")
    m = T5SeqPretrainEncoder.__new__(T5SeqPretrainEncoder)
    inp = g.inputs()
    ids, mask, tp, tn = m._batch(inp)
    assert tuple(ids.shape) == (3, 1, 12) and ids.dtype == torch.int32 and int(mask[0].sum()) == 5 and tp.shape == (1,)
    bad = g.inputs()
    bad["tokenized_neg_query"]["input_ids"] = bad["tokenized_neg_query"]["input_ids"].clone()
    bad["tokenized_neg_query"]["input_ids"][0, 1] += 1
    with pytest.raises(ValueError, match="same query tokens"):
        m._batch(bad)
    for key in ("tokenized_pos_query", "tokenized_neg_doc"):
        bad = g.inputs()
        bad[key]["decoder_input_ids"] = torch.tensor([[-1, 3]])
        with pytest.raises(ValueError, match="commit-loss branch"):
            m._batch(bad)
    bad = g.inputs()
    bad["tokenized_pos_doc"]["decoder_input_ids"] = torch.tensor([[0]])
    with pytest.raises(ValueError, match=r"must be \[-1\]"):
        m._batch(bad)


@pytest.fixture(scope="module")
def route_driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_route_dense") / "attn_route_dense_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "attn_route_dense_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def _plans(driver, dkv, Lt):
    rows, admitted = {}, None
    for line in subprocess.run([driver, "plan", str(dkv), str(Lt)], check=True, capture_output=True, text=True).stdout.splitlines():
        if line.startswith("admitted"):
            admitted = bool(int(line.split()[1]))
            continue
        site, plan = line.split(" | ")
        kernel, invalid, grid, block, smem = plan.split()
        rows[site] = (kernel, int(invalid), int(grid), int(block), int(smem))
    return rows, admitted


@pytest.mark.parametrize("dkv,Lt,admitted", [(64, 5, True), (64, 91, True), (64, 92, True), (64, 256, True), (128, 91, True),
                                             (128, 92, False)])
def test_every_attention_launch_of_a_one_position_decoder_has_a_plan(route_driver, dkv, Lt, admitted):
    """L = 1, docs = 1 (S = 6 sequences, 12 heads): every launch of the step has a valid plan within the 160 KB of LDS of a CU, or
    the shape is refused before anything runs. The decoder's sites see one key (self) and one row per sequence (cross, n = 1);
    the 91 | 92 boundary moves the ENCODER's backward from the resident carve to the tiles (64-dim heads) or out (128-dim)."""
    rows, adm = _plans(route_driver, dkv, Lt)
    assert adm is admitted
    assert set(rows) == {"enc_self_fwd", "dec_self_fwd", "cross_fwd", "enc_self_bwd", "dec_self_bwd", "cross_bwd", "enc_self_bwd_drop",
                         "dec_self_bwd_drop", "cross_bwd_drop", "enc_self_drop_fwd", "dec_self_drop_fwd", "cross_drop_fwd"}
    if not admitted:
        assert any(v[1] for v in rows.values())          # the refusal comes from a launch without a plan
        assert rows["enc_self_bwd"] == ("NONE", 1, 0, 256, 0)
        return
    for site, (kernel, invalid, grid, block, smem) in rows.items():
        assert not invalid and kernel != "NONE" and grid >= 1 and block in (128, 256) and smem <= 160 * 1024, (site, rows[site])
    # the decoder of ONE position: the MFMA tile forward and backward (64-dim heads), the resident cross-attention with n = 1
    if dkv == 64:
        assert rows["dec_self_fwd"][0] == "TRAIN_SELF_MFMA" and rows["dec_self_bwd"][0] == "TRAIN_BWD_MFMA"
        assert rows["dec_self_bwd_drop"][0] == "TRAIN_BWD_VALU"
        assert rows["enc_self_bwd"][0] == ("TRAIN_BWD_MFMA" if Lt <= 32 else "TRAIN_BWD_VALU" if Lt <= 91 else "TRAIN_SELF_BWD_TILED")
        assert rows["enc_self_drop_fwd"][0] == ("TRAIN_SELF_DROP_FWD" if Lt <= 91 else "TRAIN_SELF_DROP_FWD_TILED")
    else:
        assert rows["dec_self_bwd"][0] == "TRAIN_BWD_VALU128" and rows["enc_self_bwd"][0] == "TRAIN_BWD_VALU128"
    assert rows["cross_bwd"][0] == ("TRAIN_CROSS_BWD" if dkv == 64 else "TRAIN_CROSS_BWD128")
    assert rows["cross_bwd"][4] == 4 * (2 * 65 + 2 * Lt * 65 + 2 * (Lt + 1) + Lt)       # n = 1 stays resident up to 256 keys
    assert rows["cross_drop_fwd"][0] == ("TRAIN_CROSS_DROP_FWD" if dkv == 64 else "TRAIN_CROSS_DROP_FWD128")


def test_abi_exports_the_dense_step():
    import __graft_entry__ as ge
    ge.build()
    from ripor_amd import _lib
    lib = _lib.load()
    assert lib.rpr_abi_version() == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    for name in ("rpr_dense_mse_forward", "rpr_dense_mse_backward", "rpr_dense_mse_backward_buckets"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert "dense_head.hip" in ge.SOURCES
    # NULL arguments are refused without a device
    assert lib.rpr_dense_mse_forward(None, None, None, None, 1, 1, None, None, None, None, None, None) == -1
    assert lib.rpr_dense_mse_backward(None, None, None, None, 1, 1, None, None, None, None, None) == -1
