"""The Python side of the 256-token training limit, without a GPU: engine._s2s_args and the seq2seq --max_length check of
main.py take 256 and refuse 257 with a message that names the limit; main.py goes on refusing the loss types it never built."""
import types

import pytest
import torch


def test_s2s_args_take_256_tokens_and_refuse_257():
    from ripor_amd import engine as E
    model = types.SimpleNamespace(ctx=types.SimpleNamespace(device=torch.device("cpu")))
    labels = torch.zeros((2, 8), dtype=torch.int64)
    for Lq in (129, 256):
        ids = torch.ones((2, Lq), dtype=torch.int64)
        got = E._s2s_args(model, ids, ids, labels)
        assert got[3:] == (2, Lq, 8) and got[0].dtype == torch.int32 and got[0].shape == (2, Lq)
    ids = torch.ones((2, 257), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"queries of 257 tokens: the training passes take at most 256 encoder positions \(use max_length <= 256\)"):
        E._s2s_args(model, ids, ids, labels)


def test_command_line_takes_max_length_256_and_refuses_257(tmp_path):
    from ripor_amd import main as M
    base = ["--loss_type", "t5seq_aq_encoder_seq2seq", "--pretrained_path", "p", "--output_dir", str(tmp_path),
            "--query_to_docid_path", str(tmp_path / "missing.jsonl"), "--docid_to_smtid_path", str(tmp_path / "missing.json")]
    with pytest.raises(SystemExit, match="--max_length 257: the training passes take at most 256 query tokens"):
        M.main(base + ["--max_length", "257"])
    # 256 and the old bound's neighbour 129 pass the check: the run gets as far as opening its (missing) example file
    from ripor_amd._lib import RiporHipError
    for n in ("129", "256"):
        with pytest.raises(RiporHipError, match="cannot open .*missing.json"):
            M.main(base + ["--max_length", n])
    for lt in ("t5seq_aq_encoder_margin_mse", "t5seq_pretrain_margin_mse"):
        with pytest.raises(NotImplementedError, match="outside this repository"):
            M.main(["--loss_type", lt, "--pretrained_path", "p", "--output_dir", str(tmp_path), "--max_length", "256"])
