"""Host side of exact dense retrieval (mmap / retrieve / aq_to_flat_index_search_evaluate): the numpy restatement itself,
the ABI surface, the CLI flags and refusals, and the chunk-file and run.json writers over a stubbed engine. No GPU."""
import json
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_search_ref as ref  # noqa: E402
import rq_search_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_by_hand():
    q = np.array([[1, 2]], dtype=np.float32)
    x = np.array([[1, 0], [1, 0], [0, 2], [-0.0, 0], [0, 0]], dtype=np.float32)   # scores 1 1 4 -0 0
    idx, sc = ref.search(q, x, 7, row_base=10)
    np.testing.assert_array_equal(idx[0], [12, 10, 11, 13, 14, -1, -1])            # ties to the smaller row, -0.0 = +0.0
    np.testing.assert_array_equal(sc[0], [4, 1, 1, 0, 0, -np.inf, -np.inf])
    assert not np.signbit(sc[0, 3]) and idx.dtype == np.int64 and sc.dtype == np.float32


def test_fast_topk_equals_the_stable_sort():
    sc = np.random.default_rng(0).integers(-5, 6, size=(4, 3000)).astype(np.float32)   # heavy ties, N > 4 k
    for k in (1, 200):
        a, b = ref.topk(sc, k), rq_search_ref.topk(sc, k)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


@pytest.mark.parametrize("k", [5, 200])
def test_merge_of_two_halves_equals_the_whole(k):
    rng = np.random.default_rng(k)
    q = rng.integers(-3, 4, size=(6, 32)).astype(np.float32)
    x = rng.integers(-3, 4, size=(301, 32)).astype(np.float32)
    whole = ref.search(q, x, k)
    a, b = ref.search(q, x[:123], k), ref.search(q, x[123:], k, row_base=123)
    for first, second in ((a, b), (b, a)):
        got = ref.merge(first, second, k)
        np.testing.assert_array_equal(got[0], whole[0])
        np.testing.assert_array_equal(got[1], whole[1])
    empty = (np.full((6, k), -1, dtype=np.int64), np.full((6, k), -np.inf, dtype=np.float32))
    got = ref.merge(empty, whole, k)
    np.testing.assert_array_equal(got[0], whole[0])
    short = ref.merge(ref.search(q, x[:3], k), ref.search(q, x[3:4], k, row_base=3), k)   # fewer rows than k: -1 / -inf tail
    np.testing.assert_array_equal(short[0], ref.search(q, x[:4], k)[0])


def test_signature_in_header_and_binding_and_the_scratch_constant():
    from ripor_amd import _lib, engine as E
    header = open(os.path.join(REPO, "include", "ripor_hip.h")).read()
    assert "rpr_flat_search" in _lib.SIGNATURES and len(_lib.SIGNATURES["rpr_flat_search"][1]) == 12
    m = re.search(r"\bint rpr_flat_search\(([^;]*)\);", header)
    assert m and m.group(1).count(",") + 1 == 12
    assert _lib.ABI_VERSION == 5
    common = open(os.path.join(REPO, "ripor_amd", "csrc", "common.h")).read()
    m = re.search(r"FLAT_SCRATCH_BYTES = \(size_t\)(\d+) << (\d+);", common)
    assert m and int(m.group(1)) << int(m.group(2)) == E.FLAT_SCRATCH_BYTES
    import __graft_entry__ as g
    assert "flat_search.hip" in g.SOURCES


def test_cli_accepts_the_new_flags():
    from ripor_amd import evaluate as ev
    a = ev.get_args(["--task=mmap", "--pretrained_path=/m", "--collection_path=/c", "--index_dir=/x/mmap", "--max_length=128",
                     "--index_retrieve_batch_size=64", "--encoder_type=t5seq_pretrain_encoder"])
    assert (a.task, a.collection_path, a.index_dir, a.max_length, a.index_retrieve_batch_size, a.encoder_type) == \
        ("mmap", "/c", "/x/mmap", 128, 64, "t5seq_pretrain_encoder")
    d = ev.get_args([])   # absent unless given (tests/test_prune_margin_host.py pins the namespace); the reference's defaults apply
    assert not any(hasattr(d, f) for f in ev.DENSE_DEFAULTS)
    assert ev.DENSE_DEFAULTS == dict(collection_path=None, max_length=256, index_retrieve_batch_size=256, encoder_type=None)
    assert ev._dense_flag(d, "max_length") == 256 and ev._dense_flag(a, "max_length") == 128
    assert ev.RETRIEVE_BATCH == 128
    for fn in (ev.mmap, ev.retrieve, ev.aq_to_flat_index_search_evaluate):
        assert callable(fn)


@pytest.mark.parametrize("task,flags", [("mmap", "--pretrained_path, --collection_path, --index_dir"),
                                        ("retrieve", "--pretrained_path, --out_dir"),
                                        ("aq_to_flat_index_search_evaluate", "--pretrained_path, --docid_to_smtid_path, --out_dir")])
def test_tasks_without_their_flags_are_refused(task, flags):
    from ripor_amd import evaluate as ev
    with pytest.raises(ValueError, match=f"task: {task} is not valid without {flags}"):
        ev.main([f"--task={task}"])


def test_partly_given_flags_are_named(tmp_path):
    from ripor_amd import evaluate as ev
    with pytest.raises(ValueError, match="is not valid without --collection_path$"):
        ev.main(["--task=mmap", f"--pretrained_path={tmp_path}", f"--index_dir={tmp_path}/mmap"])
    with pytest.raises(ValueError, match="is not valid without --mmap_dir"):
        ev.main(["--task=retrieve", f"--pretrained_path={tmp_path}", f"--out_dir={tmp_path}/out"])
    with pytest.raises(ValueError, match='must contain "mmap"'):
        ev.main(["--task=mmap", f"--pretrained_path={tmp_path}", f"--index_dir={tmp_path}/index", f"--collection_path={tmp_path}"])
    for task in ("index", "index_2"):   # faiss files: still refused
        with pytest.raises(ValueError, match=f"task: {task} is not valid"):
            ev.main([f"--task={task}"])


def test_retrieve_without_the_memmap_says_what_makes_it(tmp_path):
    from ripor_amd import evaluate as ev
    (tmp_path / "index").mkdir()
    (tmp_path / "index" / "model.index").write_bytes(b"faiss")
    for flag in ("--mmap_dir", "--index_dir"):
        with pytest.raises(ValueError, match=r"doc_embeds\.mmap not found: faiss index files .* are not read.*--task=mmap and --task=mmap_2"):
            ev.main(["--task=retrieve", f"--pretrained_path={tmp_path}", f"{flag}={tmp_path}/index", f"--out_dir={tmp_path}/out"])
    _mmap_files(tmp_path / "mmap", np.zeros((3, 32), dtype=np.float32), [1, 2, 3])
    with pytest.raises(ValueError, match="bert_encoder is not valid"):   # checked before the checkpoint is read
        ev.main(["--task=retrieve", f"--pretrained_path={tmp_path}", f"--mmap_dir={tmp_path}/mmap", f"--out_dir={tmp_path}/out",
                 "--encoder_type=bert_encoder"])


def _mmap_files(mmap_dir, X, ids):
    os.makedirs(mmap_dir)
    X.tofile(os.path.join(mmap_dir, "doc_embeds.mmap"))
    with open(os.path.join(mmap_dir, "text_ids.tsv"), "w") as f:
        f.writelines(f"{i}\n" for i in ids)
    pickle.dump({"num_embeddings": len(ids)}, open(os.path.join(mmap_dir, "meta.pkl"), "wb"))


class _WordTokenizer:
    """One token per word plus an end token; truncates like the real one."""

    def __call__(self, texts, add_special_tokens=True, padding=False, truncation=None, max_length=256, **kw):
        assert padding is False
        return {"input_ids": [([7 + len(w) for w in t.split()] + [1])[-max_length:] for t in texts]}


@pytest.mark.parametrize("world", [1, 2])
def test_embed_collection_writes_the_reference_chunk_layout(tmp_path, monkeypatch, world):
    from ripor_amd import engine as E
    from ripor_amd.dataset.sharding import shard_indices
    from ripor_amd.tasks import dense_indexer, rq_indexer
    coll = tmp_path / "coll"
    coll.mkdir()
    n = 11
    with open(coll / "raw.tsv", "w") as f:
        for i in range(n):
            f.write(f"{500 + i}\t" + " ".join(["w"] * (1 + (i * 5) % 7)) + "\n")
    batches = []

    def fake_embed(model, ids, mask):
        # an embedding that names the text: its token count and the sum of its tokens; padding must be masked zeros
        assert ((ids != 0) == (mask != 0)).all()
        batches.append(ids.shape)
        out = torch.zeros((ids.shape[0], 32))
        out[:, 0] = mask.sum(1)
        out[:, 1] = ids.sum(1)
        return out

    monkeypatch.setattr(E, "embed", fake_embed)
    model = types.SimpleNamespace(d_model=32)
    out_dir = str(tmp_path / "mmap")
    for rank in range(world):
        plan = dense_indexer.embed_collection(model, _WordTokenizer(), str(coll), out_dir, rank, world, batch_size=2, chunk_size=4)
    per_rank = len(shard_indices(n, world, 0))
    assert plan == {"nranks": world, "num_chunks": -(-per_rank // 4), "index_path": os.path.join(out_dir, "model.index")}
    assert json.load(open(os.path.join(out_dir, "plan.json"))) == plan
    assert max(b[0] for b in batches) == 2 and len({b[1] for b in batches}) > 1   # batches of 2, padded to their own longest
    for rank in range(world):
        mine = shard_indices(n, world, rank)
        ids = np.concatenate([np.load(os.path.join(out_dir, f"ids_{rank}_{c}.npy")) for c in range(plan["num_chunks"])])
        embs = np.concatenate([np.load(os.path.join(out_dir, f"embs_{rank}_{c}.npy")) for c in range(plan["num_chunks"])])
        assert ids.dtype == np.int64 and embs.dtype == np.float32 and embs.shape == (per_rank, 32)
        np.testing.assert_array_equal(ids, [500 + i for i in mine])                 # the sampler's order, not the sorted one
        np.testing.assert_array_equal(embs[:, 0], [1 + (i * 5) % 7 + 2 for i in mine])   # + the "document:" prefix and the end token
    # what mmap_2 makes of it
    rq_indexer.aggregate_embs_to_mmap(out_dir)
    X = rq_indexer.load_doc_embeds(out_dir)
    assert X.shape == (per_rank * world, 32) and len(rq_indexer.read_text_ids(out_dir)) == per_rank * world
    assert not [f for f in os.listdir(out_dir) if f.startswith("embs_")]


class _StubModel:
    def __init__(self, d):
        em = types.SimpleNamespace(d_model=d, ctx=types.SimpleNamespace(device=torch.device("cpu")))
        self.base_model = types.SimpleNamespace(engine_model=lambda: em)


def test_flat_search_index_writes_the_reference_run_layout(tmp_path, monkeypatch):
    from ripor_amd import engine as E
    from ripor_amd.tasks import dense_indexer
    seen = []

    def fake_embed(model, ids, mask):
        return torch.zeros((ids.shape[0], 32))

    def fake_flat_search(ctx, q, x, topk, row_base=0, state=None):
        seen.append((row_base, x.shape[0], topk, state is not None))
        idx = torch.tensor([[2, 0, -1]] * q.shape[0])
        return idx, torch.tensor([[1.5, 0.25, float("-inf")]] * q.shape[0])

    monkeypatch.setattr(E, "embed", fake_embed)
    monkeypatch.setattr(E, "flat_search", fake_flat_search)
    # the loader of a memmap needs a device; an index over given blocks does not
    index = dense_indexer.FlatIndex.from_blocks(None, [(0, torch.zeros((4, 32))), (4, torch.zeros((3, 32)))],
                                                text_ids=[str(1000 + i) for i in range(7)])
    assert (index.n, index.d) == (7, 32)
    loader = [{"input_ids": torch.zeros((2, 4), dtype=torch.long), "attention_mask": torch.ones((2, 4), dtype=torch.long),
               "id": torch.tensor([900, 901])},
              {"input_ids": torch.zeros((1, 4), dtype=torch.long), "attention_mask": torch.ones((1, 4), dtype=torch.long),
               "id": torch.tensor([902])}]
    out_dir = str(tmp_path / "out" / "MSMARCO")
    dense_indexer.flat_search_index(_StubModel(32), loader, index, out_dir, topk=3)
    run = json.load(open(os.path.join(out_dir, "run.json")))
    assert run == {q: {"1002": 1.5, "1000": 0.25} for q in ("900", "901", "902")}
    assert seen == [(0, 4, 3, False), (4, 3, 3, True)] * 2            # the blocks are chained through the state
    with pytest.raises(ValueError, match="d_model is 64"):
        dense_indexer.flat_search_index(_StubModel(64), [], index, out_dir, topk=3)


def test_pretrain_encoder_mirror():
    from ripor_amd.modeling.t5_generative_retriever import T5SeqAQEncoder, T5SeqPretrainEncoder
    import t5_pretrainer.modeling.t5_generative_retriever as alias
    assert issubclass(T5SeqPretrainEncoder, T5SeqAQEncoder) and alias.T5SeqPretrainEncoder is T5SeqPretrainEncoder
    calls = []
    m = T5SeqPretrainEncoder.__new__(T5SeqPretrainEncoder)
    m.query_encode = lambda **kw: calls.append(kw) or "rep"
    assert m.doc_encode(input_ids=1, attention_mask=2) == "rep" and calls == [{"input_ids": 1, "attention_mask": 2}]
