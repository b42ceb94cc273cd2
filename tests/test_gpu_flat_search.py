"""-m gpu: exact dense retrieval on the device. rpr_flat_search against the numpy restatement tests/flat_search_ref.py
(bit for bit where the arithmetic is exact: integer-valued inputs, entries in -3 .. 3, every sum an integer below 2^24;
within the derived rounding bound otherwise), its edge cases, its invariances (partition, batch, sub-block walk, run to
run), its limits, the FlatIndex wrapper, and the reference's mmap -> mmap_2 -> retrieve steps and the quantizer sanity
check through the command line."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_search_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

STEP_LOGIT_TOL = 5e-4  # tests/test_gpu_api.py: step logits against the reference


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


def _search(ctx, q, x, topk, row_base=0, state=None):
    from ripor_amd import engine as E
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    idx, sc = E.flat_search(ctx, q, xd, topk, row_base=row_base, state=state)
    return idx.cpu().numpy(), sc.cpu().numpy()


def _integer_case(seed, d, N, Q):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(Q, d)).astype(np.float32)
    x = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    assert 9 * d < 2 ** 24
    return q, x


@pytest.fixture(scope="module")
def big(ctx):
    """(768, 30000, 130): more than one 128-row query tile, N above the 8192-entry candidate list. Searched once."""
    q, x = _integer_case(768 + 30000, 768, 30000, 130)
    want = ref.search(q, x, 200)
    xd = torch.from_numpy(x).cuda()
    got = _search(ctx, q, xd, 200)
    return q, xd, want, got


def test_heavy_ties_small(ctx):
    q, x = _integer_case(32 + 5000, 32, 5000, 5)
    want_idx, want_sc = ref.search(q, x, 200)
    idx, sc = _search(ctx, q, x, 200)
    np.testing.assert_array_equal(sc, want_sc)
    np.testing.assert_array_equal(idx, want_idx)
    assert (np.diff(want_sc, axis=1) == 0).any(axis=1).all()   # the inputs do what the case is about: ties in every row


def test_heavy_ties_two_query_tiles(big):
    _, _, (want_idx, want_sc), (idx, sc) = big
    np.testing.assert_array_equal(sc, want_sc)
    np.testing.assert_array_equal(idx, want_idx)
    assert (np.diff(want_sc, axis=1) == 0).any(axis=1).all()


@pytest.mark.parametrize("N", [1, 63, 257])
def test_small_and_ragged_n_pads(ctx, N):
    q, x = _integer_case(N, 32, N, 5)
    want_idx, want_sc = ref.search(q, x, 200)
    idx, sc = _search(ctx, q, x, 200)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)
    if N < 200:
        assert (idx[:, N:] == -1).all() and np.isneginf(sc[:, N:]).all()


@pytest.mark.parametrize("topk", [1, 2048])
def test_topk_extremes(ctx, topk):
    q, x = _integer_case(topk, 32, 5000, 5)
    want_idx, want_sc = ref.search(q, x, topk)
    idx, sc = _search(ctx, q, x, topk)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)


def test_all_scores_equal_takes_the_first_rows(ctx):
    # far more equal scores than the candidate list holds: the selection goes on into the row bits
    q = np.random.default_rng(3).standard_normal((3, 32)).astype(np.float32)
    idx, sc = _search(ctx, q, torch.zeros((100_000, 32), device="cuda"), 200)
    np.testing.assert_array_equal(idx, np.tile(np.arange(200), (3, 1)))
    assert (sc == 0).all() and not np.signbit(sc).any()


def test_negative_zero_ties_with_zero(ctx):
    # rows 0, 2, 4: the only non-zero factor meets a zero, the product is -0.0; rows 1, 3: +0.0 throughout; row 5 scores 1 and 2
    q = np.zeros((2, 32), dtype=np.float32); q[:, 0] = [-1, -2]
    x = np.zeros((6, 32), dtype=np.float32)
    x[[1, 3], 1] = 5.0
    x[5, 0] = -1.0
    assert np.signbit(q[0, 0] * x[0, 0]) and not np.signbit(q[0, 1] * x[1, 1])
    idx, sc = _search(ctx, q, x, 6)
    np.testing.assert_array_equal(idx, np.tile([5, 0, 1, 2, 3, 4], (2, 1)))
    np.testing.assert_array_equal(sc, np.array([[1, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]], dtype=np.float32))
    assert not np.signbit(sc).any()
    want_idx, want_sc = ref.search(q, x, 6)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)


def test_sub_block_boundary(ctx):
    from ripor_amd import engine as E
    Q, d = 130, 32
    N = E.FLAT_SCRATCH_BYTES // (4 * Q) + 1          # one row more than a sub-block can hold: the walk takes two
    assert E.FLAT_SCRATCH_BYTES == 256 << 20
    q, x = _integer_case(N, d, N, Q)
    x[N - 1] = 3 * np.where(q[0] >= 0, 1, -1)        # the last row, alone in its sub-block's tail, is query 0's best
    sc32 = q @ x.T                                   # integers below 2^24: the fp32 product is the exact one
    want_idx, want_sc = ref.topk(sc32 + np.float32(0.0), 200)
    idx, sc = _search(ctx, q, x, 200)
    np.testing.assert_array_equal(sc, want_sc)
    np.testing.assert_array_equal(idx, want_idx)
    assert want_idx[0, 0] == N - 1


def test_partition_invariance(ctx):
    q, x = _integer_case(7, 32, 30000, 5)
    xd = torch.from_numpy(x).cuda()
    want_idx, want_sc = ref.search(q, x, 200)
    idx, sc = _search(ctx, q, xd, 200)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)
    from ripor_amd import engine as E
    cut = 12345
    parts = [(0, xd[:cut]), (cut, xd[cut:])]
    for order in (parts, parts[::-1]):
        state = None
        for base, xb in order:
            state = E.flat_search(ctx, q, xb, 200, row_base=base, state=state)
        np.testing.assert_array_equal(state[0].cpu().numpy(), idx)
        np.testing.assert_array_equal(state[1].cpu().numpy(), sc)
    # the restatement's own merge says the same
    a, b = ref.search(q, x[:cut], 200), ref.search(q, x[cut:], 200, row_base=cut)
    mi, ms = ref.merge(b, a, 200)
    np.testing.assert_array_equal(mi, idx)
    np.testing.assert_array_equal(ms, sc)


def test_batch_invariance_and_determinism(ctx, big):
    q, xd, _, (idx, sc) = big
    i1, s1 = _search(ctx, q[7:8], xd, 200)
    np.testing.assert_array_equal(i1[0], idx[7])
    np.testing.assert_array_equal(s1[0], sc[7])
    i2, s2 = _search(ctx, q, xd, 200)
    np.testing.assert_array_equal(i2, idx)
    np.testing.assert_array_equal(s2.view(np.uint32), sc.view(np.uint32))


@pytest.mark.parametrize("d,share", [(64, 0.01), (768, 0.05)])
def test_gaussian_against_fp64(ctx, d, share):
    """b = 1.01 d 2^-24 sum_i |q_i| |x_i|: the gamma_d bound of a d-term fp32 chain, derived, not measured. The condition
    on the inputs (documents within 2 max b of the threshold; the restatement counts 8 and 27 of 1600) is checked on the
    fp64 scores alone before the device is asked."""
    N, Q, topk = 30000, 8, 200
    rng = np.random.default_rng(d + N)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    x = rng.standard_normal((N, d)).astype(np.float32)
    s64 = ref.scores(q, x)
    b = ref.rounding_bound(q, x)
    bmax = float(b.max())
    t = np.sort(s64, axis=1)[:, ::-1][:, topk - 1]
    undecided = int((np.abs(s64 - t[:, None]) <= 2 * bmax).sum())
    print(f"d {d}: max bound {bmax:.3g}, documents within 2 max b of the threshold: {undecided}")
    assert undecided <= share * Q * topk, undecided
    idx, sc = _search(ctx, q, x, topk)
    assert ((idx >= 0) & (idx < N)).all()
    rows = np.arange(Q)[:, None]
    err = np.abs(sc.astype(np.float64) - s64[rows, idx])
    print(f"max |score - fp64| {err.max():.3g}, max err / bound {(err / b[rows, idx]).max():.3g}")
    assert (err <= b[rows, idx]).all()
    assert (s64[rows, idx] >= t[:, None] - 2 * bmax).all()
    for qi in range(Q):
        must = np.flatnonzero(s64[qi] > t[qi] + 2 * bmax)
        assert np.isin(must, idx[qi]).all()
        assert len(set(idx[qi].tolist())) == topk
    assert (np.diff(sc, axis=1) <= 0).all()


def test_equals_the_quantizer_search_on_decoded_vectors(ctx):
    from ripor_amd import engine as E
    d, M, K, N = 32, 3, 64, 5000
    rng = np.random.default_rng(d + M + K)
    q = rng.integers(-3, 4, size=(5, d)).astype(np.float32)
    books = rng.integers(-3, 4, size=(M, K, d)).astype(np.float32)
    codes = rng.integers(0, K, size=(N, M)).astype(np.uint16)
    decoded = sum(books[m][codes[:, m]] for m in range(M)).astype(np.float32)   # integers: exact
    ri, rs = E.rq_search(ctx, q, books, codes, 200)
    idx, sc = _search(ctx, q, decoded, 200)
    np.testing.assert_array_equal(idx, ri.cpu().numpy())
    np.testing.assert_array_equal(sc, rs.cpu().numpy())


def test_limits_are_refused_by_name(ctx):
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    with pytest.raises(RiporHipError, match="multiple of 32"):
        E.flat_search(ctx, z(2, 48), z(10, 48), 10)
    with pytest.raises(RiporHipError, match="multiple of 32"):
        E.flat_search(ctx, z(2, 0), z(10, 0), 10)
    with pytest.raises(RiporHipError, match="Q must be at least 1"):
        E.flat_search(ctx, z(0, 32), z(10, 32), 10)
    with pytest.raises(RiporHipError, match="n must be at least 1"):
        E.flat_search(ctx, z(2, 32), z(0, 32), 10)
    with pytest.raises(RiporHipError, match="row_base must be at least 0"):
        E.flat_search(ctx, z(2, 32), z(10, 32), 10, row_base=-1)
    with pytest.raises(RiporHipError, match=r"row_base \+ n out of range \(at most 2\^31 - 1\)"):
        E.flat_search(ctx, z(2, 32), z(10, 32), 10, row_base=2 ** 31 - 10)
    for topk in (0, 2049):
        with pytest.raises(RiporHipError, match=r"topk out of range \(1 \.\. 2048\)"):
            E.flat_search(ctx, z(2, 32), z(10, 32), topk)
    with pytest.raises(ValueError, match="width"):
        E.flat_search(ctx, z(2, 32), z(10, 64), 10)
    # the last rows the limit admits
    idx, sc = _search(ctx, z(2, 32), z(10, 32), 4, row_base=2 ** 31 - 11)
    np.testing.assert_array_equal(idx, np.tile(np.arange(4) + 2 ** 31 - 11, (2, 1)))


def test_empty_state_merges_like_no_state(ctx):
    q, x = _integer_case(11, 32, 5000, 5)
    idx, sc = _search(ctx, q, x, 200)
    empty = (torch.full((5, 200), -1, dtype=torch.int64), torch.full((5, 200), float("-inf")))
    i2, s2 = _search(ctx, q, x, 200, state=empty)
    np.testing.assert_array_equal(i2, idx)
    np.testing.assert_array_equal(s2, sc)


def _write_mmap(mmap_dir, X, ids):
    import pickle
    os.makedirs(mmap_dir)
    np.asarray(X, dtype=np.float32).tofile(os.path.join(mmap_dir, "doc_embeds.mmap"))
    with open(os.path.join(mmap_dir, "text_ids.tsv"), "w") as f:
        f.writelines(f"{i}\n" for i in ids)
    pickle.dump({"num_embeddings": len(ids)}, open(os.path.join(mmap_dir, "meta.pkl"), "wb"))


def test_flat_index_in_small_blocks_equals_one_search(ctx, tmp_path):
    from ripor_amd.tasks.dense_indexer import FlatIndex
    q, x = _integer_case(13, 64, 3001, 9)
    mmap_dir = str(tmp_path / "mmap")
    _write_mmap(mmap_dir, x, np.arange(3001) + 5000)
    index = FlatIndex(mmap_dir, 0, block_bytes=700 * 64 * 4)
    assert len(index.blocks) == 5 and index.text_ids[0] == "5000"
    idx, sc = index.search(q, 200)
    want_idx, want_sc = _search(ctx, q, x, 200)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(sc.cpu().numpy(), want_sc)
    with pytest.raises(ValueError, match="mmap_2"):
        FlatIndex(str(tmp_path), 0)


# ---- the tasks --------------------------------------------------------------------------------------------------------------

def test_cli_mmap_mmap_2_retrieve_and_the_quantizer_check(tmp_path):
    from test_gpu_cli import _make_world, _run
    from transformers import AutoTokenizer
    from ripor_amd import engine as E
    from ripor_amd.evaluate import QueryCollection, query_batches
    from ripor_amd.modeling.t5_generative_retriever import T5AQEncoder
    from ripor_amd.tasks.dense_indexer import FlatIndex, read_collection
    root = str(tmp_path / "model")
    ckpt, d2s_path, qdir, codes, queries, dims = _make_world(root)
    rnd = random.Random(5)
    words = ["what", "is", "the", "how", "to", "of", "in", "a", "best", "price", "weather", "define"] + [f"w{i}" for i in range(200)]
    coll_dir = os.path.join(root, "msmarco_toyset", "full_collection")
    os.makedirs(coll_dir)
    with open(os.path.join(coll_dir, "raw.tsv"), "w") as f:
        for i in range(300):
            f.write(f"{7000 + i}\t" + " ".join(rnd.choice(words) for _ in range(rnd.randint(3, 40))) + "\n")
    mmap_dir, out_dir = os.path.join(root, "mmap"), os.path.join(root, "out")
    _run(["-m", "t5_pretrainer.evaluate", "--task=mmap", f"--pretrained_path={ckpt}", f"--collection_path={coll_dir}",
          f"--index_dir={mmap_dir}", "--encoder_type=t5seq_pretrain_encoder", "--index_retrieve_batch_size=128"])
    plan = json.load(open(os.path.join(mmap_dir, "plan.json")))
    assert plan["nranks"] == 1 and plan["num_chunks"] == 1 and plan["index_path"].endswith("model.index")
    _run(["-m", "t5_pretrainer.evaluate", "--task=mmap_2", f"--index_dir={mmap_dir}", f"--mmap_dir={mmap_dir}"])

    # the memmap: E.embed of the same tokenised texts, ids in file order
    model = T5AQEncoder.from_pretrained(ckpt).to(0)
    em = model.base_model.engine_model()
    ctx = E.Context.get(0)
    ctx.set_precision("f16x2")
    tok = AutoTokenizer.from_pretrained(ckpt)
    ids, texts = read_collection(coll_dir)
    assert ids == [7000 + i for i in range(300)] and texts[0].startswith("document: ")
    enc = tok(texts, add_special_tokens=True, padding="longest", truncation="longest_first", max_length=256, return_attention_mask=True)
    want = E.embed(em, torch.tensor(enc["input_ids"]), torch.tensor(enc["attention_mask"])).cpu().numpy()
    index = FlatIndex(mmap_dir, 0)
    assert index.text_ids == [str(i) for i in ids]
    got = np.fromfile(os.path.join(mmap_dir, "doc_embeds.mmap"), dtype=np.float32).reshape(300, dims.d_model)
    print("max |memmap - embed|:", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, atol=STEP_LOGIT_TOL, rtol=0)

    # retrieve: run.json = FlatIndex.search on the task's own memmap
    coll = QueryCollection(qdir)
    batch = next(query_batches(coll, tok, list(range(len(coll))), 128, 256))
    emb = E.embed(em, batch["input_ids"], batch["attention_mask"])
    idx, sc = index.search(emb, 100)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()

    def top_doc(i):   # trec_eval's order: score, then docid string, both descending (utils/metrics.py)
        return max(str(ids[int(r)]) for r, s in zip(idx[i], sc[i]) if s == sc[i, 0])

    qrel_path = os.path.join(root, "msmarco_toyset", "dev_qrel.json")
    json.dump({str(qid): {top_doc(i): 1} for i, qid in enumerate(batch["id"].tolist())}, open(qrel_path, "w"))
    _run(["-m", "t5_pretrainer.evaluate", "--task=retrieve", f"--pretrained_path={ckpt}", f"--mmap_dir={mmap_dir}",
          f"--out_dir={out_dir}", "--q_collection_paths=" + json.dumps([qdir]), "--eval_qrel_path=" + json.dumps([qrel_path]),
          "--eval_metric=" + json.dumps([["mrr_10", "recall"]]), "--topk=100", "--encoder_type=t5seq_pretrain_encoder"])
    run = json.load(open(os.path.join(out_dir, "MSMARCO", "run.json")))
    assert set(run) == set(queries)
    for i, qid in enumerate(batch["id"].tolist()):
        assert len(run[str(qid)]) == 100
        assert run[str(qid)] == {str(ids[int(r)]): float(s) for r, s in zip(idx[i], sc[i])}
    assert json.load(open(os.path.join(out_dir, "MSMARCO", "perf.json")))["mrr_10"] == 1.0

    # the quantizer's sanity check: every entry is <embed(query), decode(codes)> within the rounding bound of the search
    out2 = os.path.join(root, "out_flat")
    _run(["-m", "t5_pretrainer.evaluate", "--task=aq_to_flat_index_search_evaluate", f"--pretrained_path={ckpt}",
          f"--docid_to_smtid_path={d2s_path}", f"--out_dir={out2}", "--q_collection_paths=" + json.dumps([qdir])])
    run2 = json.load(open(os.path.join(out2, "MSMARCO", "run.json")))
    sd = model.base_model.state_dict()
    name = "list_decoder_embeds" if model.config.shared_output_input_embeds else "list_output_embeds"
    X = None
    for m in range(codes.shape[1]):   # fp32, levels ascending, as the task adds them
        rows = sd[f"{name}.{m}.weight"].cpu().numpy().astype(np.float32)[codes[:, m].astype(np.int64)]
        X = rows if X is None else (X + rows).astype(np.float32)
    qn = emb.cpu().numpy()
    s64, b = ref.scores(qn, X), ref.rounding_bound(qn, X)
    assert set(run2) == set(queries)
    for i, qid in enumerate(batch["id"].tolist()):
        docs = run2[str(qid)]
        assert len(docs) == 200
        for docid, s in docs.items():
            r = int(docid) - 100
            assert abs(s - s64[i, r]) <= b[i, r], (qid, docid, s, s64[i, r], b[i, r])
