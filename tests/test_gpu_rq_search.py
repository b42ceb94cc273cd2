"""-m gpu: searching the residual-quantizer index on the device. rpr_rq_search against the numpy restatement
tests/rq_search_ref.py (bit for bit where the arithmetic is exact, within the derived rounding bound otherwise), its edge
cases, determinism and limits; rpr_embed against the CPU oracle and against rpr_lngknp_forward; and the reference's
mmap_2 -> aq_index -> aq_evaluate steps through the command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rq_search_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

POS_SCORE_TOL = 1e-3   # tests/test_gpu_train.py: position scores against the reference
STEP_LOGIT_TOL = 5e-4  # tests/test_gpu_api.py: step logits against the reference


@pytest.fixture(scope="module")
def ctx():
    from ripor_amd import engine as E
    return E.Context.get(0)


def _search(ctx, q, books, codes, topk):
    from ripor_amd import engine as E
    idx, sc = E.rq_search(ctx, q, books, codes, topk)
    return idx.cpu().numpy(), sc.cpu().numpy()


def _integer_case(seed, d, M, K, N, Q):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(Q, d)).astype(np.float32)
    books = rng.integers(-3, 4, size=(M, K, d)).astype(np.float32)
    codes = rng.integers(0, K, size=(N, M)).astype(np.uint16)
    return q, books, codes


# every product and sum is an integer below 2^24 (|score| <= 9 d M): fp32 is exact in any order, ties are exact ties.
# (768, 32, 256, 30000, 130): four queries to a block, 33 groups with a ragged last one, 16-byte code loads, N above the
# candidate list: histogram passes; (32, 1, 64, 30000, 3): one level, at most 64 distinct scores per query
@pytest.mark.parametrize("d,M,K,N,Q", [(32, 3, 64, 5000, 5), (768, 32, 256, 30000, 130), (32, 1, 64, 30000, 3)])
def test_exact_arithmetic_heavy_ties(ctx, d, M, K, N, Q):
    q, books, codes = _integer_case(d + M, d, M, K, N, Q)
    assert 9 * d * M < 2 ** 24
    want_idx, want_sc = ref.topk(ref.scores(ref.lut(q, books, np.float64), codes).astype(np.float32), 200)
    idx, sc = _search(ctx, q, books, codes, 200)
    np.testing.assert_array_equal(sc, want_sc)
    np.testing.assert_array_equal(idx, want_idx)
    assert (np.diff(want_sc, axis=1) == 0).any(axis=1).all()   # the inputs do what the case is about: ties in every row


@pytest.mark.parametrize("N", [1, 63, 257])
def test_small_and_ragged_n_pads(ctx, N):
    q, books, codes = _integer_case(N, 32, 3, 64, N, 5)
    want_idx, want_sc = ref.search(q, books, codes, 200)
    idx, sc = _search(ctx, q, books, codes, 200)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)
    if N < 200:
        assert (idx[:, N:] == -1).all() and np.isneginf(sc[:, N:]).all()


@pytest.mark.parametrize("topk", [1, 2048])
def test_topk_extremes(ctx, topk):
    q, books, codes = _integer_case(topk, 32, 3, 64, 5000, 5)
    want_idx, want_sc = ref.search(q, books, codes, topk)
    idx, sc = _search(ctx, q, books, codes, topk)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(sc, want_sc)


def test_all_scores_equal_takes_the_first_rows(ctx):
    # every candidate ties: far more equal scores than the candidate list holds, the selection goes on into the row index
    rng = np.random.default_rng(3)
    N, M, K, d = 100_000, 4, 64, 32
    q = rng.standard_normal((3, d)).astype(np.float32)
    codes = rng.integers(0, K, size=(N, M)).astype(np.uint16)
    idx, sc = _search(ctx, q, np.zeros((M, K, d), dtype=np.float32), codes, 200)
    np.testing.assert_array_equal(idx, np.tile(np.arange(200), (3, 1)))
    assert (sc == 0).all() and not np.signbit(sc).any()


def _gaussian_case(seed, N, d, M, K, Q, distinct_codes=False):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    books = rng.standard_normal((M, K, d)).astype(np.float32)
    if distinct_codes:
        codes = np.stack([rng.permutation(K)[:N] for _ in range(M)], axis=1).astype(np.uint16)
    else:
        codes = rng.integers(0, K, size=(N, M)).astype(np.uint16)
    return q, books, codes


def _check_against_fp64(ctx, q, books, codes, topk=200):
    """The checks of a float-valued case: b = the derived rounding bound of every (query, document) score."""
    Q, N = q.shape[0], codes.shape[0]
    s64 = ref.scores(ref.lut(q, books, np.float64), codes)
    b = ref.rounding_bound(q, books, codes)
    bmax = float(b.max())
    t = np.sort(s64, axis=1)[:, ::-1][:, topk - 1]                         # fp64 topk-th score of every query
    undecided = int((np.abs(s64 - t[:, None]) <= 2 * bmax).sum())
    print(f"max bound {bmax:.3g}, score spread {s64.std():.3g}, documents within 2 max b of the threshold: {undecided}")
    assert undecided <= 0.01 * Q * topk, undecided                         # on the fp64 scores alone
    idx, sc = _search(ctx, q, books, codes, topk)
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
    d_sc = np.diff(sc, axis=1)
    assert (d_sc <= 0).all()
    assert ((d_sc < 0) | (np.diff(idx, axis=1) > 0)).all()                 # equal scores: ascending rows


def test_gaussian_against_fp64(ctx):
    _check_against_fp64(ctx, *_gaussian_case(17, 20011, 64, 4, 256, 7))


# (4, 1024, 64): a 16 KB level; (4, 192, 96): K off the 128 grid; (16, 1024, 32): two queries to a block; (64, 1024, 32): a table
# over the LDS budget, read from global memory; (8, 256, 64): 16-byte code loads with float scores.
# (1, 1024, 64): one level — a score is a LUT entry, so documents with the same code tie exactly and any threshold has
# whole groups of them on it; the codes are a permutation (N <= K) so that the fp64 cap of the check is meaningful
@pytest.mark.parametrize("M,K,d,N", [(4, 1024, 64, 20011), (4, 192, 96, 20011), (16, 1024, 32, 20011), (64, 1024, 32, 9001),
                                     (8, 256, 64, 20011), (1, 1024, 64, 1000)])
def test_other_code_paths(ctx, M, K, d, N):
    _check_against_fp64(ctx, *_gaussian_case(M + K + d, N, d, M, K, 7, distinct_codes=M == 1))


def test_codes_past_k_are_clamped(ctx):
    q, books, codes = _gaussian_case(2, 3000, 32, 8, 64, 3)
    wild = codes.copy()
    wild[::7] = 65535
    idx, sc = _search(ctx, q, books, wild, 50)
    idx2, sc2 = _search(ctx, q, books, np.minimum(wild, 63).astype(np.uint16), 50)
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(sc, sc2)


def test_determinism_and_split_invariance(ctx):
    from ripor_amd import engine as E
    N, topk = 40_000, 200
    q, books, codes = _gaussian_case(23, N, 64, 8, 256, 9)
    codes[1::2] = codes[::2]                                    # pairs of equal scores everywhere
    cd = torch.from_numpy(codes.view(np.int16)).cuda()
    idx, sc = E.rq_search(ctx, q, books, cd, topk)
    idx2, sc2 = E.rq_search(ctx, q, books, cd, topk)
    assert torch.equal(idx, idx2) and torch.equal(sc, sc2)
    h = N // 2
    ia, sa = E.rq_search(ctx, q, books, cd[:h], topk)
    ib, sb = E.rq_search(ctx, q, books, cd[h:], topk)
    mi = torch.cat([ia, ib + h], dim=1).cpu().numpy()
    ms = torch.cat([sa, sb], dim=1).cpu().numpy()
    for qi in range(q.shape[0]):
        order = np.lexsort((mi[qi], -ms[qi]))[:topk]           # score descending, then row ascending
        np.testing.assert_array_equal(idx[qi].cpu().numpy(), mi[qi][order])
        np.testing.assert_array_equal(sc[qi].cpu().numpy(), ms[qi][order])
    # one query at a time = the batch
    i1, s1 = E.rq_search(ctx, q[4:5], books, cd, topk)
    assert torch.equal(i1[0], idx[4]) and torch.equal(s1[0], sc[4])


def test_invalid_shapes_refused(ctx):
    from ripor_amd import engine as E
    from ripor_amd._lib import RiporHipError
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    codes = torch.zeros((100, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(RiporHipError, match="multiple of 32"):
        E.rq_search(ctx, z(2, 48), z(2, 64, 48), codes, 10)
    with pytest.raises(RiporHipError, match="multiple of 64"):
        E.rq_search(ctx, z(2, 32), z(2, 96, 32), codes, 10)
    with pytest.raises(RiporHipError, match="at most 1024"):
        E.rq_search(ctx, z(2, 32), z(2, 2048, 32), codes, 10)
    with pytest.raises(RiporHipError, match=r"M out of range \(1 \.\. 64\)"):
        E.rq_search(ctx, z(2, 32), z(65, 64, 32), torch.zeros((100, 65), dtype=torch.int16, device="cuda"), 10)
    for topk in (0, 2049):
        with pytest.raises(RiporHipError, match=r"topk out of range \(1 \.\. 2048\)"):
            E.rq_search(ctx, z(2, 32), z(2, 64, 32), codes, topk)
    with pytest.raises(RiporHipError, match=r"N out of range"):
        E.rq_search(ctx, z(2, 32), z(2, 64, 32), codes[:0], 10)
    with pytest.raises(RiporHipError, match="Q must be at least 1"):
        E.rq_search(ctx, z(0, 32), z(2, 64, 32), codes, 10)
    with pytest.raises(ValueError, match="levels"):
        E.rq_search(ctx, z(2, 32), z(3, 64, 32), codes, 10)


# ---- rpr_embed ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mini():
    """The mini model of tests/test_gpu_cli.py::_make_world on the device, a few ragged queries, and the oracle."""
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    from oracle import t5_ref
    dims = synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=128, vocab_size=512)
    sd = synth.make_state_dict(dims, seed=77)
    ids, mask = synth.make_queries(6, vocab_size=dims.vocab_size, seed=5, max_len=13)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, sd, dims)
    oracle = t5_ref.T5Ref(sd, dims)
    with torch.no_grad():
        enc = oracle.encode(torch.from_numpy(ids).long(), torch.from_numpy(mask).long())
        want = oracle.last_logits(torch.full((len(ids), 1), -1, dtype=torch.long), enc, torch.from_numpy(mask).long()).numpy()
    yield ctx, model, oracle, torch.from_numpy(ids), torch.from_numpy(mask), want
    ctx.set_precision("f16x2")


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_embed_equals_the_oracle(mini, precision):
    from ripor_amd import engine as E
    ctx, model, oracle, ids, mask, want = mini
    ctx.set_precision(precision)
    emb = E.embed(model, ids, mask)
    assert emb.shape == (ids.shape[0], model.d_model) and emb.dtype == torch.float32
    got = emb.cpu().double().numpy() @ oracle.out_embed(0).double().numpy().T
    print("max |logit - oracle|:", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, atol=STEP_LOGIT_TOL, rtol=0)
    assert torch.equal(emb, E.embed(model, ids, mask))
    if precision == "f32":   # one fixed fp32 chain per output: a text's embedding does not depend on its batch
        assert torch.equal(emb[2:3], E.embed(model, ids[2:3], mask[2:3]))


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_embed_equals_lngknp_forward_at_position_0(mini, precision):
    from ripor_amd import engine as E
    ctx, model, oracle, ids, mask, _ = mini
    ctx.set_precision(precision)
    rng = np.random.default_rng(1)
    codes = torch.from_numpy(rng.integers(0, 256, size=(ids.shape[0], 2, 8)).astype(np.int32))
    _, pos = E.lngknp_forward(model, ids, mask, codes)
    emb = E.embed(model, ids, mask).cpu().double()
    e0 = oracle.out_embed(0).double()
    got = torch.einsum("bd,bnd->bn", emb, e0[codes[:, :, 0].long()]).numpy()
    print("max |<embed, E_out[0][c]> - position score|:", np.abs(got - pos[:, :, 0].cpu().numpy()).max())
    np.testing.assert_allclose(got, pos[:, :, 0].cpu().numpy(), atol=POS_SCORE_TOL, rtol=0)


def test_query_encode_and_decode_of_the_modeling_mirror(mini):
    from ripor_amd import engine as E
    from ripor_amd.modeling.t5_generative_retriever import T5AQEncoder
    from ripor_amd.utils import synth
    ctx, model, oracle, ids, mask, _ = mini
    ctx.set_precision("f32")
    m = T5AQEncoder.from_synthetic(synth.mini_dims(L=8, V=256, enc_layers=2, d_ff=128, vocab_size=512), seed=77).to(0)
    rep = m.query_encode(input_ids=ids, attention_mask=mask, decoder_input_ids=torch.full((ids.shape[0], 1), -1))
    assert torch.equal(rep, E.embed(model, ids, mask))
    enc = torch.tensor([[1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 0, 0, 0, 0, 0, 0]])
    want = sum(oracle.out_embed(i)[enc[:, i]] for i in range(8))
    torch.testing.assert_close(m.decode(enc), want)
    with pytest.raises(ValueError, match="decoder_input_ids"):
        m.query_encode(input_ids=ids, attention_mask=mask, decoder_input_ids=torch.zeros((ids.shape[0], 1), dtype=torch.long))


# ---- the task -------------------------------------------------------------------------------------------------------------

def test_cli_mmap_2_aq_index_aq_evaluate(tmp_path):
    from test_gpu_cli import _make_world, _run
    from test_gpu_rq import _hierarchy
    root = str(tmp_path / "model")
    ckpt, _, qdir, _, queries, dims = _make_world(root)
    M, bits, N, d = len(dims.decoder_vocab_sizes), 8, 3000, dims.d_model
    mmap_dir, index_dir, out_dir = os.path.join(root, "mmap"), os.path.join(root, "aq_index"), os.path.join(root, "out")
    os.makedirs(mmap_dir)
    X = _hierarchy(N, d, 3, 16, seed=3, scales=[4.0, 2.0, 1.0])
    np.save(os.path.join(mmap_dir, "embs_0_0.npy"), X)
    np.save(os.path.join(mmap_dir, "ids_0_0.npy"), np.arange(N) + 5000)
    json.dump({"nranks": 1, "num_chunks": 1, "index_path": ""}, open(os.path.join(mmap_dir, "plan.json"), "w"))
    _run(["-m", "t5_pretrainer.evaluate", "--task=mmap_2", f"--index_dir={mmap_dir}", f"--mmap_dir={mmap_dir}"])
    _run(["-m", "t5_pretrainer.evaluate", "--task=aq_index", f"--num_subvectors_for_pq={M}", f"--codebook_bits={bits}",
          f"--index_dir={index_dir}", f"--mmap_dir={mmap_dir}"])

    # what the task must write: the Python API on the same tokenised queries
    from transformers import AutoTokenizer
    from ripor_amd import engine as E
    from ripor_amd.evaluate import QueryCollection, query_batches
    from ripor_amd.modeling.t5_generative_retriever import T5AQEncoder
    model = T5AQEncoder.from_pretrained(ckpt).to(0)
    ctx = E.Context.get(0)
    ctx.set_precision("f16x2")
    coll = QueryCollection(qdir)
    batch = next(query_batches(coll, AutoTokenizer.from_pretrained(ckpt), list(range(len(coll))), 128, 256))
    books = torch.from_numpy(np.load(os.path.join(index_dir, "rq_codebooks.npy"))).cuda()
    codes, _ = E.rq_encode(ctx, X, books)
    emb = E.embed(model.base_model.engine_model(), batch["input_ids"], batch["attention_mask"])
    idx, sc = E.rq_search(ctx, emb, books, codes, 200)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()

    # qrels that mark every query's top document. Documents with the same codes tie exactly; the evaluation ranks like
    # trec_eval (score, then docid string, both descending: utils/metrics.py), so that is the top document it sees
    def top_doc(i):
        return max(str(5000 + int(r)) for r, s in zip(idx[i], sc[i]) if s == sc[i, 0])

    qrel_path = os.path.join(root, "msmarco_toyset", "dev_qrel.json")
    json.dump({str(qid): {top_doc(i): 1} for i, qid in enumerate(batch["id"].tolist())}, open(qrel_path, "w"))
    _run(["-m", "t5_pretrainer.evaluate", "--task=aq_evaluate", f"--pretrained_path={ckpt}", f"--mmap_dir={mmap_dir}",
          f"--index_dir={index_dir}", f"--out_dir={out_dir}", "--q_collection_paths=" + json.dumps([qdir]),
          "--eval_qrel_path=" + json.dumps([qrel_path]), "--eval_metric=" + json.dumps([["mrr_10", "recall"]])])
    run = json.load(open(os.path.join(out_dir, "MSMARCO", "run.json")))
    text_ids = {line.strip() for line in open(os.path.join(mmap_dir, "text_ids.tsv"))}
    assert set(run) == set(queries)
    for i, qid in enumerate(batch["id"].tolist()):
        docs = run[str(qid)]
        assert len(docs) == 200 and set(docs) <= text_ids
        assert docs == {str(5000 + int(r)): float(s) for r, s in zip(idx[i], sc[i])}
    perf = json.load(open(os.path.join(out_dir, "MSMARCO", "perf.json")))
    assert perf["mrr_10"] == 1.0
