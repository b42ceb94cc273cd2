"""Docid creation without faiss: the dense document embeddings are gathered into one memmap (reference
``DenseIndexing.aggregate_embs_to_mmap``, tasks/evaluator.py:637-690), a residual quantizer is trained on the device
(replaces ``AddictvieQuantizeIndexer.index``, tasks/evaluator.py:405-421, faiss.IndexResidualQuantizer) and every
document is encoded into its smtid (aq_preprocess/create_customized_smtid_file.py).

The quantizer is greedy residual k-means (DESIGN.md "Residual quantization"): its codes are not faiss's codes, and the
index directory holds ``rq_codebooks.npy`` + ``rq.json`` instead of faiss's ``model.index``."""
from __future__ import annotations

import json
import os
import pickle

import numpy as np


def aggregate_embs_to_mmap(mmap_dir: str) -> None:
    """``embs_{rank}_{chunk}.npy`` / ``ids_{rank}_{chunk}.npy`` (layout in ``plan.json``) -> ``doc_embeds.mmap`` (raw fp32
    [N, d]), ``text_ids.tsv``, ``meta.pkl``; the chunk files are removed (reference tasks/evaluator.py:637-690)."""
    with open(os.path.join(mmap_dir, "plan.json")) as fin:
        plan = json.load(fin)
    print("mmap_dir is: {}".format(mmap_dir))
    print("plan: ", plan)
    nranks, num_chunks = plan["nranks"], plan["num_chunks"]
    names = [(f"embs_{i}_{c}.npy", f"ids_{i}_{c}.npy") for i in range(nranks) for c in range(num_chunks)]
    embs = [np.load(os.path.join(mmap_dir, e), mmap_mode="r") for e, _ in names]
    text_ids = np.concatenate([np.load(os.path.join(mmap_dir, i)) for _, i in names])
    N = sum(len(e) for e in embs)
    assert N == len(text_ids), (N, len(text_ids))
    assert text_ids.ndim == 1, text_ids.shape
    d = embs[0].shape[1]
    print("embs size: ", (N, d), "ids dtype: ", text_ids.dtype)
    fp = np.memmap(os.path.join(mmap_dir, "doc_embeds.mmap"), dtype=np.float32, mode="w+", shape=(N, d))
    lo = 0
    for e in embs:   # chunk by chunk: the collection never has to fit the host memory twice
        fp[lo:lo + len(e)] = np.asarray(e, dtype=np.float32)
        lo += len(e)
    fp.flush()
    del fp
    with open(os.path.join(mmap_dir, "text_ids.tsv"), "w") as fout:
        for tid in text_ids:
            fout.write(f"{tid}\n")
    meta = {"text_ids": text_ids, "num_embeddings": len(text_ids)}
    with open(os.path.join(mmap_dir, "meta.pkl"), "wb") as f:
        pickle.dump(meta, f)
    del embs
    for e, i in names:
        os.remove(os.path.join(mmap_dir, e))
        os.remove(os.path.join(mmap_dir, i))


def load_doc_embeds(mmap_dir: str) -> np.memmap:
    """``doc_embeds.mmap`` as a read-only [N, d] memmap (N from ``meta.pkl``)."""
    with open(os.path.join(mmap_dir, "meta.pkl"), "rb") as f:
        n = int(pickle.load(f)["num_embeddings"])
    path = os.path.join(mmap_dir, "doc_embeds.mmap")
    total = os.path.getsize(path) // 4
    if n <= 0 or total % n:
        raise ValueError(f"{path}: {total} floats do not divide into {n} rows")
    return np.memmap(path, dtype=np.float32, mode="r", shape=(n, total // n))


def train_index(mmap_dir: str, index_dir: str, M: int, bits: int, niter: int = None, seed: int = None, device=None) -> dict:
    """Trains the M x 2^bits residual quantizer on the device and writes ``rq_codebooks.npy`` and ``rq.json``."""
    import torch
    from .. import engine as E
    niter = E.RQ_NITER if niter is None else niter
    seed = E.RQ_SEED if seed is None else seed
    K = 1 << int(bits)
    X = load_doc_embeds(mmap_dir)
    N, d = X.shape
    S, init = E.rq_training_plan(N, M, K, seed)
    if init is None:
        raise ValueError(f"{N} documents are fewer than the {K} codewords of a level")
    ctx = E.Context.get(device)
    x_train = torch.from_numpy(np.ascontiguousarray(X[S])).to(ctx.device)
    print(f"Training residual quantizer: M = {M}, K = {K}, d = {d}, {len(S)} training points of {N}, niter = {niter}")
    books, mse = E.rq_train(ctx, x_train, M, K, init, niter=niter)
    for m, v in enumerate(mse):
        print(f"[level {m}] training MSE after the level: {v:.6g}")
    os.makedirs(index_dir, exist_ok=True)
    np.save(os.path.join(index_dir, "rq_codebooks.npy"), books.cpu().numpy())
    info = dict(M=int(M), K=int(K), d=int(d), niter=int(niter), seed=int(seed), n_train=int(len(S)), num_embeddings=int(N),
                level_mse=[float(v) for v in mse], method="greedy residual k-means")
    with open(os.path.join(index_dir, "rq.json"), "w") as f:
        json.dump(info, f, indent=2)
    return info


def load_index(index_dir: str):
    """-> (codebooks fp32 [M, K, d], rq.json dict)."""
    with open(os.path.join(index_dir, "rq.json")) as f:
        info = json.load(f)
    books = np.load(os.path.join(index_dir, "rq_codebooks.npy"))
    assert books.shape == (info["M"], info["K"], info["d"]), (books.shape, info)
    return books, info


def check_index(mmap_dir: str, index_dir: str, d_model: int = None):
    """The files ``search_index`` needs, or a ValueError that names what is missing or does not fit."""
    for path in (os.path.join(index_dir, "rq.json"), os.path.join(index_dir, "rq_codebooks.npy"),
                 os.path.join(mmap_dir, "text_ids.tsv"), os.path.join(mmap_dir, "doc_embeds.mmap"),
                 os.path.join(mmap_dir, "meta.pkl")):
        if not os.path.exists(path):
            raise ValueError(f"{path} not found: run --task=mmap_2 and --task=aq_index first")
    with open(os.path.join(index_dir, "rq.json")) as f:
        info = json.load(f)
    if d_model is not None and int(info["d"]) != int(d_model):
        raise ValueError(f"the index in {index_dir} holds vectors of width {info['d']}, the model's d_model is {d_model}")
    return info


def read_text_ids(mmap_dir: str):
    with open(os.path.join(mmap_dir, "text_ids.tsv")) as f:
        return [line.strip() for line in f if line.strip()]


def search_index(model, loader, mmap_dir: str, index_dir: str, out_dir: str, topk: int = 200) -> dict:
    """Searches the residual-quantizer index for every query of ``loader`` (replaces ``AddictvieQuantizeIndexer.search``,
    reference tasks/evaluator.py:423-443, faiss.IndexResidualQuantizer.search with METRIC_INNER_PRODUCT): the collection is
    encoded with the trained codebooks (streamed, nothing cached on disk) and the codes stay on the device; every query batch
    is embedded (``model.query_encode``) and searched (``engine.rq_search``); ``out_dir/run.json`` = {qid: {docid: score}}.
    ``loader`` yields dicts with ``input_ids``, ``attention_mask`` and ``id``; ``model`` is a T5SeqAQEncoder on a HIP device."""
    import torch
    from .. import engine as E
    em = model.base_model.engine_model()
    check_index(mmap_dir, index_dir, em.d_model)
    books, info = load_index(index_dir)
    X = load_doc_embeds(mmap_dir)
    text_ids = read_text_ids(mmap_dir)
    if X.shape[1] != info["d"] or len(text_ids) != X.shape[0]:
        raise ValueError(f"{mmap_dir}: {X.shape[0]} x {X.shape[1]} embeddings, {len(text_ids)} ids, index width {info['d']}")
    ctx = em.ctx
    books_dev = torch.from_numpy(np.ascontiguousarray(books)).to(ctx.device)
    codes, _ = E.rq_encode(ctx, X, books_dev)
    codes_dev = torch.from_numpy(codes.view(np.int16)).to(ctx.device)
    qid_to_rankdata = {}
    for batch in loader:
        q = E.embed(em, batch["input_ids"], batch["attention_mask"])
        idx, scores = E.rq_search(ctx, q, books_dev, codes_dev, topk)
        idx, scores = idx.cpu().tolist(), scores.cpu().tolist()
        for qid, rows, scs in zip(batch["id"].tolist(), idx, scores):
            qid_to_rankdata[str(qid)] = {str(text_ids[r]): float(s) for r, s in zip(rows, scs) if r >= 0}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump(qid_to_rankdata, f)
    return qid_to_rankdata
