"""Exact dense retrieval without faiss: the collection is embedded into the chunk files ``mmap_2`` gathers (reference
``DenseIndexing.store_embs``, tasks/evaluator.py:494-555), and the gathered memmap is searched exactly on the device
(replaces ``faiss.IndexFlatIP`` behind ``DenseRetriever.retrieve``, tasks/evaluator.py:694-) with ``rpr_flat_search``
(DESIGN.md §9e). faiss index files (``model.index``) are neither written nor read."""
from __future__ import annotations

import json
import os

import numpy as np

from .rq_indexer import load_doc_embeds, read_text_ids

DOC_PREFIX = "document: "   # reference dataset/dataset.py (add_prefix=True, is_query=False)
FLAT_BLOCK_BYTES = 4 << 30   # the matrix goes to the device as blocks of at most this size


def read_collection(collection_path: str):
    """``raw.tsv`` (``id\\ttext``) -> (ids, texts with the "document: " prefix), in file order."""
    ids, texts = [], []
    with open(os.path.join(collection_path, "raw.tsv")) as reader:
        for line in reader:
            if len(line) > 1:
                id_, *data = line.split("\t")
                ids.append(int(id_.strip()))
                texts.append(DOC_PREFIX + " ".join(" ".join(data).splitlines()))
    return ids, texts


def embed_collection(model, tokenizer, collection_path: str, out_dir: str, rank: int = 0, world: int = 1, batch_size: int = 256,
                     max_length: int = 256, chunk_size: int = 50_000) -> dict:
    """Restates the reference's ``DenseIndexing.store_embs``: this rank's share of ``collection_path/raw.tsv`` is embedded
    (``engine.embed``: the model's ``doc_encode``) and written as ``embs_{rank}_{chunk}.npy`` (fp32 [rows, d]) and
    ``ids_{rank}_{chunk}.npy`` (int64), a chunk holding ``chunk_size // batch_size`` batches; rank 0 writes ``plan.json``
    (``nranks``, ``num_chunks``, ``index_path``).

    The share is ``DistributedSampler(shuffle=False)``'s (``dataset.sharding.shard_indices``), wrap-around padding included:
    every rank gets the same number of rows and so writes the ``num_chunks`` chunks the one ``plan.json`` promises. With
    ``world > 1`` and a collection that is no multiple of it, the first few documents therefore appear twice in the gathered
    memmap. That is the reference's behaviour and is kept.

    Inside a chunk the texts are tokenized once, sorted by token count so that a batch pads to its own longest text, and the
    rows are put back in the sampler's order before they are written. ``model``: a ``DeviceModel``."""
    from .. import engine as E
    from ..dataset.sharding import shard_indices
    import torch
    ids, texts = read_collection(collection_path)
    mine = shard_indices(len(ids), world, rank)
    rows_per_chunk = max(1, chunk_size // batch_size) * batch_size
    os.makedirs(out_dir, exist_ok=True)
    chunk_idx = 0
    for lo in range(0, len(mine), rows_per_chunk):
        sel = mine[lo:lo + rows_per_chunk]
        enc = tokenizer([texts[i] for i in sel], add_special_tokens=True, padding=False, truncation="longest_first",
                        max_length=max_length)["input_ids"]
        order = sorted(range(len(sel)), key=lambda j: len(enc[j]))
        embs = np.empty((len(sel), model.d_model), dtype=np.float32)
        for b in range(0, len(order), batch_size):
            rows = order[b:b + batch_size]
            width = max(len(enc[j]) for j in rows)
            tok = torch.zeros((len(rows), width), dtype=torch.long)
            mask = torch.zeros((len(rows), width), dtype=torch.long)
            for r, j in enumerate(rows):
                tok[r, :len(enc[j])] = torch.tensor(enc[j], dtype=torch.long)
                mask[r, :len(enc[j])] = 1
            embs[rows] = E.embed(model, tok, mask).cpu().numpy()
        np.save(os.path.join(out_dir, f"embs_{rank}_{chunk_idx}.npy"), embs)
        np.save(os.path.join(out_dir, f"ids_{rank}_{chunk_idx}.npy"), np.array([ids[i] for i in sel], dtype=np.int64))
        chunk_idx += 1
    plan = {"nranks": world, "num_chunks": chunk_idx, "index_path": os.path.join(out_dir, "model.index")}
    print("plan: ", plan)
    if rank == 0:
        with open(os.path.join(out_dir, "plan.json"), "w") as fout:
            json.dump(plan, fout)
    return plan


def check_mmap(mmap_dir: str) -> None:
    for name in ("doc_embeds.mmap", "text_ids.tsv", "meta.pkl"):
        path = os.path.join(mmap_dir, name)
        if not os.path.exists(path):
            raise ValueError(f"{path} not found: faiss index files (model.index) are not read here; --task=mmap and "
                             "--task=mmap_2 write the doc_embeds.mmap, text_ids.tsv and meta.pkl that retrieve searches")


class FlatIndex:
    """The gathered collection (``doc_embeds.mmap`` + ``text_ids.tsv`` + ``meta.pkl``) resident on one device, searched
    exactly. The matrix is copied once, through a pinned buffer, as blocks of at most ``block_bytes``; ``search`` chains
    ``engine.flat_search`` over the blocks (any block size gives the same bits). A matrix larger than the free HBM is refused:
    streaming it from the host is not implemented."""

    def __init__(self, mmap_dir: str, device=None, block_bytes: int = FLAT_BLOCK_BYTES):
        import torch
        from .. import engine as E
        check_mmap(mmap_dir)
        X = load_doc_embeds(mmap_dir)
        self.text_ids = read_text_ids(mmap_dir)
        if len(self.text_ids) != X.shape[0]:
            raise ValueError(f"{mmap_dir}: {X.shape[0]} embeddings, {len(self.text_ids)} ids")
        self.ctx = E.Context.get(device)
        self.n, self.d = int(X.shape[0]), int(X.shape[1])
        need = self.n * self.d * 4
        free, _ = torch.cuda.mem_get_info(self.ctx.device)
        if need + E.FLAT_SCRATCH_BYTES > free:
            raise ValueError(f"{mmap_dir}: the embedding matrix takes {need} bytes (plus {E.FLAT_SCRATCH_BYTES} of search "
                             f"scratch), the device has {free} bytes free; streaming from the host is not implemented")
        rows = max(1, min(self.n, int(block_bytes) // (self.d * 4)))
        pinned = torch.empty((rows, self.d), dtype=torch.float32).pin_memory()
        self.blocks = []   # (row_base, device tensor)
        for lo in range(0, self.n, rows):
            k = min(rows, self.n - lo)
            pinned[:k].numpy()[:] = X[lo:lo + k]
            self.blocks.append((lo, pinned[:k].to(self.ctx.device)))   # blocking copy: the buffer is free again afterwards
        del pinned

    @classmethod
    def from_blocks(cls, ctx, blocks, text_ids=None) -> "FlatIndex":
        """An index over row blocks that are on the device already: [(row_base, fp32 tensor [n, d])] (benchmarks, tests)."""
        self = cls.__new__(cls)
        self.ctx, self.blocks = ctx, list(blocks)
        self.n, self.d = sum(int(b.shape[0]) for _, b in self.blocks), int(self.blocks[0][1].shape[1])
        self.text_ids = text_ids
        return self

    def search(self, q, topk: int):
        """-> (rows int64 [Q, topk] into ``text_ids``, scores fp32 [Q, topk]) on the device."""
        from .. import engine as E
        state = None
        for lo, xb in self.blocks:
            state = E.flat_search(self.ctx, q, xb, topk, row_base=lo, state=state)
        return state


def add_to_run(run: dict, qids, idx, scores, text_ids) -> None:
    """run[qid] = {docid: score} for the rows >= 0 of every query."""
    for qid, rows, scs in zip(qids, idx.cpu().tolist(), scores.cpu().tolist()):
        run[str(qid)] = {str(text_ids[r]): float(s) for r, s in zip(rows, scs) if r >= 0}


def flat_search_index(model, loader, index: FlatIndex, out_dir: str, topk: int) -> dict:
    """Embeds every query batch of ``loader`` (``model.query_encode``'s pass) and searches ``index`` exactly;
    ``out_dir/run.json`` = {qid: {docid: score}}, the layout of ``rq_indexer.search_index``. ``model``: an encoder whose
    ``base_model.engine_model()`` lives on the index's device."""
    from .. import engine as E
    em = model.base_model.engine_model()
    if em.d_model != index.d:
        raise ValueError(f"the embeddings are {index.d} wide, the model's d_model is {em.d_model}")
    run: dict = {}
    for batch in loader:
        q = E.embed(em, batch["input_ids"], batch["attention_mask"])
        idx, scores = index.search(q, topk)
        add_to_run(run, batch["id"].tolist(), idx, scores, index.text_ids)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump(run, f)
    return run
