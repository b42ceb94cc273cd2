"""CLI-compatible replacement of reference aq_preprocess/create_customized_smtid_file.py:14-80.

Encodes every row of ``model_dir/mmap/doc_embeds.mmap`` with the residual quantizer of ``model_dir/aq_index`` on the
device (rpr_rq_encode, or rpr_rq_encode_beam with ``--max_beam_size`` above 1; the reference runs faiss's
``rq.compute_codes`` on the CPU, whose beam is 5) and writes
``model_dir/aq_smtid/docid_to_smtid.json`` = {docid: [-1, c_1 .. c_M]}, plus the binary trie cache beside it
(``list_smtid_to_nextids.rprtrie``) so that the first retrieval does not parse the JSON."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

if __package__ in (None, ""):   # run by file path, as the reference's scripts do
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def get_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_dir", default="", type=str)
    ap.add_argument("--M", default=32, type=int)
    ap.add_argument("--bits", default=8, type=int)
    ap.add_argument("--max_beam_size", default=1, type=int,
                    help="candidate encodings kept per document through the levels (1: greedy; faiss's default is 5)")
    return ap.parse_args(argv)


def write_docid_to_smtid(path: str, docids, codes: np.ndarray) -> None:
    """{docid: [-1, c_1 .. c_M]} in row order, written line-free as ujson.dump writes it."""
    with open(path, "w") as fout:
        fout.write("{")
        for i, (docid, row) in enumerate(zip(docids, codes)):
            fout.write(("," if i else "") + json.dumps(docid) + ":[-1," + ",".join(map(str, row.tolist())) + "]")
        fout.write("}")


def smtid_stats(codes: np.ndarray) -> dict:
    """Unique-smtid statistics of the reference (:63-80): smtids held by one document, all smtids, docs per smtid."""
    _, counts = np.unique(np.ascontiguousarray(codes), axis=0, return_counts=True)
    unique = int((counts == 1).sum())
    return dict(unique_smtid_num=unique, total_smtid=int(len(counts)),
                quantiles=np.quantile(counts, [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]))


def main(argv=None):
    args = get_args(argv)
    from ripor_amd import engine as E
    from ripor_amd.aq_preprocess.build_list_smtid_to_nextids import cache_path
    from ripor_amd.tasks.rq_indexer import load_doc_embeds, load_index
    import torch

    model_dir, M, K = args.model_dir, args.M, 1 << args.bits
    print("model_dir: ", model_dir, "codebook_num: ", M, "codebook_size: ", K)
    mmap_dir = os.path.join(model_dir, "mmap")
    with open(os.path.join(mmap_dir, "text_ids.tsv")) as fin:
        docids = [line.strip() for line in fin]
    print("size of idx_to_docid = {}".format(len(docids)))
    X = load_doc_embeds(mmap_dir)
    books, info = load_index(os.path.join(model_dir, "aq_index"))
    if (info["M"], info["K"]) != (M, K):
        raise ValueError(f"the index holds M = {info['M']}, K = {info['K']}; --M {M} --bits {args.bits} asks for K = {K}")
    assert len(docids) == X.shape[0], (len(docids), X.shape)
    ctx = E.Context.get(None)
    codes, mse = E.rq_encode(ctx, X, torch.from_numpy(books).to(ctx.device), beam=args.max_beam_size)
    for m, v in enumerate(mse):
        print(f"[level {m}] encoding MSE after the level: {v:.6g}")
    print("size of docid_to_smtid = {}".format(len(docids)))

    out_dir = os.path.join(model_dir, "aq_smtid")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "docid_to_smtid.json")
    write_docid_to_smtid(path, docids, codes)
    E.build_trie_file(codes, K, cache_path(path), docids=docids, source_path=path)

    st = smtid_stats(codes)
    print("unique_smtid_num = {}, total_smtid = {}".format(st["unique_smtid_num"], st["total_smtid"]))
    print("percentage of smtid is unique = {:.3f}".format(st["unique_smtid_num"] / st["total_smtid"]))
    print("distribution of lengths: ", st["quantiles"])
    return codes


if __name__ == "__main__":
    main()
