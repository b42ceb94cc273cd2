"""Teacher scoring of the self-training loop (reference t5_pretrainer/rerank.py), on the HIP cross-encoder.

Built tasks, with the reference's ``RerankArguments`` flag names (reference arguments.py:215-248):

* ``--task=cross_encoder_rerank_for_qid_smtid_docids`` (reference rerank.py:587-623): rank ``r`` of a world of ``w`` takes
  every qid of ``--qid_smtid_docids_path`` with ``i % w == r`` in file order, scores every (query, passage) pair of its
  ``{qid: {smtid: [docids]}}`` with ``CrossEncoder`` and writes ``{qid: {smtid: [[docid, score], ...]}}``.
* ``--task=cross_encoder_rerank_for_qid_smtid_docids_2`` (:625-654): merges the shards found in ``--out_dir`` into
  ``qid_smtid_docids_teacher_score.train.json`` and deletes them.
* ``--task=rerank_for_create_trainset`` (:41-65): scores every (query, passage) pair of ``--run_json_path``
  (``--json_type=json``: ``{qid: {docid: score}}``; ``jsonl``: lines of ``{"qid", "docids"}``) and writes
  ``<out_dir>/rerank_<rank>.json`` = ``{qid: {docid: score}}``. The pairs are sharded by qid like the task above (the
  reference shards the pairs with a ``DistributedSampler``, which pads the last ranks with repeated pairs).
* ``--task=rerank_for_create_trainset_2`` (:67-105): merges the ``rerank_<rank>.json`` shards of ``--out_dir``, sorts every
  query's passages by score (descending, stable), keeps the first 200 and writes one ``{"qid", "docids", "scores"}`` line per
  query to ``qid_docids_teacher_scores.train.json`` — what ``aq_preprocess/add_qrel_to_rerank_run.py`` turns into the
  examples of the rank-oriented training stage — then deletes the shards.

Differences by design:

* The shard file is ``<dir>/<basename without ".train.json">_teacher_score_<rank>.train.json``. The reference takes
  ``path.split(".")[0]`` as the prefix, which cuts a path such as ``./out/x.train.json`` at its first dot (to an empty
  string); for the paths the reference scripts pass (no dot before the extension) both give the same file.
* Scores are exact fp32 by default (the reference runs the teacher under fp16 autocast), and a batch is packed: its
  padding is never computed. ``--teacher_precision=fp16`` (not a reference flag) takes the reference's arithmetic instead:
  f16 matrix operands with fp32 accumulation (``rpr_xenc_set_precision``). A score that left the f16 range
  on the way is non-finite, as under autocast; the task then stops and points to fp32.
* The merge does not assert that the number of shards equals ``torch.cuda.device_count()``: it may run on any machine.
* The process group and the device follow ``evaluate.py``: ``ddp_setup`` (``RPR_DIST_BACKEND``), ``RPR_EVAL_DEVICE``.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

MERGED_NAME = "qid_smtid_docids_teacher_score.train.json"
TRAINSET_NAME = "qid_docids_teacher_scores.train.json"
TRAINSET_TOPK = 200   # passages kept per query (reference rerank.py:96-98)
BUILT_TASKS = ("cross_encoder_rerank_for_qid_smtid_docids", "cross_encoder_rerank_for_qid_smtid_docids_2",
               "rerank_for_create_trainset", "rerank_for_create_trainset_2")
# the other branches of the reference's dispatch (rerank.py:660-691)
UNBUILT_TASKS = ("rerank_for_eval", "rerank_for_evaluate_2", "assign_scores_for_pseudo_queries", "assign_scores_for_pseudo_queries_2", "query_to_docid_rerank_for_qid_smtids",
                 "query_to_docid_rerank_for_qid_smtids_2", "teacher_rerank_for_qid_smtids", "teacher_rerank_for_qid_smtids_2",
                 "cross_encoder_rerank_for_same_prefix_docid", "cross_encoder_rerank_for_same_prefix_docid_2",
                 "cross_encoder_rerank_for_same_reldocid_hard_docids", "cross_encoder_rerank_for_same_reldocid_hard_docids_2")

# --teacher_precision -> CrossEncoder precision
TEACHER_PRECISIONS = {"fp32": "f32", "fp16": "f16"}

Triple = Tuple[str, str, str]   # (qid, docid, smtid)


def shard_qids(qid_to_smtid_to_docids: Dict[str, dict], world: int, rank: int) -> Dict[str, dict]:
    """reference rerank.py:597-600: every qid with ``i % world == rank``, in file order."""
    return {qid: v for i, (qid, v) in enumerate(qid_to_smtid_to_docids.items()) if i % world == rank}


def build_triples(qid_to_smtid_to_docids: Dict[str, dict]) -> List[Triple]:
    """reference dataset.py:209-213 (CrossEncRerankForSamePrefixPair): qid, then smtid, then docid, as nested."""
    return [(qid, docid, smtid) for qid, by_smtid in qid_to_smtid_to_docids.items()
            for smtid, docids in by_smtid.items() for docid in docids]


def triple_ids_to_json_output(scores: Sequence[float], triple_ids: Sequence[Triple]) -> Dict[str, Dict[str, list]]:
    """reference tasks/reranker.py:211-226 (the tuples become lists in the JSON file)."""
    out: Dict[str, Dict[str, list]] = {}
    assert len(scores) == len(triple_ids)
    for s, (qid, docid, smtid) in zip(scores, triple_ids):
        out.setdefault(str(qid), {}).setdefault(str(smtid), []).append([str(docid), float(s)])
    return out


def read_tsv(path: str) -> Dict[str, str]:
    """``id \\t text`` per line (reference dataset.py:195-204)."""
    out = {}
    with open(path) as fin:
        for line in fin:
            key, text = line.strip().split("\t")
            out[key] = text
    return out


def teacher_score_path(qid_smtid_docids_path: str, rank: int) -> str:
    d, base = os.path.split(qid_smtid_docids_path)
    if base.endswith(".train.json"):
        base = base[:-len(".train.json")]
    return os.path.join(d, f"{base}_teacher_score_{rank}.train.json")


def score_triples(triples: Sequence[Triple], qid_to_query: Dict[str, str], docid_to_doc: Dict[str, str], tokenizer,
                  score_fn: Callable, batch_size: int, max_length: int,
                  require_finite: bool = False) -> List[float]:
    """The loader and the loop of reference dataloader.py:142-152 / tasks/reranker.py:61-76: batches of ``batch_size``
    triples in order, the reference's tokenizer call, ``score_fn(qd_kwargs)`` -> [bz] scores. ``require_finite`` (the f16
    teacher): a non-finite score of a batch, which is on the host by then, raises."""
    import math
    scores: List[float] = []
    for b0 in range(0, len(triples), batch_size):
        chunk = triples[b0:b0 + batch_size]
        queries = [qid_to_query[qid] for qid, _, _ in chunk]
        docs = [docid_to_doc[docid] for _, docid, _ in chunk]
        qd_kwargs = tokenizer(queries, docs, padding=True, truncation='longest_first', return_attention_mask=True,
                              return_tensors="pt", max_length=max_length)
        got = score_fn(qd_kwargs).cpu().tolist()
        if require_finite and not all(math.isfinite(v) for v in got):
            bad = [chunk[i] for i, v in enumerate(got) if not math.isfinite(v)]
            raise FloatingPointError(f"the fp16 teacher gave a non-finite score for {len(bad)} pairs (first: qid, docid, smtid = "
                                     f"{bad[0]}): an activation left the f16 range; run with --teacher_precision=fp32")
        scores.extend(got)
    return scores


def start_teacher(args):
    """Joins the process group and binds the cross-encoder on this rank's device -> (model, precision, rank, world)."""
    import torch.distributed as dist
    from .evaluate import _device_index, ddp_setup
    from .modeling.cross_encoder import CrossEncoder
    ddp_setup()
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    local_rank = max(0, int(args.local_rank if args.local_rank >= 0 else os.environ.get("LOCAL_RANK", 0)))
    print("model_name_or_path for cross_encoder: ", args.model_name_or_path)
    precision = TEACHER_PRECISIONS[args.teacher_precision]
    if rank == 0:
        print("teacher precision: ", args.teacher_precision)
    model = CrossEncoder(args.model_name_or_path, precision=precision)
    model.to(_device_index(local_rank))
    model.eval()
    return model, precision, rank, world


def cross_encoder_rerank_for_qid_smtid_docids(args):
    from transformers import AutoTokenizer
    model, precision, rank, world = start_teacher(args)
    with open(args.qid_smtid_docids_path) as fin:
        qid_to_smtid_to_docids = json.load(fin)
    print("qid_smtid_docids_path: ", args.qid_smtid_docids_path)
    sampled = shard_qids(qid_to_smtid_to_docids, world, rank)
    print("size of sampled_data = {}, original data = {}".format(len(sampled), len(qid_to_smtid_to_docids)))
    triples = build_triples(sampled)
    tokenizer = AutoTokenizer.from_pretrained(args.model_name_or_path)
    scores = score_triples(triples, read_tsv(args.train_queries_path), read_tsv(os.path.join(args.collection_path, "raw.tsv")),
                           tokenizer, lambda kw: model.rerank_forward(kw)["scores"], args.batch_size, args.max_length,
                           require_finite=precision == "f16")
    out_path = teacher_score_path(args.qid_smtid_docids_path, rank)
    with open(out_path, "w") as fout:
        json.dump(triple_ids_to_json_output(scores, triples), fout)
    print(f"wrote {len(triples)} scored pairs to {out_path}")
    return out_path


def merge_shards(out_dir: str) -> Dict[str, Dict[str, list]]:
    """reference rerank.py:625-654 without the device-count assertion."""
    merged_path = os.path.join(out_dir, MERGED_NAME)
    if os.path.exists(merged_path):
        print(f"old {MERGED_NAME} exists.")
        os.remove(merged_path)
    merged: Dict[str, Dict[str, list]] = {}
    shards = [p for p in os.listdir(out_dir) if "qid_smtid_docids_teacher_score" in p]
    for sub in shards:
        with open(os.path.join(out_dir, sub)) as fin:
            part = json.load(fin)
        for qid, by_smtid in part.items():
            for smtid, rows in by_smtid.items():
                cur = merged.setdefault(qid, {})
                if smtid not in cur:
                    cur[smtid] = rows
                else:
                    cur[smtid] += rows
    print("total size of qids = {}".format(len(merged)))
    with open(merged_path, "w") as fout:
        json.dump(merged, fout)
    for sub in shards:
        os.remove(os.path.join(out_dir, sub))
    return merged


def cross_encoder_rerank_for_qid_smtid_docids_2(args):
    return merge_shards(args.out_dir)


def read_run(run_json_path: str, json_type: str) -> Dict[str, List[str]]:
    """reference dataset.py:19-38 (RerankDataset): the docids of every qid in file order. ``jsonl``: lines of ``{"qid",
    "docids"}`` (a qid on several lines keeps all of them); anything else: one ``{qid: {docid: score}}`` object."""
    run: Dict[str, List[str]] = {}
    with open(run_json_path) as fin:
        if json_type == "jsonl":
            for line in fin:
                if line.strip():
                    ex = json.loads(line)
                    run.setdefault(str(ex["qid"]), []).extend(str(d) for d in ex["docids"])
        else:
            for qid, rankdata in json.load(fin).items():
                run[str(qid)] = [str(d) for d in rankdata]
    return run


def pair_ids_to_json_output(scores: Sequence[float], triples: Sequence[Triple]) -> Dict[str, Dict[str, float]]:
    """reference tasks/reranker.py (pair_ids_to_json_output): ``{qid: {docid: score}}``."""
    out: Dict[str, Dict[str, float]] = {}
    assert len(scores) == len(triples)
    for s, (qid, docid, _) in zip(scores, triples):
        out.setdefault(str(qid), {})[str(docid)] = float(s)
    return out


def rerank_for_create_trainset(args):
    from transformers import AutoTokenizer
    from .dataset.lng_knp import CollectionDatasetPreLoad
    model, precision, rank, world = start_teacher(args)
    run = read_run(args.run_json_path, args.json_type)
    sampled = shard_qids(run, world, rank)
    print("size of sampled_data = {}, original data = {}".format(len(sampled), len(run)))
    triples = [(qid, docid, "") for qid, docids in sampled.items() for docid in docids]
    queries = CollectionDatasetPreLoad(args.q_collection_path, id_style="content_id").data_dict
    docs = CollectionDatasetPreLoad(args.collection_path, id_style="content_id").data_dict
    tokenizer = AutoTokenizer.from_pretrained(args.model_name_or_path)
    scores = score_triples(triples, queries, docs, tokenizer, lambda kw: model.rerank_forward(kw)["scores"], args.batch_size,
                           args.max_length, require_finite=precision == "f16")
    os.makedirs(args.out_dir, exist_ok=True)
    out_path = os.path.join(args.out_dir, f"rerank_{rank}.json")
    qid_to_rankdata = pair_ids_to_json_output(scores, triples)
    print("Write reranking to path: {}".format(out_path))
    with open(out_path, "w") as fout:
        json.dump(qid_to_rankdata, fout)
    return out_path


def is_rerank_shard(name: str) -> bool:
    """``rerank_<rank>.json``. (The reference takes every file with "rerank" in its name for a shard.)"""
    stem, ext = os.path.splitext(name)
    return ext == ".json" and stem.startswith("rerank_") and stem[len("rerank_"):].isdigit()


def merge_rerank_shards(out_dir: str, topk: int = TRAINSET_TOPK) -> List[dict]:
    """reference rerank.py:67-105 without the device-count assertion: a qid present in several shards gets the union of its
    passages; per qid the passages sorted by score, descending, with Python's stable sort (equal scores keep the order in
    which they were read); the first ``topk``."""
    merged_path = os.path.join(out_dir, TRAINSET_NAME)
    if os.path.exists(merged_path):
        print(f"old {TRAINSET_NAME} exists.")
        os.remove(merged_path)
    shards = sorted((p for p in os.listdir(out_dir) if is_rerank_shard(p)), key=lambda p: int(p[len("rerank_"):-len(".json")]))
    qid_to_rankdata: Dict[str, Dict[str, float]] = {}
    for sub in shards:
        with open(os.path.join(out_dir, sub)) as fin:
            for qid, rankdata in json.load(fin).items():
                qid_to_rankdata.setdefault(qid, {}).update(rankdata)
    print("length of qids in qid_to_rankdata: {}".format(len(qid_to_rankdata)))
    examples = []
    for qid, rankdata in qid_to_rankdata.items():
        ranked = sorted(rankdata.items(), key=lambda x: x[1], reverse=True)[:topk]
        examples.append({"qid": qid, "docids": [d for d, _ in ranked], "scores": [s for _, s in ranked]})
    with open(merged_path, "w") as fout:
        for ex in examples:
            fout.write(json.dumps(ex) + "\n")
    for sub in shards:
        os.remove(os.path.join(out_dir, sub))
    return examples


def rerank_for_create_trainset_2(args):
    return merge_rerank_shards(args.out_dir)


def get_args(argv=None):
    """The reference's RerankArguments (arguments.py:215-248), same names and defaults where they are not site paths."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--collection_path", default="")
    ap.add_argument("--out_dir", default="")
    ap.add_argument("--model_name_or_path", default="cross-encoder/ms-marco-MiniLM-L-6-v2")
    ap.add_argument("--max_length", type=int, default=256)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--q_collection_path", default="")
    ap.add_argument("--run_json_path", default="")
    ap.add_argument("--local_rank", "--local-rank", type=int, default=-1)
    ap.add_argument("--task", default=None)
    ap.add_argument("--pseudo_queries_path", default=None)
    ap.add_argument("--docid_pseudo_qids_path", default=None)
    ap.add_argument("--json_type", default="jsonl")
    ap.add_argument("--qid_smtid_docids_path", default=None)
    ap.add_argument("--docid_to_smtid_path", default="")
    ap.add_argument("--pretrained_path", default="")
    ap.add_argument("--dev_queries_path", default="")
    ap.add_argument("--dev_qrels_path", default="")
    ap.add_argument("--qid_docids_path", default="")
    ap.add_argument("--query_to_smtid_tokenizer_type", default="t5-base")
    ap.add_argument("--qid_smtid_rank_path", default="")
    ap.add_argument("--train_qrels_path", default="")
    ap.add_argument("--train_queries_path", default="")
    ap.add_argument("--qid_to_reldocid_hard_docids_path", default=None)
    ap.add_argument("--eval_qrel_path", default=None)
    ap.add_argument("--eval_metrics", default=None)
    # not a reference flag: fp32 = exact fp32 (default), fp16 = f16 operands with fp32 accumulation (the reference's autocast)
    ap.add_argument("--teacher_precision", choices=sorted(TEACHER_PRECISIONS), default="fp32")
    return ap.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    if args.task == "cross_encoder_rerank_for_qid_smtid_docids":
        cross_encoder_rerank_for_qid_smtid_docids(args)
    elif args.task == "cross_encoder_rerank_for_qid_smtid_docids_2":
        cross_encoder_rerank_for_qid_smtid_docids_2(args)
    elif args.task == "rerank_for_create_trainset":
        rerank_for_create_trainset(args)
    elif args.task == "rerank_for_create_trainset_2":
        rerank_for_create_trainset_2(args)
    else:
        raise NotImplementedError(f"rerank task {args.task!r} is not built; built tasks: {', '.join(BUILT_TASKS)}")


if __name__ == "__main__":
    main()
