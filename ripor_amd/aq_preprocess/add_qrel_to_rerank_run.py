"""Replacement of reference aq_preprocess/add_qrel_to_rerank_run.py, with its three hard-coded paths as flags.

Turns the merged teacher run of ``rerank.py --task=rerank_for_create_trainset_2`` (``qid_docids_teacher_scores.train.json``:
one ``{"qid", "docids", "scores"}`` line per query, best first) into the examples the rank-oriented stage trains on
(``qrel_added_qid_docids_teacher_scores.train.json``): one example per (qid, relevant docid) of
``qid_to_reldocid_to_score.json``. A relevant docid that is not among the query's docids is put in front with its score, so
that entry 0 — the positive of ``MarginMSEforT5SeqAQDataset`` — is relevant; otherwise the example is the line unchanged."""
from __future__ import annotations

import argparse
import json
import os
import sys

if __package__ in (None, ""):   # run by file path, as the reference's scripts do
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def get_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--qid_to_reldocid_to_score_path", required=True, help="{qid: {relevant docid: teacher score}}")
    ap.add_argument("--teacher_score_path", required=True, help="jsonl of {qid, docids, scores} (rerank_for_create_trainset_2)")
    ap.add_argument("--out_path", required=True)
    return ap.parse_args(argv)


def add_qrels(examples, qid_to_reldocid_to_score):
    """-> (train examples, number of examples whose relevant docid had to be put in front)."""
    out, added = [], 0
    for ex in examples:
        qid, docids, scores = ex["qid"], ex["docids"], ex["scores"]
        for reldocid, score in qid_to_reldocid_to_score[qid].items():
            if reldocid not in docids:
                out.append({"qid": qid, "docids": [reldocid] + docids, "scores": [score] + scores})
                added += 1
            else:
                out.append({"qid": qid, "docids": docids, "scores": scores})
    return out, added


def main(argv=None):
    args = get_args(argv)
    with open(args.qid_to_reldocid_to_score_path) as fin:
        qid_to_reldocid_to_score = json.load(fin)
    with open(args.teacher_score_path) as fin:
        examples = [json.loads(line) for line in fin if line.strip()]
    train_examples, added = add_qrels(examples, qid_to_reldocid_to_score)
    print("size of train_examples = {}".format(len(train_examples)))
    print("ignored num = {}".format(added))
    with open(args.out_path, "w") as fout:
        for ex in train_examples:
            fout.write(json.dumps(ex) + "\n")


if __name__ == "__main__":
    main()
