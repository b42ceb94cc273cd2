"""CLI-compatible replacement of reference aq_preprocess/argparse_from_qid_smtid_rank_to_qid_smtid_docids.py: the host step
between the rank-data pass and the teacher scoring. Reads ``root_dir/qid_smtid_rankdata.json``
(``{qid: {smtid: {docid: score}}}``), writes ``root_dir/qid_smtid_docids.train.json`` (``{qid: {smtid: [docids]}}``, in
file order); an smtid without docids is dropped, its qid stays."""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict


def rankdata_to_docids(qid_to_smtid_to_rank: Dict[str, dict]):
    """-> ({qid: {smtid: [docids]}}, smtids seen, smtids dropped)"""
    out: Dict[str, Dict[str, list]] = {}
    total = ignored = 0
    for qid, by_smtid in qid_to_smtid_to_rank.items():
        out[qid] = {}
        for smtid, rank_data in by_smtid.items():
            total += 1
            if len(rank_data) == 0:
                ignored += 1
            else:
                out[qid][smtid] = list(rank_data.keys())
    return out, total, ignored


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", default=None, type=str)
    args = ap.parse_args(argv)
    print("root_dir: ", args.root_dir)
    with open(os.path.join(args.root_dir, "qid_smtid_rankdata.json")) as fin:
        qid_to_smtid_to_rank = json.load(fin)
    out, total, ignored = rankdata_to_docids(qid_to_smtid_to_rank)
    print("total_num = {}, ignore_num = {}, ratio = {:.3f}".format(total, ignored, ignored / max(total, 1)))
    with open(os.path.join(args.root_dir, "qid_smtid_docids.train.json"), "w") as fout:
        json.dump(out, fout)


if __name__ == "__main__":
    main()
