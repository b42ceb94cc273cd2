"""Data side of the seq2seq docid step (loss_type ``t5seq_aq_encoder_seq2seq``): a jsonl of ``{"docid", "query"}`` pairs and
``docid_to_smtid.json`` -> batches in the layout ``T5SeqAQEncoderForSeq2Seq`` consumes.

Same class names, constructor arguments, item tuples and batch keys as the reference (``Seq2SeqForT5SeqAQDataset``
dataset/dataset.py:527-550, ``Seq2SeqForT5SeqAQCollator`` dataset/data_collator.py:90-113):

* item = ``(query, smtid[:-1], smtid[1:])`` with ``smtid = docid_to_smtid[docid]`` starting with -1, ``len(smtid)`` in
  {2, 5, 9, 17, 33};
* batch = ``{"tokenized_query": tokenizer(queries) + decoder_input_ids, "labels": LongTensor [bz, L]}``.

``docid_to_smtid.json`` (1.28 GB for MS MARCO) goes through the streaming reader of the search path
(``engine.read_docid_to_smtid``, host only) instead of ``ujson.load``: the codes stay one uint16 matrix.
"""
from __future__ import annotations

import json

import torch

from .. import engine as E


class Seq2SeqForT5SeqAQDataset(torch.utils.data.Dataset):
    def __init__(self, example_path, docid_to_smtid_path):
        docids, codes = E.read_docid_to_smtid(docid_to_smtid_path)
        row = {d: i for i, d in enumerate(docids)}
        self.codes = codes
        self.examples = []
        with open(example_path) as fin:
            for line in fin:
                if not line.strip():
                    continue
                example = json.loads(line)
                docid, query = str(example["docid"]), example["query"]
                self.examples.append((query, row[docid]))   # KeyError for a docid the map does not know, like the reference

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, idx):
        query, r = self.examples[idx]
        smtid = [-1] + [int(x) for x in self.codes[r]]
        query_decoder_input_ids = smtid[:-1]
        query_smtids = smtid[1:]
        assert len(smtid) in [2, 5, 9, 17, 33], len(smtid)
        assert len(query_smtids) == len(query_decoder_input_ids) and query_decoder_input_ids[0] == -1
        return query, query_decoder_input_ids, query_smtids


class Seq2SeqForT5SeqAQCollator:
    """``tokenizer_type``: a checkpoint directory / model name for ``AutoTokenizer.from_pretrained``, or a tokenizer object."""

    def __init__(self, tokenizer_type, max_length):
        self.max_length = max_length
        if isinstance(tokenizer_type, str):
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(tokenizer_type)
        else:
            self.tokenizer = tokenizer_type

    def __call__(self, batch):
        query, query_decoder_input_ids, query_smtids = [list(x) for x in zip(*batch)]
        tokenized_query = self.tokenizer(query, add_special_tokens=True, padding="longest", truncation="longest_first",
                                         max_length=self.max_length, return_attention_mask=True, return_tensors="pt")
        tokenized_query["decoder_input_ids"] = torch.LongTensor(query_decoder_input_ids)
        return {"tokenized_query": tokenized_query, "labels": torch.LongTensor(query_smtids)}
