"""Data side of the dense first-stage step (loss_type ``t5seq_pretrain_margin_mse``): a jsonl of teacher-scored candidates
``{"qid", "docids", "scores"}``, the collection and the queries (``raw.tsv``: id, tab, text) -> batches in the layout
``T5SeqPretrainEncoder.forward`` consumes.

Same class names, constructor arguments, item tuples and batch keys as the reference (``MarginMSEforPretrainDataset``
dataset/dataset.py:618-682, ``MarginMSEforPretrainCollator`` dataset/data_collator.py:152-210) in the case its training scripts
run, without ``docid_to_smtid_path``:

* item = ``("query: " + q, "query: " + q, "document: " + d+, "document: " + d-, s+, s-, [-1], [-1], [-1], [-1])``: the first
  docid of an example is the positive, the negative is drawn from the others with ``random.sample`` (seed ``random`` to
  reproduce an epoch);
* batch = ``{"tokenized_pos_query", "tokenized_neg_query", "tokenized_pos_doc", "tokenized_neg_doc"`` (each the tokenizer's
  output + ``decoder_input_ids`` ``[bz, 1]`` of -1), ``"teacher_pos_score", "teacher_neg_score"`` FloatTensor ``[bz]}``.

With a ``docid_to_smtid_path`` the reference adds the commit loss over the document's codes (decoder length > 1); that branch is
not built here and the argument is refused.
"""
from __future__ import annotations

import json
import random

import torch

from .lng_knp import CollectionDatasetPreLoad


class MarginMSEforPretrainDataset(torch.utils.data.Dataset):
    def __init__(self, dataset_path, document_dir, query_dir, qrels_path=None, docid_to_smtid_path=None):
        if docid_to_smtid_path is not None:
            raise NotImplementedError("MarginMSEforPretrainDataset with docid_to_smtid_path feeds the commit loss of the reference "
                                      "(decoder length > 1), which is not built: the dense first stage trains without it")
        self.document_dataset = CollectionDatasetPreLoad(document_dir, id_style="content_id")
        self.query_dataset = CollectionDatasetPreLoad(query_dir, id_style="content_id")
        self.examples = []
        with open(dataset_path) as fin:
            for line in fin:
                if line.strip():
                    self.examples.append(json.loads(line))

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, idx):
        example = self.examples[idx]
        positive, s_pos = example["docids"][0], example["scores"][0]
        neg_idx = random.sample(range(1, len(example["docids"])), k=1)[0]
        negative, s_neg = example["docids"][neg_idx], example["scores"][neg_idx]
        q_text = "query: " + self.query_dataset[str(example["qid"])][1].strip()
        d_pos = "document: " + self.document_dataset[positive][1].strip()
        d_neg = "document: " + self.document_dataset[negative][1].strip()
        return q_text, q_text, d_pos, d_neg, s_pos, s_neg, [-1], [-1], [-1], [-1]


class MarginMSEforPretrainCollator:
    """``tokenizer_type``: a checkpoint directory / model name for ``AutoTokenizer.from_pretrained``, or a tokenizer object."""

    def __init__(self, tokenizer_type, max_length):
        self.max_length = max_length
        if isinstance(tokenizer_type, str):
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(tokenizer_type)
        else:
            self.tokenizer = tokenizer_type

    def _tok(self, texts, decoder_input_ids):
        out = self.tokenizer(texts, add_special_tokens=True, padding="longest", truncation="longest_first",
                             max_length=self.max_length, return_attention_mask=True, return_tensors="pt")
        out["decoder_input_ids"] = torch.LongTensor(decoder_input_ids)
        return out

    def __call__(self, batch):
        if len(batch[0]) != 10:
            raise ValueError(f"the batch example with size {len(batch[0])} is not valid.")
        q_pos, q_neg, d_pos, d_neg, s_pos, s_neg, d_pos_dec, d_neg_dec, q_pos_dec, q_neg_dec = [list(x) for x in zip(*batch)]
        # (the reference gives the queries the documents' decoder inputs and the other way round: all are [-1] here)
        return {"tokenized_pos_query": self._tok(q_pos, d_pos_dec), "tokenized_neg_query": self._tok(q_neg, d_neg_dec),
                "tokenized_pos_doc": self._tok(d_pos, q_pos_dec), "tokenized_neg_doc": self._tok(d_neg, q_neg_dec),
                "teacher_pos_score": torch.FloatTensor(s_pos), "teacher_neg_score": torch.FloatTensor(s_neg)}
