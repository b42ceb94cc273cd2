"""Data side of the rank-oriented step (loss_type ``t5seq_aq_encoder_margin_mse``): the examples file with teacher scores
-> batches in the layout ``T5SeqAQEncoderForMarginMSE`` consumes.

Same class names, constructor arguments, item tuples and batch keys as the reference (``MarginMSEforT5SeqAQDataset``
dataset/dataset.py:552-616, ``MarginMSEforT5SeqAQCollator`` dataset/data_collator.py:115-150):

* examples: one JSON object per line — ``qid``, ``docids`` (or, with ``smtid_as_docid``, ``smtids`` as ``"a_b_c_d"`` strings) and
  ``scores``; entry 0 is the positive, one negative is drawn with ``random.sample(range(1, n), k=1)`` per item like the
  reference (so Python's ``random`` seed fixes the epoch);
* doc encoding = smtid[1:], decoder_input_ids = smtid[:-1] with smtid[0] = -1, looked up in ``docid_to_smtid.json`` or parsed
  from the smtid string;
* the positive and the negative example of a row carry the same query text (``"query: " + text``).

``document_dir`` is accepted and not opened: the reference preloads the passages and never reads them.
"""
from __future__ import annotations

import json
import random

import torch

from .lng_knp import CollectionDatasetPreLoad


class MarginMSEforT5SeqAQDataset(torch.utils.data.Dataset):
    def __init__(self, dataset_path, document_dir, query_dir, docid_to_smtid_path, smtid_as_docid=False):
        self.document_dataset = None
        self.query_dataset = CollectionDatasetPreLoad(query_dir, id_style="content_id")
        self.examples = []
        with open(dataset_path) as fin:
            for line in fin:
                if line.strip():
                    self.examples.append(json.loads(line))
        self.smtid_as_docid = smtid_as_docid
        if smtid_as_docid:
            assert docid_to_smtid_path is None, "smtid_as_docid: the smtids are in the examples, docid_to_smtid_path must be None"
            self.docid_to_smtid = None
        elif docid_to_smtid_path is not None:
            with open(docid_to_smtid_path) as fin:
                self.docid_to_smtid = json.load(fin)
            first = next(iter(self.docid_to_smtid.values()))
            assert first[0] == -1, first
        else:
            self.docid_to_smtid = None

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, idx):
        ex = self.examples[idx]
        key = "smtids" if self.smtid_as_docid else "docids"
        positive = ex[key][0]
        neg_idx = random.sample(range(1, len(ex[key])), k=1)[0]
        negative = ex[key][neg_idx]
        q = self.query_dataset[str(ex["qid"])][1]
        if self.smtid_as_docid:
            pos = [-1] + [int(x) for x in positive.split("_")]
            neg = [-1] + [int(x) for x in negative.split("_")]
        else:
            pos, neg = self.docid_to_smtid[str(positive)], self.docid_to_smtid[str(negative)]
        text = "query: " + q.strip()
        return text, text, pos[1:], neg[1:], ex["scores"][0], ex["scores"][neg_idx], pos[:-1], neg[:-1]


class MarginMSEforT5SeqAQCollator:
    """Tuples of the dataset above -> the ``forward(**inputs)`` dict (reference data_collator.py:115-150). ``tokenizer_type``:
    a checkpoint directory / model name for ``AutoTokenizer.from_pretrained``, or a tokenizer object."""

    def __init__(self, tokenizer_type, max_length):
        self.max_length = max_length
        if isinstance(tokenizer_type, str):
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(tokenizer_type)
        else:
            self.tokenizer = tokenizer_type

    def __call__(self, batch):
        q_pos, q_neg, pos_enc, neg_enc, s_pos, s_neg, pos_dec, neg_dec = [list(x) for x in zip(*batch)]
        tok = dict(add_special_tokens=True, padding="longest", truncation="longest_first", max_length=self.max_length,
                   return_attention_mask=True, return_tensors="pt")
        q_pos, q_neg = self.tokenizer(q_pos, **tok), self.tokenizer(q_neg, **tok)
        q_pos["decoder_input_ids"] = torch.LongTensor(pos_dec)
        q_neg["decoder_input_ids"] = torch.LongTensor(neg_dec)
        return {"pos_tokenized_query": q_pos, "neg_tokenized_query": q_neg,
                "pos_doc_encoding": torch.LongTensor(pos_enc), "neg_doc_encoding": torch.LongTensor(neg_enc),
                "teacher_pos_scores": torch.FloatTensor(s_pos), "teacher_neg_scores": torch.FloatTensor(s_neg)}
