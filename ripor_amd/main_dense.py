"""``python -m t5_pretrainer.main_dense``: training of the dense first-stage encoder, ``--loss_type=t5seq_pretrain_margin_mse``
(reference main.py:54-60, 86-88 and full_scripts/full_train_t5seq_encoder_0.sh / _1.sh: batch 64, ``--max_length=128``, bf16).
Takes the flags those two scripts pass, plus the loop's own (``--max_steps``, ``--save_steps``, ``--logging_steps``,
``--resume_from_checkpoint``, ``--dropout``, ``--local_rank``); the parser, the process start-up and the driver of
``LngKnpTrainer`` are ``main.py``'s. ``--pretrained_path`` is a checkpoint of this project's format (round 1 of the reference's
pipeline) or a plain HF T5 directory (round 0), for which ``--decoder_start_token_path`` names the start embedding.

Queries and documents go through one encoder batch padded to one length, so ``--max_length`` is at most 256. The commit loss of
the reference (``--docid_to_smtid_path``, decoder length > 1) is not built."""
from __future__ import annotations

from .main import base_parser, run_training, start_rank

LOSS_TYPE = "t5seq_pretrain_margin_mse"


def get_args(argv=None):
    ap = base_parser(LOSS_TYPE, "t5_docid_gen_encoder")
    ap.add_argument("--qrels_path", default=None, help="accepted for the reference's dataset signature; not read")
    ap.add_argument("--decoder_start_token_path", default=None,
                    help="plain T5 --pretrained_path only: the .npy with the decoder start embedding [1, 1, d_model] "
                         "(default: the checkpoint config's decoder_start_token_path)")
    ap.add_argument("--codebook_seed", type=int, default=0, help="plain T5 --pretrained_path only: seed of the (unused) codebooks")
    ap.set_defaults(max_length=128, per_device_train_batch_size=64)   # what the reference's two scripts pass
    return ap.parse_args(argv)


def main(argv=None):
    from .dataset.pretrain import MarginMSEforPretrainCollator, MarginMSEforPretrainDataset
    from .modeling.t5_generative_retriever import T5SeqPretrainEncoder
    args = get_args(argv)
    if args.loss_type != LOSS_TYPE or args.model_type != "t5_docid_gen_encoder":
        raise NotImplementedError(f"loss_type {args.loss_type!r} is outside this entry point: main_dense trains {LOSS_TYPE} only "
                                  f"(the ranking and seq2seq steps: python -m t5_pretrainer.main)")
    if args.max_length > 256:
        raise SystemExit(f"--max_length {args.max_length}: the training passes take at most 256 tokens per query or document")
    missing = [f"--{n}" for n in ("teacher_score_path", "collection_path", "queries_path") if not getattr(args, n)]
    if missing:
        raise SystemExit(f"{args.loss_type} needs {' and '.join(missing)}")
    local_rank = start_rank(args)
    dataset = MarginMSEforPretrainDataset(dataset_path=args.teacher_score_path, document_dir=args.collection_path,
                                          query_dir=args.queries_path, qrels_path=args.qrels_path, docid_to_smtid_path=None)
    collator = MarginMSEforPretrainCollator(args.model_name_or_path, max_length=args.max_length)
    model = T5SeqPretrainEncoder.from_pretrained(args.resume_from_checkpoint or args.pretrained_path,
                                                 decoder_start_token_path=args.decoder_start_token_path,
                                                 codebook_seed=args.codebook_seed)
    run_training(args, model, dataset, collator, local_rank, "dense first stage")


if __name__ == "__main__":
    main()
