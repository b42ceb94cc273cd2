"""``python -m t5_pretrainer.main_rank``: the rank-oriented training stage, ``--loss_type=t5seq_aq_encoder_margin_mse`` (reference
main.py:61-67, 89-90). The reference's scripts run it twice: as the rank-oriented fine-tune after the seq2seq docid step
(full_scripts/full_train_t5seq_seq2seq_0_1_pipeline.sh:38-72: full-length docids looked up in ``--docid_to_smtid_path``) and as
the first rung of the prefix curriculum (full_scripts/full_lng_knp_train_pipline.sh:5-45: ``--smtid_as_docid`` with smtids of 4
codes on a model of 32 positions). Takes the flags those two invocations pass, plus the loop's own (``--max_steps``,
``--save_steps``, ``--logging_steps``, ``--resume_from_checkpoint``, ``--dropout``, ``--local_rank``); the parser, the process
start-up and the driver of ``LngKnpTrainer`` are ``main.py``'s.

The step is the lng_knp step with the single prefix ``[L]`` (``T5SeqAQEncoderForMarginMSE``). ``--max_length`` is at most 256."""
from __future__ import annotations

from .main import base_parser, run_training, start_rank

LOSS_TYPE = "t5seq_aq_encoder_margin_mse"


def get_args(argv=None):
    ap = base_parser(LOSS_TYPE, "t5seq_aq_encoder_margin_mse")
    ap.add_argument("--docid_to_smtid_path", default=None)
    ap.add_argument("--smtid_as_docid", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    from .dataset.margin_mse import MarginMSEforT5SeqAQCollator, MarginMSEforT5SeqAQDataset
    from .modeling.t5_generative_retriever import T5SeqAQEncoderForMarginMSE
    args = get_args(argv)
    if args.loss_type != LOSS_TYPE or args.model_type != "t5_docid_gen_encoder":
        raise NotImplementedError(f"loss_type {args.loss_type!r} is outside this entry point: main_rank trains {LOSS_TYPE} only "
                                  f"(the lng_knp and seq2seq steps: python -m t5_pretrainer.main; the dense first stage: "
                                  f"python -m t5_pretrainer.main_dense)")
    if args.max_length > 256:
        raise SystemExit(f"--max_length {args.max_length}: the training passes take at most 256 query tokens")
    missing = [f"--{n}" for n in ("teacher_score_path", "queries_path") if not getattr(args, n)]
    if missing:
        raise SystemExit(f"{args.loss_type} needs {' and '.join(missing)}")
    if args.smtid_as_docid and args.docid_to_smtid_path is not None:
        raise SystemExit("--smtid_as_docid: the smtids are in the examples; --docid_to_smtid_path must not be given with it")
    if not args.smtid_as_docid and not args.docid_to_smtid_path:
        raise SystemExit(f"{args.loss_type} needs --docid_to_smtid_path or --smtid_as_docid")
    local_rank = start_rank(args)
    dataset = MarginMSEforT5SeqAQDataset(dataset_path=args.teacher_score_path, document_dir=args.collection_path,
                                         query_dir=args.queries_path, docid_to_smtid_path=args.docid_to_smtid_path,
                                         smtid_as_docid=args.smtid_as_docid)
    collator = MarginMSEforT5SeqAQCollator(args.model_name_or_path, max_length=args.max_length)
    model = T5SeqAQEncoderForMarginMSE.from_pretrained(args.resume_from_checkpoint or args.pretrained_path)
    run_training(args, model, dataset, collator, local_rank, "rank-oriented stage")


if __name__ == "__main__":
    main()
