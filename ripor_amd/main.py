"""``python -m t5_pretrainer.main`` for the two training tasks on this repository's path: the prefix-oriented ranking
fine-tune (``--loss_type=t5seq_aq_encoder_lng_knp_margin_mse``; reference main.py:68-74, 93-94, 127-186 and
full_scripts/full_lng_knp_train_pipline.sh:80-99) and the seq2seq docid step that teaches the model to generate docids
(``--loss_type=t5seq_aq_encoder_seq2seq``; reference main.py:75-79, 91-92 and full_16_1024_scripts/full_train_t5seq_aq_encoder.sh).
Same flags as the reference's ``Arguments`` as far as those tasks read them; every other loss type is out of scope
 and refused.

One process per GPU (``torchrun --nproc-per-node N -m t5_pretrainer.main ...``): ``torch.distributed`` backend "nccl" = RCCL;
the gradient exchange is bucketed and overlapped with the backward inside ``training_step``."""
from __future__ import annotations

import argparse
import json
import os

import torch


def base_parser(loss_type, run_name):
    """The flags every training entry point takes (this module, main_dense and main_rank)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss_type", default=loss_type)
    ap.add_argument("--model_type", default="t5_docid_gen_encoder")
    ap.add_argument("--model_name_or_path", default="t5-base", help="tokenizer source (a directory works offline)")
    ap.add_argument("--pretrained_path", required=True)
    ap.add_argument("--teacher_score_path", default=None, help="the examples with teacher scores (lng_knp, dense: required there)")
    ap.add_argument("--collection_path", default=None)
    ap.add_argument("--queries_path", default=None, help="the query collection directory (lng_knp, dense: required there)")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--run_name", default=run_name)
    ap.add_argument("--max_length", type=int, default=64)
    ap.add_argument("--per_device_train_batch_size", type=int, default=96)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--warmup_ratio", type=float, default=0.04)
    ap.add_argument("--epochs", type=float, default=3)
    ap.add_argument("--max_steps", type=int, default=-1)
    ap.add_argument("--logging_steps", type=int, default=50)
    ap.add_argument("--save_steps", type=int, default=15_000)
    ap.add_argument("--resume_from_checkpoint", default=None,
                    help="an output_dir/checkpoint-<step> directory: weights, AdamW moments, step count and RNG states are restored "
                         "and the loop continues at the recorded step (HF TrainingArguments.resume_from_checkpoint)")
    ap.add_argument("--task_names", default=None, help='JSON list, e.g. ["rank","rank_4"]')
    ap.add_argument("--ln_to_weight", default=None, help="JSON dict of task weights (only 1.0 is built)")
    ap.add_argument("--use_fp16", action="store_true", help="bf16 GEMM operands, like the reference (main.py:152 bf16=args.use_fp16)")
    ap.add_argument("--dropout", default="off",
                    help="off | config | <rate in [0, 1)>: dropout of the training step. off (default): evaluation arithmetic; config: "
                         "the checkpoint's dropout_rate, what the reference trains with (model.train()). Deviation from the reference: "
                         "the encoder runs once per query, so the positive and the negative pass share ONE encoder mask (the "
                         "reference draws two); decoder-side masks are independent per document")
    ap.add_argument("--wandb_project_name", default=None, help="accepted and ignored (no network)")
    ap.add_argument("--local_rank", type=int, default=-1)
    return ap


def get_args(argv=None):
    ap = base_parser("t5seq_aq_encoder_lng_knp_margin_mse", "lng_knp")
    ap.add_argument("--query_to_docid_path", default=None, help="seq2seq: jsonl of {\"docid\", \"query\"} (required there)")
    ap.add_argument("--multi_vocab_sizes", action="store_true",
                    help="seq2seq: per-position mean of the cross-entropy (the same value with one codebook size for every position)")
    ap.add_argument("--docid_to_smtid_path", default=None)
    ap.add_argument("--smtid_as_docid", action="store_true")
    return ap.parse_args(argv)


def resolve_dropout(flag: str, config_rate: float, log=print) -> float:
    """--dropout=off|config|<float> against the checkpoint's dropout_rate -> the rate the trainer applies."""
    if flag == "off":
        if config_rate:
            log(f"--dropout=off: the checkpoint's dropout_rate {config_rate} is NOT applied (the reference trains with it; "
                f"--dropout=config applies it)")
        return 0.0
    rate = float(config_rate) if flag == "config" else float(flag)
    if not 0.0 <= rate < 1.0:
        raise SystemExit(f"--dropout {flag}: the rate must be in [0, 1)")
    return rate


def start_rank(args) -> int:
    """The local rank of this process; joins the process group of a multi-process launch (torchrun)."""
    import torch.distributed as dist
    local_rank = max(0, int(args.local_rank if args.local_rank >= 0 else os.environ.get("LOCAL_RANK", 0)))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=os.environ.get("RPR_DIST_BACKEND", "nccl"))
    return local_rank


def run_training(args, model, dataset, collator, local_rank: int, what: str) -> None:
    """Drive LngKnpTrainer over (model, dataset, collator) as the flags say and leave the final model under output_dir/checkpoint."""
    import torch.distributed as dist
    from .tasks.trainer import LngKnpTrainer, LngKnpTrainingArgs
    model.to(local_rank)
    dropout_rate = resolve_dropout(args.dropout, float(getattr(model.config, "dropout_rate", 0.0)),
                                   log=print if local_rank == 0 else (lambda s: None))
    targs = LngKnpTrainingArgs(output_dir=args.output_dir, learning_rate=args.learning_rate, warmup_ratio=args.warmup_ratio,
                               per_device_train_batch_size=args.per_device_train_batch_size, num_train_epochs=args.epochs,
                               max_steps=args.max_steps, logging_steps=args.logging_steps, save_steps=args.save_steps,
                               bf16=args.use_fp16, task_names=json.loads(args.task_names) if args.task_names else None,
                               ln_to_weight=json.loads(args.ln_to_weight) if args.ln_to_weight else {},
                               dropout_rate=dropout_rate)
    os.makedirs(args.output_dir, exist_ok=True)
    trainer = LngKnpTrainer(model, dataset, collator, targs)
    if trainer.rank == 0:
        print(f"{args.loss_type} ({what}): {len(dataset)} examples, {trainer.world} rank(s) x {targs.per_device_train_batch_size}, "
              f"{trainer.max_steps} steps ({trainer.warmup_steps} warm-up), lr {targs.learning_rate}, "
              f"{'bf16' if targs.bf16 else 'fp32-equivalent'} GEMMs, dropout {targs.dropout_rate or 'off'}")
    trainer.train(resume_from_checkpoint=args.resume_from_checkpoint or None)
    trainer.save_torch_model_and_tokenizer(collator.tokenizer)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    from .dataset.lng_knp import LngKnpMarginMSEforT5SeqAQCollator, LngKnpMarginMSEforT5SeqAQDataset
    from .modeling.t5_generative_retriever import T5SeqAQEncoderForLngKnpMarginMSE, T5SeqAQEncoderForSeq2Seq
    args = get_args(argv)
    built = ("t5seq_aq_encoder_lng_knp_margin_mse", "t5seq_aq_encoder_seq2seq")
    if args.loss_type not in built or args.model_type != "t5_docid_gen_encoder":
        raise NotImplementedError(f"loss_type {args.loss_type!r} is outside this repository's path (SURVEY.md §2); "
                                  f"built: {', '.join(built)} (t5seq_pretrain_margin_mse: python -m t5_pretrainer.main_dense; "
                                  f"t5seq_aq_encoder_margin_mse: python -m t5_pretrainer.main_rank)")
    seq2seq = args.loss_type == "t5seq_aq_encoder_seq2seq"
    need = ("query_to_docid_path", "docid_to_smtid_path") if seq2seq else ("teacher_score_path", "queries_path")
    missing = [f"--{n}" for n in need if not getattr(args, n)]
    if missing:
        raise SystemExit(f"{args.loss_type} needs {' and '.join(missing)}")
    local_rank = start_rank(args)
    if seq2seq:
        from .dataset.seq2seq import Seq2SeqForT5SeqAQCollator, Seq2SeqForT5SeqAQDataset
        if args.max_length > 256:
            raise SystemExit(f"--max_length {args.max_length}: the training passes take at most 256 query tokens")
        dataset = Seq2SeqForT5SeqAQDataset(example_path=args.query_to_docid_path, docid_to_smtid_path=args.docid_to_smtid_path)
        collator = Seq2SeqForT5SeqAQCollator(args.model_name_or_path, max_length=args.max_length)
        model = T5SeqAQEncoderForSeq2Seq.from_pretrained(args.resume_from_checkpoint or args.pretrained_path,
                                                         multi_vocab_sizes=args.multi_vocab_sizes)
    else:
        dataset = LngKnpMarginMSEforT5SeqAQDataset(dataset_path=args.teacher_score_path, document_dir=args.collection_path,
                                                   query_dir=args.queries_path, docid_to_smtid_path=args.docid_to_smtid_path,
                                                   smtid_as_docid=args.smtid_as_docid)
        collator = LngKnpMarginMSEforT5SeqAQCollator(args.model_name_or_path, max_length=args.max_length)
        model = T5SeqAQEncoderForLngKnpMarginMSE.from_pretrained(args.resume_from_checkpoint or args.pretrained_path)
    run_training(args, model, dataset, collator, local_rank, "seq2seq docid step" if seq2seq else "lng_knp fine-tune")


if __name__ == "__main__":
    main()
