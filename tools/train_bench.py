#!/usr/bin/env python3
"""Time the ranking fine-tune step (BASELINE config 5): t5-base dims (--dims t5-3b: d_model 1024, 32 heads of 128, d_ff 16384,
24 + 24 layers, the dims of bench.py's secondary_t5_3b; --dims t5-v1.1-base: the t5-base stack with d_ff 2048 and the gated-GELU
feed-forward of T5 v1.1 / Flan-T5 / mT5), bz examples per step PER GPU, two teacher-forced
passes of L = 32 positions over queries of ~16 tokens, backward, gradient all-reduce (RCCL when launched on several
ranks), AdamW. --loss seq2seq: the seq2seq docid cross-entropy step instead (one teacher-forced pass per query, the
codebook-logit head). Rank 0 prints one JSON line (examples/s of the whole job, max step time over the ranks).
--lq N: every query N tokens long (92 .. 256: the tiled attention backward) instead of the ~16 of the fine-tune data.
--precision and --loss take comma-separated lists: one JSON line per (precision, loss) on ONE model load (t5-3b: 11 GB of
weights to generate and upload). --embed: before the steps, time rpr_embed on 128 texts of ~16 tokens and 128 texts of 128
tokens (one JSON line).
--step dense (--step is --loss by another name): the dense first-stage step (t5seq_pretrain_margin_mse; the reference trains it
with --bz 64): bz queries of the usual ~16-token mix, bz positive and bz negative documents of --doc_len (128) tokens, all padded
to the document length in one encoder batch of 3 bz sequences, one decoder position each. Its JSON line also reports
query_padding_share: the share of the 3 bz x doc_len encoder rows that are padding behind a query.
--step rank: the rank-oriented step (t5seq_aq_encoder_margin_mse): the lng_knp step with the single prefix [L]. --L 32,4: one leg
per smtid length on the model of --len positions (4 codes on 32 positions is the first rung of the prefix curriculum).
Usage: python tools/train_bench.py [--bz 128] [--steps 5] [--loss lngknp|seq2seq|dense|rank] [--L 32,4] [--dims t5-base|t5-3b|t5-v1.1-base]
                                   [--embed] [--lq N]
       python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P tools/train_bench.py"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripor_amd import engine as E
from ripor_amd.utils import synth

PRECISIONS, LOSSES = ["f16x2", "f32", "bf16"], ["lngknp", "seq2seq", "dense", "rank"]


def listed(choices):
    def parse(v):
        got = v.split(",")
        if any(x not in choices for x in got):
            raise argparse.ArgumentTypeError(f"comma-separated values of {choices}")
        return got
    return parse


ap = argparse.ArgumentParser()
ap.add_argument("--bz", type=int, default=128)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--len", type=int, default=32, dest="L")
ap.add_argument("--precision", default=["f16x2"], type=listed(PRECISIONS))
ap.add_argument("--loss", "--step", dest="loss", default=["lngknp"], type=listed(LOSSES))
ap.add_argument("--L", dest="rank_L", default=None, type=lambda v: [int(x) for x in v.split(",")],
                help="--step rank: smtid lengths, comma-separated, each from 2 to --len (default: --len)")
ap.add_argument("--doc_len", type=int, default=128, help="--step dense: tokens per document (at most 256)")
ap.add_argument("--dims", default="t5-base", choices=["t5-base", "t5-3b", "t5-v1.1-base"])
ap.add_argument("--embed", action="store_true")
ap.add_argument("--lq", type=int, default=0, help="all queries this many tokens long (default: ~16, as the fine-tune data)")
args = ap.parse_args()
L, V, bz = args.L, 256, args.bz
rank_Ls = args.rank_L or [L]
if any(not 2 <= k <= L for k in rank_Ls):
    ap.error(f"--L: smtid lengths from 2 to --len ({L})")
if args.dims == "t5-3b":
    dims = synth.ModelDims(d_model=1024, d_kv=128, d_ff=16384, num_layers=24, num_decoder_layers=24, num_heads=32,
                           decoder_vocab_sizes=[V] * L)
elif args.dims == "t5-v1.1-base":
    dims = synth.t5_v11_base_dims(L=L, V=V)
else:
    dims = synth.t5_base_dims(L=L, V=V)
ff_kind = "gated-gelu" if args.dims == "t5-v1.1-base" else "relu"
ff_mats = 3 if ff_kind == "gated-gelu" else 2          # d_model x d_ff matrices of a feed-forward block
rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
torch.cuda.set_device(local)
if world > 1:
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
ctx = E.Context.get(local)
ctx.set_precision(args.precision[0])
model = E.DeviceModel(ctx, synth.make_state_dict(dims, feed_forward_proj=ff_kind), dims)
state = E.TrainState(model)
qlen = dict(fixed_len=args.lq) if args.lq else dict(mean_len=16, std_len=5, min_len=6, max_len=64)
ids, mask = synth.make_queries(bz * world, vocab_size=dims.vocab_size, seed=5, **qlen)
ids, mask = ids[rank::world], mask[rank::world]          # every rank its own examples, one padded length for all
Lq = ids.shape[1] if args.lq else (ids.shape[1] + 7) // 8 * 8
ids = np.pad(ids, ((0, 0), (0, Lq - ids.shape[1]))); mask = np.pad(mask, ((0, 0), (0, Lq - mask.shape[1])))
codes = synth.make_codes(2 * bz, L, V, seed=5).astype(np.int64).reshape(2, bz, L).transpose(1, 0, 2).copy()
prefix = [L, 4, 8, 16][: {8: 2, 16: 3, 32: 4}[L]]
tp = torch.from_numpy(np.stack([synth.uniform_f32(f"tb/p{k}", (bz,), 30.0) for k in prefix]))
tn = torch.from_numpy(np.stack([synth.uniform_f32(f"tb/n{k}", (bz,), 30.0) for k in prefix]))
ids_t, mask_t, codes_t = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(codes).cuda()


labels_t = codes_t[:, 0].contiguous()   # seq2seq: one smtid per query
if "dense" in args.loss:   # [3, bz, doc_len]: the queries (padded to the document length), the positive and the negative documents
    Ld = max(args.doc_len, ids.shape[1])
    d_ids, d_mask = synth.make_queries(2 * bz, vocab_size=dims.vocab_size, seed=6 + rank, fixed_len=args.doc_len)
    pad = lambda a: np.pad(a, ((0, 0), (0, Ld - a.shape[1])))   # noqa: E731
    dense_ids = torch.from_numpy(np.stack([pad(ids), pad(d_ids[:bz]), pad(d_ids[bz:])])).cuda()
    dense_mask = torch.from_numpy(np.stack([pad(mask), pad(d_mask[:bz]), pad(d_mask[bz:])])).cuda()
    dense_tp, dense_tn = torch.from_numpy(synth.uniform_f32("tb/dp", (bz,), 30.0)), torch.from_numpy(synth.uniform_f32("tb/dn", (bz,), 30.0))


def embed_leg():   # dense embeddings (rpr_embed): 128 texts per call, queries of ~16 tokens and passages of 128
    out = {"task": "rpr_embed, " + args.dims + " dims, 128 texts per call", "ms_per_call": {}}
    for prec in [p for p in args.precision if p != "bf16"] or ["f16x2"]:   # (bf16 is the arithmetic of the training steps only)
        ctx.set_precision(prec)
        for name, kw in (("16_tokens", dict(mean_len=16, std_len=5, min_len=6, max_len=64)), ("128_tokens", dict(fixed_len=128))):
            ei, em = synth.make_queries(128, vocab_size=dims.vocab_size, seed=5, **kw)
            ei, em = torch.from_numpy(ei).cuda(), torch.from_numpy(em).cuda()
            E.embed(model, ei, em); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                E.embed(model, ei, em)
            torch.cuda.synchronize()
            out["ms_per_call"][f"{prec}/{name}"] = round((time.perf_counter() - t0) / args.steps * 1e3, 3)
    ctx.set_precision(args.precision[0])
    print(json.dumps(out), flush=True)


def leg(precision, loss, Lr=None):
    """Lr: the smtid length of a rank leg (the first Lr codes of every smtid, one loss over all of them)."""
    ctx.set_precision(precision)
    if loss == "rank":
        r_codes, r_prefix, r_tp, r_tn = codes_t[:, :, :Lr].contiguous(), [Lr], tp[:1], tn[:1]

    def step():   # backward with the bucketed gradient exchange overlapped (RPR_GRAD_OVERLAP=0: serial), clip, AdamW
        if loss == "seq2seq":
            return E.seq2seq_train_step(model, state, ids_t, mask_t, labels_t, lr=1e-6)
        if loss == "dense":
            return E.dense_mse_train_step(model, state, dense_ids, dense_mask, dense_tp, dense_tn, lr=1e-6)
        if loss == "rank":
            return E.train_step(model, state, ids_t, mask_t, r_codes, r_tp, r_tn, r_prefix, lr=1e-6)
        return E.train_step(model, state, ids_t, mask_t, codes_t, tp, tn, prefix, lr=1e-6)

    first = step(); torch.cuda.synchronize()
    if world > 1: dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    if world > 1: dist.barrier()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    if world > 1:
        t = torch.tensor([dt], device="cuda"); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t)
    ctx.profile_reset(); ctx.profile_enable(True)
    if loss == "seq2seq":
        E.seq2seq_backward(model, state, ids_t, mask_t, labels_t)
    elif loss == "dense":
        E.dense_mse_backward(model, state, dense_ids, dense_mask, dense_tp, dense_tn)
    elif loss == "rank":
        E.lngknp_backward(model, state, ids_t, mask_t, r_codes, r_tp, r_tn, r_prefix)
    else:
        E.lngknp_backward(model, state, ids_t, mask_t, codes_t, tp, tn, prefix)
    torch.cuda.synchronize()
    st = ctx.profile_get(); ctx.profile_enable(False)
    dm, inner, dff, nd = dims.d_model, dims.inner, dims.d_ff, dims.num_decoder_layers
    Lpos = Lr if loss == "rank" else L     # decoder positions per document
    flops_fwd = 2.0 * (bz * float(mask.sum(1).mean()) * (dims.num_layers * (4 * dm * inner + ff_mats * dm * dff) + nd * 2 * dm * inner)
                       + bz * (1 if loss == "seq2seq" else 2) * Lpos * nd * (6 * dm * inner + ff_mats * dm * dff)
                       + (bz * L * V * dm if loss == "seq2seq" else 0))
    extra = {}
    if loss == "dense":   # real tokens of the 3 bz sequences through the encoder and the cross K/V, one decoder row per sequence
        tokens = float(dense_mask.sum())
        flops_fwd = 2.0 * (tokens * (dims.num_layers * (4 * dm * inner + ff_mats * dm * dff) + nd * 2 * dm * inner)
                           + 3 * bz * nd * (6 * dm * inner + ff_mats * dm * dff))
        rows = float(dense_mask.numel())
        extra = {"doc_len": args.doc_len, "encoder_rows": int(rows), "padding_share": round(1.0 - tokens / rows, 4),
                 "query_padding_share": round(float((1 - dense_mask[0]).sum()) / rows, 4)}
    if rank == 0:
        task = {"seq2seq": "seq2seq docid cross-entropy step", "dense": "dense first-stage margin-MSE step",
                "rank": "rank-oriented margin-MSE step"}.get(loss, "lng_knp margin-MSE fine-tune step")
        print(json.dumps({"task": task + " (forward + backward + gradient all-reduce + AdamW), " + args.dims + " dims", "loss": loss,
                          "gemm_precision": precision, "n_gpus": world, "scaling": "weak", "bz_per_gpu": bz,
                          "bz": bz, "L": Lpos, "model_positions": L, "enc_len_padded": int(dense_ids.shape[2] if loss == "dense" else Lq), **extra, "ms_per_step": dt * 1e3, "examples_per_s": world * bz / dt,
                          "loss_first": [float(x) for x in first], "loss_last": [float(x) for x in last],
                          "params": state.total, "approx_tflops": 3 * flops_fwd / dt / 1e12,
                          "backward_kernel_ms": {k: round(v["total_ms"], 3) for k, v in st.items()}}), flush=True)


if args.embed and rank == 0:
    embed_leg()
for precision in args.precision:
    for loss in args.loss:
        for Lr in (rank_Ls if loss == "rank" else [None]):
            leg(precision, loss, Lr)
