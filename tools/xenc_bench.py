"""Cross-encoder teacher benchmark: times engine.xenc_score (rpr_xenc_score) at the dimensions of
cross-encoder/ms-marco-MiniLM-L-6-v2 (6 layers, hidden 384, 12 heads of 32, d_ff 1536, vocab 30522) with seeded random
weights on --pairs (query, passage) pairs, for two seeded inputs:

  full  every pair --max_len tokens long (no padding anywhere);
  mix   a length mix as MS MARCO pairs give it: lengths 20 .. --max_len, mean about 90, padded to the longest.

Per input: pairs/s (best and median of --repeats warm calls by device events, the packing and the upload included), then
one profiled call (per-kernel-class device events) for the rate of the GEMMs against the peak of the mode (--precision f32:
the 157.3 TF/s fp32 MFMA peak; f16: the 2516.6 TF/s dense f16 MFMA peak) and the share of device time in attention. As the yardstick on the same card and inputs, HF BertForSequenceClassification
in torch on the padded batch, in fp32 and under fp16 autocast (how the reference runs its teacher). One JSON line on stdout.

  python tools/xenc_bench.py --pairs 256 --max_len 256 [--precision f16]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_TFLOPS = 157.3
PEAK_F16_TFLOPS = 2516.6   # dense f16 MFMA
DIMS = dict(vocab_size=30522, hidden=384, layers=6, heads=12, d_ff=1536, max_pos=512, type_vocab=2)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def make_inputs(kind, pairs, max_len, seed):
    rng = np.random.default_rng(seed)
    if kind == "full":
        lens = np.full(pairs, max_len)
    else:   # 20 + a gamma tail, clipped: mean about 90
        lens = np.clip(20 + rng.gamma(2.0, 35.0, size=pairs), 20, max_len).astype(np.int64)
    L = int(lens.max())
    ids = torch.from_numpy(rng.integers(1000, DIMS["vocab_size"], size=(pairs, L)))
    mask = (torch.arange(L)[None] < torch.from_numpy(lens)[:, None]).long()
    types = ((torch.arange(L)[None] >= 12) & (mask == 1)).long()
    return ids * mask, types, mask, lens


def hf_model(weights, cfg):
    from transformers import BertConfig, BertForSequenceClassification
    hc = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                    intermediate_size=cfg.d_ff, max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, num_labels=1,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = BertForSequenceClassification(hc).eval()
    H = cfg.hidden
    sd = {"bert.embeddings.word_embeddings.weight": weights["word_emb"], "bert.embeddings.position_embeddings.weight": weights["pos_emb"],
          "bert.embeddings.token_type_embeddings.weight": weights["type_emb"], "bert.embeddings.LayerNorm.weight": weights["emb_ln_w"],
          "bert.embeddings.LayerNorm.bias": weights["emb_ln_b"], "bert.pooler.dense.weight": weights["pool_w"],
          "bert.pooler.dense.bias": weights["pool_b"], "classifier.weight": weights["cls_w"][None], "classifier.bias": weights["cls_b"]}
    for n in range(cfg.layers):
        p = f"bert.encoder.layer.{n}."
        for i, x in enumerate(("query", "key", "value")):
            sd[p + f"attention.self.{x}.weight"] = weights["qkv_w"][n, i * H:(i + 1) * H]
            sd[p + f"attention.self.{x}.bias"] = weights["qkv_b"][n, i * H:(i + 1) * H]
        for ours, theirs in (("ao", "attention.output.dense"), ("ff1", "intermediate.dense"), ("ff2", "output.dense")):
            sd[p + theirs + ".weight"], sd[p + theirs + ".bias"] = weights[ours + "_w"][n], weights[ours + "_b"][n]
        for ours, theirs in (("ln1", "attention.output.LayerNorm"), ("ln2", "output.LayerNorm")):
            sd[p + theirs + ".weight"], sd[p + theirs + ".bias"] = weights[ours + "_w"][n], weights[ours + "_b"][n]
    missing = m.load_state_dict(sd, strict=False)
    assert not [k for k in missing.missing_keys if "position_ids" not in k and "token_type_ids" not in k], missing
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--max_len", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no_torch", action="store_true", help="skip the HF yardstick")
    ap.add_argument("--precision", choices=("f32", "f16"), default="f32", help="engine.XencModel.set_precision")
    args = ap.parse_args()
    from ripor_amd import engine as E
    ctx = E.Context.get(0)
    cfg = E.XencConfig(**DIMS)
    g = torch.Generator().manual_seed(0)
    weights = {}
    for name, shape in E.xenc_weight_shapes(cfg).items():
        n = torch.randn(shape, generator=g)
        weights[name] = (1.0 + 0.2 * n) if name.endswith("ln_w") or name in ("ln1_w", "ln2_w") else \
            (0.1 * n) if name.endswith("_b") else n if name.endswith("_emb") else n / cfg.hidden ** 0.5
    model = E.XencModel(ctx, weights, cfg)
    model.set_precision(args.precision)
    peak = PEAK_F16_TFLOPS if args.precision == "f16" else PEAK_F32_TFLOPS
    hf = None if args.no_torch else hf_model(weights, cfg).cuda()
    out = dict(dims=DIMS, pairs=args.pairs, max_len=args.max_len, precision=model.precision, peak_f32_tflops=PEAK_F32_TFLOPS,
               peak_f16_tflops=PEAK_F16_TFLOPS, inputs={})
    for kind in ("full", "mix"):
        ids, types, mask, lens = make_inputs(kind, args.pairs, args.max_len, seed=11)
        run = lambda: E.xenc_score(model, ids, types, mask)  # noqa: E731
        cold, ours = _timed(run)
        warm = sorted(_timed(run)[0] for _ in range(max(3, args.repeats)))
        ctx.profile_reset(); ctx.profile_enable(True)
        run(); torch.cuda.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        dev_ms = sum(v["total_ms"] for v in prof.values())
        gemm = prof["gemm"]
        r = dict(tokens=int(lens.sum()), mean_len=float(lens.mean()), padded_len=int(mask.shape[1]), cold_s=cold, best_s=warm[0],
                 median_s=warm[len(warm) // 2], pairs_per_s=args.pairs / warm[0], pairs_per_s_median=args.pairs / warm[len(warm) // 2],
                 kernel_ms=dev_ms, gemm_ms=gemm["total_ms"], gemm_tflops=gemm["flops"] / (gemm["total_ms"] * 1e-3) / 1e12,
                 attn_ms=prof["enc_attn"]["total_ms"], attn_share=prof["enc_attn"]["total_ms"] / dev_ms,
                 other_ms=prof["other"]["total_ms"])
        r["gemm_frac_of_peak"] = r["gemm_tflops"] / peak
        r["gemm_gbytes_per_s"] = gemm["bytes"] / (gemm["total_ms"] * 1e-3) / 1e9   # operands and results once: a lower bound
        r["finite"] = bool(torch.isfinite(ours).all())
        r["score_sha256"] = __import__("hashlib").sha256(ours.cpu().numpy().tobytes()).hexdigest()
        if hf is not None:
            kw = {"input_ids": ids.cuda(), "token_type_ids": types.cuda(), "attention_mask": mask.cuda()}
            for label, amp in (("torch_fp32", False), ("torch_fp16_autocast", True)):
                def hf_run():
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                        return hf(**kw).logits.view(-1).float()
                _, y = _timed(hf_run)
                t = sorted(_timed(hf_run)[0] for _ in range(max(3, args.repeats)))
                r[label] = dict(best_s=t[0], median_s=t[len(t) // 2], pairs_per_s=args.pairs / t[0],
                                max_abs_diff_to_ours=float((y - ours).abs().max()))
        out["inputs"][kind] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
