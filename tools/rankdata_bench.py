#!/usr/bin/env python3
"""The rank-data pass's beam-search time, two ways (t5-base dims, the bench's 8.8 M-doc trie, beam 100; the reference script's
flags: 4 queries per search, and the batch evaluate.search_batch_size forms from them):

  separate   three searches, max_new_token 4, 8 and 16 — what full_evaluate_t5seq_aq_encoder.sh:117-147 runs
  one        one search of 16 tokens that also reports its beams at 4 and 8 (E.search(..., prefix_lengths=(4, 8)))

Same ctx settings (optimistic forced tail, as search_guarded runs it), same seeded queries and warm graphs for both; a
measurement is the median of --repeats timed repeats, and --rounds such measurements show the run-to-run spread
((max - min) / median). Also printed: per prefix length, how the one search's beams agree with the separate search's by the
test suite's rule (tests/test_gpu_prefix_depths.py: tokens equal or scores within 2e-4 at every live rank, max score
difference <= 3e-5, ranges equal where the tokens are).

--lib PATH loads another build of the library (the parent's, for the A/B); one without rpr_search_prefixes measures the
separate searches only; --forms picks the forms of this process. One JSON line on stdout; --out FILE appends it there too.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCORE_TOL, ORDER_TOL = 1e-4, 2e-4
LENGTHS, DEPTHS, L, B = (4, 8, 16), (4, 8), 16, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libripor_hip.so (default: the tree's)")
    ap.add_argument("--docs", type=int, default=8_841_823)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="4,auto", help="queries per search: numbers, 'auto' = evaluate.search_batch_size(--batch_size=4)")
    ap.add_argument("--forms", default="separate,one",
                    help="which forms this process measures. A batch large enough for the lane split keeps two lane workspaces "
                         "for the separate searches and a third, unsplit one for the search with prefix lengths: at the "
                         "HBM-filling 'auto' batch measure the two forms in two processes")
    ap.add_argument("--forced-tail", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from ripor_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        import ctypes
        probe = ctypes.CDLL(_lib.LIB_PATH)
        if not hasattr(probe, "rpr_search_prefixes"):
            del _lib.SIGNATURES["rpr_search_prefixes"]
    has_prefixes = "rpr_search_prefixes" in _lib.SIGNATURES
    from ripor_amd import engine as E
    from ripor_amd import evaluate
    from ripor_amd.utils import synth

    dev = torch.device("cuda", 0)
    dims = synth.t5_base_dims(L=L)
    V = dims.decoder_vocab_sizes[0]
    ctx = E.Context.get(0)
    ctx.set_forced_tail(args.forced_tail)
    model = E.DeviceModel(ctx, synth.make_state_dict(dims), dims)
    t0 = time.time()
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes_fast(args.docs, L, V), V)
    print(f"[rankdata_bench] trie of {trie.N:,} docs in {time.time() - t0:.1f}s; library {_lib.LIB_PATH}", file=sys.stderr)

    def batches_of(Q, n=2, seed=707):
        ids, mask = synth.make_queries(Q * n, vocab_size=dims.vocab_size, seed=seed)
        lq = (int(mask.sum(1).max()) + 7) // 8 * 8
        ids = np.pad(ids, ((0, 0), (0, max(0, lq - ids.shape[1]))))[:, :lq]
        mask = np.pad(mask, ((0, 0), (0, max(0, lq - mask.shape[1]))))[:, :lq]
        return [(torch.from_numpy(ids[i * Q:(i + 1) * Q]).to(dev, torch.int32), torch.from_numpy(mask[i * Q:(i + 1) * Q]).to(dev, torch.int32))
                for i in range(n)]

    def separate(b):
        return {p: E.search(model, trie, b[0], b[1], B, p) for p in LENGTHS}

    def one(b):
        r = E.search(model, trie, b[0], b[1], B, L, prefix_lengths=DEPTHS)
        out = dict(r.prefixes)
        out[L] = r
        return out

    def measure(fn, batches):
        """median over the timed repeats of one call of fn (ms); the graphs are warm"""
        ts = []
        for i in range(args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(batches[i % len(batches)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts)

    def agreement(got, ref):
        same = (got.tokens == ref.tokens).all(dim=2)
        live = ref.scores > -1e6
        close = (got.scores - ref.scores).abs() <= ORDER_TOL
        err = float(((got.scores - ref.scores).abs() * live).max())
        both = same & live
        ranges = bool(torch.equal(got.row_lo[both], ref.row_lo[both]) and torch.equal(got.row_hi[both], ref.row_hi[both]))
        return {"live_ranks": int(live.sum()), "identical_ranks": int(both.sum()), "max_score_diff": err,
                "passes_rule": bool((same | close | ~live).all()) and err <= 0.3 * SCORE_TOL and ranges}

    out = {"tool": "rankdata_bench", "library": os.path.basename(_lib.LIB_PATH), "has_prefixes": has_prefixes, "docs": int(trie.N),
           "beams": B, "lengths": list(LENGTHS), "depths": list(DEPTHS), "forced_tail": args.forced_tail, "repeats": args.repeats,
           "rounds": args.rounds, "batches": {}}
    for spec in args.batches.split(","):
        Q = evaluate.search_batch_size(dims, 4, B, L, -1, 0) if spec == "auto" else int(spec)
        batches = batches_of(Q)
        forms = [(n, f) for n, f in (("separate", separate), ("one", one))
                 if n in args.forms.split(",") and (n != "one" or has_prefixes)]
        rec = {"queries_per_search": Q}
        ctx.status(clear=True)
        for name, fn in forms:
            for b in batches:        # warm: workspace, graphs of every length, the layer-0 table
                fn(b)
                fn(b)
            torch.cuda.synchronize()
        for name, fn in forms:
            rounds = [measure(fn, batches) for _ in range(args.rounds)]
            med = statistics.median(rounds)
            rec[name] = {"ms": med, "ms_per_query": med / Q, "rounds_ms": rounds, "spread": (max(rounds) - min(rounds)) / med}
        rec["leftover_flag"] = bool(ctx.status(clear=True) & E._lib.STATUS_TAIL_LEFTOVER)   # optimistic mode: a flagged call's outputs are void
        rec["forks_last_search"] = ctx.last_fork_stats()
        if len(forms) == 2:
            rec["speedup"] = rec["separate"]["ms"] / rec["one"]["ms"]
            ctx.set_forced_tail(min(args.forced_tail, 1))   # (the exact mode: an optimistic call that raised the flag has void outputs)
            try:
                sep, got = separate(batches[0]), one(batches[0])
                torch.cuda.synchronize()
            finally:
                ctx.set_forced_tail(args.forced_tail)
            rec["agreement"] = {str(p): agreement(got[p], sep[p]) for p in LENGTHS}
        out["batches"][spec] = rec
        print(f"[rankdata_bench] {spec}: {json.dumps(rec)}", file=sys.stderr)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
