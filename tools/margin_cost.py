#!/usr/bin/env python3
"""Cost of margin mode (GPU diagnostic; `python tools/margin_cost.py [docs]`): the same search with and without the pruning
margins (rpr_search_margins vs rpr_search), t5-base dims on a synthetic trie, at the headline shape (beam 10, length 32, 2150
queries: two lanes) and at beam 1000 with one query. hipGraph replays, alternating, median of the repeats; one JSON line."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripor_amd import engine as E
from ripor_amd.utils import synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
ctx = E.Context.get(0)
L, V = 32, 256
dims = synth.t5_base_dims(L=L, V=V)
model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=5), dims)
trie = E.DeviceTrie.from_codes(ctx, synth.make_codes_fast(N, L, V, seed=5), V)
out = {"docs": N, "model": "t5-base dims", "L": L}
for name, Q, B, reps in (("headline_q2150_b10", 2150, 10, 5), ("q1_b1000", 1, 1000, 9)):
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=6)
    ids, mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    ms = {False: [], True: []}
    for rep in range(reps + 1):                 # the first round captures the graphs
        for mg in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            E.search(model, trie, ids, mask, B, L, margins=mg)
            b.record()
            torch.cuda.synchronize()
            if rep:
                ms[mg].append(a.elapsed_time(b))
    plain, marg = float(np.median(ms[False])), float(np.median(ms[True]))
    out[name] = {"search_ms": round(plain, 3), "search_margins_ms": round(marg, 3), "extra_ms": round(marg - plain, 3),
                 "extra_pct": round(100 * (marg - plain) / plain, 2),
                 "spread_ms": [round(min(ms[False]), 3), round(max(ms[False]), 3)], "forks": ctx.fork_depths(model, trie, Q, B, L)}
    print(name, out[name], flush=True)
print(json.dumps(out))
