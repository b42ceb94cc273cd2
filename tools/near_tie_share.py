#!/usr/bin/env python3
"""How many queries sit on a pruning near-tie, and what the near-tie guard buys (GPU diagnostic;
`python tools/near_tie_share.py [queries_per_beam] [seed]`). Mini-dims models over synthetic tries (the shapes of
tools/fuzz_parity.py), beams 10, 100 and 1000, at least 200 queries each. Per beam count:

  * the share of queries whose split-precision pruning margin (rpr_search_margins) is below 1e-3;
  * the share whose f16x2 smtid SET differs from the exact-fp32 search of the same queries;
  * the share of those differences the guard catches (margin below the threshold, so the query would be re-run in fp32).

Prints one line per beam count and a JSON summary line."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripor_amd import engine as E
from ripor_amd.utils import synth

EPS = 1e-3
n_queries = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1234
ctx = E.Context.get(0)
L, V, N = 8, 256, 300_000
dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=seed), dims)
trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(N, L, V, seed=seed), V)
ids, mask = synth.make_queries(n_queries, vocab_size=dims.vocab_size, seed=seed, max_len=14)
ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)


def sets(tokens):
    t = tokens.cpu().numpy()
    return [{tuple(int(x) for x in row) for row in q} for q in t]


out = {"queries_per_beam": n_queries, "threshold": EPS, "docs": N, "L": L, "V": V, "beams": {}}
for B in (10, 100, 1000):
    step = {10: 200, 100: 50, 1000: 10}[B]
    margins, differ = [], []
    for q0 in range(0, n_queries, step):
        a, m = ids[q0:q0 + step], mask[q0:q0 + step]
        ctx.set_precision("f16x2")
        h = E.search(model, trie, a, m, B, L, margins=True)
        torch.cuda.synchronize()
        ctx.set_precision("f32")
        try:
            f = E.search(model, trie, a, m, B, L)
            torch.cuda.synchronize()
        finally:
            ctx.set_precision("f16x2")
        margins += h.margins.cpu().tolist()
        differ += [x != y for x, y in zip(sets(h.tokens), sets(f.tokens))]
    margins, differ = np.array(margins), np.array(differ)
    near = margins < EPS
    rec = {"near_tie_share": float(near.mean()), "set_differs_share": float(differ.mean()), "set_differs": int(differ.sum()),
           "caught_by_guard": int((differ & near).sum()),
           "caught_share": float((differ & near).sum() / differ.sum()) if differ.any() else None,
           "finite_margins": int(np.isfinite(margins).sum()), "median_margin": float(np.median(margins[np.isfinite(margins)])) if np.isfinite(margins).any() else None}
    out["beams"][str(B)] = rec
    print(f"beam {B:4d}: margin < {EPS:g} for {100 * rec['near_tie_share']:.1f} % of {n_queries} queries; f16x2 set != f32 set for "
          f"{rec['set_differs']} ({100 * rec['set_differs_share']:.1f} %), {rec['caught_by_guard']} of them under the threshold", flush=True)
assert ctx.status(clear=True) & 1 == 0, "saturation flag"
print(json.dumps(out))
