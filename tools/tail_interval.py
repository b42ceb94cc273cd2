#!/usr/bin/env python3
"""Per lane and step of a rocprofv3 --kernel-trace rocpd database of bench.py: time and launches between the end of the
first tail pass's tail_rank_kernel and the end of the step's last kernel (what a search enqueues behind its first fork: the
leftover stage, its fork and tail pass), with the kernels of that interval. A search starts with mask_lengths_kernel; the
lanes are told apart by their stream. Usage: tail_interval.py results.db out.json [last_step_kernels.csv]"""
import csv
import json
import sqlite3
import sys
from collections import defaultdict

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
cols = [d[0] for d in cur.execute("select * from kernels limit 1").description]
print("columns:", cols)
scol = "start" if "start" in cols else "start_time"
idcols = [c for c in ("stream_id", "queue_id", "stream", "queue", "tid") if c in cols]
rows = list(cur.execute(f"select name, {scol}, duration, {', '.join(idcols)} from kernels order by {scol}"))


def short(n):
    return n.replace("(anonymous namespace)::", "").split("(")[0].replace("rpr::", "")


# the lane column: the one whose values split the gemm_h2_pp launches into two large groups
lane_col = None
for k, c in enumerate(idcols):
    cnt = defaultdict(int)
    for r in rows:
        if "gemm_h2_pp" in r[0]:
            cnt[r[3 + k]] += 1
    print("id column", c, dict(cnt))
    if lane_col is None and len(cnt) >= 2:
        lane_col = k
        lanes = sorted(cnt, key=lambda v: -cnt[v])[:2]
if lane_col is None:
    raise SystemExit("no column separates the lanes")
print("lane column:", idcols[lane_col], "lanes:", lanes)

out = {"lane_column": idcols[lane_col], "steps": []}
dump = []
for li, lane in enumerate(lanes):
    mine = [(short(r[0]), r[1], r[2]) for r in rows if r[3 + lane_col] == lane]
    # a search starts with mask_lengths_kernel
    starts = [i for i, r in enumerate(mine) if r[0].startswith("mask_lengths_kernel")] + [len(mine)]
    for si in range(len(starts) - 1):
        seg = mine[starts[si]:starts[si + 1]]
        t0 = seg[0][1]
        t_end = max(s + d for _, s, d in seg)
        ranks = [i for i, r in enumerate(seg) if r[0].startswith("tail_rank_kernel")]
        rec = {"lane": li, "step": si, "launches": len(seg), "step_ms": (t_end - t0) / 1e6, "tail_rank_launches": len(ranks)}
        if ranks:
            i0 = ranks[0]
            e0 = seg[i0][1] + seg[i0][2]
            after = seg[i0 + 1:]
            rec["after_first_tail_rank_ms"] = (t_end - e0) / 1e6
            rec["after_first_tail_rank_launches"] = len(after)
            rec["after_kernel_time_ms"] = sum(d for _, _, d in after) / 1e6
            rec["after_share_of_step"] = (t_end - e0) / (t_end - t0)
            agg = defaultdict(lambda: [0, 0.0])
            for n, _, d in after:
                agg[n][0] += 1
                agg[n][1] += d
            rec["after_by_kernel"] = {n: {"calls": c, "total_us": t / 1e3} for n, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:12]}
        out["steps"].append(rec)
        print({k: v for k, v in rec.items() if k != "after_by_kernel"})
        if si == len(starts) - 2:
            dump += [(li, n, s - t0, d) for n, s, d in seg]
json.dump(out, open(sys.argv[2], "w"), indent=1)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["lane", "kernel", "start_ns_in_step", "duration_ns"])
        w.writerows(dump)
