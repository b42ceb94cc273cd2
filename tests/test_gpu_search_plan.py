"""-m gpu: the graph cache tells every search plan apart (ripor_amd/csrc/search_plan.h: SearchPlan is the graph key).

One ctx, one model, one trie, one batch; the settings that change what a search enqueues are visited in turn, twice: on
the second round every setting finds the cache filled by all the others, and a plan that compared equal to another one
would replay that one's graph. Every visit is compared with an eager run (no graph) under the same settings, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, B, L, V, N, SEED = 6, 4, 8, 256, 3000, 5
DEFAULT = dict(forced_tail=1, forks=None, extras=-1, precision="f16x2", lane_split=None, margins=False, log_softmax=False)
SETTINGS = [
    ("default", {}),
    ("no forced tail", dict(forced_tail=0)),
    ("fork [3], no extras", dict(forks=[3], extras=0)),
    ("fork [3], extras 2", dict(forks=[3], extras=2)),
    ("fork [3], extras 2, optimistic", dict(forks=[3], extras=2, forced_tail=2)),
    ("margins", dict(margins=True)),
    ("exact fp32", dict(precision="f32")),
    ("two lanes", dict(lane_split=8)),          # 24 decoder rows >= 8: the six queries run as 3 + 3
    ("log-softmax", dict(log_softmax=True)),
]


def _apply(ctx, s, saved_split):
    ctx.set_forced_tail(s["forced_tail"])
    ctx.set_fork_depths(s["forks"])
    ctx.set_tail_extras(s["extras"])
    if ctx.get_precision() != s["precision"]:     # (a switch makes the layer-0 table again: only when it is one)
        ctx.set_precision(s["precision"])
    ctx.set_lane_split(saved_split if s["lane_split"] is None else s["lane_split"])


def test_graph_cache_distinguishes_every_plan():
    from ripor_amd import engine as E
    from ripor_amd.utils import synth
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128)
    sd = synth.make_state_dict(dims, seed=SEED)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=SEED, max_len=12)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, sd, dims)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(N, L, V, seed=SEED), V)
    saved_split = ctx.lane_split() or 10240
    saved = dict(DEFAULT, forced_tail=ctx.forced_tail(), extras=ctx.tail_extras(), precision=ctx.get_precision())

    def run(s, use_graph):
        ctx.status(clear=True)
        r = E.search(model, trie, ti, tm, B, L, apply_log_softmax_for_scores=s["log_softmax"], use_graph=use_graph, margins=s["margins"])
        torch.cuda.synchronize()
        return r, ctx.last_fork_stats(), ctx.status(clear=True)

    try:
        for visit in (1, 2):
            for name, change in SETTINGS:
                s = dict(DEFAULT, **change)
                _apply(ctx, s, saved_split)
                label = f"{name}, visit {visit}"
                got, got_forks, got_status = run(s, True)
                ref, ref_forks, ref_status = run(s, False)
                print(f"[search plan] {label}: forks {got_forks}, status {got_status}")
                assert torch.equal(got.tokens, ref.tokens) and torch.equal(got.scores, ref.scores), label
                assert torch.equal(got.row_lo, ref.row_lo) and torch.equal(got.row_hi, ref.row_hi), label
                if s["margins"]:
                    assert torch.equal(got.margins, ref.margins), label
                assert got_forks == ref_forks and got_status == ref_status, (label, got_forks, ref_forks, got_status, ref_status)
    finally:
        _apply(ctx, saved, saved_split)
