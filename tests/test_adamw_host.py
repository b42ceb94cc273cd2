"""CPU: tests/adamw_ref.py, the float64 restatement tests/test_gpu_adamw.py holds rpr_adamw_step against.

1. The restatement IS clip_grad_norm_ + torch.optim.AdamW: six carried steps in float64, three hyperparameter sets, the bias
   tables in a param group without weight decay. Both sides are a handful of float64 roundings per element in different
   orders, plus the order in which the 722 816 squares of the norm are added (torch adds per-tensor norms; a random walk of
   sqrt(n) 2^-53 = 1e-13, which the clip coefficient carries into every moment): the norm and each moment within 1e-12 (of
   the tensor's largest entry), the parameters within 16 float64 ulps of the weight + 1e-12 lr. Measured: under 1e-12 lr.
2. The GPU test has power: each documented fault of FAULTS, evaluated in float64 on the inputs the GPU test uses, lands
   beyond the GPU test's bar (4 x the float32 floor) in at least one checked quantity of at least one call.
"""
import numpy as np
import pytest
import torch

import adamw_ref as R


def _torch_steps(layout, p0, hp, grads):
    ps = [torch.from_numpy(p0[s.offset:s.offset + s.numel].astype(np.float64)).requires_grad_() for s in layout]
    lr, b1, b2, eps, wd, mx = (float(np.float32(x)) for x in hp)
    opt = torch.optim.AdamW([dict(params=[p for p, s in zip(ps, layout) if s.decay], weight_decay=wd),
                             dict(params=[p for p, s in zip(ps, layout) if not s.decay], weight_decay=0.0)],
                            lr=lr, betas=(b1, b2), eps=eps)
    for step, g in grads:
        for p, s in zip(ps, layout):
            p.grad = torch.from_numpy(g[s.offset:s.offset + s.numel].astype(np.float64))
        norm = float(torch.nn.utils.clip_grad_norm_(ps, mx)) if mx > 0 else None
        opt.step()
        cat = lambda f: np.concatenate([f(p).numpy() for p in ps])
        yield (cat(lambda p: p.detach()), cat(lambda p: opt.state[p]["exp_avg"]), cat(lambda p: opt.state[p]["exp_avg_sq"]), norm)


@pytest.mark.parametrize("case", ["defaults", "decay_no_clip", "decay_always_clips"])
def test_restatement_is_torch_adamw_with_clip_grad_norm(case):
    layout, decays, p0, hp, grads = R.case_inputs("own_codebooks", case)
    grads = grads[:6]
    assert [s for s, _ in grads] == [1, 2, 3, 4, 5, 6]
    assert [s.name for s in layout if not s.decay] == ["enc_rel", "dec_rel"]
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    starts = [s.offset for s in layout]
    worst = 0.0
    for (step, g), (tp, tm, tv, tnorm) in zip(grads, _torch_steps(layout, p0, hp, grads)):
        p, m, v, norm, _ = R.adamw_step(p, g, m, v, decays, step, hp)
        if tnorm is not None:
            assert abs(float(norm) - tnorm) <= 1e-12 * tnorm
        err = np.abs(p - tp)
        worst = max(worst, float(err.max()))
        assert (err <= 16 * np.spacing(np.abs(tp)) + 1e-12 * float(hp.lr)).all(), (case, step, float(err.max()))
        for a, b in ((m, tm), (v, tv)):
            top = np.maximum.reduceat(np.abs(b), starts)
            assert (np.maximum.reduceat(np.abs(a - b), starts) <= 1e-12 * top).all(), (case, step)
    print(f"[adamw-ref] {case}: worst parameter distance from torch.optim.AdamW over six steps {worst / float(hp.lr):.1e} lr")


def test_float32_floors_are_the_recorded_ones():
    """The floors the GPU test's docstring records (its bars are 4 x what this computes at run time): a drift of the inputs
    or of the restatement shows here, without a GPU."""
    f = R.floors()
    print(f"[adamw-ref] float32 floors: {f}")
    assert 1.0 <= f.param <= 5.0          # ulp of the weight + rounding of the update
    assert 5e-8 <= f.exp_avg <= 4e-7 and 5e-8 <= f.exp_avg_sq <= 4e-7
    assert f.norm <= 2.0 ** -24           # one rounding of a double to float


# the cases a fault can show in (a fault of the decay needs weight_decay > 0, the clip fault its own case)
_WHERE = {"bc2_without_sqrt": ["defaults"], "bc_of_step_minus_1": ["defaults"], "betas_swapped": ["defaults"],
          "decay_on_bias_tables": ["decay_no_clip", "decay_always_clips"], "coupled_l2": ["decay_no_clip", "decay_always_clips"],
          "clip_without_1e-6": ["small_norm"]}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_documented_fault_exceeds_the_gpu_bars(fault):
    bar = R.bars()
    over = {}

    def visit(k, step, p, g, m, v, decays, hp, layout, ref, got):
        if fault == "bc_of_step_minus_1" and step == 1:
            return                      # 1 - beta^0 = 0: the faulty update is infinite there, which proves nothing
        bad = R.adamw_step(p, g, m, v, decays, step, hp, fault=fault)
        e = R.errors(bad[:4], ref, layout)
        over[(case, step)] = max(x / b for x, b in zip(e, bar) if b > 0)

    for case in _WHERE[fault]:
        R.walk("own_codebooks", case, visit)
    best = max(over, key=over.get)
    print(f"[adamw-ref] {fault}: {over[best]:.3g} x the bar at {best}; calls beyond the bar: {sum(v > 1 for v in over.values())} of {len(over)}")
    assert over[best] > 1.0, (fault, over)
    if fault == "clip_without_1e-6":
        # the case built for it: the coefficient moves by about 10 %
        _, _, _, hp, grads = R.case_inputs("own_codebooks", "small_norm")
        n = float(np.sqrt(np.sum(grads[0][1].astype(np.float64) ** 2)))
        c, c_bad = hp.max_grad_norm / (n + 1e-6), hp.max_grad_norm / n
        assert abs(n - 1e-5) < 1e-8 and 0.08 < (c_bad - c) / c < 0.12
