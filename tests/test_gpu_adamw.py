"""-m gpu: rpr_adamw_step (sumsq_*_kernel + adamw_multi_kernel) against the float64 restatement of tests/adamw_ref.py, beyond
the first step: chosen gradients written straight into TrainState.grads, six consecutive calls with carried moments, then the
ABI's step 1000 and 100000 on the same moments; non-default betas, eps and weight decay, clipping on, off and marginal.

Every call is checked on its own: the reference starts from the float32 state the device left after the previous call, so
nothing accumulates. Checked per tensor: the parameters, exp_avg, exp_avg_sq; and out_grad_norm.

Units, floors and bars (adamw_ref.errors / floors / bars; the bar is 4 x the floor, computed at run time from the same inputs):

    quantity     unit                                                        float32 floor   device, worst call
    parameters   one fp32 ulp of the weight + one rounding of the update     3.64            3.46
    exp_avg      the tensor's largest entry                                  1.70e-07        1.70e-07
    exp_avg_sq   the tensor's largest entry                                  3.04e-07        3.04e-07
    grad norm    the norm                                                    5.4e-08         5.4e-08

(MI355X; the other two models: 3.46 / 1.85e-07 / 2.90e-07 / 4.7e-08 and 3.29 / 1.63e-07 / 2.53e-07 / 2.9e-08 against floors
of 3.46 / 1.85e-07 / 2.90e-07 / 4.7e-08 and 3.36 / 1.63e-07 / 2.53e-07 / 2.9e-08.) The device sits at the floor: its moments
are the host's float32 ones almost bit for bit. The floor is the float32 evaluation of the restatement against its float64
evaluation on these inputs; tests/test_adamw_host.py shows that each documented fault (a bias correction of step - 1 or
without its square root, decay on the bias tables or folded into the gradient, the clip coefficient without its 1e-6,
swapped betas) lands at least 50 bars away on them (decay on the bias tables: 57; every other one beyond 1e5).

Models (adamw_ref.model_dims): the smallest dims the loader accepts; it refused none. shared.weight (515 x 128) ends in a
partial 4096-element chunk, the norms and bias tables are smaller than one chunk; `shared_codebooks` has no slot for the
output codebooks. The kernel's scalar branch (a tensor whose offset or size is off the 4-element grid) cannot be reached
while rel_buckets x heads is a multiple of 4 — true of every T5 checkpoint — but the loader accepts 31 buckets and one head:
`odd_bias_tables` puts every tensor behind the bias tables on that branch and leaves the flat buffer 2 elements past a
multiple of 4 (the norm kernel's tail).
"""
import numpy as np
import pytest
import torch

import adamw_ref as R

pytestmark = pytest.mark.gpu

_ONE_CASE = ("decay_always_clips",)      # what the two extra models run (weight decay, clipping, all eight calls)


class _Device:
    """A model of adamw_ref.model_dims on the device, its TrainState, and the flat views the reference works on."""

    def __init__(self, variant):
        from ripor_amd import engine as E
        from ripor_amd.utils import synth
        self.E = E
        dims = R.model_dims(variant)
        self.sd = synth.make_state_dict(dims, seed=41)
        self.ctx = E.Context.get(0)
        self.model = E.DeviceModel(self.ctx, self.sd, dims)
        self.state = E.TrainState(self.model)
        self.layout = R.flat_layout(dims)
        self.decays = R.decay_mask(self.layout)
        # the header's order, restated by adamw_ref.flat_layout
        assert [(n, off) for _, n, off in self.state.layout] == [(s.numel, s.offset) for s in self.layout]
        by_ptr = {t.data_ptr(): t for _, t, _ in self.model.named_device_params()}
        self.tensors = [by_ptr[ptr] for ptr, _, _ in self.state.layout]
        assert np.array_equal(self.params(), R.pack(self.sd, self.layout))

    def params(self):
        return torch.cat([t.reshape(-1) for t in self.tensors]).cpu().numpy()

    def moments(self):
        return self.state.exp_avg.cpu().numpy(), self.state.exp_avg_sq.cpu().numpy()

    def step(self, g, step, hp, norm_out=True):
        """One rpr_adamw_step with gradients g at the ABI's `step` -> (p, m, v, norm) as the device left them."""
        E, st = self.E, self.state
        st.grads.copy_(torch.from_numpy(g))
        if norm_out:
            st.step = step - 1
            E.adamw_step(self.model, st, hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, weight_decay=hp.weight_decay,
                         max_grad_norm=hp.max_grad_norm)
        else:
            E.check(self.ctx.lib.rpr_adamw_step(self.ctx.handle, self.model.handle, st.grads.data_ptr(), st.exp_avg.data_ptr(),
                                                st.exp_avg_sq.data_ptr(), step, hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay,
                                                hp.max_grad_norm, None, E._stream_ptr(self.ctx.device)), "rpr_adamw_step")
        torch.cuda.synchronize()
        return (self.params(),) + self.moments() + (float(st.grad_norm),)


def _run_case(dev, variant, case, cases):
    layout, decays, p0, hp, grads = R.case_inputs(variant, case)
    bar = R.bars(variant, cases)
    p, (m, v) = dev.params(), dev.moments()
    assert np.array_equal(p, p0) and not m.any() and not v.any()
    worst, norms = R.Errors(0.0, 0.0, 0.0, 0.0), []
    for step, g in grads:
        ref = R.adamw_step(p, g, m, v, decays, step, hp)
        got = dev.step(g, step, hp)
        e = R.errors(got, ref, layout)
        print(f"[adamw] {variant} {case} step {step}: norm {float(ref.norm):.4g}, errors {tuple(f'{x:.3g}' for x in e)} "
              f"(bars {tuple(f'{x:.3g}' for x in bar)})")
        worst = R.Errors(*(max(a, b) for a, b in zip(worst, e)))
        norms.append(float(ref.norm))
        for name, x, b in zip(R.Errors._fields, e, bar):
            assert x <= b, (variant, case, step, name, x, b)
        assert not np.array_equal(got[0], p), "the parameters did not move"
        p, m, v = got[0], got[1], got[2]
    print(f"[adamw] {variant} {case}: worst {tuple(f'{x:.3g}' for x in worst)}")
    return norms


@pytest.mark.parametrize("case", list(R.CASES))
def test_adamw_step_matches_the_float64_restatement(case):
    """The four hyperparameter sets on the model with its own output codebooks (module docstring for units and bars)."""
    norms = _run_case(_Device("own_codebooks"), "own_codebooks", case, tuple(R.CASES))
    if case == "defaults":       # max_grad_norm 1: calls that clip, calls that do not, and the all-zero call
        assert max(norms) > 100.0 and 0.0 < sorted(norms)[1] < 0.1 and min(norms) == 0.0
    if case == "small_norm":
        assert all(abs(n - 1e-5) < 1e-8 for n in norms)


@pytest.mark.parametrize("variant", ["shared_codebooks", "odd_bias_tables"])
def test_adamw_step_on_the_other_tensor_tables(variant):
    """No slot for the output codebooks; and the scalar branch of adamw_multi_kernel with the norm kernel's tail (module
    docstring). Weight decay, clipping, all eight calls."""
    dev = _Device(variant)
    if variant == "shared_codebooks":
        assert "out_emb" not in [s.name for s in dev.layout] and dev.model.out_embeds is dev.model.in_embeds
    else:
        assert dev.state.total % 4 == 2 and sum((s.offset | s.numel) % 4 != 0 for s in dev.layout) == len(dev.layout) - 1
    _run_case(dev, variant, _ONE_CASE[0], _ONE_CASE)


def test_adamw_step_without_a_norm_output():
    """out_grad_norm == NULL through the C ABI: the same update, and nothing written where the norm would go."""
    variant, case = "own_codebooks", "decay_always_clips"
    dev = _Device(variant)
    layout, decays, p0, hp, grads = R.case_inputs(variant, case)
    bar = R.bars(variant, tuple(R.CASES))
    dev.state.grad_norm.fill_(-7.0)
    z = np.zeros_like(p0)
    step, g = grads[0]
    ref = R.adamw_step(p0, g, z, z, decays, step, hp)
    got = dev.step(g, step, hp, norm_out=False)
    assert got[3] == -7.0
    e = R.errors(got[:3] + (float(ref.norm),), ref, layout)
    assert e.param <= bar.param and e.exp_avg <= bar.exp_avg and e.exp_avg_sq <= bar.exp_avg_sq, e


def test_grad_norm_squares_in_double():
    """Entries of 1e-25 (float32 squares underflow to 0) and of 1e18 (a float32 sum of their squares overflows; the norm, 5e20, fits): the
    norm within the norm bar of the float64 one. And the n % 4 trailing elements of the odd model's buffer, alone: 3, 4 -> 5."""
    from ripor_amd.utils import synth
    hp = R.CASES["defaults"][0]
    bar = R.bars("own_codebooks", tuple(R.CASES))
    for scale in (1e-25, 1e18):
        dev = _Device("own_codebooks")
        g = (synth.uniform_f32(f"adamw/norm/{scale}", (dev.state.total,), 1.0).astype(np.float64) * scale).astype(np.float32)
        want = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        assert 0.2 * scale * dev.state.total ** 0.5 < want < np.finfo(np.float32).max
        with np.errstate(over="ignore", under="ignore"):                # what float32 squares would have made of it
            sq = g * g
            assert (not sq.any()) if scale < 1 else np.isinf(np.sum(sq, dtype=np.float32))
        p, m, v, norm = dev.step(g, 1, hp)
        print(f"[adamw] norm of entries ~{scale:g}: {norm:.9g} vs {want:.9g}")
        assert abs(norm - want) <= bar.norm * want, (scale, norm, want)
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
    dev = _Device("odd_bias_tables")
    g = np.zeros(dev.state.total, dtype=np.float32)
    g[-2:] = (3.0, 4.0)
    assert dev.step(g, 1, hp)[3] == 5.0


@pytest.mark.parametrize("variant", ["own_codebooks", "odd_bias_tables"])
def test_weight_decay_exempts_exactly_the_two_bias_tables(variant):
    """All-zero gradients from all-zero moments with weight decay: the update term is exactly 0, so the two
    relative-attention-bias tables come back bit for bit and every other tensor — the T5 layer-norm weights included, as the
    header documents — is float32(p) * (1.f - lr * wd) in float32. lr = 2^-7 and wd = 2^-3: their product is exact, so the
    factor is the same float whether or not the device contracts 1.f - lr * wd into one fused multiply-add."""
    dev = _Device(variant)
    hp = R.Hyper(2.0 ** -7, 0.9, 0.999, 1e-8, 2.0 ** -3, 1.0)
    p0 = dev.params()
    p, m, v, norm = dev.step(np.zeros(dev.state.total, dtype=np.float32), 1, hp)
    assert norm == 0.0 and not m.any() and not v.any()
    factor = np.float32(1) - np.float32(hp.lr) * np.float32(hp.weight_decay)
    exempt = []
    for s in dev.layout:
        a, b = p[s.offset:s.offset + s.numel], p0[s.offset:s.offset + s.numel]
        if s.decay:
            assert np.array_equal(a, b * factor), s.name
            assert not np.array_equal(a, b), s.name
        else:
            assert np.array_equal(a, b), s.name
            exempt.append(s.name)
    assert exempt == ["enc_rel", "dec_rel"]
    assert any("ln" in s.name and s.decay for s in dev.layout)
