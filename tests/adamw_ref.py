"""float64 restatement of rpr_adamw_step as include/ripor_hip.h documents it, for tests/test_adamw_host.py (pinned to
torch.optim.AdamW + clip_grad_norm_ there) and tests/test_gpu_adamw.py (the device optimizer against it):

    norm = sqrt(sum g^2) over the flat buffer            clip = min(1, max_grad_norm / (norm + 1e-6)), 1 when max_grad_norm <= 0
    g' = clip g      m = b1 m + (1 - b1) g'      v = b2 v + (1 - b2) g'^2
    p *= 1 - lr wd   (every tensor except the two relative-attention-bias tables)
    p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Everything works on the flat layout of rpr_param_info (flat_layout restates the header's order from the model's dims, so
the host test needs no device). The hyperparameters are rounded to float32 first, as the C ABI receives them; states and
gradients are taken as given. ``dtype=np.float32`` evaluates the same formulas in float32 — with the norm and the clip
coefficient summed and divided in double and rounded once, which is what the norm kernel does: the distance between the two
evaluations is the floor the device tolerances are multiples of (floors()).

The cases (CASES), their gradients (make_grads) and the error measures (errors) live here so that the host test can show,
without a GPU, that each documented fault (FAULTS) exceeds the GPU test's bars on the very inputs the GPU test uses.
"""
import functools
from collections import namedtuple

import numpy as np

from ripor_amd.utils import synth

Slot = namedtuple("Slot", "name parts numel offset decay")
Hyper = namedtuple("Hyper", "lr beta1 beta2 eps weight_decay max_grad_norm")
Step = namedtuple("Step", "p m v norm unit")
Errors = namedtuple("Errors", "param exp_avg exp_avg_sq norm")

FAULTS = ("bc2_without_sqrt", "bc_of_step_minus_1", "decay_on_bias_tables", "coupled_l2", "clip_without_1e-6", "betas_swapped")


# ---- models and the flat layout ---------------------------------------------------------------------------------------------
def model_dims(variant):
    """The smallest dims rpr_load_model accepts (d_kv must be 64, d_model and d_ff multiples of 32; nothing was refused):
    d_model 128, 2 heads of 64, d_ff 256, 1 + 2 layers, L 8, V 64, vocab 515 — shared.weight has 16 chunks of 4096 elements
    and a partial one of 384, the layer norms, bias tables and start embedding are smaller than one chunk.
      own_codebooks     the default
      shared_codebooks  shared_output_input_embeds: no slot for the output codebooks
      odd_bias_tables   1 head and 31 relative-attention buckets: the bias tables have 31 elements each, so every tensor
                        behind them starts off the 4-element grid (the kernel's scalar branch) and the flat buffer's length
                        is no multiple of 4 (the norm kernel's tail)"""
    kw = dict(vocab_size=515, d_model=128, d_kv=64, d_ff=256, num_layers=1, num_decoder_layers=2, num_heads=2,
              decoder_vocab_sizes=[64] * 8)
    if variant == "shared_codebooks":
        kw["shared_output_input_embeds"] = True
    elif variant == "odd_bias_tables":
        kw.update(num_heads=1, relative_attention_num_buckets=31)
    else:
        assert variant == "own_codebooks", variant
    return synth.ModelDims(**kw)


def flat_layout(dims):
    """The tensors of the flat buffers in the header's order: (name, checkpoint tensors concatenated in it, numel, offset,
    decays?)."""
    out, off = [], 0

    def add(name, parts, numel, decay=True):
        nonlocal off
        out.append(Slot(name, tuple(parts), int(numel), off, decay))
        off += int(numel)

    dm, inner, dff, L = dims.d_model, dims.inner, dims.d_ff, len(dims.decoder_vocab_sizes)
    V = int(dims.decoder_vocab_sizes[0])
    rel = dims.relative_attention_num_buckets * dims.num_heads
    add("shared", ["shared.weight"], dims.vocab_size * dm)
    add("enc_rel", ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], rel, decay=False)
    add("dec_rel", ["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], rel, decay=False)
    add("enc_fln", ["encoder.final_layer_norm.weight"], dm)
    add("dec_fln", ["decoder.final_layer_norm.weight"], dm)
    add("start", ["start_token_embed"], dm)
    add("in_emb", [f"list_decoder_embeds.{i}.weight" for i in range(L)], L * V * dm)
    if not dims.shared_output_input_embeds:
        add("out_emb", [f"list_output_embeds.{i}.weight" for i in range(L)], L * V * dm)
    add("xkv", [f"decoder.block.{i}.layer.1.EncDecAttention.{w}.weight" for i in range(dims.num_decoder_layers) for w in "kv"],
        dims.num_decoder_layers * 2 * inner * dm)
    for i in range(dims.num_layers):
        p = f"encoder.block.{i}.layer"
        add(f"enc{i}.ln0", [p + ".0.layer_norm.weight"], dm)
        add(f"enc{i}.qkv", [p + f".0.SelfAttention.{w}.weight" for w in "qkv"], 3 * inner * dm)
        add(f"enc{i}.o", [p + ".0.SelfAttention.o.weight"], dm * inner)
        add(f"enc{i}.ln1", [p + ".1.layer_norm.weight"], dm)
        add(f"enc{i}.wi", [p + ".1.DenseReluDense.wi.weight"], dff * dm)
        add(f"enc{i}.wo", [p + ".1.DenseReluDense.wo.weight"], dm * dff)
    for i in range(dims.num_decoder_layers):
        p = f"decoder.block.{i}.layer"
        add(f"dec{i}.ln0", [p + ".0.layer_norm.weight"], dm)
        add(f"dec{i}.qkv", [p + f".0.SelfAttention.{w}.weight" for w in "qkv"], 3 * inner * dm)
        add(f"dec{i}.o", [p + ".0.SelfAttention.o.weight"], dm * inner)
        add(f"dec{i}.ln1", [p + ".1.layer_norm.weight"], dm)
        add(f"dec{i}.xq", [p + ".1.EncDecAttention.q.weight"], inner * dm)
        add(f"dec{i}.xo", [p + ".1.EncDecAttention.o.weight"], dm * inner)
        add(f"dec{i}.ln2", [p + ".2.layer_norm.weight"], dm)
        add(f"dec{i}.wi", [p + ".2.DenseReluDense.wi.weight"], dff * dm)
        add(f"dec{i}.wo", [p + ".2.DenseReluDense.wo.weight"], dm * dff)
    return out


def pack(state_dict, layout):
    """The model's float32 weights as one flat vector in the layout's order."""
    flat = np.concatenate([np.asarray(state_dict[n], dtype=np.float32).reshape(-1) for s in layout for n in s.parts])
    assert flat.size == layout[-1].offset + layout[-1].numel
    return flat


def decay_mask(layout):
    return np.concatenate([np.full(s.numel, 1.0 if s.decay else 0.0) for s in layout])


# ---- the update -------------------------------------------------------------------------------------------------------------
def adamw_step(p, g, m, v, decays, step, hp, dtype=np.float64, fault=None):
    """One rpr_adamw_step over flat vectors. ``decays``: 1.0 where weight decay applies, 0.0 on the bias tables. ``fault``:
    one of FAULTS, a deliberately wrong optimizer (the host test measures what the GPU test would make of it). Returns
    Step(p, m, v, norm, unit) in ``dtype``; unit (float64) is what a parameter error is measured in: one float32 ulp of the
    weight plus one float32 rounding (2^-24) of the update, the update taken without cancellation inside exp_avg."""
    T = np.dtype(dtype).type
    lr, b1, b2, eps, wd, mx = (np.float32(x) for x in hp)          # the C ABI takes floats
    if fault == "betas_swapped":
        b1, b2 = b2, b1
    g64 = np.asarray(g, dtype=np.float64)
    norm = np.sqrt(np.sum(g64 * g64))
    clip = 1.0
    if mx > 0:
        with np.errstate(divide="ignore"):
            clip = min(1.0, float(np.float64(mx) / (norm + (0.0 if fault == "clip_without_1e-6" else 1e-6))))
    norm, clip = T(norm), T(clip)
    lr, b1, b2, eps, wd, one = T(lr), T(b1), T(b2), T(eps), T(wd), T(1)
    # the two bias corrections are scalars the entry point computes on the host, in double from the float betas, and hands
    # to the kernel as floats: 1.0f - (float)pow(b1, t) and (float)sqrt(1.0 - pow(b2, t)). (Taking 1 - b2^t in float32 instead
    # would lose 3e-5 of it at t = 2: not a rounding of the update, and not what the floor is meant to measure.)
    t = float(step - 1 if fault == "bc_of_step_minus_1" else step)
    bc1 = one - T(np.power(np.float64(b1), t))
    bc2 = 1.0 - np.power(np.float64(b2), t)
    bc2s = T(bc2 if fault == "bc2_without_sqrt" else np.sqrt(bc2))
    pT, m, v = np.asarray(p, dtype=T), np.asarray(m, dtype=T), np.asarray(v, dtype=T)
    dk = np.asarray(decays, dtype=T)
    if fault == "decay_on_bias_tables":
        dk = np.ones_like(dk)
    gc = np.asarray(g, dtype=T) * clip
    if fault == "coupled_l2":                                        # torch.optim.Adam's weight_decay
        gc = gc + wd * dk * pT
        dk = np.zeros_like(dk)
    m2 = b1 * m + (one - b1) * gc
    v2 = b2 * v + (one - b2) * gc * gc
    ssz = lr / bc1
    den = np.sqrt(v2) / bc2s + eps
    p2 = pT * (one - (lr * wd) * dk)
    p2 = p2 - ssz * m2 / den
    d = np.float64
    mag = np.maximum(np.abs(pT.astype(d)), np.abs(p2.astype(d))).astype(np.float32)
    upd = d(ssz) * (d(b1) * np.abs(m.astype(d)) + d(one - b1) * np.abs(gc.astype(d))) / den.astype(d)
    unit = np.spacing(mag).astype(d) + 2.0 ** -24 * upd
    return Step(p2, m2, v2, norm, unit)


def errors(got, ref, layout):
    """Worst per-tensor errors of a step's results ``got`` (p, m, v, norm) against the float64 Step ``ref``: the parameters in
    ref.unit, each moment relative to its tensor's largest entry, the norm relative to itself. A quantity that must be zero
    and is not counts as infinitely wrong."""
    d = np.float64
    starts = [s.offset for s in layout]

    def rel_to_tensor_max(a, b):
        err = np.maximum.reduceat(np.abs(np.asarray(a, dtype=d) - np.asarray(b, dtype=d)), starts)
        top = np.maximum.reduceat(np.abs(np.asarray(b, dtype=d)), starts)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.max(np.where(err == 0, 0.0, err / top)))

    pe = float(np.max(np.abs(np.asarray(got[0], dtype=d) - ref.p.astype(d)) / ref.unit))
    n_got, n_ref = float(got[3]), float(ref.norm)
    ne = 0.0 if n_got == n_ref else (abs(n_got - n_ref) / n_ref if n_ref > 0 else np.inf)
    return Errors(pe, rel_to_tensor_max(got[1], ref.m), rel_to_tensor_max(got[2], ref.v), ne)


# ---- the cases --------------------------------------------------------------------------------------------------------------
# (ABI step, gain): the gradients of the k-th call are make_grads(case, k, ...) times gain; gain None = all zero (the update
# comes from momentum alone; norm 0, clip 1); gain "norm=X" = rescaled so that the global norm is X.
_SIX_THEN_LATE = [(1, 1.0), (2, 1e-6), (3, 1.0), (4, None), (5, 1e-3), (6, 1.0), (1000, 1.0), (100000, 1e-6)]
CASES = {
    # the reference's defaults. The largest tensor scale is 1e2: calls with gain 1 clip (norm >> 1), those with gain 1e-6 do not
    "defaults": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0), _SIX_THEN_LATE),
    "decay_no_clip": (Hyper(5e-4, 0.8, 0.95, 1e-6, 0.1, 0.0), _SIX_THEN_LATE),
    "decay_always_clips": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 0.05), _SIX_THEN_LATE),
    # the clip coefficient's + 1e-6: norm 1e-5 against max_grad_norm 1e-6, the coefficient is 1/11 and would be 1/10 without
    "small_norm": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1e-6), [(1, "norm=1e-5"), (2, "norm=1e-5")]),
}


def make_grads(case, k, layout, eps, gain):
    """float32 gradients of the k-th call of a case, seeded per (case, call, tensor): every tensor uniform in a scale drawn
    log-uniformly from 1e-8 .. 1e2, 10 % exact zeros, 2 % entries of the order of eps (eps/4 .. 4 eps)."""
    total = layout[-1].offset + layout[-1].numel
    if gain is None:
        return np.zeros(total, dtype=np.float32)
    g = np.empty(total, dtype=np.float64)
    for s in layout:
        name = f"adamw/{case}/{k}/{s.name}"
        u = float(synth.hash_u64(name + "/scale", 1)[0] >> np.uint64(11)) / 2.0 ** 53
        x = synth.uniform_f32(name, (s.numel,), 1.0).astype(np.float64)
        kind = synth.hash_u64(name + "/kind", s.numel) % np.uint64(50)
        x *= 10.0 ** (-8.0 + 10.0 * u)
        tiny = kind == 5
        frac = (synth.hash_u64(name + "/tiny", s.numel) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
        x[tiny] = np.where(x[tiny] < 0, -1.0, 1.0) * float(eps) * (0.25 + 3.75 * frac[tiny])
        x[kind < 5] = 0.0
        g[s.offset:s.offset + s.numel] = x
    if isinstance(gain, str):
        g *= float(gain.split("=")[1]) / np.sqrt(np.sum(g * g))
    else:
        g *= gain
    return g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_inputs(variant, case):
    """(layout, decays, initial flat float32 parameters, hyperparameters, [(ABI step, float32 gradients)]). Computed once
    and shared: nobody writes into these arrays."""
    dims = model_dims(variant)
    layout = flat_layout(dims)
    hp, calls = CASES[case]
    grads = [(step, make_grads(case, k, layout, hp.eps, gain)) for k, (step, gain) in enumerate(calls)]
    return layout, decay_mask(layout), pack(synth.make_state_dict(dims, seed=41), layout), hp, grads


_FLOORS = {}


def walk(variant, case, visit):
    """The case's calls carried in float32 (the state a device would carry): visit(k, step, p, g, m, v, decays, hp, layout,
    ref64, got32) before each state moves on."""
    layout, decays, p, hp, grads = case_inputs(variant, case)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for k, (step, g) in enumerate(grads):
        ref = adamw_step(p, g, m, v, decays, step, hp)
        got = adamw_step(p, g, m, v, decays, step, hp, dtype=np.float32)
        visit(k, step, p, g, m, v, decays, hp, layout, ref, got)
        p, m, v = got.p, got.m, got.v


def floors(variant="own_codebooks", cases=tuple(CASES)):
    """Errors(param, exp_avg, exp_avg_sq, norm): the worst distance, over every call of the given cases, of the float32
    evaluation from the float64 one on the same float32 inputs."""
    key = (variant, tuple(cases))
    if key not in _FLOORS:
        worst = []

        def visit(k, step, p, g, m, v, decays, hp, layout, ref, got):
            worst.append(errors(got[:4], ref, layout))

        for case in cases:
            walk(variant, case, visit)
        _FLOORS[key] = Errors(*(max(w[i] for w in worst) for i in range(4)))
    return _FLOORS[key]


def bars(variant="own_codebooks", cases=tuple(CASES)):
    """The device's bars: 4 x the floor of each quantity (the device may contract multiply-adds, and its division and square
    root may sit an ulp from the host's)."""
    return Errors(*(4.0 * f for f in floors(variant, cases)))
