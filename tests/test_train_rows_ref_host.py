"""not-gpu: the definitions, bounds and inputs of tests/train_rows_ref.py, checked on the CPU before any GPU run.

  * the definitions against torch.autograd in float64 where autograd applies (RMSNorm backward, gold score, margin-MSE, dense MSE,
    the cross-entropy head): relative difference at most 1e-12;
  * the plain numpy fp32 evaluation of every bounded output, in the natural and in a permuted summation order, stays within the
    bound (the bound is not too tight); the exact restatements (f16 planes, the fixed-point scatter, bf16 of the normalised rows)
    stay within theirs;
  * every mutant of the definitions — a mistake one of these kernels can make — leaves the bound by 10x or more (or changes bits of
    an exact output) in every case it applies to, and applies somewhere.
Run with -s for the figures (profiles/r28_train_rows_direct_summary.txt records them)."""
import numpy as np
import pytest
import torch

import train_rows_ref as T

F64, F32 = np.float64, np.float32
_by_kernel = {}
for _c in T.cases():
    _by_kernel.setdefault(_c.kernel, []).append(_c)


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _t(a):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=True)


# ---------------------------------------------------------------------------------------------- against autograd
def _norm(x, w, eps, post):
    return post * w * x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)


def test_definitions_against_autograd():
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for c in _by_kernel["launch_rmsnorm_bwd"]:
        p = c.p
        x, w = _t(p["x"]), _t(p["w"])
        h = _norm(x, w, p["eps"], p["post"])
        h.backward(torch.tensor(p["dh"].astype(F64)))
        r = T.rmsnorm_bwd(p)
        dx = x.grad.numpy() + (p["dres"].astype(F64) if "dres" in p else 0)
        dw = w.grad.numpy() + (p["dw0"].astype(F64) if p.get("accumulate") else 0)
        note("rmsnorm_bwd dx", _rel(r["dx"], dx)); note("rmsnorm_bwd dw", _rel(r["dw"], dw))
        note("rmsnorm_bwd w_part", _rel(r["w_part"].sum(0) + (p["dw0"].astype(F64) if p.get("accumulate") else 0), dw))
    for c in _by_kernel["launch_gold_score_bwd"]:
        p = c.p
        L, V, d = p["E"].shape
        x, ln, E = _t(p["x"]), _t(p["ln"]), _t(p["E"].reshape(-1, d))
        h = _norm(x, ln, p["eps"], p["post"])
        h.retain_grad()
        idx = torch.tensor(p["out_idx"].astype(np.int64))
        e = E[idx]
        e.retain_grad()
        s = (h * e).sum(-1)
        s.backward(torch.tensor(p["dscores"].astype(F64)))
        r = T.gold_score_bwd(p)
        note("gold_score_bwd de", _rel(r["de"], e.grad.numpy())); note("gold_score_bwd dh", _rel(r["dh"], h.grad.numpy()))
        note("gold_scores", _rel(T.gold_scores(p)["scores"], s.detach().numpy()))
        pos = np.arange(x.shape[0]) % L       # out_idx is position * V + clamped code
        assert np.array_equal(p["out_idx"], pos * V + np.clip(p["codes"].reshape(-1), 0, V - 1))
    for c in _by_kernel["launch_margin_mse"] + _by_kernel["launch_margin_mse_bwd"]:
        p = dict(c.p)
        bz, L = p["bz"], p["L"]
        sc = _t(p["scores"])
        tot = 0
        losses = []
        for q, k in enumerate(p["prefix_lens"]):
            m = sc[:, 0, :k].sum(-1) - sc[:, 1, :k].sum(-1)       # slicing beyond L stops at L, as the reference's does
            t = torch.tensor(p["teacher_pos"][q].astype(F64) - p["teacher_neg"][q].astype(F64))
            losses.append(torch.nn.functional.mse_loss(m, t))
            tot = tot + losses[-1]
        tot.backward()
        r = T.margin_mse(p)
        note("margin_mse losses", _rel(r["losses"], [float(l.detach()) for l in losses]))
        p["margins"] = r["margins"]
        note("margin_mse_bwd dscores", _rel(T.margin_mse_bwd(p)["dscores"], sc.grad.numpy()))
    for c in _by_kernel["launch_dense_mse_head"]:
        p = dict(c.p)
        hF = _t(p["hF"])
        bz = hF.shape[0] // 3
        q, dp, dn = hF[:bz], hF[bz:2 * bz], hF[2 * bz:]
        m = (q * dp).sum(-1) - (q * dn).sum(-1)
        m.retain_grad()
        loss = torch.nn.functional.mse_loss(m, torch.tensor(p["teacher_pos"].astype(F64) - p["teacher_neg"].astype(F64)))
        loss.backward()
        r = T.dense_mse(p)
        note("dense_mse loss", _rel(r["loss"], float(loss.detach()))); note("dense_mse g", _rel(r["g"], m.grad.numpy()))
        p["g_in"] = r["g"]
        note("dense_mse dhF", _rel(T.dense_mse(p)["dhF"], hF.grad.numpy()))
    for c in _by_kernel["launch_s2s_head"]:
        p = dict(c.p)
        L, V, d = p["E"].shape
        n = p["hF"].shape[0]
        hF, E = _t(p["hF"]), _t(p["E"])
        pos = torch.arange(n) % L
        logits = torch.einsum("nd,nvd->nv", hF, E[pos])
        logits.retain_grad()
        lab = torch.tensor(np.clip(p["labels"], 0, V - 1).astype(np.int64))
        loss = torch.nn.functional.cross_entropy(logits, lab)
        loss.backward()
        r = T.s2s_head(p)
        note("s2s loss", _rel(r["loss"], float(loss.detach()))); note("s2s dlogits", _rel(r["dlogits"], logits.grad.numpy()))
        p["dl_in"] = r["dlogits"]
        r = T.s2s_head(p)
        note("s2s dH", _rel(r["dH"], hF.grad.numpy())); note("s2s dE", _rel(r["dE"], E.grad.numpy()))
    print("\nrelative difference to torch.autograd (float64):")
    for k, v in worst.items():
        print(f"  {k}: {v:.3e}")
    assert max(worst.values()) <= 1e-12, worst


# ---------------------------------------------------------------------------------------------- fp32 restatement against the bound
def _ratio(val, ref, bound):
    err = np.abs(np.asarray(val, F64) - np.asarray(ref, F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / np.asarray(bound, F64), 0.0)
    return float(r.max()) if r.size else 0.0


def test_fp32_restatement_stays_within_the_bound():
    worst = {}
    for c in T.cases():
        if c.define is None:
            continue
        for order, perm in (("natural", None), ("permuted", "a")):
            r = c.define(c.p, F32, perm)
            for name, ex in c.expect.items():
                x = _ratio(r[c.keys[name]], ex.ref, ex.bound)
                k = (c.kernel, name, order)
                if x > worst.get(k, (-1, ""))[0]:
                    worst[k] = (x, c.name)
                assert x <= 1.0, (c.name, name, order, x)
    print("\nnumpy fp32 evaluation / bound, worst per launcher and output:")
    for (k, name, order), (x, cn) in sorted(worst.items()):
        print(f"  {k} {name} {order}: {x:.4f} ({cn})")


def test_exact_restatements_stay_within_their_bounds():
    worst = {}
    for c in _by_kernel["launch_scatter_rows_fix+launch_fix_flush"]:
        ex = c.expect["table"]
        x = _ratio(T.scatter_flush(c.p, F32)["table"], ex.ref, ex.bound)
        worst["scatter+flush"] = max(worst.get("scatter+flush", 0), x)
        assert x <= 1.0, (c.name, x)
    for c in _by_kernel["launch_split_dyn"] + _by_kernel["launch_split_dyn_T"]:
        xs = c.p["xs"]
        hi, lo = T.split_planes(xs)
        x = _ratio(hi.astype(F64) + lo.astype(F64), xs, T.plane_bound(xs))
        worst["split_dyn planes"] = max(worst.get("split_dyn planes", 0), x)
        assert x <= 1.0, (c.name, x)
    for c in _by_kernel["launch_train_dec_embed"]:
        r = T.dec_embed(c.p)
        x = _ratio(r["hi"].astype(F64) + r["lo"].astype(F64), r["xs"], r["b_planes"])
        rec = ((r["hi"].astype(F32) + r["lo"].astype(F32)) * F32(16)).astype(F32)
        ss = (rec * rec).sum(1, dtype=F32)
        fix = np.floor((ss * F32(T.SSQ_FIX) + F32(0.5)).astype(F64))
        y = _ratio(fix, r["ssq"], r["b_ssq_planes"])
        worst["dec_embed planes"] = max(worst.get("dec_embed planes", 0), x)
        worst["dec_embed ssq"] = max(worst.get("dec_embed ssq", 0), y)
        assert x <= 1.0 and y <= 1.0, (c.name, x, y)
    for c in _by_kernel["launch_rmsnorm_bf16_T"]:          # bf16 of the fp32 evaluation against bf16 of the definition: at most 1 %
        ex = c.expect["out_p"]
        for perm in (None, "a"):
            h32 = T.gold_scores(c.p, F32, perm)["hidden"].astype(F32)
            bits = T.bf16_bits(h32)
            diff = bits != ex.ref
            key = T.bf16_order(bits)
            assert ((key >= ex.flips[0]) & (key <= ex.flips[1]))[diff].all(), c.name
            frac = diff.mean()
            worst["rmsnorm_bf16_T other neighbour"] = max(worst.get("rmsnorm_bf16_T other neighbour", 0), float(frac))
            assert frac <= 0.01, (c.name, frac)
    print("\nexact restatements / bound:")
    for k, v in worst.items():
        print(f"  {k}: {v:.4f}")


# ---------------------------------------------------------------------------------------------- mutants
def _applies(mut_out, ref):
    return bool(np.abs(np.asarray(mut_out, F64) - np.asarray(ref, F64)).max() > 2.0 ** -24 * max(1.0, float(np.abs(ref).max())))


def _mutant_ratios(mut):
    """[(ratio, case name)] over every case the mutant applies to; inf = an exact output changed."""
    out = []
    for c in T.cases():
        if c.define is not None:
            try:
                r = c.define(c.p, F64, None, mut)
            except TypeError:
                continue
            best, hit = 0.0, False
            for name, ex in c.expect.items():
                m = r[c.keys[name]]
                if _applies(m, ex.ref):
                    hit = True
                    best = max(best, _ratio(m, ex.ref, ex.bound))
            if hit:
                out.append((best, c.name))
        elif c.kernel.startswith("launch_scatter") and mut == "start_row_scattered":
            m = T.scatter_flush(c.p, F64, mut)["table"]
            ex = c.expect["table"]
            if _applies(m, ex.ref):
                out.append((_ratio(m, ex.ref, ex.bound), c.name))
        elif c.kernel in ("launch_train_indices", "launch_train_dec_embed") and mut == "in_idx_i":
            if c.kernel == "launch_train_indices":
                changed = not np.array_equal(T.train_indices(c.p["codes"], c.p["V"], mut)[0], c.expect["in_idx"].ref)
            else:
                changed = not np.array_equal(T.dec_embed(c.p, mut)["out"], T.dec_embed(c.p)["out"])
            if changed:
                out.append((np.inf, c.name))
        elif mut == "pad_from_neighbour" and c.kernel in ("launch_transpose_pad", "launch_to_bf16_T", "launch_split_dyn_T"):
            R, C, Rpad = c.p["R"], c.p["C"], c.p["Rpad"]
            v = np.arange(1, R * C + 1, dtype=F64).reshape(R, C)
            if not np.array_equal(T.transposed(v, Rpad, Rpad, 0.0, mut), T.transposed(v, Rpad, Rpad, 0.0)):
                out.append((np.inf, c.name))      # a zero column holds a value: bits (and a bound of 0) are left
        elif mut == "relu_ge" and (c.kernel == "launch_relu_bwd" or (c.kernel == "launch_to_bf16_T" and c.p.get("relu"))):
            if c.kernel == "launch_relu_bwd":
                changed = not np.array_equal(T.relu_gate(c.p["dy"], c.p["act"], mut), c.expect["dy"].ref)
            else:
                C = c.p["C"]
                x, a = c.p["x"][:, :C], c.p["act"][:, :C]
                changed = not np.array_equal(T.bf16_bits(T.relu_gate(x, a, mut)), T.bf16_bits(T.relu_gate(x, a)))
            if changed:
                out.append((np.inf, c.name))
        elif mut == "lo_dropped" and c.kernel in ("launch_split_dyn", "launch_split_dyn_T"):
            xs = c.p["xs"]
            hi, lo = T.split_planes(xs, mut)
            out.append((_ratio(hi.astype(F64) + lo.astype(F64), xs, T.plane_bound(xs)), c.name))
    return out


@pytest.mark.parametrize("mut", T.MUTANTS)
def test_mutant_is_caught(mut):
    rs = _mutant_ratios(mut)
    assert rs, f"{mut} applies to no case"
    lo = min(rs)
    print(f"\n{mut}: applies to {len(rs)} cases, smallest |mutant - ref| / bound {lo[0]:.3g} ({lo[1]}), largest {max(rs)[0]:.3g}")
    assert lo[0] >= 10, (mut, lo)
