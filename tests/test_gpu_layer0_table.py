"""The decoder's layer-0 Q/K/V table (ripor_amd/csrc/passes.hip: ensure_l0_table): the layer-0 self-attention
projection is a function of (position, token) alone, so a search reads q | k | v of its rows from a table the model makes
once instead of running the projection. The same searches with the table off (`Context.set_l0_table(0)`), gated on the
route planner (1, the default: only launches the 256 x 256 ping-pong kernel would run, the kernel that made the table —
same bits) and forced on (2: every layer-0 launch, whatever kernel it would have taken — scores move by that kernel's
rounding, within the 3e-5 tests/test_gpu_forced_tail.py::test_lane_split_gives_the_results_of_one_call allows for a route
change). The mode is a setting of the ctx, so one process compares them.
Reference semantics: T5Attention q / k / v projections of decoder block 0 on T5LayerNorm(inputs_embeds)
(t5_pretrainer/modeling/t5_generative_retriever.py:194-214 builds inputs_embeds from list_decoder_embeds)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import compare_ranked

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_TOL = 3e-5   # scores after a change of GEMM route (see the module docstring)


def _engine():
    from ripor_amd import engine as E
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return E


def _search(E, model, trie, ids, mask, B, L, mode, forks="auto", log_softmax=False, profile=False):
    """One search with the table mode and the fork depths given; the ctx is left as it was found."""
    ctx = model.ctx
    ctx.set_l0_table(mode)
    if forks != "auto":
        ctx.set_fork_depths(forks)
    try:
        if profile:
            ctx.profile_enable(True)
            ctx.profile_reset()
        res = E.search(model, trie, torch.from_numpy(ids), torch.from_numpy(mask), B, L, apply_log_softmax_for_scores=log_softmax)
        torch.cuda.synchronize()
        out = dict(tokens=res.tokens.cpu().numpy(), scores=res.scores.cpu().numpy(), row_lo=res.row_lo.cpu().numpy(),
                   row_hi=res.row_hi.cpu().numpy(), forks=ctx.last_fork_stats(), table_bytes=ctx.l0_table_bytes(model))
        if profile:
            prof = ctx.profile_get()
            out["gemm_launches"] = prof["gemm"]["launches"] + prof["gemm_small"]["launches"]
            out["other_bytes"] = prof["other"]["bytes"]
        return out
    finally:
        if profile:
            ctx.profile_enable(False)
        ctx.set_fork_depths(None)
        ctx.set_l0_table(1)


def _same_bits(a, b):
    for k in ("tokens", "row_lo", "row_hi", "scores"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _same_within_route_tol(a, b, label):
    for k in ("tokens", "row_lo", "row_hi"):
        assert (a[k] == b[k]).all(), (label, k)
    err = float(np.abs(a["scores"].astype(np.float64) - b["scores"]).max())
    print(f"[layer0 table] {label}: max score difference {err:.3g}")
    assert err <= ROUTE_TOL, (label, err)


def _plan(tmp_path, **kw):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "gemm_route_driver.cpp")], check=True)
    out = subprocess.run([exe, "plan"] + [f"{k}={int(v)}" for k, v in kw.items()], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


@pytest.mark.gpu
def test_gated_table_gives_the_bits_of_the_projection(tmp_path):
    """Headline layer shapes (d_model 768, 12 heads of 64, d_ff 3072, 32 x 256 codebooks; one encoder and one decoder layer):
    16 queries, beam 10, fork at depth 8 — a tail pass of 16 * 10 * 24 = 3840 rows = 15 x 9 tiles of 256 x 256, which the
    planner sends to the ping-pong kernel. Table on (gated) against table off: every output bit for bit, with one GEMM
    launch fewer in the profile counters (so the test cannot pass with the table silently off)."""
    E = _engine()
    from ripor_amd.utils import synth
    Q, B, L, V, T = 16, 10, 32, 256, 8
    # the tail pass's layer-0 launch as passes.hip::linear states it: device-side live count, fused-norm consumer, scratch lent
    p = _plan(tmp_path, M=Q * B * (L - T), N=3 * 768, K=768, m_dev=1, row_ssq=1, part=1, mid_split=1, part_cap=(9 << 20))
    assert not p["invalid"] and [(s["family"], s["ksplit"]) for s in p["steps"]] == [("pp", 1)], p
    assert (p["steps"][0]["tiles_m"], p["steps"][0]["tiles_n"]) == (15, 9)
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=3072, num_decoder_layers=1)
    assert (dims.d_model, dims.d_kv, dims.num_heads) == (768, 64, 12)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=17), dims)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(20000, L, V, seed=17), V)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=17, max_len=16)
    off = _search(E, model, trie, ids, mask, B, L, 0, forks=[T])
    on = _search(E, model, trie, ids, mask, B, L, 1, forks=[T])
    assert off["table_bytes"] == 0 and on["table_bytes"] == (L * V + 1) * 3 * 768 * 4
    assert on["forks"][0]["depth"] == T and on["forks"][0]["forced"] > 0, on["forks"]
    _same_bits(on, off)
    off_p = _search(E, model, trie, ids, mask, B, L, 0, forks=[T], profile=True)
    on_p = _search(E, model, trie, ids, mask, B, L, 1, forks=[T], profile=True)
    _same_bits(on_p, off)
    _same_bits(off_p, off)
    print(f"[layer0 table] GEMM launches: {off_p['gemm_launches']} without the table, {on_p['gemm_launches']} with it")
    assert on_p["gemm_launches"] == off_p["gemm_launches"] - 1       # the tail's layer-0 launch; the steps' 160 rows keep their GEMM
    live = on["forks"][0]["forced"] * B * (L - T)
    assert on_p["other_bytes"] - off_p["other_bytes"] == pytest.approx(2.0 * live * 3 * 768 * 4)   # the gather: a row read, a row written


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g1_mini_b4_l8", "g1_mini_b4_l8_v100", "g1_mini_b2_l4_v1024", "g1_mini_b4_l8_shared",
                                  "g1_mini_b4_l8_logsoftmax"])
def test_forced_table_on_the_mini_goldens(golden_cache, name):
    """Every layer-0 Q/K/V launch from the table (mode 2): shared step 0 (the start-token row), steps behind a fork
    (compacted stages, device-side live counts), tail passes — on shapes whose GEMMs take the skinny / wave-split routes, so
    the scores differ by a route change and nothing else. The reference's golden output still holds at mode 2."""
    E = _engine()
    g = golden_cache(name)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, g.state_dict, g.dims)
    trie = E.DeviceTrie.from_codes(ctx, g.codes, g.V)
    rows = g.L * g.V + 1
    for forks in ("auto", [1], [2, 3], [1, g.L - 1]):
        off = _search(E, model, trie, g.input_ids, g.attention_mask, g.B, g.L, 0, forks=forks, log_softmax=g.log_softmax)
        on = _search(E, model, trie, g.input_ids, g.attention_mask, g.B, g.L, 2, forks=forks, log_softmax=g.log_softmax)
        assert on["table_bytes"] == rows * 3 * g.dims.inner * 4
        assert on["forks"] == off["forks"]
        _same_within_route_tol(on, off, f"{name} forks {forks}")
        compare_ranked(g, on["tokens"], on["scores"], label=f" (layer-0 table, forks {forks})")
    off_p = _search(E, model, trie, g.input_ids, g.attention_mask, g.B, g.L, 0, profile=True, log_softmax=g.log_softmax)
    on_p = _search(E, model, trie, g.input_ids, g.attention_mask, g.B, g.L, 2, profile=True, log_softmax=g.log_softmax)
    assert on_p["gemm_launches"] < off_p["gemm_launches"], (on_p["gemm_launches"], off_p["gemm_launches"])


@pytest.mark.gpu
def test_ragged_and_empty_tails():
    """Beam 3 and a fork at depth 3 of 8: tail rows = forced queries x 15, not a multiple of the four rows a block of the
    gather holds. A first fork at depth 1 forces nobody (a dozen documents share every first code): live count 0, the gather
    exits like tail_embed_kernel and everybody walks on in the compacted stage, whose steps read the table too."""
    E = _engine()
    from ripor_amd.utils import synth
    Q, B, L, V = 5, 3, 8, 256
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128, num_decoder_layers=2)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=23), dims)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(3000, L, V, seed=23), V)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=23, max_len=12)
    for forks in ([3], [1, 3], [1]):
        off = _search(E, model, trie, ids, mask, B, L, 0, forks=forks)
        on = _search(E, model, trie, ids, mask, B, L, 2, forks=forks)
        assert on["forks"] == off["forks"]
        if forks[0] == 1:
            assert on["forks"][0]["forced"] == 0 and on["forks"][0]["left"] == Q, on["forks"]
        else:
            assert 0 < on["forks"][0]["forced"] and (on["forks"][0]["forced"] * B * (L - 3)) % 4 != 0, on["forks"]
        _same_within_route_tol(on, off, f"beam 3 forks {forks}")


@pytest.mark.gpu
def test_table_follows_the_weights_and_the_precision():
    """A training step replaces in_embeds, dec_ln0[0] and dec_qkv[0] on the live model; a precision switch drops the table
    too. The next search makes it again: it returns the bits of a fresh model loaded with the updated weights, not those of
    the search before the step. Mode 2, so that these small searches do read the table."""
    E = _engine()
    from ripor_amd.utils import synth
    L, V, bz, B = 8, 256, 4, 4
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128, num_decoder_layers=2)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=41), dims)
    state = E.TrainState(model)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(2000, L, V, seed=5), V)
    ids, mask = synth.make_queries(bz, vocab_size=dims.vocab_size, seed=9, max_len=12)
    before = _search(E, model, trie, ids, mask, B, L, 2)
    nbytes = before["table_bytes"]
    assert nbytes == (L * V + 1) * 3 * dims.inner * 4
    # precision round trip: the table is gone, then made again with the same content
    ctx.set_precision("f32")
    try:
        assert ctx.l0_table_bytes(model) == 0
        exact = _search(E, model, trie, ids, mask, B, L, 2)
        assert exact["table_bytes"] == 0                      # exact fp32 keeps its GEMM
    finally:
        ctx.set_precision("f16x2")
    assert ctx.l0_table_bytes(model) == 0
    again = _search(E, model, trie, ids, mask, B, L, 2)
    assert again["table_bytes"] == nbytes
    _same_bits(again, before)
    assert (exact["tokens"] == before["tokens"]).all() and np.abs(exact["scores"] - before["scores"]).max() < 1e-4
    # a training step
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    doc = torch.from_numpy(synth.make_codes(2 * bz, L, V, seed=6).astype(np.int64).reshape(2, bz, L).transpose(1, 0, 2).copy())
    prefix = [L, 4]
    tp = torch.from_numpy(np.stack([synth.uniform_f32(f"l0/p{k}", (bz,), 30.0) for k in prefix]))
    tn = torch.from_numpy(np.stack([synth.uniform_f32(f"l0/n{k}", (bz,), 30.0) for k in prefix]))
    qkv_before = model.export_state_dict()["decoder.block.0.layer.0.SelfAttention.q.weight"].clone()
    E.train_step(model, state, ti.cuda(), tm.cuda(), doc.cuda(), tp, tn, prefix, lr=3e-3)     # a large step: results must move
    torch.cuda.synchronize()
    assert not torch.equal(model.export_state_dict()["decoder.block.0.layer.0.SelfAttention.q.weight"], qkv_before)
    assert ctx.l0_table_bytes(model) == 0                     # dropped by the optimizer step
    after = _search(E, model, trie, ids, mask, B, L, 2)
    fresh_model = E.DeviceModel(ctx, {k: v.cpu().numpy() for k, v in model.export_state_dict().items()}, dims)
    fresh = _search(E, fresh_model, trie, ids, mask, B, L, 2)
    fresh_gemm = _search(E, fresh_model, trie, ids, mask, B, L, 0)
    _same_bits(after, fresh)
    _same_within_route_tol(after, fresh_gemm, "after a training step, table against projection")
    assert not np.array_equal(after["scores"], before["scores"]), "the step did not change the scores: the test checks nothing"


def test_table_cap_admits_the_documented_models(tmp_path):
    """Host arithmetic of the size cap (ripor_amd/csrc/gemm_route.h: l0_table_fits), no device memory involved."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "cap.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "%s"\n'
                   'int main(int, char** v) { const int L = atoi(v[1]), V = atoi(v[2]), inner = atoi(v[3]);\n'
                   '  printf("%%zu %%d\\n", rpr::l0_table_bytes(L, V, inner), (int)rpr::l0_table_fits(L, V, inner)); }\n'
                   % os.path.join(REPO, "ripor_amd", "csrc", "gemm_route.h"))
    exe = str(tmp_path / "cap")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, str(src)], check=True)

    def fits(L, V, inner):
        nbytes, ok = subprocess.run([exe, str(L), str(V), str(inner)], check=True, capture_output=True, text=True).stdout.split()
        assert int(nbytes) == (L * V + 1) * 3 * inner * 4
        return bool(int(ok))

    assert fits(32, 256, 768)          # t5-base, 32 x 256: 75 MB
    assert fits(16, 1024, 768)         # t5-base, 16 x 1024: 151 MB
    assert fits(32, 256, 1024)         # t5-large, 32 x 256: 101 MB
    assert not fits(32, 256, 4096)     # t5-3b (32 heads of 128), 32 x 256: 403 MB
    assert not fits(18, 1024, 768)     # the model of test_over_cap_model_keeps_its_gemm: 170 MB


@pytest.mark.gpu
def test_over_cap_model_keeps_its_gemm():
    """18 x 1024 codebooks at inner = 768 ask for a 170 MB table, over the cap: none is made (nor allocated), every mode runs
    the projection and returns the same bits."""
    E = _engine()
    from ripor_amd.utils import synth
    Q, B, L, V = 3, 4, 18, 1024
    dims = synth.mini_dims(L=L, V=V, enc_layers=1, d_ff=128, num_decoder_layers=1, shared_output_input_embeds=True)
    ctx = E.Context.get(0)
    model = E.DeviceModel(ctx, synth.make_state_dict(dims, seed=29), dims)
    trie = E.DeviceTrie.from_codes(ctx, synth.make_codes(3000, L, V, seed=29), V)
    ids, mask = synth.make_queries(Q, vocab_size=dims.vocab_size, seed=29, max_len=12)
    off = _search(E, model, trie, ids, mask, B, L, 0, profile=True)
    on = _search(E, model, trie, ids, mask, B, L, 2, profile=True)
    assert on["table_bytes"] == 0
    assert on["gemm_launches"] == off["gemm_launches"]
    _same_bits(on, off)
