"""The shape -> kernel table of the attention launches (ripor_amd/csrc/attn_route.h), checked on the CPU.

tests/attn_route_driver.cpp includes the header and is compiled here with the host C++ compiler. Every expectation below
was worked out by hand from the launchers as they stood before the planners were split out of them (launch_enc_attn,
launch_dec_self_attn, launch_dec_cross_attn, launch_tail_self_attn, launch_tail_cross_attn, launch_step_cross_attn,
launch_self_attn_bwd); the arithmetic is in the docstrings — none comes from running the planner. H = 12 heads throughout
unless a case says otherwise: HB = ceil(12 / 4) = 3 blocks of four heads."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4 * 32 * 64 * 4          # second-generation tiles: four waves x one 32 x 64 fp32 strip = 32768 bytes
KB = 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("attn_route") / "attn_route_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "attn_route_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def plan(driver, site, **kw):
    argv = [driver, site] + [f"{k}={int(v)}" for k, v in kw.items()]
    return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)


def got(p, *keys):
    return tuple(p[k] for k in keys)


LAUNCH = ("kernel", "invalid", "grid", "block", "smem")


def test_header_is_host_only():
    """The driver's build proves that the header compiles with -Wall -Werror; it must not reach for a HIP header either."""
    src = open(os.path.join(REPO, "ripor_amd", "csrc", "attn_route.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert set(includes) <= {"<algorithm>", "<cstddef>", '"../../include/ripor_hip.h"'}, includes


def test_tail_self_attention(driver):
    """40 sequences x 12 heads. Second generation (L <= 32, T <= 8): a block per (sequence, four heads) = 40 * 3 = 120 blocks,
    one 8-KB strip per wave. First generation: a wave per (sequence, head) = 480 / 4 = 120 blocks; per wave V [32 NKT][64] +
    64 bias floats, and with two key tiles a 32 x 64 output strip: 4 * (2048 + 64) * 4 = 33792, 4 * (4096 + 64 + 2048) * 4 = 99328."""
    base = dict(nseq_cap=40, B=10, H=12)
    assert got(plan(driver, "tail_self", L=32, T=4, **base), *LAUNCH, "HB") == ("TAIL_SELF_V2", 0, [120, 1], 256, TILE, 3)
    assert got(plan(driver, "tail_self", L=32, T=8, **base), "kernel") == ("TAIL_SELF_V2",)
    assert got(plan(driver, "tail_self", L=16, T=4, **base), "kernel") == ("TAIL_SELF_V2",)
    assert got(plan(driver, "tail_self", L=32, T=9, **base), *LAUNCH) == ("TAIL_SELF_G1_NKT1", 0, [120, 1], 256, 4 * (32 * 64 + 64) * 4)
    # 10 heads: HB is still 3, but the first generation packs 400 waves into 100 blocks
    assert got(plan(driver, "tail_self", L=32, T=4, nseq_cap=40, B=10, H=10), "kernel", "grid") == ("TAIL_SELF_V2", [120, 1])
    assert got(plan(driver, "tail_self", L=32, T=9, nseq_cap=40, B=10, H=10), "kernel", "grid") == ("TAIL_SELF_G1_NKT1", [100, 1])
    for L in (33, 64):
        assert got(plan(driver, "tail_self", L=L, T=4, **base), *LAUNCH) == ("TAIL_SELF_G1_NKT2", 0, [120, 1], 256, 4 * (64 * 64 + 64 + 32 * 64) * 4)
    # 128-dim heads: a block per (sequence, head) = 480; K [L][129] + V [L][128] + 4 x 64 weights + 64 bias floats:
    # (32 * 129 + 32 * 128 + 256 + 64) * 4 = 8544 * 4 = 34176
    assert got(plan(driver, "tail_self", L=32, T=4, dkv=128, **base), *LAUNCH) == ("TAIL_SELF_VALU128", 0, [480, 1], 256, 34176)
    for L, T in ((65, 4), (32, 0), (32, 32)):
        assert plan(driver, "tail_self", L=L, T=T, **base)["invalid"] == 1
    assert got(plan(driver, "tail_self", L=32, T=4, gen=1, **base), "kernel", "smem") == ("TAIL_SELF_G1_NKT1", 33792)
    assert got(plan(driver, "tail_self", L=40, T=4, gen=1, **base), "kernel") == ("TAIL_SELF_G1_NKT2",)


def test_tail_cross_attention_tiles_per_wave(driver):
    """220 rows per query = 7 tiles of 32: Q * 12 * 7 waves of one tile reach 32768 at Q = 391 (390: 32760, 391: 32844).
    Below: one tile per wave, 7 groups, 390 * 7 * 3 = 8190 blocks (OCC 4, prefetch). At the bar: nine tiles per wave, one
    group, 391 * 3 = 1173 blocks (OCC 3, no prefetch). 640 rows = 20 tiles at Q = 137 (32880 waves): ceil(20 / 9) = 3 groups."""
    p = plan(driver, "tail_cross", Q=390, B=220, H=12, Lq=32)
    assert got(p, *LAUNCH, "HB", "groups", "tpw", "tiles") == ("TAIL_CROSS_V2_TPW1", 0, [8190, 1], 256, TILE, 3, 7, 1, 7)
    p = plan(driver, "tail_cross", Q=391, B=220, H=12, Lq=32)
    assert got(p, *LAUNCH, "HB", "groups", "tpw", "tiles") == ("TAIL_CROSS_V2_TPW9", 0, [1173, 1], 256, TILE, 3, 1, 9, 7)
    p = plan(driver, "tail_cross", Q=137, B=640, H=12, Lq=32)
    assert got(p, "kernel", "grid", "groups", "tpw") == ("TAIL_CROSS_V2_TPW9", [137 * 3 * 3, 1], 3, 9)


def test_tail_cross_attention_by_query_length(driver):
    """Q = 4, 100 rows = 4 tiles, 4 * 12 * 4 = 192 waves. Lq = 32: second generation, 4 groups of one tile, 4 * 4 * 3 = 48
    blocks. Lq = 33 / 64: first generation with two key tiles, 192 / 4 = 48 blocks, V [64][64] per wave = 65536 bytes.
    Lq = 65: the block kernel; its LDS is (Lq * (68 + 64) + rows * (68 + 2 (Lq + 1)) + 4) * 4 = (8580 + 200 rows + 4) * 4:
    100 rows 114336 > 64 KB, 64 rows 85536 > 64 KB, 32 rows 59936: chunks of 32 rows, ceil(100 / 32) = 4 over blockIdx.y."""
    base = dict(Q=4, B=100, H=12)
    assert got(plan(driver, "tail_cross", Lq=32, **base), *LAUNCH, "groups") == ("TAIL_CROSS_V2_TPW1", 0, [48, 1], 256, TILE, 4)
    for Lq in (33, 64):
        assert got(plan(driver, "tail_cross", Lq=Lq, **base), *LAUNCH, "tiles") == ("TAIL_CROSS_G1_NKT2", 0, [48, 1], 256, 4 * 64 * 64 * 4, 4)
    assert got(plan(driver, "tail_cross", Lq=65, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [48, 4], 256, 59936, 32)
    assert got(plan(driver, "tail_cross", Lq=32, gen=1, **base), *LAUNCH, "tiles") == ("TAIL_CROSS_G1_NKT1", 0, [48, 1], 256, 4 * 32 * 64 * 4, 4)
    # 128-dim heads: the block kernel at any Lq. (32 * 260 + rows * (132 + 66) + 4) * 4: 100 rows 112496 > 96 KB, 64 rows
    # (8320 + 12672 + 4) * 4 = 83984: two chunks of 64
    assert got(plan(driver, "tail_cross", Lq=32, dkv=128, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK128", 0, [48, 2], 256, 83984, 64)


def test_tail_cross_attention_32bit_offsets(driver):
    """The second generation addresses a query's rows with 32-bit offsets: rows * 12 * 64 < 2^29 = 536870912 holds up to
    699050 rows (536870400) and fails at 699051 (536871168). Both are 21846 tiles, 262152 waves of one tile (>= 32768: nine per
    wave, ceil(21846 / 9) = 2428 groups, 2428 * 3 = 7284 blocks); past the bound the first generation, 262152 / 4 = 65538 blocks."""
    p = plan(driver, "tail_cross", Q=1, B=699050, H=12, Lq=32)
    assert got(p, "kernel", "grid", "groups", "tiles") == ("TAIL_CROSS_V2_TPW9", [7284, 1], 2428, 21846)
    p = plan(driver, "tail_cross", Q=1, B=699051, H=12, Lq=32)
    assert got(p, *LAUNCH, "tiles") == ("TAIL_CROSS_G1_NKT1", 0, [65538, 1], 256, 4 * 32 * 64 * 4, 21846)


def test_step_cross_attention(driver):
    """16-row tiles, one 16 x 68 strip per wave = 4 * 16 * 68 * 4 = 17408 bytes. Beam 10: one tile, the kernel without a tile
    loop, 100 * 3 = 300 blocks. Beam 100 = 7 tiles: Q * 12 * 7 reaches 32768 at Q = 391 — below it one tile per wave (7 groups,
    390 * 7 * 3 = 8190 blocks), at it min(7, 8) = 7 per wave (one group, 1173 blocks). Beam 1000 = 63 tiles, Q = 44 (33264
    waves): capped at 8 per wave, ceil(63 / 8) = 8 groups, 44 * 8 * 3 = 1056 blocks."""
    smem = 4 * 16 * 68 * 4
    p = plan(driver, "step_cross", Q=100, B=10, H=12, Lq=32)
    assert got(p, *LAUNCH, "HB", "groups", "tpw", "tiles") == ("STEP_CROSS16_ONE", 0, [300, 1], 256, smem, 3, 1, 1, 1)
    assert got(plan(driver, "step_cross", Q=100, B=16, H=12, Lq=32), "kernel") == ("STEP_CROSS16_ONE",)
    assert got(plan(driver, "step_cross", Q=100, B=17, H=12, Lq=32), "kernel", "tiles", "groups") == ("STEP_CROSS16_MULTI", 2, 2)
    p = plan(driver, "step_cross", Q=390, B=100, H=12, Lq=32)
    assert got(p, *LAUNCH, "groups", "tpw", "tiles") == ("STEP_CROSS16_MULTI", 0, [8190, 1], 256, smem, 7, 1, 7)
    p = plan(driver, "step_cross", Q=391, B=100, H=12, Lq=32)
    assert got(p, *LAUNCH, "groups", "tpw", "tiles") == ("STEP_CROSS16_MULTI", 0, [1173, 1], 256, smem, 1, 7, 7)
    p = plan(driver, "step_cross", Q=44, B=1000, H=12, Lq=32)
    assert got(p, "kernel", "grid", "groups", "tpw", "tiles") == ("STEP_CROSS16_MULTI", [1056, 1], 8, 8, 63)


def test_step_cross_attention_falls_back(driver):
    """Q = 100, beam 10. Lq = 33: the block kernel, (33 * 132 + 10 * (68 + 68) + 4) * 4 = 22880 bytes, 1200 blocks.
    step_cross = 1: the tail's 32-row tile kernel (one tile, 1200 waves: one per wave, 300 blocks). step_cross = 0, or the
    first generation with step_cross = 2: the block kernel, (32 * 132 + 10 * (68 + 66) + 4) * 4 = 22272 bytes. 128-dim heads:
    the block kernel, (32 * 260 + 10 * (132 + 66) + 4) * 4 = 41216 bytes."""
    base = dict(Q=100, B=10, H=12)
    assert got(plan(driver, "step_cross", Lq=33, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [1200, 1], 256, 22880, 0)
    assert got(plan(driver, "step_cross", Lq=32, step_cross=1, **base), *LAUNCH, "groups") == ("TAIL_CROSS_V2_TPW1", 0, [300, 1], 256, TILE, 1)
    assert got(plan(driver, "step_cross", Lq=32, step_cross=0, **base), *LAUNCH) == ("CROSS_BLOCK64", 0, [1200, 1], 256, 22272)
    assert got(plan(driver, "step_cross", Lq=32, step_cross=2, gen=1, **base), *LAUNCH) == ("CROSS_BLOCK64", 0, [1200, 1], 256, 22272)
    assert got(plan(driver, "step_cross", Lq=32, step_cross=1, gen=1, **base), "kernel") == ("CROSS_BLOCK64",)
    assert got(plan(driver, "step_cross", Lq=32, dkv=128, **base), *LAUNCH) == ("CROSS_BLOCK128", 0, [1200, 1], 256, 41216)


def test_block_cross_attention_64(driver):
    """LDS = (Lq * 132 + rows * (68 + 2 (Lq + 1)) + 4) * 4 against a 64-KB bar.
    Lq = 32: (4228 + 134 rows) * 4 — 10 rows 22272 (no chunking); 1000 rows over the bar, 64 rows 51216: 16 chunks of 64.
    Lq = 65, 100 rows: chunks of 32 (59936 bytes; 64 rows would take 85536).
    Lq = 256: (33796 + 582 rows) * 4 — 10 rows 158464 > 64 KB and even one row (137512) stays over the bar: the loop ends at
    one row per block, which the 160 KB of a CU still hold. Lq = 257: refused."""
    base = dict(Q=5, H=12)
    assert got(plan(driver, "cross_block", Lq=32, B=10, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [60, 1], 256, 22272, 0)
    assert got(plan(driver, "cross_block", Lq=32, B=1000, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [60, 16], 256, 51216, 64)
    assert got(plan(driver, "cross_block", Lq=65, B=100, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [60, 4], 256, 59936, 32)
    assert got(plan(driver, "cross_block", Lq=256, B=10, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK64", 0, [60, 10], 256, 137512, 1)
    assert plan(driver, "cross_block", Lq=257, B=10, **base)["invalid"] == 1


def test_block_cross_attention_128(driver):
    """LDS = (Lq * 260 + rows * (132 + 2 (Lq + 1)) + 4) * 4 against a 96-KB bar.
    Lq = 32: 10 rows 41216; 100 rows 112496 > 96 KB, 64 rows 83984: two chunks.
    Lq = 256, 10 rows: (66560 + 646 rows + 4) * 4 — one row is 268840 > 160 KB: one wave per (row, head) over the encoder
    rows instead, 2 * 10 * 12 = 240 waves = 60 blocks, no LDS."""
    base = dict(Q=2, H=12, dkv=128)
    assert got(plan(driver, "cross_block", Lq=32, B=10, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK128", 0, [24, 1], 256, 41216, 0)
    assert got(plan(driver, "cross_block", Lq=32, B=100, **base), *LAUNCH, "bchunk") == ("CROSS_BLOCK128", 0, [24, 2], 256, 83984, 64)
    assert got(plan(driver, "cross_block", Lq=256, B=10, **base), *LAUNCH, "bchunk") == ("CROSS_WAVE128", 0, [60, 1], 256, 0, 0)
    assert plan(driver, "cross_block", Lq=257, B=10, **base)["invalid"] == 1


def test_step_self_attention(driver):
    """One wave per (beam, head): 4 * 10 * 12 = 480 waves = 120 blocks, no dynamic LDS. 64-dim heads hold four keys per register
    group: t + 1 <= 8 / 16 / 24 / 32 / 36 keys take <2> / <4> / <6> / <8> / <9>, more the generic kernel. 128-dim heads hold two
    per group: <4> / <8> / <12> / <18>, then the generic kernel."""
    want = {8: "SELF_FAST2", 9: "SELF_FAST4", 16: "SELF_FAST4", 17: "SELF_FAST6", 24: "SELF_FAST6", 25: "SELF_FAST8", 32: "SELF_FAST8",
            33: "SELF_FAST9", 36: "SELF_FAST9", 37: "SELF_GENERIC"}
    for nk, kernel in want.items():
        assert got(plan(driver, "dec_self", Q=4, B=10, H=12, t=nk - 1), *LAUNCH) == (kernel, 0, [120, 1], 256, 0), nk
    want = {8: "SELF_FAST4_D128", 16: "SELF_FAST8_D128", 24: "SELF_FAST12_D128", 36: "SELF_FAST18_D128", 37: "SELF_GENERIC_D128"}
    for nk, kernel in want.items():
        assert got(plan(driver, "dec_self", Q=4, B=10, H=12, t=nk - 1, dkv=128), *LAUNCH) == (kernel, 0, [120, 1], 256, 0), nk
    assert plan(driver, "dec_self", Q=4, B=10, H=12, t=256, dkv=128)["invalid"] == 1     # 257 keys
    # the wave index is divided by B and by H by multiplication, exact below 2^32 / max(B, H): beam 1000 -> 4294967 items;
    # 357 * 1000 * 12 = 4284000 is inside, 358 * 1000 * 12 = 4296000 is refused
    assert got(plan(driver, "dec_self", Q=357, B=1000, H=12, t=3), "kernel", "invalid", "grid") == ("SELF_FAST2", 0, [1071000, 1])
    assert plan(driver, "dec_self", Q=358, B=1000, H=12, t=3)["invalid"] == 1


def enc_smem(Lq, D, stage_v=True):
    """enc_attn_kernel: K [Lq][D + 1], V [Lq][D] (unless read from global memory), 4 x Lq weights, 2 Lq bias floats,
    4 x 8 q rows of D, Lq mask words."""
    return (Lq * (D + 1) + (Lq * D if stage_v else 0) + 4 * Lq + 2 * Lq + 4 * 8 * D + Lq) * 4


def test_encoder_attention(driver):
    """Search encoder, 100 queries: at Lq <= 32 with a key mask a wave per (query, head), 100 * 3 = 300 blocks of four heads.
    Otherwise the VALU kernel, a block per (query, head) = 1200: (33 * 65 + 33 * 64 + 6 * 33 + 2048 + 33) * 4 = 26144 bytes at
    Lq = 33, (32 * 65 + 32 * 64 + 6 * 32 + 2048 + 32) * 4 = 25600 at Lq = 32."""
    assert enc_smem(33, 64) == 26144 and enc_smem(32, 64) == 25600
    base = dict(Q=100, H=12, buckets=32)
    for packed in (0, 1):
        assert got(plan(driver, "enc", Lq=32, mask=1, offs=packed, out_h=1, **base), *LAUNCH, "HB") == ("ENC_V2", 0, [300, 1], 256, TILE, 3)
    assert got(plan(driver, "enc", Lq=33, mask=1, **base), *LAUNCH) == ("ENC_VALU64", 0, [1200, 1], 256, 26144)
    for other in (dict(mask=1, causal=1), dict(mask=0), dict(mask=1, enc_mfma=0), dict(mask=1, gen=1)):
        assert got(plan(driver, "enc", Lq=32, **base, **other), *LAUNCH) == ("ENC_VALU64", 0, [1200, 1], 256, 25600), other
    assert plan(driver, "enc", Lq=32, mask=1, Q=100, H=12, buckets=65)["invalid"] == 1
    assert plan(driver, "enc", Lq=257, mask=1, **base)["invalid"] == 1


def test_training_forward_attention(driver):
    """256 sequences x 12 heads = 3072 waves = 768 blocks; per wave V [32][64] + 64 bias floats: 4 * 2112 * 4 = 33792 bytes.
    Longer sequences, packed rows or a plane output stay on the VALU kernel — never on the search encoder's tile, whose
    summation order differs."""
    base = dict(Q=256, H=12, buckets=32, mfma=1, mask=1)
    for causal in (0, 1):
        assert got(plan(driver, "enc", Lq=32, causal=causal, **base), *LAUNCH) == ("TRAIN_SELF_MFMA", 0, [768, 1], 256, 33792)
    assert got(plan(driver, "enc", Lq=33, **base), *LAUNCH) == ("ENC_VALU64", 0, [3072, 1], 256, 26144)
    assert got(plan(driver, "enc", Lq=32, offs=1, **base), *LAUNCH) == ("ENC_VALU64", 0, [3072, 1], 256, 25600)
    assert got(plan(driver, "enc", Lq=32, out_h=1, **base), *LAUNCH) == ("ENC_VALU64", 0, [3072, 1], 256, 25600)
    assert plan(driver, "enc", Lq=0, **base)["invalid"] == 1


def test_encoder_attention_128(driver):
    """128-dim heads: K [Lq][129] and V [Lq][128] in LDS while they fit 160 KB — Lq = 120: (15480 + 15360 + 720 + 4096 + 120) * 4
    = 143104; Lq = 256: 286720 with V, 155648 with K alone: V from global memory."""
    assert enc_smem(120, 128) == 143104 and enc_smem(256, 128) == 286720 and enc_smem(256, 128, False) == 155648
    base = dict(Q=7, H=32, buckets=32, mask=1, dkv=128)
    assert got(plan(driver, "enc", Lq=120, **base), *LAUNCH) == ("ENC_VALU128", 0, [224, 1], 256, 143104)
    assert got(plan(driver, "enc", Lq=256, **base), *LAUNCH) == ("ENC_VALU128_VG", 0, [224, 1], 256, 155648)
    assert got(plan(driver, "enc", Lq=32, mfma=1, **base), "kernel") == ("ENC_VALU128",)


def test_training_backward_attention(driver):
    """The launch is admitted by the VALU kernel's LDS, (4 Ls * 65 + 2 Ls (Ls + 1) + 64 + 5 Ls) * 4 = (2 Ls^2 + 267 Ls + 64) * 4
    <= 160 KB: Ls = 91 gives 40923 floats = 163692 bytes, Ls = 92 gives 41556 floats: refused. Ls <= 32: a wave per
    (sequence, head), two per block: 3072 / 2 = 1536 blocks of 128 threads, 2 * (3 * 2048 + 64 + 96 + 64 + 64) * 4 = 51456 bytes
    (15 waves: 8 blocks). Ls = 33: a block per (sequence, head), (8580 + 2244 + 64 + 165) * 4 = 44212 bytes."""
    base = dict(S=256, H=12, buckets=32)
    assert got(plan(driver, "bwd", Ls=32, **base), *LAUNCH) == ("TRAIN_BWD_MFMA", 0, [1536, 1], 128, 51456)
    assert got(plan(driver, "bwd", Ls=32, S=3, H=5, buckets=32), "kernel", "grid") == ("TRAIN_BWD_MFMA", [8, 1])
    assert got(plan(driver, "bwd", Ls=33, **base), *LAUNCH) == ("TRAIN_BWD_VALU", 0, [3072, 1], 256, 44212)
    assert got(plan(driver, "bwd", Ls=91, **base), *LAUNCH) == ("TRAIN_BWD_VALU", 0, [3072, 1], 256, 163692)
    assert 163692 <= 160 * KB < 41556 * 4
    assert plan(driver, "bwd", Ls=92, **base)["invalid"] == 1
    assert plan(driver, "bwd", Ls=32, S=256, H=12, buckets=65)["invalid"] == 1
    assert plan(driver, "bwd", Ls=0, **base)["invalid"] == 1
