"""not-gpu: the route of the training self-attention backward at 128-dim heads (t5-3b), as host arithmetic (ripor_amd/csrc/
attn_route.h compiled with the host compiler, like tests/test_attn_route.py). 128-dim heads go through the 64-column LDS rows of
the VALU kernel in two halves, so the carve — and with it the lengths admitted — is that of 64-dim heads: 91 is the last, 92 is
refused; the fp32-MFMA plan is a 64-dim tile and is never taken. Every plan at 64 stays what it was: the expected values below
are those of tests/test_attn_route.py and the formula of self_attn_bwd_smem, written out, not read from the planner."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 32, 33, 64, 91, 92]
S, H, BUCKETS = 256, 12, 32

_SRC = r"""
#include <cstdio>
#include "%(csrc)s/attn_route.h"
using namespace rpr;
static void row(const char* name, int Ls, int dkv, bool def, bool last) {
  SelfAttnBwdIn in{%(S)d, Ls, %(H)d, %(B)d};            // the four members every caller before this route filled
  if (!def) in.dkv = dkv;
  const AttnLaunch p = plan_self_attn_bwd(in);
  printf("\"%%s_%%d\": {\"kernel\": \"%%s\", \"invalid\": %%d, \"grid\": [%%u, %%u], \"block\": %%d, \"smem\": %%zu}%%s\n", name, Ls,
         attn_kernel_name(p.kernel), (int)p.invalid, p.grid_x, p.grid_y, p.block, p.smem, last ? "" : ",");
}
int main() {
  const int Ls[] = {%(lengths)s};
  const int n = sizeof(Ls) / sizeof(Ls[0]);
  printf("{\"default_dkv\": %%d, \"lds_max\": %%zu,\n", SelfAttnBwdIn().dkv, LDS_MAX);
  for (int i = 0; i < n; ++i) { row("d128", Ls[i], 128, false, false); row("d64", Ls[i], 64, false, false); row("default", Ls[i], 0, true, false); }
  row("d96", 8, 96, false, true);
  printf("}\n");
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("heads128_plan")
    src = d / "driver.cpp"
    src.write_text(_SRC % {"csrc": os.path.join(REPO, "ripor_amd", "csrc"), "S": S, "H": H, "B": BUCKETS,
                           "lengths": ", ".join(map(str, LENGTHS))})
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, str(src)], check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def _smem(Ls):
    """self_attn_bwd_kernel's carve: Q, K, V, dO [Ls][65], P and dS [Ls][Ls + 1], 64 bias slots, 5 Ls of diagonals / masks."""
    return 4 * (4 * Ls * 65 + 2 * Ls * (Ls + 1) + 64 + 5 * Ls)


def test_128_dim_heads_take_the_valu_kernel_at_every_admitted_length(plans):
    assert plans["lds_max"] == 160 * 1024
    for Ls in LENGTHS[:-1]:
        p = plans[f"d128_{Ls}"]
        assert p["invalid"] == 0 and p["kernel"] == "TRAIN_BWD_VALU128", (Ls, p)     # never the 64-dim MFMA tile
        assert p["grid"] == [S * H, 1] and p["block"] == 256
        assert p["smem"] == _smem(Ls) <= 160 * 1024
    assert plans["d128_91"]["smem"] == 163692
    assert plans["d128_92"]["invalid"] == 1 and _smem(92) > 160 * 1024
    assert all(plans[f"d128_{Ls}"]["kernel"] != "TRAIN_BWD_MFMA" for Ls in LENGTHS)
    assert plans["d96_8"]["invalid"] == 1                                             # 64 or 128, nothing else


def test_the_lengths_admitted_do_not_depend_on_the_head_dim(plans):
    for Ls in LENGTHS:
        assert plans[f"d128_{Ls}"]["invalid"] == plans[f"d64_{Ls}"]["invalid"] == (1 if Ls > 91 else 0)


def test_plans_at_64_are_what_they_were(plans):
    """Kernel, grid, block and LDS of tests/test_attn_route.py's table (S 256, H 12), with the head dim left at its default and
    named."""
    assert plans["default_dkv"] == 64
    mfma_lds = 2 * (3 * 32 * 64 + 64 + 96 + 64 + 64) * 4
    want = {1: ("TRAIN_BWD_MFMA", 0, [S * H // 2, 1], 128, mfma_lds), 32: ("TRAIN_BWD_MFMA", 0, [1536, 1], 128, 51456),
            33: ("TRAIN_BWD_VALU", 0, [3072, 1], 256, 44212), 64: ("TRAIN_BWD_VALU", 0, [3072, 1], 256, _smem(64)),
            91: ("TRAIN_BWD_VALU", 0, [3072, 1], 256, 163692)}
    assert mfma_lds == 51456
    for Ls, w in want.items():
        for which in ("default", "d64"):
            p = plans[f"{which}_{Ls}"]
            assert (p["kernel"], p["invalid"], p["grid"], p["block"], p["smem"]) == w, (which, Ls, p)
    assert plans["default_92"]["invalid"] == 1 and plans["d64_92"]["invalid"] == 1
