"""not-gpu: where the 16x16x32 form of the 256 x 256 split-precision GEMM can appear, as host arithmetic (ripor_amd/csrc/search_plan.h,
gemm_route.h compiled with the host compiler, like tests/test_search_plan.py): the ctx setting (rpr_set_gemm_mfma16) is part of a
search's plan and so of its graph key; a (tail-pass) launch carries the flag only on the ping-pong step of a split-precision plan — never on
bf16 (training) launches, split-K launches, the row-split remainder or the small-tile kernels, and never without being asked."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <cstdio>
#include "%(csrc)s/search_plan.h"
#include "%(csrc)s/gemm_route.h"
using namespace rpr;
static SearchPlan plan(int mfma16, int precision, bool f32_only) {
  SearchSettings s; s.gemm_mfma16 = mfma16; s.precision = precision; s.forced_tail = 0;
  SearchModel m; m.V = 256; m.f32_only = f32_only;
  SearchCall a; a.Q = 8; a.Lq = 16; a.B = 4; a.L = 8;
  return plan_search(s, m, a, [] { return TrieStats{nullptr, nullptr}; });
}
static void steps(const char* name, GemmRouteIn in, bool last = false) {
  GemmTuning t;
  const GemmPlan p = plan_gemm_h2(in, t);
  printf("\"%%s\": [", name);
  for (int i = 0; i < p.n; ++i)
    printf("%%s[%%d, %%d, %%d, %%d]", i ? ", " : "", p.step[i].family == GEMM_PP, (int)p.step[i].m16, (int)p.step[i].bf16, p.step[i].ksplit);
  printf("]%%s\n", last ? "" : ",");
}
int main() {
  printf("{\"default_setting\": %%d,\n", SearchSettings().gemm_mfma16);
  printf("\"plan_on\": %%d, \"plan_off\": %%d, \"plan_f32\": %%d, \"plan_f32_only\": %%d, \"plain_plan\": %%d,\n", plan(1, RPR_PREC_F16X2, false).mfma16,
         plan(0, RPR_PREC_F16X2, false).mfma16, plan(1, RPR_PREC_F32, false).mfma16, plan(1, RPR_PREC_F16X2, true).mfma16, plain_plan(8, 16, 1, 1).mfma16);
  printf("\"key_differs\": %%d, \"key_same\": %%d,\n", (int)!(plan(1, RPR_PREC_F16X2, false) == plan(0, RPR_PREC_F16X2, false)),
         (int)(plan(1, RPR_PREC_F16X2, false) == plan(1, RPR_PREC_F16X2, false)));
  GemmRouteIn big; big.M = 10752; big.N = 2304; big.K = 768; big.cus = 128; big.part = true; big.mid_split = true; big.part_cap = (size_t)9 << 20;
  GemmRouteIn on = big; on.mfma16 = true;
  steps("search_on", on); steps("search_off", big);
  GemmRouteIn split = on; split.M = 27000; split.N = 768; split.cus = 0;             // 318 tiles: ping-pong rows + a 128-row remainder
  steps("row_split_on", split);
  GemmRouteIn small = on; small.M = 640; steps("small_on", small);                    // mid-size: split-K / wave-split kernels
  GemmRouteIn forced = big; forced.M = 300; forced.force_pp = true; steps("l0_table", forced);   // the table's launch: never flagged
  GemmRouteIn bf = on; bf.bf16 = true; bf.M = 16384; bf.mid_split = false; bf.split_n = bf.N; steps("bf16_flagged", bf);
  GemmRouteIn wg = big; wg.M = 768; wg.N = 3072; wg.K = 8192; wg.cus = 0; wg.mid_split = false; wg.part_cap = (size_t)64 << 20; wg.split_n = wg.N;
  steps("train_wgrad", wg);                                                           // training: split-K through the ping-pong kernel
  GemmRouteIn wgf = wg; wgf.mfma16 = true; steps("splitk_flagged", wgf, true);
  printf("}\n");
}
"""


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("mfma16_plan")
    src = d / "driver.cpp"
    src.write_text(_SRC % {"csrc": os.path.join(REPO, "ripor_amd", "csrc")})
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, str(src)], check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def test_the_setting_is_part_of_the_graph_key(facts):
    assert facts["default_setting"] == 1
    assert facts["plan_on"] == 1 and facts["plan_off"] == 0
    assert facts["key_differs"] == 1 and facts["key_same"] == 1
    # exact fp32 (asked for, or forced by weights that do not fit the planes) has no split-precision launches to flag;
    # the plan of a call that only sizes buffers (rpr_encode, the training step) never carries it
    assert facts["plan_f32"] == 0 and facts["plan_f32_only"] == 0 and facts["plain_plan"] == 0


def test_only_the_ping_pong_step_of_a_flagged_plan_changes_shape(facts):
    # rows: [ping-pong family, m16, bf16, ksplit]
    assert facts["search_on"] == [[1, 1, 0, 1]] and facts["search_off"] == [[1, 0, 0, 1]]
    assert facts["row_split_on"] == [[1, 1, 0, 1], [0, 0, 0, 1]]           # the 128-row remainder keeps its kernel
    assert facts["small_on"] and all(s[1] == 0 for s in facts["small_on"])
    assert facts["l0_table"] == [[1, 0, 0, 1]]                             # the layer-0 table is made on 32x32x16


def test_training_and_grouped_plans_never_carry_the_flag(facts):
    """The training step never sets GemmH2Args::mfma16 (its Launcher leaves it 0; the grouped kernel has no such argument
    and compiles M16 = false); the planner refuses it for bf16 and for split-K ping-pong launches even when it is set."""
    assert facts["train_wgrad"] and all(s[1] == 0 for s in facts["train_wgrad"])
    assert any(s[0] == 1 and s[3] > 1 for s in facts["train_wgrad"])       # (the weight-gradient split-K route was taken)
    assert facts["bf16_flagged"] and all(s[1] == 0 and s[2] == 1 for s in facts["bf16_flagged"])
    assert facts["splitk_flagged"] == facts["train_wgrad"]
