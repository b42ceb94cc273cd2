"""The layout of the training step (ripor_amd/csrc/train_layout.h), checked on the CPU.

tests/train_layout_driver.cpp includes the header and is compiled here with the host C++ compiler. Every expectation below
was worked out by hand from the formulas train_api.hip held before the layout was derived from one table of sub-blocks
(``Dims::enc_stride`` / ``dec_stride``, ``enc_act`` / ``dec_act``, the two switches of ``XtLayout``, the dY^T sizes of
``alloc_train``, the ``K_*`` lists of ``build_params`` and ``layer_numel``); the arithmetic is in the docstrings — none comes
from running the header. inner = heads x d_kv = 12 x 64 = 768 throughout, except where the last section says otherwise: the same
table names a model's weights for rpr_load_model and the forward passes (shapes, folded norms, the ABI's field of every slot)."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF, CROSS, FF = 0, 1, 2
# the parameter kinds as build_params numbered them
(K_SHARED, K_ENC_REL, K_DEC_REL, K_ENC_FLN, K_DEC_FLN, K_START, K_IN_EMB, K_OUT_EMB, K_XKV, K_ENC_LN0, K_ENC_QKV, K_ENC_O, K_ENC_LN1,
 K_ENC_WI, K_ENC_WO, K_DEC_LN0, K_DEC_QKV, K_DEC_O, K_DEC_LN1, K_DEC_XQ, K_DEC_XO, K_DEC_LN2, K_DEC_WI, K_DEC_WO) = range(24)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("train_layout") / "train_layout_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "train_layout_driver.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def layout(driver, **kw):
    argv = [driver] + [f"{k}={int(v)}" for k, v in kw.items()]
    return json.loads(subprocess.run(argv, check=True, capture_output=True, text=True).stdout)


BASE = dict(vocab=32128, buckets=32, H=12, dkv=64, dm=768, dff=3072, ne=12, nd=12, Lm=32, V=256)
MINI = dict(vocab=512, buckets=32, H=12, dkv=64, dm=768, dff=256, ne=2, nd=12, Lm=8, V=256)


def enc_expect(T, Tp, dm, inner, dff, layer, xt_layer, act_stride):
    """enc_act: x | qkv [T][3 inner] | attn [T][inner] | xm [T][dm] | ff [T][dff]; XtLayout::enc: qkv at 0, o at Tp dm, wi at
    Tp (dm + inner), wo at Tp (2 dm + inner). Per sub-block [x, in, mid, xt_in, xt_out]; the FF block has no mid (= in)."""
    a, o = layer * act_stride, layer * xt_layer
    return [[a, a + T * dm, a + T * (dm + 3 * inner), o, o + Tp * dm],
            [a + T * (dm + 4 * inner), a + T * (2 * dm + 4 * inner), a + T * (2 * dm + 4 * inner), o + Tp * (dm + inner), o + Tp * (2 * dm + inner)]]


def dec_expect(R, Rp, dm, inner, dff, layer, dec_off, xt_layer, act_stride):
    """dec_act: x0 | qkv [R][3 inner] | a0 [R][inner] | x1 | qx [R][inner] | a1 [R][inner] | x2 | ff [R][dff]; XtLayout::dec from
    dec_off + layer dec_layer: qkv 0, o Rp dm, xq Rp (dm + inner), xo Rp (2 dm + inner), wi Rp (2 dm + 2 inner), wo Rp (3 dm + 2 inner)."""
    a, o = layer * act_stride, dec_off + layer * xt_layer
    return [[a, a + R * dm, a + R * (dm + 3 * inner), o, o + Rp * dm],
            [a + R * (dm + 4 * inner), a + R * (2 * dm + 4 * inner), a + R * (2 * dm + 5 * inner), o + Rp * (dm + inner), o + Rp * (2 * dm + inner)],
            [a + R * (2 * dm + 6 * inner), a + R * (3 * dm + 6 * inner), a + R * (3 * dm + 6 * inner), o + Rp * (2 * dm + 2 * inner),
             o + Rp * (3 * dm + 2 * inner)]]


def test_header_is_host_only():
    """The driver's build proves that the header compiles with -Wall -Werror; it must not reach for a HIP header either."""
    src = open(os.path.join(REPO, "ripor_amd", "csrc", "train_layout.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert set(includes) <= {"<algorithm>", "<cmath>", "<cstddef>", "<vector>", '"../../include/ripor_hip.h"'}, includes


def test_sub_blocks_of_the_stacks(driver):
    """Encoder = {SELF, FF}, decoder = {SELF, CROSS, FF}; (n_in, k_out) = (3 inner, inner), (inner, inner), (d_ff, d_ff)."""
    y = layout(driver, bz=128, Lq=64, L=32, docs=2, **BASE)
    sub = lambda kind, n_in, k_out: dict(kind=kind, n_in=n_in, k_out=k_out)
    assert y["enc"]["sub"] == [sub(SELF, 2304, 768), sub(FF, 3072, 3072)]
    assert y["dec"]["sub"] == [sub(SELF, 2304, 768), sub(CROSS, 768, 768), sub(FF, 3072, 3072)]


def test_t5_base_batch_128(driver):
    """t5-base, bz 128, Lq 64, L 32, two docs: T = 128 * 64 = 8192, S = 256, R = 256 * 32 = 8192, both their own pad64.
    enc_stride = T (2 dm + 4 inner + d_ff) = 8192 * (1536 + 3072 + 3072) = 8192 * 7680 = 62914560;
    dec_stride = R (3 dm + 6 inner + d_ff) = 8192 * (2304 + 4608 + 3072) = 8192 * 9984 = 81788928.
    X^T: enc_layer = Tp (2 dm + inner + d_ff) = 8192 * 5376 = 44040192; xkv_off = 12 * 44040192 = 528482304; dec_off = xkv_off +
    Tp dm = 528482304 + 6291456 = 534773760; dec_layer = Rp (3 dm + 2 inner + d_ff) = 8192 * 6912 = 56623104; total = 534773760 +
    12 * 56623104 = 1214251008. The encoder's last stream sits behind its 12 layers: 12 * 62914560 = 754974720."""
    y = layout(driver, bz=128, Lq=64, L=32, docs=2, **BASE)
    assert y["dims"] == dict(S=256, R=8192, T=8192, inner=768, xld=12 * 2 * 768)
    enc, dec = y["enc"], y["dec"]
    assert (enc["rows"], enc["ld"], enc["act_stride"], enc["xt_stride"], enc["xt_base"]) == (8192, 8192, 62914560, 44040192, 0)
    assert (dec["rows"], dec["ld"], dec["act_stride"], dec["xt_stride"], dec["xt_base"]) == (8192, 8192, 81788928, 56623104, 534773760)
    assert (y["xt_xkv"], y["xt_total"]) == (528482304, 1214251008)
    assert enc["x_end"] == 754974720
    for i in range(12):
        assert enc["layer"][i]["at"] == enc_expect(8192, 8192, 768, 768, 3072, i, 44040192, 62914560), i
        assert dec["layer"][i]["at"] == dec_expect(8192, 8192, 768, 768, 3072, i, 534773760, 56623104, 81788928), i
    # spot values of the two switches, layer 3: encoder wi = 3 * 44040192 + 8192 * 1536; decoder xo = dec_off + 3 * 56623104 + 8192 * 2304
    assert enc["layer"][3]["at"][1][3] == 132120576 + 12582912 == 144703488
    assert dec["layer"][3]["at"][1][4] == 534773760 + 169869312 + 18874368 == 723517440


def test_padded_rows(driver):
    """d_model 768, d_ff 256, 2 + 12 layers, bz 3, Lq 14, L 8, two docs: T = 42, S = 6, R = 48; both pad to 64.
    enc_stride = 42 * (1536 + 3072 + 256) = 42 * 4864 = 204288; dec_stride = 48 * (2304 + 4608 + 256) = 48 * 7168 = 344064.
    X^T: enc_layer = 64 * (1536 + 768 + 256) = 64 * 2560 = 163840; xkv_off = 2 * 163840 = 327680; dec_off = 327680 + 64 * 768 =
    376832; dec_layer = 64 * (2304 + 1536 + 256) = 64 * 4096 = 262144; total = 376832 + 12 * 262144 = 3522560.
    dY^T of a layer's group, n_in + d_model rows of ldT per sub-block: decoder (3 dm + d_ff + 4 inner) Rp = 5632 * 64 = 360448,
    encoder (2 dm + d_ff + 3 inner) Tp = 4096 * 64 = 262144, cross K/V xld Tp = 12 * 2 * 768 * 64 = 18432 * 64 = 1179648: the
    largest, so WGradSide::create gets 2 * 1179648 + 2048 = 2361344 bytes."""
    y = layout(driver, bz=3, Lq=14, L=8, docs=2, **MINI)
    assert y["dims"] == dict(S=6, R=48, T=42, inner=768, xld=18432)
    enc, dec = y["enc"], y["dec"]
    assert (enc["rows"], enc["ld"], enc["act_stride"], enc["xt_stride"], enc["xt_base"]) == (42, 64, 204288, 163840, 0)
    assert (dec["rows"], dec["ld"], dec["act_stride"], dec["xt_stride"], dec["xt_base"]) == (48, 64, 344064, 262144, 376832)
    assert (y["xt_xkv"], y["xt_total"]) == (327680, 3522560)
    assert (dec["dyT_elems"], enc["dyT_elems"], y["dyT_xkv"], y["dyT_max"]) == (360448, 262144, 1179648, 1179648)
    assert 2 * y["dyT_max"] + 8 * 256 == 2361344
    assert enc["x_end"] == 2 * 204288
    for i in range(2):
        assert enc["layer"][i]["at"] == enc_expect(42, 64, 768, 768, 256, i, 163840, 204288), i
    for i in range(12):
        assert dec["layer"][i]["at"] == dec_expect(48, 64, 768, 768, 256, i, 376832, 262144, 344064), i


def mini_params(own_out):
    """build_params for the mini model (vocab 512, 32 buckets x 12 heads, L 8, V 256): [(kind, layer, numel)] in order."""
    dm, inner, dff = 768, 768, 256
    p = [(K_SHARED, -1, 512 * dm), (K_ENC_REL, -1, 32 * 12), (K_DEC_REL, -1, 32 * 12), (K_ENC_FLN, -1, dm), (K_DEC_FLN, -1, dm),
         (K_START, -1, dm), (K_IN_EMB, -1, 8 * 256 * dm)]
    if own_out:
        p.append((K_OUT_EMB, -1, 8 * 256 * dm))
    p.append((K_XKV, -1, 12 * 2 * inner * dm))
    for i in range(2):
        p += [(K_ENC_LN0, i, dm), (K_ENC_QKV, i, 3 * inner * dm), (K_ENC_O, i, dm * inner), (K_ENC_LN1, i, dm), (K_ENC_WI, i, dff * dm),
              (K_ENC_WO, i, dm * dff)]
    for i in range(12):
        p += [(K_DEC_LN0, i, dm), (K_DEC_QKV, i, 3 * inner * dm), (K_DEC_O, i, dm * inner), (K_DEC_LN1, i, dm), (K_DEC_XQ, i, inner * dm),
              (K_DEC_XO, i, dm * inner), (K_DEC_LN2, i, dm), (K_DEC_WI, i, dff * dm), (K_DEC_WO, i, dm * dff)]
    return p


@pytest.mark.parametrize("own_out", (1, 0))
def test_flat_parameter_order(driver, own_out):
    """The order rpr_param_info and the checkpoints see, with separate and with shared codebooks (K_OUT_EMB absent).
    In front of the layers: 512 * 768 + 2 * 384 + 3 * 768 + 1572864 (+ 1572864) + 14155776 = 16124928 (17697792 with the
    output codebooks). An encoder layer holds 768 + 1769472 + 589824 + 768 + 196608 + 196608 = 2754048 elements, a decoder
    layer 768 + 1769472 + 589824 + 768 + 589824 + 589824 + 768 + 196608 + 196608 = 3934464; a layer's bucket is K_*_LN0 up
    to the end of K_*_WO, i.e. the whole layer; the last bucket is everything in front of encoder layer 0."""
    y = layout(driver, bz=3, Lq=14, L=8, docs=2, own_out=own_out, **MINI)
    want, off = [], 0
    for kind, layer, numel in mini_params(own_out):
        want.append([kind, layer, numel, off])
        off += numel
    front = 16124928 + (1572864 if own_out else 0)
    assert off == front + 2 * 2754048 + 12 * 3934464
    assert y["params"] == want
    assert y["params_total"] == off and y["index_ok"] == 1
    assert y["first_bucket"] == [0, front]
    globals_ = 9 if own_out else 8
    for i in range(2):
        assert y["enc"]["layer"][i]["bucket"] == [front + i * 2754048, 2754048], i
        assert y["enc"]["layer"][i]["first_param"] == globals_ + 6 * i
    for i in range(12):
        assert y["dec"]["layer"][i]["bucket"] == [front + 2 * 2754048 + i * 3934464, 3934464], i
        assert y["dec"]["layer"][i]["first_param"] == globals_ + 12 + 9 * i


def test_one_doc_per_query(driver):
    """The seq2seq step: docs = 1, S = bz. t5-base, bz 5, Lq 20, L 8: T = 100 (pads to 128), R = 5 * 8 = 40 (pads to 64).
    enc_stride = 100 * 7680 = 768000; dec_stride = 40 * 9984 = 399360; enc_layer = 128 * 5376 = 688128; xkv_off = 12 * 688128 =
    8257536; dec_off = 8257536 + 128 * 768 = 8355840; dec_layer = 64 * 6912 = 442368; total = 8355840 + 12 * 442368 = 13664256.
    dY^T: decoder (2304 + 3072 + 3072) * 64 = 540672, encoder (1536 + 3072 + 2304) * 128 = 884736, cross K/V 18432 * 128 = 2359296."""
    y = layout(driver, bz=5, Lq=20, L=8, docs=1, **BASE)
    assert y["dims"] == dict(S=5, R=40, T=100, inner=768, xld=18432)
    enc, dec = y["enc"], y["dec"]
    assert (enc["rows"], enc["ld"], enc["act_stride"], enc["xt_stride"]) == (100, 128, 768000, 688128)
    assert (dec["rows"], dec["ld"], dec["act_stride"], dec["xt_stride"], dec["xt_base"]) == (40, 64, 399360, 442368, 8355840)
    assert (y["xt_xkv"], y["xt_total"]) == (8257536, 13664256)
    assert (dec["dyT_elems"], enc["dyT_elems"], y["dyT_xkv"]) == (540672, 884736, 2359296)
    assert enc["layer"][11]["at"] == enc_expect(100, 128, 768, 768, 3072, 11, 688128, 768000)
    assert dec["layer"][11]["at"] == dec_expect(40, 64, 768, 768, 3072, 11, 8355840, 442368, 399360)


# ---- the model's weights as the loader and the forward passes get them (ParamOrder::weight, ParamOrder::fill) ---------------
WIDE = dict(vocab=512, buckets=32, H=32, dkv=128, dm=1024, dff=16384, ne=2, nd=3, Lm=8, V=256)
# per stack and sub-block: W_in [N, K], its elements, the folded norm (position of the sub-block's ln in the layer), W_out [N, K],
# its elements. t5-base: inner = 12 * 64 = 768 = d_model, 3 inner = 2304; 2304 * 768 = 1769472, 768 * 768 = 589824, 3072 * 768 = 2359296.
BASE_WEIGHTS = dict(enc=[((2304, 768), 1769472, 0, (768, 768), 589824), ((3072, 768), 2359296, 3, (768, 3072), 2359296)],
                    dec=[((2304, 768), 1769472, 0, (768, 768), 589824), ((768, 768), 589824, 3, (768, 768), 589824),
                         ((3072, 768), 2359296, 6, (768, 3072), 2359296)])
# inner = 32 * 128 = 4096 != d_model = 1024, 3 inner = 12288: 12288 * 1024 = 12582912, 4096 * 1024 = 4194304, 16384 * 1024 = 16777216
WIDE_WEIGHTS = dict(enc=[((12288, 1024), 12582912, 0, (1024, 4096), 4194304), ((16384, 1024), 16777216, 3, (1024, 16384), 16777216)],
                    dec=[((12288, 1024), 12582912, 0, (1024, 4096), 4194304), ((4096, 1024), 4194304, 3, (1024, 4096), 4194304),
                         ((16384, 1024), 16777216, 6, (1024, 16384), 16777216)])


@pytest.mark.parametrize("model,want", ((BASE, BASE_WEIGHTS), (WIDE, WIDE_WEIGHTS)), ids=("t5_base", "inner_4096_dm_1024"))
def test_weights_of_every_sub_block(driver, model, want):
    """W_in [n_in, d_model] carries the ln of its own sub-block, W_out [d_model, k_out] nothing: enc_qkv: ln0, enc_wi: ln1,
    dec_qkv: ln0, dec_xq: ln1, dec_wi: ln2. With codebooks of their own 9 tensors stand in front of the layers; encoder layer i
    starts at slot 9 + 6 i, decoder layer i at 9 + 6 ne + 9 i; sub-block j holds (ln, W_in, W_out) at 3 j, 3 j + 1, 3 j + 2."""
    y = layout(driver, bz=1, Lq=1, L=1, docs=1, **model)
    for stack, first, per_layer, layers in (("enc", 9, 6, model["ne"]), ("dec", 9 + 6 * model["ne"], 9, model["nd"])):
        assert len(y["weights"][stack]) == layers
        for i, layer in enumerate(y["weights"][stack]):
            base = first + per_layer * i
            assert len(layer) == len(want[stack])
            for j, (got, (nk_in, numel_in, ln_at, nk_out, numel_out)) in enumerate(zip(layer, want[stack])):
                assert ln_at == 3 * j
                assert got == dict(ln=base + ln_at, w_in=[base + 3 * j + 1, numel_in, *nk_in, base + ln_at],
                                   w_out=[base + 3 * j + 2, numel_out, *nk_out, -1]), (stack, i, j)
                assert y["params"][got["w_in"][0]][2] == numel_in and y["params"][got["w_out"][0]][2] == numel_out


# the per-layer fields of rpr_model_desc in the order of include/ripor_hip.h, which is the order of the layer kinds
FIELDS = ["enc_ln0", "enc_qkv", "enc_o", "enc_ln1", "enc_wi", "enc_wo",
          "dec_ln0", "dec_qkv", "dec_o", "dec_ln1", "dec_xq", "dec_xo", "dec_ln2", "dec_wi", "dec_wo"]
FIELD_KIND = dict(zip(FIELDS, (K_ENC_LN0, K_ENC_QKV, K_ENC_O, K_ENC_LN1, K_ENC_WI, K_ENC_WO, K_DEC_LN0, K_DEC_QKV, K_DEC_O, K_DEC_LN1,
                               K_DEC_XQ, K_DEC_XO, K_DEC_LN2, K_DEC_WI, K_DEC_WO)))


def test_every_layer_slot_points_into_its_field(driver):
    """Two encoder and three decoder layers: slot (kind, layer) holds element `layer` of the field of that kind, 6 * 2 + 9 * 3 = 39
    slots in the order of the layers."""
    f = layout(driver, **MINI)["fields"]
    assert f["fill_ok"] == 1 and f["globals_ok"] == 1
    want = [[FIELD_KIND[name], i, FIELDS.index(name), i] for i in range(2) for name in FIELDS[:6]]
    want += [[FIELD_KIND[name], i, FIELDS.index(name), i] for i in range(3) for name in FIELDS[6:]]
    assert len(want) == 39 and f["slots"] == want


@pytest.mark.parametrize("field", FIELDS)
def test_a_null_entry_is_reported(driver, field):
    """The last element of every field in turn (encoder: layer 1, decoder: layer 2), and the field's whole array."""
    k = FIELDS.index(field)
    for elem in (1 if k < 6 else 2, 0, -1):
        f = layout(driver, null_field=k, null_elem=elem, **MINI)["fields"]
        assert f["fill_ok"] == 0, (field, elem)
        assert len(f["slots"]) == (38 if elem >= 0 else 39 - (2 if k < 6 else 3))
