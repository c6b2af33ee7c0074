"""Host-side half of the bit-exact tests of the first-layer kernels (yolo_conv1_nchw_f32_fwd, its stride-2 form,
yolo_conv1_pool_nchw_f32_fwd), the depthwise kernels (yolo_dwconv3x3_fwd, yolo_dwconv_fwd, yolo_dwconv_f32_fwd) and squeeze-and-excitation
(yolo_se_fwd, yolo_se_f32_fwd) - no GPU.  Every case of the tables in tests/_exact_cases.py has a reference that determines every bit and
exercises the rounding (the references of tests/helpers.py reject it otherwise, so the GPU file can never meet a rejected case), and the
reference alone tells a subtly wrong kernel from a right one: one perturbed reference per failure class, each must change at least
1 % of the outputs.  tests/test_pointwise_exact_gpu.py launches the same tables and takes the tensors from the same cache."""
import ctypes

import pytest
import torch

import _exact_cases as E
from helpers import (dw_geometry, exact_dw, exact_dw_reference, exact_first_layer, exact_rounding_shares, exact_se,
                     first_layer_reference, se_means_reference, se_rescale_reference, se_scales_reference)

BF16, F32 = torch.bfloat16, torch.float32
FIRST_IDS = [E.first_id(s) for s, _ in E.FIRST_CASES]
DW3_IDS = ["n%d_c%d_%dx%d_s%d" % (shape + (stride,)) for shape, _, stride in E.DW3_ROWS]
DW_ROWS, DW_F32_ROWS = E.dw_rows(), E.dw_f32_rows()
DW_IDS = ["k%d_s%d_%dx%d_%s_c%d" % r[:6] for r in DW_ROWS]
DW_F32_IDS = ["k%d_s%d_%dx%d_%s_c%d" % r[:6] for r in DW_F32_ROWS]
SE_ROWS = [(s, BF16) for s in E.SE_CASES] + [(s, F32) for s in E.SE_F32_CASES]
SE_IDS = ["n%d_%dx%d_c%d_sq%d_" % s + ("bf16" if t == BF16 else "f32") for s, t in SE_ROWS]


def _differs(a, b):
    assert a.shape == b.shape
    return float((a.float() != b.float()).float().mean())


# ---- first-layer kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", E.FIRST_CASES, ids=FIRST_IDS)
def test_first_layer_reference_conditions(shape, seed):
    """first_layer_reference's guards pass: >= 50 % of the caller's float32 x needs rounding to bf16 and >= 10 % are exact ties; the fp32
    conv of bf16(x) equals the fp64 conv; >= 15 % negative pre-activations (LeakyReLU) / >= 2 % at each clamp (ReLU6); >= 25 % of the
    outputs need rounding, >= 2 % are ties."""
    x, wt, bias, y, stats = exact_first_layer(shape, seed)
    n, cin, h, w, cout, stride, act, pool = shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert y.dtype == BF16 and y.shape == ((n, cout, ho // 2, wo // 2) if pool else (n, cout, ho, wo)) and bool(torch.isfinite(y.float()).all())
    assert stats["x_nonrep"] >= 0.50 and stats["x_ties"] >= 0.10 and stats["out_nonrep"] >= 0.25 and stats["out_ties"] >= 0.02
    assert not torch.equal(x.to(BF16).float(), x)
    if act == "leaky":
        assert stats["s0_negative"] >= 0.15
    if act == "relu6":
        assert min(stats["s0_at0"], stats["s0_at6"]) >= 0.02


@pytest.mark.parametrize("shape,seed", E.FIRST_CASES, ids=FIRST_IDS)
def test_first_layer_reference_notices_how_x_is_narrowed(shape, seed):
    """x truncated to bf16 instead of rounded to nearest even, and x not narrowed at all (a kernel that multiplied the float32 pixels):
    each changes at least 1 % of the outputs of every case."""
    x, wt, bias, y, _ = exact_first_layer(shape, seed)
    for narrow in ("trunc", "wide"):
        y2, _ = first_layer_reference(x, wt, bias, stride=shape[5], act=shape[6], pool=shape[7], narrow=narrow)
        assert _differs(y, y2) >= 0.01, narrow


def test_first_layer_cases_cover_every_instantiation():
    """conv1_nchw_kernel<COUT, POOL, CINR>: cout {16, 32} x pool x (cin_real 3 | generic, by 1 and by 8 channels), each on the map of
    two tile rows and a group of three plus a group of one tile; conv1_s2_nchw_kernel<CINR>: cin_real 3 and 1, both activations, odd and
    even edges, wo = 82 (five tiles and one)."""
    s1 = {(s[4], s[7], s[1]) for s, _ in E.FIRST_S1_CASES if s[2:4] == (19, 50)}
    assert s1 == {(co, p, ci) for co in (16, 32) for p in (False, True) for ci in (3, 1, 8)}
    assert {s[6] for s, _ in E.FIRST_S1_CASES} == {"leaky", "relu6", "none"}
    assert any(s[2:4] == (2, 2) and s[7] for s, _ in E.FIRST_S1_CASES) and any(s[2:4] == (2, 2) and not s[7] for s, _ in E.FIRST_S1_CASES)
    assert {s[2:4] for s, _ in E.FIRST_S1_CASES if s[7]} >= {(21, 35)}
    s2 = {(s[1], s[2], s[3], s[6]) for s, _ in E.FIRST_S2_CASES}
    assert s2 == {(ci, h, w, a) for ci in (3, 1) for h, w in ((35, 163), (36, 164)) for a in ("relu6", "leaky")}
    assert all((s[3] - 1) // 2 + 1 == 82 and s[4] == 32 and s[0] == 2 for s, _ in E.FIRST_S2_CASES)
    assert len({seed for _, seed in E.FIRST_CASES}) == len(E.FIRST_CASES)


# ---- depthwise kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", E.DW_ACTS)
@pytest.mark.parametrize("nchw,seed,stride", E.DW3_ROWS, ids=DW3_IDS)
def test_dwconv3x3_reference_conditions(nchw, seed, stride, act):
    """exact_dw_reference's guards pass for every row of the yolo_dwconv3x3_fwd table with every exact activation."""
    x, wt, bias, ho, wo, pad, y, stats = exact_dw(E.dw3_shape(nchw, stride, act), seed, BF16, "torch")
    n, c, h, w = nchw
    assert pad == 1 and (ho, wo) == ((h - 1) // stride + 1, (w - 1) // stride + 1) and y.shape == (n, c, ho, wo) and y.dtype == BF16
    assert stats["nonrep"] >= 0.25 and stats["ties"] >= 0.02
    assert min(stats["at0"], stats["at6"]) >= 0.02 if act == "relu6" else stats["negative"] >= 0.15


@pytest.mark.parametrize("act", E.DW_ACTS)
@pytest.mark.parametrize("row", DW_ROWS, ids=DW_IDS)
def test_dwconv_reference_conditions(row, act):
    """... and for every row of the yolo_dwconv_fwd table: the padded input the reference builds by hand gives ho x wo outputs."""
    k, stride, h, w, geometry, c, seed = row
    x, wt, bias, ho, wo, pad, y, stats = exact_dw((2, c, h, w, k, stride, act), seed, BF16, geometry)
    assert y.shape == (2, c, ho, wo) and y.dtype == BF16 and stats["nonrep"] >= 0.25 and stats["ties"] >= 0.02
    assert min(stats["at0"], stats["at6"]) >= 0.02 if act == "relu6" else stats["negative"] >= 0.15


@pytest.mark.parametrize("row", DW_F32_ROWS, ids=DW_F32_IDS)
def test_dwconv_f32_reference_conditions(row):
    """The float32 table: the conv of eleven-bit integers times {-1, 0, 1} is exact in fp32, and x itself is NOT representable in bf16 (a
    kernel that narrowed an operand would lose low bits)."""
    k, stride, h, w, geometry, c, seed = row
    for act in E.DW_ACTS:
        x, wt, bias, ho, wo, pad, y, stats = exact_dw((2, c, h, w, k, stride, act), seed, F32, geometry)
        assert y.shape == (2, c, ho, wo) and y.dtype == F32
        assert exact_rounding_shares(x, BF16)[0] > 0.5
        assert c % 4 == 0 and c % 8 != 0


def test_dwconv_tables_cover_the_geometries():
    """Both kernel sizes and strides on even, odd and one-pixel maps; torch's pad k // 2 wherever it is another geometry than "same"
    (even maps at stride 2); leading pads 0, 1 and 2; c = 8 and 24."""
    geos = {r[:5] for r in DW_ROWS}
    assert {(k, s, h, w) for k, s, h, w, _ in geos} == {(k, s, h, w) for k in (3, 5) for s in (1, 2) for h, w in ((6, 8), (7, 9), (1, 1))}
    assert {g[:4] for g in geos if g[4] == "torch"} == {(3, 2, 6, 8), (5, 2, 6, 8)}
    assert {dw_geometry(h, w, k, s, geo)[2] for k, s, h, w, geo in geos} == {0, 1, 2}
    assert {r[5] for r in DW_ROWS} == {8, 24} and {r[:5] for r in DW_F32_ROWS} == geos
    # the strip kernel's table: a last strip of one row, h below the strip, odd and even h at stride 2, three channel groups, two images
    shapes = [s for s, _ in E.DW3_CASES]
    assert any(h % 8 == 1 and h > 8 for _, _, h, _ in shapes) and any(h < 8 for _, _, h, _ in shapes) and any(c == 24 for _, c, _, _ in shapes)
    assert {h % 2 for _, _, h, _ in shapes if h > 1} == {0, 1} and sum(n == 2 for n, _, _, _ in shapes) >= 4


def _dw3_fault(nchw, seed, stride, act, fault):
    x, wt, bias, ho, wo, pad, y, _ = exact_dw(E.dw3_shape(nchw, stride, act), seed, BF16, "torch")
    y2, _ = exact_dw_reference(x, wt, bias, stride=stride, pad=pad, ho=ho, wo=wo, act=act, dtype=BF16, fault=fault)
    return y, y2


def test_dwconv3x3_reference_notices_a_tap_lost_at_a_strip_edge():
    """The tap below the centre lost on the last row of every 8-row strip: changes >= 1 % of the outputs of at least one row of the
    table, only in rows 7, 15, ..., and every row of the table that HAS a strip edge inside the map notices it."""
    worst = 0.0
    for nchw, seed, stride in E.DW3_ROWS:
        ho = (nchw[2] - 1) // stride + 1
        y, y2 = _dw3_fault(nchw, seed, stride, "leaky", "drop_tap_row")
        bad = (y.float() != y2.float()).nonzero()
        assert bool((bad[:, 2] % 8 == 7).all())
        if ho > 8:
            assert len(bad), (nchw, stride)
        worst = max(worst, _differs(y, y2))
    assert worst >= 0.01


def test_dwconv3x3_reference_notices_the_next_images_row():
    """The row below an image's last row taken from the next image (what a kernel reads that bounds the row index by n * h instead of
    h): changes >= 1 % of the outputs of at least one row of the table, only in the last output row of the images before the last.
    (At stride 2 an even h has no row below the last window.)"""
    worst = 0.0
    for nchw, seed, stride in E.DW3_ROWS:
        n, c, h, w = nchw
        ho = (h - 1) // stride + 1
        if n < 2 or (ho - 1) * stride + 2 - 1 < h:
            continue
        y, y2 = _dw3_fault(nchw, seed, stride, "none", "next_image_row")
        bad = (y.float() != y2.float()).nonzero()
        assert len(bad) and bool((bad[:, 2] == ho - 1).all()) and bool((bad[:, 0] < n - 1).all()), (nchw, stride)
        worst = max(worst, _differs(y, y2))
    assert worst >= 0.01


def test_dwconv3x3_reference_notices_relu_treated_as_no_activation():
    """What yolo_dwconv3x3_fwd did with YOLO_ACT_RELU before it applied every activation: >= 1 % of the outputs of EVERY row."""
    for nchw, seed, stride in E.DW3_ROWS:
        y, y2 = _dw3_fault(nchw, seed, stride, "relu", "relu_as_none")
        assert _differs(y, y2) >= 0.01, (nchw, stride)
        assert bool((y2.float()[y.float() != y2.float()] < 0).all())


def test_dwconv3x3_rejects_an_unknown_activation_without_a_gpu():
    """(The check itself is part of test_argument_errors_are_reported_without_a_gpu; here: every value of the enum passes it and reaches
    the next argument check.)"""
    from pytorch_yolo_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for act in (_lib.ACT_NONE, _lib.ACT_LEAKY01, _lib.ACT_RELU6, _lib.ACT_RELU, _lib.ACT_SWISH):
        assert lib.yolo_dwconv3x3_fwd(p, p, p, p, 1, 4, 4, 8, 8, 0, 7, 7, 8, 0, 1, act, None) == -1 and b"bad output size" in lib.yolo_last_error()
    for act in (-1, 5):
        assert lib.yolo_dwconv3x3_fwd(p, p, p, p, 1, 4, 4, 8, 8, 0, 4, 4, 8, 0, 1, act, None) == -1 and b"activation" in lib.yolo_last_error()


# ---- squeeze-and-excitation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", SE_ROWS, ids=SE_IDS)
def test_se_references(shape, dtype):
    """The operands determine the means (integer x, exact partial sums), float32 x is not representable in bf16, and the bound on the
    scales is a bound: a float32 evaluation of the two FCs on this CPU lies within it.  It is a worst-case bound, linear in c and sq:
    below 1e-4 up to c = 128, 3.9e-3 for c = 1152 and sq = 64 - under half of the 1e-2 of the tolerance tests everywhere."""
    n, h, w, c, sq = shape
    x, w1, b1, w2, b2, means = exact_se(shape, E.SE_SEED, dtype)
    assert means.shape == (n, c) and means.dtype == F32 and c % (8 if dtype == BF16 else 4) == 0
    assert torch.equal(x.to(dtype).float(), x) and (dtype == BF16 or exact_rounding_shares(x, BF16)[0] > 0.5)
    scale, bound = se_scales_reference(means, w1, b1, w2, b2)
    assert 0.0 < float(bound.min()) and float(bound.max()) < (1e-4 if c <= 128 else 5e-3)
    assert 0.001 < float(scale.min()) and float(scale.max()) < 0.999 and float(scale.std()) > 0.05    # (no saturated sigmoid: the scales matter)
    v = means @ w1.t() + b1
    got = torch.sigmoid((v * torch.sigmoid(v)) @ w2.t() + b2)
    assert got.dtype == F32 and bool(((got.double() - scale).abs() <= bound).all())
    y = se_rescale_reference(x, got, dtype)
    assert y.dtype == dtype and y.shape == x.shape
    if dtype == BF16:
        nonrep, ties = exact_rounding_shares(x * got.view(n, c, 1, 1), BF16)
        assert nonrep >= 0.25                                                                         # the rescale's narrowing rounds


def test_se_means_tell_a_multiply_from_a_division():
    """sum * (1 / hw) and sum / hw differ in the last bit on a share of the channels wherever hw is no power of two: the bit-equal
    comparison of the means pins which one each kernel uses."""
    seen = 0
    for shape, dtype in SE_ROWS:
        x = exact_se(shape, E.SE_SEED, dtype)[0]
        a, b = se_means_reference(x, BF16), se_means_reference(x, F32)
        hw = shape[1] * shape[2]
        if hw & (hw - 1) == 0:
            assert torch.equal(a, b)
        else:
            seen += int(not torch.equal(a, b))
    assert seen >= 8


def test_se_cases_reach_every_group_width():
    """cgb = the power of two <= min(chunks, 32) (yolo_se_fwd): 1, 2, 4, 8, 16, 32, with a partial last group; pixel ranges: the split
    rule of yolo_se_fwd / yolo_se_f32_fwd repeated by hand (as many doublings as keep n * groups * splits < 512 and >= 256 pixels)."""
    for cases, per in ((E.SE_CASES, 8), (E.SE_F32_CASES, 4)):
        widths, splits_seen = set(), set()
        for n, h, w, c, sq in cases:
            cg = c // per
            cgb = 32 if cg >= 32 else 1 << (cg.bit_length() - 1)
            groups = -(-cg // cgb)
            splits = 1
            while splits < 32 and n * groups * splits < 512 and h * w // (splits * 2) >= 256:
                splits *= 2
            widths.add(cgb)
            splits_seen.add(splits)
            assert c % per == 0 and 1 <= sq <= 64
        assert widths == {1, 2, 4, 8, 16, 32} and splits_seen == {1, 2, 8}
        assert any((c // per) % 32 not in (0, c // per) for _, _, _, c, _ in cases) and any(h * w < 256 // 32 * 2 for _, h, w, _, _ in cases)
    assert {sq for *_, sq in E.SE_CASES} == {1, 4, 48, 64}
