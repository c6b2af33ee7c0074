"""Bit-exact tests of the kernels every shipped model starts with and of the element kernels of the depthwise encoder families, on the
operands of tests/helpers.py - torch.equal, no tolerance (tests/test_pointwise_exact_cpu.py has checked every reference's guards and
that the reference alone notices each failure class):
  * yolo_conv1_nchw_f32_fwd (stride 1, cout 16 / 32, cin_real 3 / 1 / 8), its stride-2 form and yolo_conv1_pool_nchw_f32_fwd.  They
    narrow the caller's float32 pixels themselves: two thirds of x need rounding, a fifth are exact ties - a kernel that truncated
    x, multiplied the float32 values or rounded otherwise than yolo_pack_input_nchw_f32 would not reproduce the reference;
  * yolo_dwconv3x3_fwd in its three forms (8-row strips as shipped, the one-pixel form and 4-row strips under knob 9 of
    yolo_set_tuning), yolo_dwconv_fwd and yolo_dwconv_f32_fwd, with every activation whose result is determined (none, LeakyReLU,
    ReLU6, ReLU); swish keeps a tolerance;
  * yolo_se_fwd / yolo_se_f32_fwd stage by stage: the pooled means and the rescaled output bit for bit, the scales between them within
    a bound derived from the operands (helpers.se_scales_reference).
Views as in test_conv_exact_gpu.py: bf16 / float32 NHWC inputs sit at a channel offset inside wider buffers whose other channels
hold NaN, outputs among -77 values that must survive; every operand - the float32 NCHW batch, weights, biases and the workspace too -
sits between the poisoned margins of tests/_guard.py, once per poison."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _exact_cases as E
import _guard as G
from helpers import exact_dw, exact_first_layer, exact_se, se_rescale_reference, se_scales_reference
from test_conv_exact_gpu import DEV, _assert_equal, _nhwc
from test_fused_exact_gpu import _check_view, knob
from test_guard_bands_gpu import _act, _lib_call, _stream
from test_pointwise_exact_cpu import DW3_IDS, DW_F32_IDS, DW_F32_ROWS, DW_IDS, DW_ROWS, FIRST_IDS, SE_IDS, SE_ROWS

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


# ---- first-layer kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", E.FIRST_CASES, ids=FIRST_IDS)
def test_first_layer_from_nchw_exact(shape, seed):
    """Every instantiation of conv1_nchw_kernel (conv3x3_halo.hip) and conv1_s2_nchw_kernel (conv_small.hip) straight from the float32
    NCHW batch: conv3x3 of bf16(x), bias, activation, one narrowing, and MaxPool2d(2, 2) of the narrowed map for the pooled form."""
    from pytorch_yolo_amd import kernels as K
    n, cin, h, w, cout, stride, act, pool = shape
    x, wt, bias, y_ref, _ = exact_first_layer(shape, seed)
    wp, bp, kpad, cpad = K.pack_conv_weight(wt, bias, 8)
    assert torch.equal(wp.float()[:cout, :72].reshape(cout, 9, 8)[:, :, :cin], wt.permute(0, 2, 3, 1).reshape(cout, 9, cin)) and torch.equal(bp[:cout], bias)
    d = K.conv_desc(n=n, h=h, w=w, cin=8, in_c_total=8, in_c_offset=0, cout=cout, out_c_total=cout + 16, out_c_offset=8, ksize=3,
                    stride=stride, act=_act(act), kpad=kpad, cout_pad=cpad)
    ho, wo = (h // 2, w // 2) if pool else (d.ho, d.wo)
    assert y_ref.shape == (n, cout, ho, wo)
    fn = "yolo_conv1_pool_nchw_f32_fwd" if pool else "yolo_conv1_nchw_f32_fwd"
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        y = g.alloc("y", (n, ho, wo, cout + 16), BF16, -77.0)
        xd, wd, bd = g.like("x (float32 NCHW)", x.contiguous()), g.like("packed weights", wp), g.like("bias", bp)
        _lib_call(fn, xd.data_ptr(), cin, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), C.byref(d), _stream())
        torch.cuda.synchronize()
        _check_view(y, 8, cout, y_ref, f"y (poison 0x{poison:02X})")
        g.assert_intact()


def test_pack_input_rounds_the_same_pixels_to_nearest_even():
    """yolo_pack_input_nchw_f32 on the x of a first-layer case (a fifth of it exact ties): the bits of torch's round-to-nearest-even,
    which is what the first-layer reference narrows with - the two ways into the first layer round alike."""
    from pytorch_yolo_amd import kernels as K
    shape, seed = E.FIRST_S1_CASES[0]
    x = exact_first_layer(shape, seed)[0]
    n, cin, h, w = x.shape
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        out = g.alloc("out", (n, h, w, 8), BF16, 7.0)
        K.pack_input(g.like("x", x.contiguous()), out)
        torch.cuda.synchronize()
        _assert_equal(out[..., :cin], x.to(BF16), "packed input")
        assert torch.all(out[..., cin:] == 0)
        g.assert_intact()


# ---- depthwise 3x3 / pad 1: the strip kernel and its two other forms ------------------------------------------------------------------
def _dw_in(g, x, dtype, off):
    n, c, h, w = x.shape
    xin = g.alloc("x", (n, h, w, c + 2 * off), dtype, float("nan"))
    xin[..., off:off + c] = _nhwc(x, dtype)
    return xin


def _dw3_launch(nchw, seed, stride, act, g):
    """One row of the yolo_dwconv3x3_fwd table on operands of the Guard `g`: (y buffer, reference); the view is y[..., 8:8 + c]."""
    from pytorch_yolo_amd import kernels as K
    n, c, h, w = nchw
    x, wt, bias, ho, wo, pad, y_ref, _ = exact_dw(E.dw3_shape(nchw, stride, act), seed, BF16, "torch")
    y = g.alloc("y", (n, ho, wo, c + 16), BF16, -77.0)
    K.dwconv3x3(_dw_in(g, x, BF16, 8), g.like("w", wt.reshape(c, 9).t().contiguous()), g.like("bias", bias), y, n=n, h=h, w=w, c=c,
                in_view=(c + 16, 8), out_view=(c + 16, 8), stride=stride, act=_act(act))
    torch.cuda.synchronize()
    return y, y_ref


@pytest.mark.parametrize("nchw,seed,stride", E.DW3_ROWS, ids=DW3_IDS)
def test_dwconv3x3_exact(nchw, seed, stride):
    """yolo_dwconv3x3_fwd as shipped (8-row strips) with none, LeakyReLU, ReLU6 and ReLU.  (Before the kernels applied every activation
    the ReLU rows came back un-activated.)"""
    from pytorch_yolo_amd._lib import load
    assert load().yolo_set_tuning(9, 0) == 0, "this test is about the shipped form (YOLO_DWCONV_DEBUG / knob 9 at 0)"
    for act in E.DW_ACTS:
        for poison in G.POISONS:
            g = G.Guard(poison, DEV)
            y, y_ref = _dw3_launch(nchw, seed, stride, act, g)
            _check_view(y, 8, nchw[1], y_ref, f"y ({act}, poison 0x{poison:02X})")
            g.assert_intact()


@pytest.mark.parametrize("value", [1, 2], ids=["one_pixel", "four_rows"])
def test_dwconv3x3_debug_forms_exact(value):
    """kDwOnePixel and kDwFourRows (csrc/tuning.h, knob 9) give the bits of the shipped form: the whole table, every activation and
    poison, with the knob set through yolo_set_tuning and restored afterwards."""
    with knob(9, value):
        for (nchw, seed, stride), rid in zip(E.DW3_ROWS, DW3_IDS):
            for act in E.DW_ACTS:
                for poison in G.POISONS:
                    g = G.Guard(poison, DEV)
                    y, y_ref = _dw3_launch(nchw, seed, stride, act, g)
                    _check_view(y, 8, nchw[1], y_ref, f"YOLO_DWCONV_DEBUG={value} {rid} {act} poison 0x{poison:02X}")
                    g.assert_intact()


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv3x3_swish_close(stride):
    """YOLO_ACT_SWISH through yolo_dwconv3x3_fwd (expf and a division: not bit-defined) against float64 on real activation scales, at the
    1e-2 of test_dwconv."""
    from pytorch_yolo_amd import kernels as K
    n, c, h, w = 2, 24, 17, 5
    gen = torch.Generator().manual_seed(31 + stride)
    x = torch.randn(n, c, h, w, generator=gen).to(BF16).float()
    wt, b = torch.randn(c, 1, 3, 3, generator=gen) * 0.3, torch.randn(c, generator=gen) * 0.1
    v = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=1, groups=c)
    ref = (v * torch.sigmoid(v)).float()
    ho, wo = ref.shape[2:]
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        y = g.alloc("y", (n, ho, wo, c + 16), BF16, -77.0)
        K.dwconv3x3(_dw_in(g, x, BF16, 8), g.like("w", wt.reshape(c, 9).t().contiguous()), g.like("bias", b), y, n=n, h=h, w=w, c=c,
                    in_view=(c + 16, 8), out_view=(c + 16, 8), stride=stride, act=_act("swish"))
        torch.cuda.synchronize()
        torch.testing.assert_close(y[..., 8:8 + c].float().permute(0, 3, 1, 2).cpu(), ref, rtol=1e-2, atol=1e-2)
        assert torch.all(y[..., :8] == -77.0) and torch.all(y[..., 8 + c:] == -77.0)
        g.assert_intact()


@pytest.mark.parametrize("stride", [1, 2])
def test_recorded_dwconv_relu_exact(stride):
    """Recorder.dwconv(act="relu") on a 3x3 / pad-1 layer in bf16 mode reaches yolo_dwconv3x3_fwd (emit._emit_dwconv, ksize 0): through
    engine.run_standalone it equals the exact reference.  (The fp32 mode sends the node to yolo_dwconv_f32_fwd.)"""
    from pytorch_yolo_amd import engine
    nchw, seed = E.DW3_CASES[2]
    x, wt, bias, ho, wo, pad, y_ref, _ = exact_dw(E.dw3_shape(nchw, stride, "relu"), seed, BF16, "torch")
    got = engine.run_standalone(lambda g, s: g.dwconv(s, (wt, bias), stride=stride, act="relu"), x.to(DEV))
    torch.cuda.synchronize()
    _assert_equal(got.to(BF16).permute(0, 2, 3, 1), y_ref, "recorded dwconv + ReLU")
    assert torch.equal(got.cpu(), y_ref.float()) and float((y_ref == 0).float().mean()) > 0.15


# ---- depthwise k x k with an explicit leading pad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DW_ROWS, ids=DW_IDS)
def test_dwconv_general_exact(row):
    """yolo_dwconv_fwd: k 3 and 5, strides 1 and 2, TensorFlow-"same" geometry and torch's pad k // 2, every exact activation."""
    from pytorch_yolo_amd import kernels as K
    k, stride, h, w, geometry, c, seed = row
    for act in E.DW_ACTS:
        x, wt, bias, ho, wo, pad, y_ref, _ = exact_dw((2, c, h, w, k, stride, act), seed, BF16, geometry)
        for poison in G.POISONS:
            g = G.Guard(poison, DEV)
            y = g.alloc("y", (2, ho, wo, c + 16), BF16, -77.0)
            K.dwconv(_dw_in(g, x, BF16, 8), g.like("w", wt.reshape(c, k * k).t().contiguous()), g.like("bias", bias), y, n=2, h=h, w=w, c=c,
                     in_view=(c + 16, 8), out_view=(c + 16, 8), ho=ho, wo=wo, ksize=k, stride=stride, pad=pad, act=_act(act))
            torch.cuda.synchronize()
            _check_view(y, 8, c, y_ref, f"y ({act}, poison 0x{poison:02X})")
            g.assert_intact()


@pytest.mark.parametrize("row", DW_F32_ROWS, ids=DW_F32_IDS)
def test_dwconv_f32_exact(row):
    """yolo_dwconv_f32_fwd on integers of eleven significant bits times {-1, 0, 1}: the float32 outputs bit for bit (a kernel that
    narrowed an operand would lose low bits of x), 12 channels at 4-channel offsets."""
    from pytorch_yolo_amd import kernels as K
    k, stride, h, w, geometry, c, seed = row
    for act in E.DW_ACTS:
        x, wt, bias, ho, wo, pad, y_ref, _ = exact_dw((2, c, h, w, k, stride, act), seed, F32, geometry)
        for poison in G.POISONS:
            g = G.Guard(poison, DEV)
            y = g.alloc("y", (2, ho, wo, c + 8), F32, -77.0)
            K.dwconv_f32(_dw_in(g, x, F32, 4), g.like("w", wt.reshape(c, k * k).t().contiguous()), g.like("bias", bias), y, n=2, h=h, w=w, c=c,
                         in_view=(c + 8, 4), out_view=(c + 8, 4), ho=ho, wo=wo, ksize=k, stride=stride, pad=pad, act=_act(act))
            torch.cuda.synchronize()
            _check_view(y, 4, c, y_ref, f"y ({act}, poison 0x{poison:02X})")
            g.assert_intact()


# ---- squeeze-and-excitation, stage by stage --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", SE_ROWS, ids=SE_IDS)
def test_squeeze_excite_stages(shape, dtype, capsys):
    """yolo_se_fwd / yolo_se_f32_fwd leave the means in workspace[0 : n c] and the scales in workspace[n c : 2 n c]:
      * the means equal float32(sum) * (1.f / hw) (bf16 kernel) / float32(sum) / hw (float32 kernel) in every bit - integer x makes every
        partial sum exact, whatever the channel-group width and the split of the pixel range;
      * the scales lie within the derived bound of the float64 evaluation of the two FCs from the kernel's OWN means (printed: the
        largest error / bound ratio);
      * y equals dtype(float32(x) * scale) in every bit, with the scales read back from the workspace."""
    from pytorch_yolo_amd import kernels as K
    n, h, w, c, sq = shape
    x, w1, b1, w2, b2, means_ref = exact_se(shape, E.SE_SEED, dtype)
    off = 8 if dtype == BF16 else 4
    fn = K.se if dtype == BF16 else K.se_f32
    worst = 0.0
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        y = g.alloc("y", (n, h, w, c + 2 * off), dtype, -77.0)
        ws = g.alloc("workspace", (K.se_workspace_bytes(n, c) // 4,), F32)
        fn(_dw_in(g, x, dtype, off), y, g.like("w1", w1), g.like("b1", b1), g.like("w2", w2.t().contiguous()), g.like("b2", b2), ws, n=n, h=h, w=w,
           c=c, in_view=(c + 2 * off, off), out_view=(c + 2 * off, off))
        torch.cuda.synchronize()
        means, scales = ws[:n * c].cpu().reshape(n, c), ws[n * c:2 * n * c].cpu().reshape(n, c)
        if not torch.equal(means, means_ref):
            bad = (means != means_ref).nonzero()
            pytest.fail(f"pooled means: {len(bad)} of {means.numel()} differ; first at {bad[:4].tolist()}: got {[float(means[tuple(i)]) for i in bad[:4]]}, "
                        f"want {[float(means_ref[tuple(i)]) for i in bad[:4]]}")
        want, bound = se_scales_reference(means, w1, b1, w2, b2)
        ratio = float(((scales.double() - want).abs() / bound).max())
        worst = max(worst, ratio)
        with capsys.disabled():
            print(f"\n  se scales {SE_IDS[SE_ROWS.index((shape, dtype))]} poison 0x{poison:02X}: largest error / bound = {ratio:.4f} (bound <= {float(bound.max()):.2e})")
        assert ratio <= 1.0 and bool(torch.isfinite(scales).all()), f"scales: error / bound = {ratio}"
        _check_view(y, off, c, se_rescale_reference(x, scales, dtype), f"y (poison 0x{poison:02X})")
        g.assert_intact()
