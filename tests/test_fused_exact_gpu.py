"""Bit-exact parity of the kernels that fuse several layers into one launch - the fused residual units (csrc/conv_resunit.hip,
csrc/conv_resunit_t20.hip), the fused stem (csrc/conv_stem.hip), the fused inverted-residual blocks (csrc/conv_mbconv.hip in tile and
strip form, csrc/conv_mbwide.hip) and conv + 2x2 max-pool (csrc/conv_small.hip) - against the one answer the chained operands of
tests/helpers.py allow: torch.equal, no tolerance.  tests/test_fused_exact_cpu.py has checked every reference's guards and that the
reference alone notices each failure class.

What this pins on top of tests/test_conv_exact_gpu.py: the INTERMEDIATE these kernels keep in LDS - that it is narrowed to bf16, once,
to nearest even (its values beyond 512 / from 1 on need rounding); that it is zero outside the image, whatever the first conv would
give there; that no tap of the second conv is lost at a tile edge, partial tiles included; that image b's halo never shows image
b +- 1; and the epilogue's order (activation, pre-add copy, fp32 residual add, one narrowing).  What it cannot pin: non-integer operands
and the real activation scales - tests/test_gpu_parity.py keeps those.

Views as in test_conv_exact_gpu.py::run_exact: x sits at an 8-channel offset in a wider buffer whose other channels hold NaN, y and the
pre-add copy sit at an offset among -77 values that must survive.  The forms are selected through yolo_set_tuning (knobs 3 and 4) and
restored in finally; right before every launch yolo_resunit_pick / yolo_stem_pick / yolo_mbconv_pick must name the kernel the case
stands for, under the very knob and descriptor of that launch (see the header of tests/_exact_cases.py).

Along the pixel direction every operand (x - the unit's residual too -, y, the pre-add copy, the float32 NCHW batch of the stem, every
packed weight and bias) sits between the poisoned margins of tests/_guard.py, and every case runs once per poison (0xFF, 0x7F): a
read outside an operand shows in the comparison, a write in Guard.assert_intact() after it."""
import pytest
import torch
import torch.nn.functional as F

import _exact_cases as E
import _guard as G
from helpers import exact_chain, exact_conv
from test_conv_exact_gpu import DEV, _assert_equal, _nhwc
from test_fused_exact_cpu import MB_IDS, POOL_IDS, STEM_IDS, UNIT_IDS, knob

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _view_in(x, g, margin=8):
    """x NCHW -> NHWC bf16 on the device at channel offset `margin` of a buffer 2 * margin wider, NaN elsewhere, allocated by the
    Guard `g`."""
    n, c, h, w = x.shape
    buf = g.alloc("x", (n, h, w, c + 2 * margin), BF16, float("nan"))
    buf[..., margin:margin + c] = _nhwc(x, BF16)
    return buf


def _check_view(buf, off, c, ref, what):
    _assert_equal(buf[..., off:off + c], ref, what)
    assert torch.all(buf[..., :off] == -77.0) and torch.all(buf[..., off + c:] == -77.0), f"{what}: channels outside the view were written"


@pytest.mark.parametrize("use_aux", [False, True], ids=["plain", "preadd"])
@pytest.mark.parametrize("u", E.UNIT_CASES, ids=UNIT_IDS)
def test_fused_residual_unit_exact(u, use_aux):
    """K.resunit in every form of UNIT_CASES (the id names the kernel; knob 3 selects it), with and without the pre-add copy, launched
    twice into fresh buffers: both results equal the reference, hence each other."""
    from pytorch_yolo_amd import kernels as K
    n, h, w, c, act = u["shape"]
    x, stages, res, unit, y_ref, aux_ref, _ = exact_chain("unit", u["shape"], u["seed"])
    (w1, b1, _, _, _), (w2, b2, _, _, _) = stages
    assert K.resunit_supported(c, h, w)
    w1p, b1p, kpad1, cpad1 = K.pack_conv_weight(w1, b1, c)
    w2p, b2p, kpad2, cpad2 = K.pack_conv_weight(w2, b2, c // 2)
    assert torch.equal(w1p.float()[:c // 2, :c], w1.reshape(c // 2, c)) and torch.equal(b1p[:c // 2], b1)
    d = E.unit_desc(u, use_aux, kpad2, cpad2)
    with knob(3, u["knob3"]):
        for run, poison in enumerate(G.POISONS):
            g = G.Guard(poison, DEV)
            xin = _view_in(x, g)
            dev = [g.like(name, t) for name, t in (("w1", w1p), ("b1", b1p), ("w2", w2p), ("b2", b2p))]
            y = g.alloc("y", (n, h, w, c + 16), BF16, -77.0)
            aux = g.alloc("pre-add copy", (n, h, w, c + 16), BF16, -77.0) if use_aux else None
            assert K.resunit_pick(d, use_aux).startswith(E.unit_pick_wanted(u)), K.resunit_pick(d, use_aux)
            K.resunit(xin, dev[0], dev[1], dev[2], dev[3], y, d, kpad1, cpad1, y_preadd=aux)
            torch.cuda.synchronize()
            _check_view(y, 8, c, y_ref, f"y (launch {run})")
            if use_aux:
                _check_view(aux, 8, c, aux_ref, f"pre-add copy (launch {run})")
            g.assert_intact()


@pytest.mark.parametrize("kernel,shape,tile,seed", E.STEM_CASES, ids=STEM_IDS)
def test_fused_stem_exact(kernel, shape, tile, seed):
    """K.stem from the float32 NCHW batch: stem2_kernel (3 input channels) and stem_kernel (1), LeakyReLU and ReLU6, launched twice."""
    from pytorch_yolo_amd import kernels as K
    n, cin, h, w, act = shape
    x, stages, res, unit, y_ref, _, _ = exact_chain("stem", shape, seed)
    (w1, b1, _, _, _), (w2, b2, _, _, _) = stages
    w1p, b1p, kpad1, _ = K.pack_conv_weight(w1, b1, 8)
    w2p, b2p, kpad2, cpad2 = K.pack_conv_weight(w2, b2, 32)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert y_ref.shape == (n, 64, ho, wo)
    d = E.stem_desc(shape, kpad2, cpad2)
    for run, poison in enumerate(G.POISONS):
        g = G.Guard(poison, DEV)
        xd = g.like("x (float32 NCHW)", x.contiguous())
        dev = [g.like(name, t) for name, t in (("w1", w1p), ("b1", b1p), ("w2", w2p), ("b2", b2p))]
        y = g.alloc("y", (n, ho, wo, 80), BF16, -77.0)
        assert K.stem_pick(cin, d).startswith(E.stem_pick_wanted(kernel, shape, tile)), K.stem_pick(cin, d)
        K.stem(xd, cin, dev[0], dev[1], kpad1, dev[2], dev[3], y, d)
        torch.cuda.synchronize()
        _check_view(y, 8, 64, y_ref, f"y (launch {run})")
        g.assert_intact()


@pytest.mark.parametrize("form,shape,tile", E.MBCONV_CASES, ids=MB_IDS)
def test_fused_inverted_residual_exact(form, shape, tile):
    """K.mbconv in the tile form, the row-strip form (knob 4 bit kMbStripForm) and the wide form's 13x13 and 7x7 tilings, on the ReLU6 chain: both intermediates clamped and
    narrowed, the depthwise conv padding the EXPANDED map with zeros."""
    from pytorch_yolo_amd import kernels as K
    n, h, w, cin, hidden, cout, stride = shape
    x, stages, res, unit, y_ref, _, _ = exact_chain("mbconv", shape, E.MBCONV_SEED)
    has_exp = hidden != cin
    assert len(stages) == (3 if has_exp else 2) and K.mbconv_supported(cin, hidden, cout, stride)
    we, be = (stages[0][0], stages[0][1]) if has_exp else (None, None)
    (wd, bd, _, _, _), (wp, bp, _, _, _) = stages[-2:]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    assert y_ref.shape == (n, cout, ho, wo)
    host = K.pack_mbconv(we, be, wd, bd, wp, bp, stride=stride)
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        xin = _view_in(x, g)
        y = g.alloc("y", (n, ho, wo, cout + 8), BF16, -77.0)
        packed = tuple(None if t is None else g.like(name, t) for name, t in zip(("w expand", "b expand", "w depthwise", "b depthwise", "w project", "b project"), host))
        with knob(4, E.MB_STRIP if form == "strip" else 0):
            assert E.mbconv_pick(shape).startswith(E.mbconv_pick_wanted(form, shape, tile)), E.mbconv_pick(shape)
            K.mbconv(xin, packed, y, n=n, h=h, w=w, cin=cin, hidden=hidden, cout=cout, in_view=(cin + 16, 8), out_view=(cout + 8, 4),
                     stride=stride, has_res=res is not None)
            torch.cuda.synchronize()
        _check_view(y, 4, cout, y_ref, "y")
        g.assert_intact()


@pytest.mark.parametrize("case", E.POOL_CASES, ids=POOL_IDS)
def test_small_cin_conv_with_maxpool_exact(case):
    """K.conv3x3_pool: the exact conv, then MaxPool2d(2, 2) of the NARROWED map as the two-launch path takes it (max is exact); an odd
    last row / column is computed and dropped (conv_small.hip: "MaxPool2d(2, 2): floor")."""
    from pytorch_yolo_amd import kernels as K
    n, h, w, cin, cout, pool = case
    x, wt, bias, _, conv_ref, _ = exact_conv((n, h, w, cin, cout, 3, 1, "leaky", False), E.POOL_SEED, BF16)
    y_ref = F.max_pool2d(conv_ref.float(), 2, 2).to(BF16) if pool else conv_ref
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    assert y_ref.shape == (n, cout, ho, wo)
    wp, bp, kpad, cpad = K.pack_conv_weight(wt, bias, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 16, in_c_offset=8, cout=cout, out_c_total=cout + 16, out_c_offset=8, ksize=3, stride=1,
                    act=E.ACTS["leaky"], kpad=kpad, cout_pad=cpad)
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        y = g.alloc("y", (n, ho, wo, cout + 16), BF16, -77.0)
        K.conv3x3_pool(_view_in(x, g), g.like("packed weights", wp), g.like("bias", bp), y, d, pool=pool)
        torch.cuda.synchronize()
        _check_view(y, 8, cout, y_ref, "y")
        g.assert_intact()
