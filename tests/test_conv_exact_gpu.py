"""Bit-exact conv parity on integer operands: every kernel family behind yolo_conv2d_fwd / yolo_conv2d_splitk_fwd / yolo_conv2d_f16_fwd /
yolo_conv3x3_t20_f16_fwd / yolo_conv2d_f32_fwd, and every non-decode instance of the bf16 gather kernel, against the one answer the
operands of tests/helpers.py::exact_conv_case allow - torch.equal, no tolerance.

What this pins: that every product reaches the sum (whatever the tile shape, K split, MFMA shape, stage count or gather form), the
rounding MODE of the narrowing (a quarter to two thirds of every output tensor needs rounding, a tenth and more are exact ties: truncation
and round-half-away both show), and the rounding POINTS of the epilogue (activation, pre-add copy narrowed from the activation's value,
fp32 residual add, one narrowing).  What it cannot pin: the rounding of non-integer operands on the way in, non-finite and subnormal
values - those keep their tests in test_gpu_parity.py and test_fp16_gpu.py.

Views as in test_conv_f16_kernel: x, y, the residual and the pre-add copy sit at a channel offset inside wider buffers; the channels
next to x and the residual hold NaN (a read past the view poisons the sum), those next to y and the pre-add copy hold -77 and must
still hold it afterwards.

Along the pixel direction every operand - x, y, the residual, the pre-add copy, the packed weights, the bias, the split-K workspace
and counters - sits between the poisoned margins of tests/_guard.py, and every case runs once per poison (0xFF, 0x7F): a read
outside an operand shows in the comparisons above, a write in Guard.assert_intact() after them."""
import pytest
import torch

import _exact_cases as E
import _guard as G
from _exact_cases import BF16_INSTANCES
from helpers import exact_conv
from test_conv_exact_cpu import RECIPES, assert_recipe_pick, exact_desc, tuning

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _assert_equal(got_nhwc, ref_nchw, what):
    got = got_nhwc.permute(0, 3, 1, 2).contiguous().cpu()
    assert got.dtype == ref_nchw.dtype and got.shape == ref_nchw.shape, what
    if not torch.equal(got, ref_nchw):
        bad = got.float() != ref_nchw.float()
        idx = bad.nonzero()[:4].tolist()
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} values differ ({int(torch.isnan(got.float()).sum())} NaN); first at {idx}: "
                    f"got {[float(got[tuple(i)]) for i in idx]}, want {[float(ref_nchw[tuple(i)]) for i in idx]}")


def run_exact(shape, seed, dtype, launch, view="v8", in_place_res=False, d=None):
    """An exact case through `launch(xin, wp, bp, y, d, residual, y_preadd, g)` and every comparison of this file, once per poison
    of tests/_guard.py with every operand allocated by the Guard `g` (the launch takes its workspaces from it)."""
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        _run_exact_once(shape, seed, dtype, launch, view, in_place_res, d, g)
        g.assert_intact()


def _run_exact_once(shape, seed, dtype, launch, view, in_place_res, d, g):
    from pytorch_yolo_amd import kernels as K
    n, h, w, cin, cout, k, stride, act, use_res, use_aux, up, f32 = shape
    x, wt, bias, res, y_ref, aux_ref = exact_conv(shape[:9], seed, dtype, up=up, f32_out=f32)
    d = d or exact_desc(shape, view, dtype, in_place_res)
    ho, wo, co = d.ho, d.wo, d.out_c_offset
    xin = g.alloc("x", (n, h, w, d.in_c_total), dtype, float("nan"))
    xin[..., 8:8 + cin] = _nhwc(x, dtype)
    y = g.alloc("y", (n, ho * (2 if up else 1), wo * (2 if up else 1), d.out_c_total), torch.float32 if f32 else dtype, -77.0)
    rin = None
    if use_res and in_place_res:
        y[..., co:co + cout] = _nhwc(res, dtype)
        rin = y
    elif use_res:
        rin = g.alloc("residual", (n, ho, wo, d.res_c_total), dtype, float("nan"))
        rin[..., 8:8 + cout] = _nhwc(res, dtype)
    aux = g.alloc("pre-add copy", (n, ho, wo, d.aux_c_total), dtype, -77.0) if use_aux else None
    pack = K.pack_conv_weight if dtype == torch.bfloat16 else K.pack_conv_weight_f16
    wp, bp, kpad, cout_pad = pack(wt, bias, cin)
    assert (kpad, cout_pad) == (d.kpad, d.cout_pad) and torch.equal(wp.float()[:cout, :k * k * cin].reshape(cout, k * k, cin), wt.permute(0, 2, 3, 1).reshape(cout, k * k, cin))
    launch(xin, g.like("packed weights", wp), g.like("bias", bp), y, d, rin, aux, g)
    torch.cuda.synchronize()
    _assert_equal(y[..., co:co + cout], y_ref, "y")
    assert torch.all(y[..., :co] == -77.0) and torch.all(y[..., co + cout:] == -77.0), "channels outside the output view were written"
    if use_aux:
        _assert_equal(aux[..., 8:8 + cout], aux_ref, "pre-add copy")
        assert torch.all(aux[..., :8] == -77.0) and torch.all(aux[..., 8 + cout:] == -77.0), "channels outside the pre-add view were written"


def _conv2d(xin, wp, bp, y, d, rin, aux, g):
    from pytorch_yolo_amd import kernels as K
    K.conv2d(xin, wp, bp, y, d, residual=rin, y_preadd=aux)


@pytest.mark.parametrize("name,r", RECIPES, ids=[n for n, _ in RECIPES])
def test_bf16_gather_instance_exact(name, r):
    """Every non-decode instance of YOLO_IGEMM_INSTANCES (csrc/conv_igemm.hip), reached by its recipe; the pick is asserted first."""
    from pytorch_yolo_amd import kernels as K
    d = assert_recipe_pick(name, r)
    shape = r["shape"]
    if name in E.SPLITK_PLAIN:
        splits, ws_bytes, n_cnt = K.conv2d_splitk_plan(d, shape[8], shape[9])
        assert splits >= 2


        def splitk(xin, wp, bp, y, d, rin, aux, g):
            ws = g.alloc("split-K workspace", (ws_bytes // 4,), torch.float32, float("nan"))
            cnt = g.alloc("split-K counters", (n_cnt,), torch.int32)
            K.conv2d_splitk(xin, wp, bp, y, d, splits, ws, cnt, residual=rin, y_preadd=aux)
            assert int(cnt.abs().sum()) == 0
        run_exact(shape, 1, torch.bfloat16, splitk, d=d)
        return
    with tuning(r["knob0"], r["knob1"]):
        run_exact(shape, 1, torch.bfloat16, _conv2d, view=r["view"], d=d)


@pytest.mark.parametrize("fam,knob1,knob2,shape", E.FAMILY_CASES, ids=[f"{c[0]}_{c[1]}_{E.case_id(c[3])}" for c in E.FAMILY_CASES])
def test_bf16_other_families_exact(fam, knob1, knob2, shape):
    """The 20x20-tile kernels (forced), the halo kernel (by the shipped rule) and both streaming 1x1 forms (forced)."""
    from pytorch_yolo_amd import kernels as K
    d = exact_desc(shape)
    with tuning(-1, knob1, knob2):
        pick = K.conv2d_pick(d, shape[8], shape[9])
        assert pick.startswith(fam) and (fam != "stream1x1" or pick.startswith("stream1x1p<") == (shape[4] == 128 and not knob1)), pick
        run_exact(shape, 2, torch.bfloat16, _conv2d, d=d)


def _f16_cases():
    from test_fp16_gpu import CONV_F16_CASES
    return CONV_F16_CASES


@pytest.mark.parametrize("case", _f16_cases(), ids=lambda c: E.case_id(c[:12]) + "_" + c[12])
def test_f16_gather_instance_exact(case):
    """CONV_F16_CASES (tests/test_fp16_gpu.py): the fp16 table's instances, same body, dtype float16."""
    from pytorch_yolo_amd import kernels as K
    from test_fp16_gpu import F16_INSTANCES
    shape, inst = case[:12], case[12]
    d = exact_desc(shape, dtype=torch.float16)
    want = F16_INSTANCES[inst].split("|")
    pick = K.conv2d_f16_pick(d, shape[8], shape[9])
    assert pick.startswith("igemm_f16" + want[0] + " grid "), f"{inst}: picked {pick}"
    run_exact(shape, 3, torch.float16, lambda xin, wp, bp, y, d, rin, aux, g: K.conv2d_f16(xin, wp, bp, y, d, residual=rin, y_preadd=aux), d=d)


def _t20_f16_cases():
    from test_fp16_t20_gpu import T20_F16_CASES
    return T20_F16_CASES


@pytest.mark.parametrize("case", _t20_f16_cases(), ids=lambda c: "n%d_%dx%d_c%d-%d_s%d_%s_r%d_a%d" % tuple(int(v) if not isinstance(v, str) else v for v in c))
def test_f16_t20_exact(case):
    """T20_F16_CASES (tests/test_fp16_t20_gpu.py) with force: both fp16 tile kernels, the residual read from the output view."""
    from pytorch_yolo_amd import kernels as K
    shape = case[:5] + (3, case[5], case[6], case[7], case[8], False, False)
    run_exact(shape, 4, torch.float16, lambda xin, wp, bp, y, d, rin, aux, g: K.conv3x3_t20_f16(xin, wp, bp, y, d, residual=rin, y_preadd=aux, force=True),
              in_place_res=True)


def _f32_cases():
    from test_gpu_parity import F32_CONV_CASES
    return F32_CONV_CASES


@pytest.mark.parametrize("case", _f32_cases(), ids=lambda c: "n%d_%dx%d_c%d-%d_k%d_s%d_%s_r%d_a%d_u%d" % tuple(int(v) if not isinstance(v, str) else v for v in c))
def test_f32_conv_multiplies_full_width_operands(case):
    """yolo_conv2d_f32_fwd on integers of eleven significant bits times {-1, 0, 1}: a kernel that narrowed an operand to bf16, fp16's
    ten bits + 1 or a reduced-precision MFMA input would lose low bits of x; with K * 2^11 < 2^24 the fp32 sums are exact."""
    from pytorch_yolo_amd import kernels as K
    n, h, w, cin, cout, k, stride, act, use_res, use_aux, up = case
    x, wt, bias, res, y_ref, aux_ref = exact_conv(case[:9], 5, torch.float32, up=up)
    f = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    ho, wo = y_ref.shape[2] // (2 if up else 1), y_ref.shape[3] // (2 if up else 1)
    c4 = K.roundup(cout, 4)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f32(wt, bias, cin)
    for poison in G.POISONS:          # every operand between poisoned margins (tests/_guard.py), once per poison
        g = G.Guard(poison, DEV)
        xin = g.alloc("x", (n, h, w, cin + 8), torch.float32, float("nan"))
        xin[..., 4:4 + cin] = f(x)
        y = g.alloc("y", (n, y_ref.shape[2], y_ref.shape[3], c4 + 8), torch.float32, -77.0)
        aux = g.alloc("pre-add copy", (n, ho, wo, c4 + 4), torch.float32, -77.0) if use_aux else None
        rin = None
        if use_res:
            rin = g.alloc("residual", (n, ho, wo, c4 + 4), torch.float32, float("nan"))
            rin[..., 4:4 + cout] = f(res)
        _f32_launch_and_compare(case, xin, y, aux, rin, g.like("packed weights", wp), g.like("bias", bp), kpad, cout_pad, c4, y_ref, aux_ref)
        g.assert_intact()


def _f32_launch_and_compare(case, xin, y, aux, rin, wp, bp, kpad, cout_pad, c4, y_ref, aux_ref):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F32
    from test_conv_exact_cpu import ACT
    n, h, w, cin, cout, k, stride, act, use_res, use_aux, up = case
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 8, in_c_offset=4, cout=cout, out_c_total=c4 + 8, out_c_offset=4, ksize=k,
                    stride=stride, act=ACT[act], kpad=kpad, cout_pad=cout_pad, upsample2x=int(up), out_dtype=DT_F32,
                    res=(c4 + 4, 4) if use_res else (0, 0), aux=(c4 + 4, 4) if use_aux else (0, 0))
    K.conv2d_f32(xin, wp, bp, y, d, residual=rin, y_preadd=aux)
    torch.cuda.synchronize()
    _assert_equal(y[..., 4:4 + cout], y_ref, "y")
    assert torch.all(y[..., :4] == -77.0) and torch.all(y[..., 4 + cout:] == -77.0)
    if use_aux:
        _assert_equal(aux[..., 4:4 + cout], aux_ref, "pre-add copy")
        assert torch.all(aux[..., :4] == -77.0) and torch.all(aux[..., 4 + cout:] == -77.0)
