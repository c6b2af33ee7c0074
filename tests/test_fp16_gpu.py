"""GPU tests of the fp16-operand mode (model.precision = "fp16"): kernels through the C ABI against torch on the
same fp16-rounded operands, models against the fp16 CPU rounding model - oracle/policy.py's bf16 policy with its operand rounding
function swapped for IEEE half -, detections against the reference's.

Tolerances (stated once):
  * conv, fp16 output: rtol = atol = 1e-3 against the fp32 conv of the same fp16-rounded operands - twice fp16's half-ulp of
    2^-11 = 4.9e-4 (one rounding of the result, plus a flip where the fp32 sums differ in their last bits);
    fp32 output: rtol 1e-5 / atol 2e-4, as for the bf16 kernels (fp32 summation order only).
  * pools / SPP / pack: bit-exact.
  * models against the fp16 CPU rounding model: the bounds the bf16 model test holds against the fp32 oracle (boxes within
    max(1.5 px, 2 %), scores within 2e-2 / rms 2e-3; YOLOv3 4e-2) divided by 8 - fp16 carries three more mantissa bits than bf16, so
    the whole fp16 drift is 8 x smaller than the bf16 drift those bounds contain, and the distance between two fp16 runs that differ
    in summation order is part of it.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases as C
from helpers import build_case, build_rule_case, load_golden, oracle_forward, strict_share

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_TOL = dict(rtol=1e-3, atol=1e-3)
F32_TOL = dict(rtol=1e-5, atol=2e-4)


def _f16r(t):
    return t.to(torch.float16).float()


def _nhwc(t):      # NCHW f32 -> NHWC fp16 on device
    return t.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV)


def _nchw(t):      # NHWC (any dtype) on device -> NCHW f32 on host
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


class fp16_policy:
    """with fp16_policy(): oracle.policy.run_policy(..., policy="bf16") rounds its operands and its residual stream to IEEE half
    instead of bf16 - the CPU rounding model of the fp16 mode (oracle/policy.py itself is not edited)."""

    def __enter__(self):
        from oracle import policy
        self.policy, self.old = policy, policy.bf16r
        policy.bf16r = lambda t: t.to(torch.float16).float()

    def __exit__(self, *exc):
        self.policy.bf16r = self.old
        return False


# every instance of the fp16 table (csrc/conv_igemm.hip, YOLO_IGEMM_F16_INSTANCES) -> what yolo_conv2d_f16_pick prints for it
F16_INSTANCES = {
    "k64x256_8w_decode": "<64x256,1x8 waves,BK64,2 stages,32x32x16,decode>",
    "k64x256_bk32_decode": "<64x256,1x4 waves,BK32,2 stages,32x32x16,decode>",
    "k64x256_bk32_generic_decode": "<64x256,1x4 waves,BK32,2 stages,generic,32x32x16,decode>",
    "k256x32_m32": "<256x32,4x1 waves,BK32,2 stages,32x32x16>|epi",
    "k256x32_m32_direct": "<256x32,4x1 waves,BK32,2 stages,32x32x16>|direct",
    "k256x32_m32_generic": "<256x32,4x1 waves,BK32,2 stages,generic,32x32x16>|epi",
    "k256x32_m32_generic_direct": "<256x32,4x1 waves,BK32,2 stages,generic,32x32x16>|direct",
    "k256x64_m32": "<256x64,4x1 waves,BK32,2 stages,32x32x16>|epi",
    "k256x64_m32_direct": "<256x64,4x1 waves,BK32,2 stages,32x32x16>|direct",
    "k256x64_m32_generic": "<256x64,4x1 waves,BK32,2 stages,generic,32x32x16>|epi",
    "k256x64_m32_generic_direct": "<256x64,4x1 waves,BK32,2 stages,generic,32x32x16>|direct",
    "k128x128_bk32_3st_m32": "<128x128,2x2 waves,BK32,3 stages,32x32x16>|epi",
    "k128x128_bk32_3st_m32_direct": "<128x128,2x2 waves,BK32,3 stages,32x32x16>|direct",
    "k128x128_bk32_3st_m32_generic": "<128x128,2x2 waves,BK32,3 stages,generic,32x32x16>|epi",
    "k128x128_bk32_3st_m32_generic_direct": "<128x128,2x2 waves,BK32,3 stages,generic,32x32x16>|direct",
    "k64x64_4st": "<64x64,2x2 waves,BK64,4 stages,16x16x32>",
    "k64x64": "<64x64,2x2 waves,BK64,2 stages,16x16x32>",
    "k64x64_m32_direct": "<64x64,2x2 waves,BK64,2 stages,32x32x16>",
    "k128x128_8w": "<128x128,2x4 waves,BK64,2 stages,16x16x32>",
    "k128x128_8w_3st": "<128x128,2x4 waves,BK64,3 stages,16x16x32>",
    "k128x128_m32_direct": "<128x128,2x2 waves,BK64,2 stages,32x32x16>",
    "k128x256_8w": "<128x256,2x4 waves,BK64,2 stages,16x16x32>",
    "k128x256_16w_3st": "<128x256,2x8 waves,BK64,3 stages,16x16x32>",
    "k256x128_8w_bk32": "<256x128,4x2 waves,BK32,2 stages,16x16x32>",
    "k256x128_8w_bk32_m32_direct": "<256x128,4x2 waves,BK32,2 stages,32x32x16>",
    "k256x256_16w": "<256x256,4x4 waves,BK64,2 stages,16x16x32>",
    "k256x256_8w_m32_direct": "<256x256,4x2 waves,BK64,2 stages,32x32x16>",
}
# (the pick string does not say which epilogue a 32x32x16 tile runs: "|epi" / "|direct" is checked against the views instead)

CONV_F16_CASES = [
    # n, h, w, cin, cout, k, stride, act, residual, aux, upsample, f32, the instance the shape is meant to exercise
    # -- the CONV_CASES of test_conv_kernel (in fp16 all of them are gather-kernel launches, the large 3x3 maps too)
    (2, 16, 16, 8, 32, 3, 1, "leaky", False, False, False, False, "k256x32_m32_generic"),
    (2, 20, 20, 64, 128, 3, 1, "leaky", True, True, False, False, "k128x128_8w"),
    (1, 33, 29, 32, 64, 3, 2, "leaky", False, False, False, False, "k256x64_m32"),
    (3, 13, 13, 256, 255, 1, 1, "none", False, False, False, True, "k64x64_m32_direct"),
    (2, 10, 10, 128, 64, 1, 1, "leaky", False, False, True, False, "k64x64_4st"),
    (1, 40, 40, 16, 16, 3, 1, "relu6", False, False, False, False, "k256x32_m32_generic_direct"),
    (2, 7, 9, 96, 24, 1, 1, "none", True, False, False, False, "k256x32_m32_direct"),
    (1, 26, 26, 384, 256, 3, 1, "leaky", False, False, False, False, "k128x256_8w"),
    (1, 9, 9, 1024, 512, 1, 1, "leaky", False, False, False, False, "k64x64"),
    (1, 80, 96, 64, 128, 3, 1, "leaky", True, True, False, False, "k128x128_8w"),
    (1, 96, 80, 128, 256, 3, 1, "leaky", True, False, False, False, "k128x256_8w"),
    (1, 112, 80, 32, 64, 3, 1, "leaky", False, False, False, False, "k256x64_m32"),
    (2, 94, 100, 96, 64, 3, 1, "none", True, False, False, False, "k256x64_m32"),
    (1, 80, 80, 192, 128, 3, 1, "relu6", False, False, False, False, "k128x128_8w"),
    # -- 1x1 layers whose cin is no multiple of 32, inside a wider buffer (the one-tap fast gather)
    (2, 12, 10, 8, 32, 1, 1, "leaky", False, False, False, False, "k256x32_m32"),
    (2, 12, 10, 24, 48, 1, 1, "none", True, False, False, False, "k256x64_m32_direct"),
    (2, 12, 10, 40, 255, 1, 1, "none", False, False, False, True, "k128x128_bk32_3st_m32_direct"),
    (1, 26, 26, 40, 128, 1, 1, "leaky", False, True, False, False, "k128x128_bk32_3st_m32"),
    # -- the rest of the table
    (1, 20, 20, 16, 64, 3, 1, "leaky", True, False, False, False, "k256x64_m32_generic"),
    (1, 20, 20, 24, 40, 3, 2, "leaky", False, False, False, False, "k256x64_m32_generic_direct"),
    (1, 20, 20, 96, 128, 3, 1, "leaky", True, True, False, False, "k128x128_bk32_3st_m32"),
    (1, 20, 20, 24, 128, 3, 1, "relu6", False, False, True, False, "k128x128_bk32_3st_m32_generic"),
    (1, 20, 20, 40, 100, 3, 1, "leaky", True, True, False, False, "k128x128_bk32_3st_m32_generic_direct"),
    (2, 13, 13, 1280, 64, 3, 1, "leaky", False, False, False, False, "k64x64_4st"),
    (8, 20, 20, 256, 512, 1, 1, "leaky", True, False, False, False, "k128x128_8w_3st"),
    (1, 26, 26, 384, 255, 3, 1, "none", False, False, False, True, "k128x128_m32_direct"),
    (8, 32, 32, 128, 512, 1, 1, "leaky", False, True, False, False, "k128x256_16w_3st"),
    (1, 200, 200, 64, 128, 1, 1, "leaky", True, False, False, False, "k256x128_8w_bk32"),
    (1, 200, 200, 64, 128, 1, 1, "none", False, False, False, True, "k256x128_8w_bk32_m32_direct"),
    (8, 52, 52, 64, 512, 3, 1, "leaky", True, True, False, False, "k256x256_16w"),
    (8, 52, 52, 64, 512, 3, 2, "leaky", False, False, False, False, "k128x256_8w"),
    (8, 52, 52, 64, 512, 1, 1, "none", False, False, False, True, "k256x256_8w_m32_direct"),
]
HEAD_F16_CASES = [
    # n, h, w, cin, k, nc, act, instance
    (2, 20, 20, 256, 1, 80, "leaky", "k64x256_8w_decode"),
    (3, 13, 13, 96, 1, 80, "none", "k64x256_bk32_decode"),
    (2, 10, 12, 40, 3, 3, "leaky", "k64x256_bk32_generic_decode"),
]


def test_every_fp16_instance_has_a_case():
    assert {c[-1] for c in CONV_F16_CASES} | {c[-1] for c in HEAD_F16_CASES} == set(F16_INSTANCES)


_ACTS = {"leaky": lambda t: F.leaky_relu(t, 0.1), "none": lambda t: t, "relu6": F.relu6}


def _act_code(act):
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU6
    return {"leaky": ACT_LEAKY01, "none": ACT_NONE, "relu6": ACT_RELU6}[act]


@pytest.mark.parametrize("case", CONV_F16_CASES, ids=lambda c: "n%d_%dx%d_c%d-%d_k%d_s%d_%s_r%d_a%d_u%d_f%d_%s" % tuple(int(v) if not isinstance(v, str) else v for v in c))
def test_conv_f16_kernel(case):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F16, DT_F32
    n, h, w, cin, cout, k, stride, act, use_res, use_aux, up, f32, inst = case
    g = torch.Generator().manual_seed(hash(case[:-1]) & 0xffff)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    res = torch.randn(n, cout, ho, wo, generator=g) if use_res else None
    # views with channel offsets on every tensor; the channels NEXT to the input view hold NaN: a gather that reads past cin shows
    in_ct, in_co = cin + 16, 8
    xin = torch.full((n, h, w, in_ct), float("nan"), dtype=torch.float16, device=DEV)
    xin[..., in_co:in_co + cin] = _nhwc(x)
    oh, ow = (2 * ho, 2 * wo) if up else (ho, wo)
    out_ct, out_co = K.roundup(cout, 8) + 8, 8
    y = torch.full((n, oh, ow, out_ct), -77.0, dtype=torch.float32 if f32 else torch.float16, device=DEV)
    aux = torch.full((n, ho, wo, K.roundup(cout, 8) + 8), -77.0, dtype=torch.float16, device=DEV) if use_aux else None
    res_ct = K.roundup(cout, 8) + 8
    rin = None
    if use_res:
        rin = torch.full((n, ho, wo, res_ct), float("nan"), dtype=torch.float16, device=DEV)
        rin[..., 8:8 + cout] = _nhwc(res)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, bias, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=in_ct, in_c_offset=in_co, cout=cout, out_c_total=out_ct, out_c_offset=out_co,
                    ksize=k, stride=stride, act=_act_code(act), kpad=kpad, cout_pad=cout_pad, upsample2x=int(up),
                    out_dtype=DT_F32 if f32 else DT_F16, res=(res_ct, 8) if use_res else (0, 0),
                    aux=(aux.shape[-1], 8) if use_aux else (0, 0))
    # the shape reaches the instance it is meant to exercise
    pick = K.conv2d_f16_pick(d, use_res, use_aux)
    want = F16_INSTANCES[inst].split("|")
    assert pick.startswith("igemm_f16" + want[0] + " grid "), f"{inst}: picked {pick}"
    if len(want) > 1:
        assert (want[1] == "epi") == (not f32 and cout % 32 == 0), inst
    K.conv2d_f16(xin, wp.to(DEV), bp.to(DEV), y, d, residual=rin, y_preadd=aux)
    torch.cuda.synchronize()
    ref = _ACTS[act](F.conv2d(_f16r(x), _f16r(wt), bias, stride=stride, padding=pad))
    pre = ref
    if use_res:
        ref = ref + _f16r(res)
    if up:
        ref = F.interpolate(ref, scale_factor=2, mode="nearest")
    got = _nchw(y[..., out_co:out_co + cout])
    torch.testing.assert_close(got, ref, **(F32_TOL if f32 else F16_TOL))
    # nothing outside the views is touched
    assert torch.all(y[..., :out_co] == -77.0) and torch.all(y[..., out_co + cout:] == -77.0)
    if use_aux:
        torch.testing.assert_close(_nchw(aux[..., 8:8 + cout]), pre, **F16_TOL)
        assert torch.all(aux[..., :8] == -77.0) and torch.all(aux[..., 8 + cout:] == -77.0)


@pytest.mark.parametrize("n,h,w,cin,k,nc,act,inst", HEAD_F16_CASES)
def test_head_decode_f16(n, h, w, cin, k, nc, act, inst):
    """fp16 head conv + decode in one launch: p = the fp32 conv of the fp16-rounded operands, io = its decode; the filter form leaves
    the compact NMS the detections of the plain NMS on that io, bit for bit."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F32
    from pytorch_yolo_amd.utils.utils import MAX_PER_CLASS, MIN_WH, nms_capacity, nms_launch, split_detections
    na, no = 3, nc + 5
    cout = na * no
    g = torch.Generator().manual_seed(cin * 7 + nc)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.5
    anchors = ((10., 13.), (16., 30.), (33., 23.))
    stride_px = 32.0
    in_ct = cin + 8
    xin = torch.full((n, h, w, in_ct), float("nan"), dtype=torch.float16, device=DEV)
    xin[..., :cin] = _nhwc(x)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, bias, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=in_ct, in_c_offset=0, cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                    ksize=k, stride=1, act=_act_code(act), kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F32)
    for filt in (False, True):
        assert K.head_decode_f16_pick(d, na, nc, filt).startswith("igemm_f16" + F16_INSTANCES[inst] + " grid "), inst
    rows = na * h * w
    io = torch.full((n, rows + 7, no), -5.0, dtype=torch.float32, device=DEV)
    p = torch.empty((n, na, h, w, no), dtype=torch.float32, device=DEV)
    K.head_decode_f16(xin, wp.to(DEV), bp.to(DEV), d, anchors, nc, stride_px, io, 3, p)
    torch.cuda.synchronize()
    ref = _ACTS[act](F.conv2d(_f16r(x), _f16r(wt), bias, padding=(k - 1) // 2))
    p_ref = ref.view(n, na, no, h, w).permute(0, 1, 3, 4, 2).contiguous()
    torch.testing.assert_close(p.cpu(), p_ref, **F32_TOL)
    # YOLOLayer.forward's eval branch (reference models/yolo_layer.py:90-96) on the p the kernel stored
    yv, xv = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    io_ref = p.cpu().clone()
    io_ref[..., 0:2] = torch.sigmoid(io_ref[..., 0:2]) + torch.stack((xv, yv), 2).float().view(1, 1, h, w, 2)
    io_ref[..., 2:4] = torch.exp(io_ref[..., 2:4]) * (torch.tensor(anchors) / stride_px).view(1, na, 1, 1, 2)
    io_ref[..., 4:] = torch.sigmoid(io_ref[..., 4:])
    io_ref[..., :4] *= stride_px
    torch.testing.assert_close(io[:, 3:3 + rows].cpu(), io_ref.view(n, rows, no), rtol=2e-5, atol=1e-4)
    assert torch.all(io[:, :3] == -5.0) and torch.all(io[:, 3 + rows:] == -5.0)
    # the filter form == the plain NMS on the io the plain form wrote
    io2 = torch.empty((n, rows, no), dtype=torch.float32, device=DEV)
    K.head_decode_f16(xin, wp.to(DEV), bp.to(DEV), d, anchors, nc, stride_px, io2, 0, None)
    conf = float((io2[..., 4] * io2[..., 5:].max(-1).values).flatten().kthvalue(int(0.9 * n * rows)).values)
    cap = nms_capacity(rows, nc)
    mk = lambda: (torch.empty((n, cap, 7), dtype=torch.float32, device=DEV), torch.empty((n, cap), dtype=torch.int32, device=DEV),
                  torch.empty((n,), dtype=torch.int32, device=DEV))
    out_a, out_b = mk(), mk()
    nms_launch(io2, conf, 0.5, out_a, slot=0)
    ws = torch.empty(K.nms_compact_workspace_bytes(n, rows, nc), dtype=torch.uint8, device=DEV)
    K.head_decode_filter_f16(xin, wp.to(DEV), bp.to(DEV), d, anchors, nc, stride_px, rows, 0, conf, ws, min_wh=MIN_WH)
    K.nms_merge_compact(ws, n, rows, nc, 0.5, *out_b, max_per_class=MAX_PER_CLASS)
    torch.cuda.synchronize()
    da, db = split_detections(*out_a), split_detections(*out_b)
    assert any(t is not None for t in da)
    assert all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for a, b in zip(da, db))


# ---- narrowing ------------------------------------------------------------------------------------
NARROW_SHAPES = [(1, 13, 13, 256, 255, 1, "none", True),       # fp32 head store (direct epilogue)
                 (1, 13, 13, 256, 255, 1, "none", False),      # fp16 store from the accumulator registers (direct epilogue)
                 (1, 20, 20, 128, 64, 1, "leaky", False),      # LDS-staged epilogue, 32x32x16 accumulators
                 (1, 40, 40, 64, 128, 3, "none", False)]       # LDS-staged epilogue, 16x16x32 accumulators


def _run_plain(shape, bias_edit, x_scale=1.0):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F16, DT_F32
    n, h, w, cin, cout, k, act, f32 = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, h, w, generator=g) * x_scale
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    bias_edit(bias)
    y = torch.zeros(n, h, w, K.roundup(cout, 8), dtype=torch.float32 if f32 else torch.float16, device=DEV)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, bias, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=y.shape[-1], out_c_offset=0,
                    ksize=k, stride=1, act=_act_code(act), kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F32 if f32 else DT_F16)
    K.conv2d_f16(_nhwc(x), wp.to(DEV), bp.to(DEV), y, d)
    torch.cuda.synchronize()
    return y.float().cpu(), K.conv2d_f16_pick(d)


@pytest.mark.parametrize("shape", NARROW_SHAPES)
def test_conv_f16_epilogue_keeps_nan_and_inf(shape):
    """test_conv_epilogue_keeps_nan_and_inf for the fp16 kernels: the overflow clamp must not turn a NaN or an inf into a number."""
    cout = shape[4]

    def edit(bias):
        bias[3], bias[17], bias[cout - 2] = float("nan"), float("inf"), float("-inf")
    got, pick = _run_plain(shape, edit)
    print(f"[fp16 nan/inf] {pick}")
    assert torch.isnan(got[..., 3]).all()
    assert (got[..., 17] == float("inf")).all() and (got[..., cout - 2] == float("-inf")).all()
    keep = [c for c in range(cout) if c not in (3, 17, cout - 2)]
    assert torch.isfinite(got[..., keep]).all()


@pytest.mark.parametrize("shape", [s for s in NARROW_SHAPES if not s[7] and s[6] == "none"])
def test_conv_f16_overflow_stores_the_largest_finite_value(shape):
    """A finite result beyond +-65504 stores exactly +-65504 (never inf), on the direct and the LDS-staged epilogue."""
    cout = shape[4]

    def edit(bias):
        bias[3], bias[17], bias[cout - 2] = 1.0e5, -1.0e5, 65530.0         # (65530 would ROUND to inf: >= 65520)
    got, pick = _run_plain(shape, edit)
    print(f"[fp16 clamp] {pick}")
    assert (got[..., 3] == 65504.0).all() and (got[..., 17] == -65504.0).all() and (got[..., cout - 2] == 65504.0).all()
    keep = [c for c in range(cout) if c not in (3, 17, cout - 2)]
    assert float(got[..., keep].abs().max()) < 100.0


@pytest.mark.parametrize("which", ["activations", "weights"])
def test_conv_f16_subnormal_operands(which):
    """What v_mfma_f32_*_f16 does with fp16 SUBNORMAL inputs: one operand holds only subnormals (multiples of 2^-24 below 2^-14), the
    other large normal values, fp32 output, no bias.  The result must be the conv of the operands as they are (subnormals honoured)
    or the conv with the subnormal operand flushed to zero (all zeros) - exactly one of the two, within the fp32-output tolerance.
    Prints which; DESIGN.md 3.10 records it."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_NONE, DT_F32
    n, h, w, cin, cout = 1, 16, 16, 64, 128
    g = torch.Generator().manual_seed(5)
    sub = lambda *shape: (torch.randint(1, 1024, shape, generator=g).float() * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)) * 2.0 ** -24
    big = lambda *shape: torch.randn(shape, generator=g) * 512.0
    x = sub(n, cin, h, w) if which == "activations" else big(n, cin, h, w)
    wt = big(cout, cin, 1, 1) if which == "activations" else sub(cout, cin, 1, 1)
    small = x if which == "activations" else wt
    assert torch.equal(_f16r(small), small) and float(small.abs().max()) < 2.0 ** -14 and float(small.abs().min()) > 0       # exact fp16 subnormals
    y = torch.zeros(n, h, w, cout, dtype=torch.float32, device=DEV)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, None, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=1,
                    stride=1, act=ACT_NONE, kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F32)
    K.conv2d_f16(_nhwc(x), wp.to(DEV), bp.to(DEV), y, d)
    torch.cuda.synchronize()
    got = _nchw(y)
    honoured = F.conv2d(_f16r(x), _f16r(wt))
    flushed = torch.zeros_like(honoured)
    assert float(honoured.abs().median()) > 50 * F32_TOL["atol"]          # the two references are far apart
    close = lambda ref: bool(torch.isclose(got, ref, **F32_TOL).all())
    is_h, is_f = close(honoured), close(flushed)
    print(f"[fp16 subnormal {which}] MFMA result matches: subnormals honoured = {is_h}, flushed to zero = {is_f}; "
          f"median |honoured| {float(honoured.abs().median()):.4f}, max |got - honoured| {float((got - honoured).abs().max()):.3e}")
    assert is_h != is_f, "the MFMA result is neither the honoured nor the flushed conv (or the test cannot tell them apart)"


# ---- pointwise -------------------------------------------------------------------------------------
def _signed_f16(shape, seed):
    """fp16 values of both signs with exact +0 / -0 entries, arranged so that no pooling window ties +0 against -0 (the maximum
    of the two is order-dependent in torch): channels [0, c/2) hold negatives and -0, channels [c/2, c) anything and +0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    half = shape[1] // 2
    x[:, :half] = -x[:, :half].abs() - 0.01
    zero = torch.rand(shape, generator=g) < 0.1
    x = _f16r(x)
    x[:, :half][zero[:, :half]] = -0.0
    x[:, half:][zero[:, half:]] = 0.0
    return x


def _bits(t):
    return t.to(torch.float16).view(torch.int16)


@pytest.mark.parametrize("k,s", [(2, 2), (2, 1), (5, 1), (9, 1), (13, 1), (3, 2)])
def test_maxpool_f16_exact(k, s):
    from pytorch_yolo_amd import kernels as K
    from oracle.blocks import max_pool
    n, c, h, w = 2, 16, 13, 20
    x = _signed_f16((n, c, h, w), 100 * k + s)
    want = max_pool(x, k, s)                      # (2, 1) is the reference's pad 1 / dilation 2 special
    pad, dil = ((1, 2) if (k, s) == (2, 1) else ((k - 1) // 2, 1))
    y = torch.full((n, want.shape[2], want.shape[3], c + 8), 3.0, dtype=torch.float16, device=DEV)
    K.maxpool_f16(_nhwc(x), y, n=n, h=h, w=w, c=c, in_view=(c, 0), out_view=(c + 8, 8), ksize=k, stride=s, pad=pad, dilation=dil)
    torch.cuda.synchronize()
    got = y.cpu()
    assert torch.equal(_bits(got[..., 8:].permute(0, 3, 1, 2)), _bits(want)) and torch.all(got[..., :8] == 3.0)
    assert bool((want == 0).any()) and bool((torch.signbit(want) & (want == 0)).any())       # both zeros occur in the result


@pytest.mark.parametrize("h,w,c", [(20, 20, 24), (13, 17, 24), (72, 72, 24), (20, 20, 128), (13, 17, 64), (22, 23, 192), (1, 9, 64)])
def test_spp_on_fp16_data_exact(h, w, c):
    """yolo_spp_fwd orders 16-bit sign-magnitude patterns as integers, so it serves IEEE half unchanged: bit-equal to torch's max pools
    on the widened tensor, negative values, -inf and both zeros included (both SPP kernels and the three-pool form)."""
    from pytorch_yolo_amd import kernels as K
    from oracle.blocks import max_pool
    x = _signed_f16((3, c, h, w), h * 100 + w)
    x[0, 0, 0, 0] = float("-inf")
    x[1, c - 1, h - 1, w - 1] = 65504.0
    x[2, 1, 0, 0] = -(2.0 ** -24)                   # the smallest subnormal: orders between -0 and the normals
    buf = torch.zeros(3, h, w, 4 * c, dtype=torch.float16, device=DEV)
    buf[..., 3 * c:] = _nhwc(x)
    K.spp(buf, n=3, h=h, w=w, c=c)
    torch.cuda.synchronize()
    want = torch.cat([max_pool(x, 5, 1), max_pool(x, 9, 1), max_pool(x, 13, 1), x], 1)
    assert torch.equal(_bits(buf.cpu().permute(0, 3, 1, 2)), _bits(want))


def test_pack_input_f16_exact():
    from pytorch_yolo_amd import kernels as K
    x = torch.rand(3, 3, 17, 23)
    x[0, 0, 0, :4] = torch.tensor([1e6, -1e6, 2.0 ** -24, 2.0 ** -26])
    out = torch.full((3, 17, 23, 8), 7.0, dtype=torch.float16, device=DEV)
    K.pack_input_f16(x.to(DEV), out)
    got = out.cpu().permute(0, 3, 1, 2)
    assert torch.equal(_bits(got[:, :3]), _bits(x.clamp(-65504.0, 65504.0))) and torch.count_nonzero(got[:, 3:]) == 0


# ---- models -----------------------------------------------------------------------------------------
def _assert_close_to_model(io, io_mod, tag, score_max, score_rms, box_abs, box_rel):
    box = (io[..., :4].double() - io_mod[..., :4].double()).abs()
    score = (io[..., 4:].double() - io_mod[..., 4:].double()).abs()
    rms = score.pow(2).mean().sqrt().item()
    print(f"[{tag}] HIP fp16 vs the fp16 CPU rounding model: max box abs {box.max().item():.4f} px, max score abs {score.max().item():.6f}, "
          f"rms score {rms:.7f}")
    assert bool((box <= torch.maximum(torch.tensor(box_abs, dtype=torch.float64), box_rel * io_mod[..., :4].double().abs())).all()), tag
    assert score.max().item() <= score_max and rms <= score_rms, tag


@pytest.mark.parametrize("name", list(C.MODEL_CASES))
def test_fp16_model_small_vs_its_rounding_model(name):
    from oracle import models as om
    from oracle.policy import run_policy
    case = C.MODEL_CASES[name]
    model, sd, x = build_case(case)
    fwd = {"spp": om.spp_forward, "tiny": om.tiny_forward, "yolov3": om.yolov3_forward, "lite": om.lite_forward}[case[0]]
    with fp16_policy():
        io_mod, p_mod = run_policy(fwd, sd, x, case[1]["anchors"], case[1]["n_class"], policy="bf16")
    io_ref, _ = oracle_forward(case, sd, x)
    model = model.to(DEV)
    model.precision = "fp16"
    with torch.no_grad():
        io, p = model(x.to(DEV))
    assert io.shape == io_mod.shape and [t.shape for t in p] == [t.shape for t in p_mod]
    s = 2.0 if case[0] == "yolov3" else 1.0          # (the bf16 test's allowance for Darknet-53's depth in front of plain heads)
    _assert_close_to_model(io.cpu(), io_mod, name, score_max=s * 2e-2 / 8, score_rms=2e-3 / 8, box_abs=1.5 / 8, box_rel=0.02 / 8)
    # ... and within the bf16 mode's own bounds of the fp32 oracle
    err = (io.cpu() - io_ref).abs()
    assert bool((err[..., :4] <= torch.maximum(torch.tensor(1.5), 0.02 * io_ref[..., :4].abs())).all()) and float(err[..., 4:].max()) <= s * 2e-2
    # the default mode of the same model object is untouched by the fp16 plan
    model.precision = "bf16"
    with torch.no_grad():
        io_b, _ = model(x.to(DEV))
    assert not torch.equal(io_b, io)


@pytest.mark.parametrize("name", ["spp_kd2_nc80", "tiny_small", "yolov3_small"])
def test_fp16_detect_is_nms_of_forward(name):
    """detect() in fp16 (the compact NMS form: the heads filter their own rows) == non_max_suppression(model(x)[0]) bit for bit;
    a second call and the HIP-graph replay give the same bits."""
    from pytorch_yolo_amd.utils.utils import non_max_suppression
    case = C.MODEL_CASES[name]
    model, sd, x = build_case(case)
    model = model.to(DEV)
    model.precision = "fp16"
    xd = x.to(DEV)
    with torch.no_grad():
        io1, p1 = model(xd)
        plan = model.plan_for(xd)
        assert plan.compact_ok and plan.precision == "fp16"
        score = io1[..., 4] * io1[..., 5:].max(-1).values
        conf = float(score.flatten().kthvalue(int(0.97 * score.numel())).values)
        dets = model.detect(xd, conf_thres=conf, nms_thres=0.5)
        want = non_max_suppression(io1, conf, 0.5)
        assert any(t is not None for t in want)
        for a, b in zip(dets, want):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        streamed = list(model.detect_stream([xd] * 3, conf, 0.5))
        assert len(streamed) == 3 and all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for lst in streamed for a, b in zip(lst, want))
        io2, _ = model(xd)
        model.use_hip_graph = True
        io3, p3 = model(xd)
        io3 = io3.clone()
        io4, _ = model(xd)
    assert torch.equal(io1, io2) and torch.equal(io1, io3) and torch.equal(io1, io4)
    assert all(torch.equal(a, b) for a, b in zip(p1, p3))


def test_fp16_bs32_streams_and_whole_batch_agree():
    """32 tiny-416 images: the two-stream plan (16 + 16), a one-stream plan and detect()'s path give the same bits."""
    from pytorch_yolo_amd import YOLOv3Tiny
    from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict
    model = YOLOv3Tiny().eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234, n_class=80))
    model = model.to(DEV)
    model.precision = "fp16"
    x = synth_images(32, 416, 416, 3).to(DEV)
    with torch.no_grad():
        model.n_streams = 2
        io2, _ = model(x)
        assert model.plan_for(x).n_streams == 2
        model.n_streams = 1
        io1, _ = model(x)
    assert torch.equal(io1, io2) and bool(torch.isfinite(io1).all())


# ---- budget and pairing on SPP-640 ---------------------------------------------------------------------
def test_fp16_path_within_its_rounding_budget():
    """The fp16 twin of test_bf16_path_within_its_rounding_budget (spp_640): per head, the distance of the HIP fp16 forward to the fp32
    reference is at most 1.25 x the distance fp16 operand rounding alone produces on the CPU (the project's head-room) + 2e-5 (20 x
    the 1e-6 relative fp32 summation-order noise of the fp32-mode tests); the same form for the score rms.  The budget comes from
    the reference arithmetic, never from the code under test."""
    from oracle import models as om
    from oracle.policy import run_policy
    case = C.FULL_CASES["spp_640"]
    model, sd, x = build_case(case)
    with fp16_policy():
        io_pol, p_pol = run_policy(om.spp_forward, sd, x, C.SPP_ANCHORS, 80, policy="bf16")
    io_ref, p_ref = oracle_forward(case, sd, x)
    model = model.to(DEV)
    model.precision = "fp16"
    with torch.no_grad():
        io, p = model(x.to(DEV))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    results = []
    for k in range(3):
        got, budget = rel(p[k].cpu(), p_ref[k]), rel(p_pol[k], p_ref[k])
        print(f"[spp_640 fp16] head {k} raw logits vs fp32 reference: rel rms {got:.6f} (fp16 CPU model {budget:.6f}); "
              f"max abs {float((p[k].cpu() - p_ref[k]).abs().max()):.4f} (model {float((p_pol[k] - p_ref[k]).abs().max()):.4f})")
        results.append((got, budget))
    rms = lambda a, b: float((a[..., 4:].double() - b[..., 4:].double()).pow(2).mean().sqrt())
    got_s, budget_s = rms(io.cpu(), io_ref), rms(io_pol, io_ref)
    print(f"[spp_640 fp16] scores vs fp32 reference: rms {got_s:.7f} (fp16 CPU model {budget_s:.7f}); max {float((io.cpu()[..., 4:] - io_ref[..., 4:]).abs().max()):.5f}")
    for k, (got, budget) in enumerate(results):
        assert got <= 1.25 * budget + 2e-5, f"head {k}: error {got} beyond the fp16 rounding budget {budget}"
    assert got_s <= 1.25 * budget_s + 2e-5


def _seeded_batch(n, hw, first_seed=0):
    from pytorch_yolo_amd.utils.synthetic import synth_images
    return torch.cat([synth_images(1, hw, hw, first_seed + i) for i in range(n)], 0)


def test_fp16_strict_pairing_rate_on_generic_weights():
    """Strict pairing (same class, IoU >= 0.9, |dconf| <= 0.03) of the fp16 mode's detections on GENERIC weights:
      * golden image, against the reference's own detections: at least 0.9 x the fp16 CPU rounding model's rate - 0.02 (the bf16 rule);
      * the 32-image bench batch, against the fp32 oracle's detections: in both directions at least the bf16 mode's rate on the
        same batch, computed here on the unchanged bf16 path; the count within 10 % of the oracle's.
    The table is printed (profiles/fp16_pairing_rate.txt holds it)."""
    from oracle import models as om, nms as onms
    from oracle.policy import run_policy
    case = C.FULL_CASES["spp_640"]
    model, sd, x0 = build_case(case)
    ref = load_golden("full_spp_640")["nms_dets_0"]
    x = _seeded_batch(32, 640)
    assert torch.equal(x[:1], x0)
    model = model.to(DEV)
    model.n_streams = 2
    dets = {}
    for mode in ("bf16", "fp16"):
        model.precision = mode
        with torch.no_grad():
            out = model.detect(x.to(DEV), **C.NMS_FULL)
        dets[mode] = [np.zeros((0, 7), np.float32) if t is None else t.cpu().numpy() for t in out]
    lines = []
    gold = {}
    for mode in ("bf16", "fp16"):
        d0 = dets[mode][0]
        gold[mode] = (strict_share(ref, d0), strict_share(d0, ref))
        lines.append(f"golden image vs the REFERENCE's detections: reference {len(ref)}, {mode} {len(d0)}; strict (IoU 0.9, dconf 0.03) "
                     f"{gold[mode][0]:.3f} / {gold[mode][1]:.3f}; loose (IoU 0.7, dconf 0.06) {strict_share(ref, d0, 0.7, 0.06):.3f} / {strict_share(d0, ref, 0.7, 0.06):.3f}")
    with fp16_policy():
        io_pol, _ = run_policy(om.spp_forward, sd, x[:1], C.SPP_ANCHORS, 80, policy="bf16")
    dp, _ = onms.non_max_suppression(io_pol.numpy().copy(), **C.NMS_FULL)
    pa, pb = strict_share(ref, dp[0]), strict_share(dp[0], ref)
    lines.append(f"golden image, fp16 CPU rounding model vs the reference: {len(dp[0])} detections; strict {pa:.3f} / {pb:.3f}")
    tot = {m: [0, 0, 0, 0] for m in dets}                        # oracle dets, paired strictly, mode dets, paired strictly
    per_image = {m: [] for m in dets}
    with torch.no_grad():
        for lo in range(0, 32, 4):
            io_ref, _ = om.spp_forward(sd, x[lo:lo + 4], C.SPP_ANCHORS, 80)
            od, _ = onms.non_max_suppression(io_ref.numpy().copy(), **C.NMS_FULL)
            for i in range(4):
                o = np.zeros((0, 7), np.float32) if od[i] is None else od[i]
                for m in dets:
                    h = dets[m][lo + i]
                    sa, sb = strict_share(o, h), strict_share(h, o)
                    per_image[m].append(min(sa, sb))
                    t = tot[m]
                    t[0] += len(o); t[1] += round(sa * len(o)); t[2] += len(h); t[3] += round(sb * len(h))
    rate = {}
    for m in ("bf16", "fp16"):
        t = tot[m]
        rate[m] = (t[1] / max(1, t[0]), t[3] / max(1, t[2]))
        lines.append(f"32-image batch vs the fp32 ORACLE's detections: oracle {t[0]}, {m} {t[2]}; strict {rate[m][0]:.3f} / {rate[m][1]:.3f}; "
                     f"per image (min of both directions): min {min(per_image[m]):.3f}, median {sorted(per_image[m])[16]:.3f}, max {max(per_image[m]):.3f}")
    for ln in lines:
        print("[fp16 pairing rate] " + ln)
    try:                                                         # (a read-only checkout keeps the committed table)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fp16_pairing_rate.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass
    assert min(gold["fp16"]) >= 0.9 * min(pa, pb) - 0.02, "the HIP fp16 path pairs worse with the reference than its CPU rounding model does"
    assert rate["fp16"][0] >= rate["bf16"][0] and rate["fp16"][1] >= rate["bf16"][1], "fp16 pairs worse with the oracle than bf16 does"
    assert abs(tot["fp16"][0] - tot["fp16"][2]) <= 0.1 * tot["fp16"][0]


@pytest.mark.parametrize("seed", C.RULE_SEEDS)
def test_fp16_rule_selected_detections_strictly_vs_reference(seed):
    """The rule-selected cases (tests/_cases.py::RULE) in fp16: every reference detection has an fp16 partner and vice versa (strict
    share >= 0.95 in both directions), same count - the bf16 mode's requirement."""
    from pytorch_yolo_amd.utils.utils import non_max_suppression
    rule = C.RULE
    model, sd, x, g = build_rule_case(seed)
    ref = g["nms_dets_0"]
    model = model.to(DEV)
    model.precision = "fp16"
    with torch.no_grad():
        io16, _ = model(x.to(DEV))
        dets16 = non_max_suppression(io16, rule["conf_thres"], rule["nms_thres"])
        det_c = model.detect(x.to(DEV), rule["conf_thres"], rule["nms_thres"])
    d16 = dets16[0].cpu().numpy()
    a, b = strict_share(ref, d16), strict_share(d16, ref)
    print(f"[rule case {seed}] reference {len(ref)} detections, fp16 {len(d16)}; strict share (IoU 0.9, dconf 0.03) {a:.3f} / {b:.3f}")
    assert min(a, b) >= 0.95 and len(d16) == len(ref)
    assert torch.equal(det_c[0], dets16[0])
