"""GPU tests of the fp16 forms of the 20x20-tile 3x3 kernels (csrc/conv3x3_t20.h, conv3x3_t20_f16.hip): the kernels
through yolo_conv3x3_t20_f16_fwd(force = 1) against torch on the same fp16-rounded operands, their narrowing, and YOLOv3-SPP with
enough images for the shipped rule to put them into the plan.

Tolerances are those of tests/test_fp16_gpu.py: fp16 output within rtol = atol = 1e-3 of the fp32 conv of the same fp16-rounded
operands (twice fp16's half-ulp 2^-11: one rounding of the result, plus a flip where the fp32 sums differ in their last bits);
the model within 1.25 x the fp16 CPU rounding model's distance to the fp32 oracle + 2e-5 per head."""
import pytest
import torch
import torch.nn.functional as F

import _cases as C
from helpers import build_case, oracle_forward

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_TOL = dict(rtol=1e-3, atol=1e-3)

_ACTS = {"leaky": lambda t: F.leaky_relu(t, 0.1), "none": lambda t: t, "relu6": F.relu6}


def _f16r(t):
    return t.to(torch.float16).float()


def _nhwc(t):      # NCHW f32 -> NHWC fp16 on device
    return t.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV)


def _nchw(t):      # NHWC (any dtype) on device -> NCHW f32 on host
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def _act_code(act):
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU6
    return {"leaky": ACT_LEAKY01, "none": ACT_NONE, "relu6": ACT_RELU6}[act]


class fp16_policy:
    """with fp16_policy(): oracle.policy.run_policy(..., policy="bf16") rounds its operands and its residual stream to IEEE half
    instead of bf16 - the CPU rounding model of the fp16 mode, as in tests/test_fp16_gpu.py."""

    def __enter__(self):
        from oracle import policy
        self.policy, self.old = policy, policy.bf16r
        policy.bf16r = lambda t: t.to(torch.float16).float()

    def __exit__(self, *exc):
        self.policy.bf16r = self.old
        return False


T20_F16_CASES = [
    # n, h, w (input), cin, cout, stride, act, residual (in place: residual == y), pre-add copy
    # -- stride 1: the shape classes of test_t20_conv_kernel
    (2, 40, 40, 64, 256, 1, "leaky", True, True),
    (1, 80, 80, 32, 128, 1, "leaky", False, False),       # one channel chunk: prologue only, no halo double-buffering
    (3, 37, 41, 96, 384, 1, "leaky", True, True),         # partial tiles on both edges of every image, three chunks, three cout tiles
    (1, 20, 20, 256, 512, 1, "relu6", False, True),       # one tile per image, eight chunks; the generic epilogue
    (2, 33, 47, 96, 128, 1, "none", True, False),         # partial tiles, generic epilogue, residual without a copy
    # -- stride 2: the shape classes of test_t20_stride2_conv_kernel (even chunk counts run the chunk-pair order)
    (2, 80, 80, 64, 128, 2, "leaky", True, False),        # whole tiles, one chunk pair
    (1, 40, 40, 256, 512, 2, "leaky", False, True),       # one tile per image, four pairs, four cout tiles
    (3, 75, 83, 96, 256, 2, "none", False, True),         # odd input sizes: 38 x 42 outputs, partial tiles, three chunks (chunk by chunk)
    (2, 41, 40, 32, 128, 2, "relu6", False, False),       # one chunk: prologue and the dummy plane only; the last input row is used
    (1, 160, 160, 128, 256, 2, "leaky", False, False),    # 16 tiles per image
    (1, 150, 146, 512, 128, 2, "leaky", True, True),      # eight pairs, partial tiles
]


@pytest.mark.parametrize("case", T20_F16_CASES, ids=lambda c: "n%d_%dx%d_c%d-%d_s%d_%s_r%d_a%d" % tuple(int(v) if not isinstance(v, str) else v for v in c))
def test_t20_f16_conv_kernel(case):
    """Both fp16 tile kernels forced onto every shape class they take: against the fp32 conv of the same fp16-rounded operands
    (the yardstick of test_conv_f16_kernel), with channel-offset views - NaN in the input channels next to the view, sentinels
    around the output and the pre-add copy -, the residual read from and written to the same view, run to run bit-identical.
    Prints the share of outputs that differ from the fp16 gather kernel's (a record: two fp32 summation orders)."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F16
    n, h, w, cin, cout, stride, act, use_res, use_aux = case
    g = torch.Generator().manual_seed(100 + T20_F16_CASES.index(case))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    res = torch.randn(n, cout, ho, wo, generator=g) if use_res else None
    in_ct, in_co = cin + 16, 8
    xin = torch.full((n, h, w, in_ct), float("nan"), dtype=torch.float16, device=DEV)
    xin[..., in_co:in_co + cin] = _nhwc(x)
    out_ct, out_co = cout + 16, 8
    aux_ct, aux_co = cout + 8, 8
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, bias, cin)
    wp, bp = wp.to(DEV), bp.to(DEV)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=in_ct, in_c_offset=in_co, cout=cout, out_c_total=out_ct, out_c_offset=out_co,
                    ksize=3, stride=stride, act=_act_code(act), kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F16,
                    res=(out_ct, out_co) if use_res else (0, 0), aux=(aux_ct, aux_co) if use_aux else (0, 0))
    assert (d.ho, d.wo) == (ho, wo)

    def run(fn, **kw):
        y = torch.full((n, ho, wo, out_ct), -77.0, dtype=torch.float16, device=DEV)
        if use_res:
            y[..., out_co:out_co + cout] = _nhwc(res)            # in place: the residual is what the output view holds
        aux = torch.full((n, ho, wo, aux_ct), -77.0, dtype=torch.float16, device=DEV) if use_aux else None
        fn(xin, wp, bp, y, d, residual=y if use_res else None, y_preadd=aux, **kw)
        torch.cuda.synchronize()
        return y, aux

    y, aux = run(K.conv3x3_t20_f16, force=True)
    pre = _ACTS[act](F.conv2d(_f16r(x), _f16r(wt), bias, stride=stride, padding=1))
    ref = pre + _f16r(res) if use_res else pre
    got = _nchw(y[..., out_co:out_co + cout])
    print(f"[t20 f16] max |got - ref| {float((got - ref).abs().max()):.3e}, max rel {float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max()):.3e}")
    torch.testing.assert_close(got, ref, **F16_TOL)
    assert torch.all(y[..., :out_co] == -77.0) and torch.all(y[..., out_co + cout:] == -77.0)
    if use_aux:
        torch.testing.assert_close(_nchw(aux[..., aux_co:aux_co + cout]), pre, **F16_TOL)
        assert torch.all(aux[..., :aux_co] == -77.0)
    y2, aux2 = run(K.conv3x3_t20_f16, force=True)
    assert torch.equal(y, y2) and (aux is None or torch.equal(aux, aux2))
    y0, aux0 = run(K.conv2d_f16)                                  # the gather kernel on the same operands and views
    differ = float((y[..., out_co:out_co + cout] != y0[..., out_co:out_co + cout]).float().mean())
    print(f"[t20 f16] {differ:.4f} of the outputs differ from yolo_conv2d_f16_fwd's ({K.conv2d_f16_pick(d, use_res, use_aux)})")


def _run_t20(stride, act, bias_edit):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F16
    n, hw, cin, cout = 1, 40 * stride, 64, 128
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, hw, hw, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    bias_edit(bias)
    y = torch.zeros(n, 40, 40, cout, dtype=torch.float16, device=DEV)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(wt, bias, cin)
    d = K.conv_desc(n=n, h=hw, w=hw, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=3,
                    stride=stride, act=_act_code(act), kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F16)
    K.conv3x3_t20_f16(_nhwc(x), wp.to(DEV), bp.to(DEV), y, d, force=True)
    torch.cuda.synchronize()
    return y.float().cpu()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", ["leaky", "none"])       # the LeakyReLU fast path (leaky4) and the generic min(max()) epilogue
def test_t20_f16_epilogue_keeps_nan_and_inf(stride, act):
    """The inputs of test_conv_f16_epilogue_keeps_nan_and_inf on the tile kernels: the overflow clamp of the narrowing must not turn a
    NaN or an inf pre-activation into a number."""
    cout = 128

    def edit(bias):
        bias[3], bias[17], bias[cout - 2] = float("nan"), float("inf"), float("-inf")
    got = _run_t20(stride, act, edit)
    assert torch.isnan(got[..., 3]).all()
    assert (got[..., 17] == float("inf")).all() and (got[..., cout - 2] == float("-inf")).all()
    keep = [c for c in range(cout) if c not in (3, 17, cout - 2)]
    assert torch.isfinite(got[..., keep]).all()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("act", ["leaky", "none"])
def test_t20_f16_overflow_stores_the_largest_finite_value(stride, act):
    """The inputs of test_conv_f16_overflow_stores_the_largest_finite_value: a finite result beyond +-65504 stores exactly +-65504,
    never inf.  (LeakyReLU scales the -1e5 channel to about -1e4, which is in range: a channel at -1e6 shows the negative clamp there.)"""
    cout = 128

    def edit(bias):
        bias[3], bias[17], bias[cout - 2], bias[40] = 1.0e5, -1.0e5, 65530.0, -1.0e6        # (65530 would ROUND to inf: >= 65520)
    got = _run_t20(stride, act, edit)
    assert (got[..., 3] == 65504.0).all() and (got[..., cout - 2] == 65504.0).all() and (got[..., 40] == -65504.0).all()
    if act == "none":
        assert (got[..., 17] == -65504.0).all()
    else:
        assert float((got[..., 17] + 1.0e4).abs().max()) <= 16.0          # 0.1 x (-1e5 + a conv sum of a few units), fp16 spacing 8
    keep = [c for c in range(cout) if c not in (3, 17, cout - 2, 40)]
    assert float(got[..., keep].abs().max()) < 100.0


def test_fwd_follows_the_rule_without_force():
    """force = 0: a layer yolo_conv3x3_t20_f16_supported refuses is YOLO_E_UNSUPPORTED and nothing is written; one it accepts runs."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F16
    for n, ok in ((1, False), (8, True)):                         # 80x80 128 -> 256: 16 tiles x 2 x images against 128 workgroups
        d = K.conv_desc(n=n, h=80, w=80, cin=128, in_c_total=128, in_c_offset=0, cout=256, out_c_total=256, out_c_offset=0, ksize=3,
                        stride=1, act=_act_code("leaky"), kpad=1152, cout_pad=256, out_dtype=DT_F16)
        assert K.conv3x3_t20_f16_supported(d) == ok
        g = torch.Generator().manual_seed(n)
        x = torch.randn(n, 128, 80, 80, generator=g)
        wt = torch.randn(256, 128, 3, 3, generator=g) * (2.0 / 1152) ** 0.5
        wp, bp, _, _ = K.pack_conv_weight_f16(wt, None, 128)
        y = torch.full((n, 80, 80, 256), -77.0, dtype=torch.float16, device=DEV)
        if not ok:
            with pytest.raises(RuntimeError, match="shipped rule"):
                K.conv3x3_t20_f16(_nhwc(x), wp.to(DEV), bp.to(DEV), y, d)
            torch.cuda.synchronize()
            assert torch.all(y == -77.0)
        else:
            K.conv3x3_t20_f16(_nhwc(x), wp.to(DEV), bp.to(DEV), y, d)
            torch.cuda.synchronize()
            torch.testing.assert_close(_nchw(y), F.leaky_relu(F.conv2d(_f16r(x), _f16r(wt), padding=1), 0.1), **F16_TOL)


def test_fp16_spp640_x16_runs_the_tile_kernels_within_the_rounding_budget():
    """FULL_CASES["spp_640"] with its image replicated to 16 images on one stream, so that the shipped rule puts OP_CONV_T20_F16 on
    the 160 / 80 / 40 / 20 maps and the first stride-2 layers.  Every replica's head logits stay within the budget of
    test_fp16_path_within_its_rounding_budget - per head rel <= 1.25 x (the fp16 CPU rounding model's distance to the fp32 oracle)
    + 2e-5, the budget computed once, on the single image, from the oracle -, all 16 replicas are bit-equal, and detect() on that
    plan is non_max_suppression(forward()[0])."""
    from oracle import models as om
    from oracle.policy import run_policy
    from pytorch_yolo_amd._lib import OP_CONV_F16, OP_CONV_T20_F16
    from pytorch_yolo_amd.utils.utils import non_max_suppression
    case = C.FULL_CASES["spp_640"]
    model, sd, x = build_case(case)
    with fp16_policy():
        _, p_pol = run_policy(om.spp_forward, sd, x, C.SPP_ANCHORS, 80, policy="bf16")
    _, p_ref = oracle_forward(case, sd, x)
    model = model.to(DEV)
    model.precision = "fp16"
    model.n_streams = 1
    xd = x.to(DEV).repeat(16, 1, 1, 1).contiguous()
    with torch.no_grad():
        io, p = model(xd)
        plan = model.plan_for(xd)
        kinds = [plan.op_array[i] for i in range(plan.n_ops)]
        t20 = [(o.conv.h, o.conv.stride) for o in kinds if o.kind == OP_CONV_T20_F16]
        print(f"[spp_640 x16 fp16] {len(t20)} OP_CONV_T20_F16 launches, {sum(o.kind == OP_CONV_F16 for o in kinds)} OP_CONV_F16; maps {sorted(set(t20))}")
        assert plan.precision == "fp16" and {(160, 1), (80, 1), (40, 1), (20, 1), (320, 2), (160, 2)} <= set(t20)
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        for k in range(3):
            budget = rel(p_pol[k], p_ref[k])
            pk = p[k].cpu()
            worst = max(rel(pk[i:i + 1], p_ref[k]) for i in range(16))
            print(f"[spp_640 x16 fp16] head {k} raw logits vs fp32 reference: worst replica rel rms {worst:.6f} (fp16 CPU model {budget:.6f})")
            assert worst <= 1.25 * budget + 2e-5, f"head {k}: error {worst} beyond the fp16 rounding budget {budget}"
            assert all(torch.equal(pk[i], pk[0]) for i in range(1, 16)), f"head {k}: replicas differ"
        assert all(torch.equal(io[i], io[0]) for i in range(1, 16))
        dets = model.detect(xd, **C.NMS_FULL)
        assert model.plan_for(xd) is plan
        want = non_max_suppression(io, C.NMS_FULL["conf_thres"], C.NMS_FULL["nms_thres"])
        assert any(t is not None for t in want)
        for a, b in zip(dets, want):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
