"""Helpers of the YOLOv3-tiny/MobileNetV2 training tests: the restated fused expand + depthwise op, its operands, the CPU
float64 op table of DEVICE_OPS_MOBILE, the torch reference of one training step and the eval trace as plain data.

The fused op restated: the operand of the depthwise conv is y = clamp_forward(zin, saved_in) of tests/_dw_train.py INSIDE the map and 0
outside it, so it is dw_forward / dw_bwd_weight of that module applied to the materialised y (their padding is a zero of y).
``inject="pad"`` is the fault the tests must see: the padding taken as the clamp of a zero zin, clamp(shift), instead of 0.
"""
import copy
import json
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import _bn as N
import _dw_train as D
import _train as T
import _train_pool as TP
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import graph

F32, F64 = np.float32, np.float64
CTOR = dict(n_class=2)
TRACE_SIZE = 416
NEW_OPS = ("conv_bn_relu6_block", "dw_bn_block", "project_bn_block", "expand_dw_bn_block")

# (n, h, w, c, stride) of the kernel tests beside tests/_dw_train.CASES: windows that are mostly padding, a partial second strip of 8
# output rows at either stride
EXTRA_CASES = [(2, 1, 1, 8, 1), (2, 2, 1, 8, 2), (1, 9, 3, 8, 1), (1, 17, 4, 8, 2)]
KERNEL_CASES = D.CASES + EXTRA_CASES


# ---- the fused op restated ---------------------------------------------------------------------------------------------------------------
def bnin_operand(zin, saved, lo=0.0, hi=6.0, rounding=True):
    """y [n, h, w, c] inside the map: tests/_dw_train.clamp_forward on the rows of zin."""
    zin = np.asarray(zin)
    return D.clamp_forward(zin.reshape(-1, zin.shape[-1]), saved, lo, hi, rounding).reshape(zin.shape)


def _pad_value(saved, lo, hi, rounding):
    """What a kernel that clamps a zero zin would take for the padding: clamp(shift)."""
    c = saved.shape[1]
    return D.clamp_forward(np.zeros((1, c), dtype=F32 if rounding else F64), saved, lo, hi, rounding)[0]


def _padded(y, saved, lo, hi, rounding):
    p = np.empty((y.shape[0], y.shape[1] + 2, y.shape[2] + 2, y.shape[3]), dtype=y.dtype)
    p[:] = _pad_value(saved, lo, hi, rounding)
    p[:, 1:-1, 1:-1] = y
    return p


def fused_forward(zin, saved, w, stride, lo=0.0, hi=6.0, rounding=True, inject=None):
    """z [n, ho, wo, c] of the depthwise conv on the batch-normed and clamped zin; w [c, 3, 3]."""
    y = bnin_operand(zin, saved, lo, hi, rounding)
    if inject is None:
        return D.dw_forward(y, w, stride, rounding)
    assert inject == "pad"
    # the same conv on the map padded by hand with clamp(shift): its stride-1 output at the centres (1 + s oh, 1 + s ow)
    full = D.dw_forward(_padded(y, saved, lo, hi, rounding), w, 1, rounding)
    return full[:, 1:-1:stride, 1:-1:stride]


def fused_bwd_weight(zin, saved, g, stride, lo=0.0, hi=6.0, rounding=True, inject=None):
    """tests/_dw_train.dw_bwd_weight's dict for the same operand."""
    y = bnin_operand(zin, saved, lo, hi, rounding)
    if inject is None:
        return D.dw_bwd_weight(y, g, stride, rounding)
    assert inject == "pad"
    g = np.asarray(g)
    gp = np.zeros((y.shape[0], y.shape[1] + 2, y.shape[2] + 2, y.shape[3]), dtype=g.dtype)
    gp[:, 1:-1:stride, 1:-1:stride] = g
    return D.dw_bwd_weight(_padded(y, saved, lo, hi, rounding), gp, 1, rounding)


def channel_shifts(c):
    """Integer shifts in [1, 4] that differ from channel to channel and from one chunk of 8 channels to the next."""
    ch = np.arange(c)
    return (1 + (3 * ch + ch // 8) % 4).astype(F32)


def integer_operands(case, seed=0):
    """zin: integers in [-4, 4]; saved = (mean 0, invstd 1, scale 1, channel_shifts); w in [-2, 2] asymmetric and g in [-7, 7] from
    tests/_dw_train.integer_operands.  a = zin + shift is an integer in [-3, 8]: both bounds of ReLU6 and the values beside them; every
    product and sum is exact (|z| <= 9 * 6 * 2 = 108 < 256).  Every shift is >= 1, so clamp(shift) != 0 in every channel."""
    n, h, wd, c, stride = case
    _, w, g = D.integer_operands(case, seed)
    zin = np.random.default_rng(8100 + seed).integers(-4, 5, (n, h, wd, c)).astype(F32)
    saved = np.stack([np.zeros(c, F32), np.ones(c, F32), np.ones(c, F32), channel_shifts(c)])
    return zin, saved, w, g


def random_operands(case, seed=0):
    """zin ~ N(0, 1) as bf16 values, saved with scale in [1, 3] and shift ~ N(3, 1) (a reaches both bounds, shift > 0 almost everywhere),
    w and g from tests/_dw_train.random_operands."""
    n, h, wd, c, stride = case
    _, w, g = D.random_operands(case, seed)
    rng = np.random.default_rng(9100 + seed)
    zin = D.bf16(rng.standard_normal((n, h, wd, c)).astype(F32))
    saved = np.stack([rng.standard_normal(c), rng.uniform(0.5, 2.0, c), rng.uniform(1.0, 3.0, c), 3.0 + rng.standard_normal(c)]).astype(F32)
    return zin, saved, w, g


# ---- the CPU op table ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=F64))).permute(0, 3, 1, 2).contiguous()


def _v(a):
    return torch.from_numpy(np.asarray(a, dtype=F64).copy())


def bn_forward(z, gamma, beta, act, running, momentum, eps, rounding):
    """tests/_dw_train.bn_forward with the BatchNorm2d's own momentum and eps; the running tensors (float64 torch or None) are updated."""
    rows = z.reshape(-1, z.shape[-1])
    rm, rv = running
    st = N.stats(rows, gamma.detach().numpy(), beta.detach().numpy(), eps, momentum, None if rm is None else rm.numpy(),
                 None if rv is None else rv.numpy(), rounding)
    if rm is not None:
        rm.copy_(_v(st["rm"]))
    if rv is not None:
        rv.copy_(_v(st["rv"]))
    y = D.clamp_forward(rows, st["saved"], act[0], act[1], rounding) if isinstance(act, tuple) else N.forward(rows, st["saved"], "none", rounding)
    return y.reshape(z.shape), dict(z=z, saved=st["saved"], act=act)


class _DenseBn(torch.autograd.Function):
    """conv (1x1 or 3x3, stride 1 or 2) -> batch statistics -> ReLU6 or nothing [-> + residual]."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, running, momentum, eps, stride, act, rounding):
        xn, wn = _np(x), w.detach().numpy()
        z = D.dense_forward(xn, wn, stride, rounding)
        y, cache = bn_forward(z, gamma, beta, act, running, momentum, eps, rounding)
        ctx.keep = (xn, wn, cache, stride, rounding)
        if residual is not None:
            y = D.bf16(y + _np(residual).astype(F32)) if rounding else y + _np(residual)
        return _t(y)

    @staticmethod
    def backward(ctx, dy):
        xn, wn, cache, stride, rounding = ctx.keep
        g, dgamma, dbeta = D.bn_backward(_np(dy), cache, rounding)
        dx, dw, _ = D.dense_backward(xn, wn, g, stride, rounding)
        return (_t(dx), _v(dw), _v(dgamma), _v(dbeta), dy if ctx.needs_input_grad[4] else None) + (None,) * 6


class _DwBn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, running, momentum, eps, stride, rounding):
        xn, wn = _np(x), w.detach().numpy()[:, 0]
        wq = D.bf16(wn.astype(F32)) if rounding else wn
        z = D.dw_forward(xn, wq, stride, rounding)
        y, cache = bn_forward(z, gamma, beta, D.RELU6, running, momentum, eps, rounding)
        ctx.keep = (xn, wq, cache, stride, rounding)
        return _t(y)

    @staticmethod
    def backward(ctx, dy):
        xn, wq, cache, stride, rounding = ctx.keep
        g, dgamma, dbeta = D.bn_backward(_np(dy), cache, rounding)
        dx = D.dw_bwd_data(g, wq, xn.shape, stride, rounding)
        dw = D.dw_bwd_weight(xn, g, stride, rounding)["dw"]
        return (_t(dx), _v(dw)[:, None], _v(dgamma), _v(dbeta)) + (None,) * 5


class _ExpandDw(torch.autograd.Function):
    """The fused op from the restatements above: y1 is never formed outside fused_forward / fused_bwd_weight."""

    @staticmethod
    def forward(ctx, x, we, gamma1, beta1, wd, gamma2, beta2, running1, running2, m1, e1, m2, e2, stride, rounding, inject):
        xn, wen, wdn = _np(x), we.detach().numpy(), wd.detach().numpy()[:, 0]
        wq = D.bf16(wdn.astype(F32)) if rounding else wdn
        z1 = D.dense_forward(xn, wen, 1, rounding)
        _, c1 = bn_forward(z1, gamma1, beta1, D.RELU6, running1, m1, e1, rounding)
        z2 = fused_forward(z1, c1["saved"], wq, stride, 0.0, 6.0, rounding, inject)
        y2, c2 = bn_forward(z2, gamma2, beta2, D.RELU6, running2, m2, e2, rounding)
        ctx.keep = (xn, wen, wq, c1, c2, stride, rounding, inject)
        return _t(y2)

    @staticmethod
    def backward(ctx, dy):
        xn, wen, wq, c1, c2, stride, rounding, inject = ctx.keep
        g2, dgamma2, dbeta2 = D.bn_backward(_np(dy), c2, rounding)
        d1 = D.dw_bwd_data(g2, wq, c1["z"].shape, stride, rounding)
        dwd = fused_bwd_weight(c1["z"], c1["saved"], g2, stride, 0.0, 6.0, rounding, inject)["dw"]
        g1, dgamma1, dbeta1 = D.bn_backward(d1, c1, rounding)
        dx, dwe, _ = D.dense_backward(xn, wen, g1, 1, rounding)
        return (_t(dx), _v(dwe), _v(dgamma1), _v(dbeta1), _v(dwd)[:, None], _v(dgamma2), _v(dbeta2)) + (None,) * 9


def _running(rm, rv):
    return (None if rm is None else rm.detach(), None if rv is None else rv.detach())


def _two(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def cpu_ops(rounding, inject=None):
    """The table of models/train.mobile_ops on the CPU: tests/_train_pool.cpu_ops plus the four ops of an inverted residual; float64
    tensors in and out.  ``inject``: the fused op's padding fault."""
    def conv_bn_relu6_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        return _DenseBn.apply(x, w, gamma, beta, None, _running(rm, rv), momentum, eps, stride, D.RELU6, rounding)

    def dw_bn_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, act="relu6", momentum=0.1, eps=1e-5, training=True):
        assert act == "relu6"
        return _DwBn.apply(x, w, gamma, beta, _running(rm, rv), momentum, eps, stride, rounding)

    def project_bn_block(x, w, gamma, beta, rm=None, rv=None, residual=None, *, momentum=0.1, eps=1e-5, training=True):
        return _DenseBn.apply(x, w, gamma, beta, residual, _running(rm, rv), momentum, eps, 1, "none", rounding)

    def expand_dw_bn_block(x, we, gamma1, beta1, rm1, rv1, wd, gamma2, beta2, rm2, rv2, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        (m1, m2), (e1, e2) = _two(momentum), _two(eps)
        return _ExpandDw.apply(x, we, gamma1, beta1, wd, gamma2, beta2, _running(rm1, rv1), _running(rm2, rv2), m1, e1, m2, e2, stride,
                               rounding, inject)

    return SimpleNamespace(**vars(TP.cpu_ops(rounding)), conv_bn_relu6_block=conv_bn_relu6_block, dw_bn_block=dw_bn_block,
                           project_bn_block=project_bn_block, expand_dw_bn_block=expand_dw_bn_block)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def randomise_bn(model, seed):
    """gamma, beta and the running tensors of every BatchNorm2d away from their defaults, from one seeded generator."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=gen) + 1.0)
                m.bias.copy_(torch.randn(c, generator=gen) * 0.5)
                m.running_mean.copy_(torch.randn(c, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=gen) + 0.5)


def training_model(seed=0, custom_bn=True):
    """YOLOv3TinyMobile(n_class=2) in training mode: seeded weights; gamma in [1, 2] and beta ~ N(2.5, 1) in every ReLU6 layer, so that
    the normalised values ~ N(2.5, 1 .. 4) reach both bounds of the clamp; running tensors away from their defaults and, with
    ``custom_bn``, a momentum and an eps that differ from layer to layer and from the defaults."""
    torch.manual_seed(seed)
    model = Y.YOLOv3TinyMobile(**CTOR)
    randomise_bn(model, seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    relu6_bns = {id(m[1]) for m in model.modules() if isinstance(m, torch.nn.Sequential) and len(m) == 3 and isinstance(m[2], torch.nn.ReLU6)}
    with torch.no_grad():
        for i, m in enumerate(b for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d)):
            if custom_bn:
                m.momentum, m.eps = 0.05 + 0.01 * (i % 7), 1e-5 * (1 + i % 3)
            if id(m) in relu6_bns:
                m.bias.copy_(2.5 + torch.randn(m.num_features, generator=gen))
    return model.train()


def step_inputs(bs, h, w, n_class=2, n_targets=24, seed=3):
    """(x float32 [bs, 3, h, w], targets float32 [n_targets, 6]) of one step: normal images; image and class uniform, centres in [0.1, 0.9],
    sizes in [0.1, 0.6] of the image (tests/_train_fire.golden_inputs' form)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n_targets, 6), dtype=F32)
    t[:, 0] = rng.integers(0, bs, n_targets)
    t[:, 1] = rng.integers(0, n_class, n_targets)
    t[:, 2:4] = rng.uniform(0.1, 0.9, (n_targets, 2))
    t[:, 4:6] = rng.uniform(0.1, 0.6, (n_targets, 2))
    return torch.randn((bs, 3, h, w), generator=torch.Generator().manual_seed(seed)), torch.from_numpy(t)


def live_layers(model):
    """tests/_loss.py's layer records from the attributes forward_train left on the model's YOLO layers."""
    out = []
    for y in model.yolo_layers:
        nx, ny = (int(v) for v in y.n_grids.cpu().tolist())
        out.append(dict(anchor_vec=y.anchor_vec.cpu().numpy().astype(F32), nx=nx, ny=ny, na=int(y.anchor_vec.shape[0])))
    return out


def reference_forward(model, x, relu6_ranges=None):
    """[p1, p2] of ``model`` (a float64 copy in training mode) by torch alone: the model's own nn.Sequential children in
    oracle.mobilenet's layer order - a ConvBNReLU as it is, ``block.conv(x)`` plus x where use_res_connect -, the heads as
    trace_tiny_heads orders them (ConvBlock = conv -> BatchNorm2d -> LeakyReLU(0.1)).  ``relu6_ranges``: a list that receives
    (numel, min, max) of every ReLU6 output."""
    hooks = []
    if relu6_ranges is not None:
        for m in model.modules():
            if isinstance(m, torch.nn.ReLU6):
                hooks.append(m.register_forward_hook(lambda mod, inp, out: relu6_ranges.append((out.numel(), float(out.detach().min()), float(out.detach().max())))))

    def encoder(seq, t):
        for m in seq:
            t = m(t) if isinstance(m, torch.nn.Sequential) else (t + m.conv(t) if m.use_res_connect else m.conv(t))
        return t

    def block(b, t):
        return F.leaky_relu(b.sequence.batch_norm(b.sequence.conv(t)), 0.1)
    try:
        route1 = encoder(model.features.sequence1, x)
        route2 = encoder(model.features.sequence2, route1)
        up = F.interpolate(block(model.sequence_branch1_1.branch1_conv1, route2), scale_factor=2, mode="nearest")
        b1 = block(model.sequence_branch1_2.branch1_conv2, torch.cat([route1, up], 1))
        h1 = model.sequence_branch1_2.branch1_conv3(b1)
        h2 = model.sequence_branch2.branch2_conv2(block(model.sequence_branch2.branch2_conv1, route2))
    finally:
        for h in hooks:
            h.remove()
    out = []
    for b, layer in zip((h1, h2), model.yolo_layers):
        bs, _, ny, nx = b.shape
        out.append(b.reshape(bs, layer.n_anchors, layer.n_classes + 5, ny, nx).permute(0, 1, 3, 4, 2).contiguous())
    return out


def reference_copy(model):
    return copy.deepcopy(model).double().train()


# ---- the eval trace -------------------------------------------------------------------------------------------------------------------------
def eval_trace_nodes():
    """The node list (tests/test_train_wiring_cpu.node_list) of YOLOv3TinyMobile's eval trace at 416, one image, as JSON data."""
    from test_train_wiring_cpu import node_list
    torch.manual_seed(0)
    model = Y.YOLOv3TinyMobile(**CTOR).eval()
    randomise_bn(model, 1)
    for name, m in model.named_modules():
        m._trace_name = name
    rec = graph.Recorder(1, 3, TRACE_SIZE, TRACE_SIZE)
    model._trace(rec, rec.input)
    assert [layer for _, layer in rec.heads] == list(model.yolo_layers)
    return json.loads(json.dumps(node_list(rec)))
