"""Helpers of the YOLOv3-tiny/ShuffleNetV2 training tests: numpy restatements of MaxPool2d(3, 2, 1) with its backward and
of the two-slot channel shuffle with its inverse, the CPU float64 op table of DEVICE_OPS_SHUFFLE, the torch reference of one training step
in torchvision's unit order, and the eval trace as plain data.

The dense and depthwise layers are the restatements of tests/_dw_train.py / tests/_train_mobile.py with the clamp (0, +inf) for ReLU and
with no activation for the linear depthwise stage."""
import copy
import json
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import _dw_train as D
import _train_mobile as M
import _train_pool as TP
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import graph

F32, F64 = np.float32, np.float64
CTOR = dict(n_class=2)
TRACE_SIZE = 416
RELU = (0.0, float("inf"))
NEW_OPS = ("conv_bn_relu_block", "dw_bn_block", "max_pool_321", "channel_shuffle2", "shuffle_unit_block")

POOL_CASES = [(2, 1, 1, 8), (1, 2, 2, 8), (2, 5, 7, 24), (2, 8, 6, 16), (1, 13, 9, 8)]          # (n, h, w, c)
SHUFFLE_CASES = [(58, 64), (116, 128), (232, 256), (8, 8), (4, 8), (3, 8)]                      # (half, slot) on a 2 x 3 x 5 map
SHUFFLE_MAP = (2, 3, 5)


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- MaxPool2d(3, 2, 1) restated -----------------------------------------------------------------------------------------------------------------
def pool_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def pool_forward(x):
    """(y, idx) of the NHWC x: tap 3i + j of window (oy, ox) is pixel (2oy - 1 + i, 2ox - 1 + j); a tap outside the map is no candidate;
    a later tap replaces the running maximum only when strictly greater."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    ho, wo = pool_out(h, w)
    y = np.empty((n, ho, wo, c), dtype=x.dtype)
    idx = np.full((n, ho, wo, c), 255, dtype=np.uint8)
    for oy in range(ho):
        for ox in range(wo):
            best, arg = None, None
            for k in range(9):
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                if not (0 <= iy < h and 0 <= ix < w):
                    continue
                tap = x[:, iy, ix]
                if best is None:
                    best, arg = tap.copy(), np.full(tap.shape, k, dtype=np.uint8)
                else:
                    m = tap > best
                    best, arg = np.where(m, tap, best), np.where(m, np.uint8(k), arg)
            y[:, oy, ox], idx[:, oy, ox] = best, arg
    return y, idx


def pool_backward(dy, idx, shape, rounding=True):
    """dx of the map ``shape``: per input pixel the terms of its windows in row-major (oy, ox) order, summed in fp32 (float64 with the
    rounding off) and rounded once."""
    ft = F32 if rounding else F64
    dy = np.asarray(dy).astype(ft)
    n, h, w, c = shape
    ho, wo = pool_out(h, w)
    acc = np.zeros(shape, dtype=ft)
    for oy in range(ho):                       # row-major over the windows: every pixel receives its terms in that order
        for ox in range(wo):
            for k in range(9):
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                if 0 <= iy < h and 0 <= ix < w:
                    acc[:, iy, ix] += np.where(idx[:, oy, ox] == k, dy[:, oy, ox], ft(0))
    return D.bf16(acc) if rounding else acc


def pool_integer_map(case, seed=0):
    """Integers in [-3, 3]: ties in every window, torch's first-maximum rule decides."""
    return np.random.default_rng(4100 + seed).integers(-3, 4, case).astype(F32)


def pool_negative_map(case, seed=0):
    """Integers in [-9, -1]: a pool that pads with 0 returns 0 at every border window."""
    return np.random.default_rng(4200 + seed).integers(-9, 0, case).astype(F32)


def pool_random_map(case, seed=0):
    return D.bf16(np.random.default_rng(4300 + seed).standard_normal(case).astype(F32))


def pool_integer_dy(case, seed=0):
    n, h, w, c = case
    return np.random.default_rng(4400 + seed).integers(-7, 8, (n,) + pool_out(h, w) + (c,)).astype(F32)


def torch_pool(x, dy):
    """(y, dx) of F.max_pool2d(x, 3, 2, 1) and its autograd in float64; NHWC arrays in and out."""
    xt = torch.from_numpy(np.asarray(x, dtype=F64)).permute(0, 3, 1, 2).contiguous().requires_grad_()
    y = F.max_pool2d(xt, 3, 2, 1)
    y.backward(torch.from_numpy(np.asarray(dy, dtype=F64)).permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy()


# ---- the two-slot channel shuffle restated ------------------------------------------------------------------------------------------------------
def shuffle_forward(a, b, half):
    """y [.., 2 slot] of the NHWC slot maps a and b: logical channel j = (a, b)[j % 2][j // 2] at physical (j // half) slot + j % half; the
    pad channels are zero."""
    slot = a.shape[-1]
    y = np.zeros(a.shape[:-1] + (2 * slot,), dtype=a.dtype)
    for j in range(2 * half):
        y[..., (j // half) * slot + j % half] = (a, b)[j % 2][..., j // 2]
    return y


def shuffle_backward(dy, half):
    """(da, db) of the two-slot dy: da[q] = dy_logical[2q], db[q] = dy_logical[2q + 1], zero for q >= half; dy's pad channels are not read."""
    slot = dy.shape[-1] // 2
    da, db = (np.zeros(dy.shape[:-1] + (slot,), dtype=dy.dtype) for _ in range(2))
    for q in range(half):
        for out, j in ((da, 2 * q), (db, 2 * q + 1)):
            out[..., q] = dy[..., (j // half) * slot + j % half]
    return da, db


def torch_channel_shuffle(x, groups=2):
    """torchvision.models.shufflenetv2.channel_shuffle."""
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).contiguous().view(b, c, h, w)


def torch_shuffle(a, b, dy, half):
    """(y, da, db) of channel_shuffle(cat(a[:half], b[:half]), 2) and its autograd in float64, given and returned in the two-slot layout
    (NHWC arrays; dy's pad channels are ignored, the pad channels of da and db are zero)."""
    slot = a.shape[-1]
    at, bt = (torch.from_numpy(np.asarray(t, dtype=F64)[..., :half]).permute(0, 3, 1, 2).contiguous().requires_grad_() for t in (a, b))
    y = torch_channel_shuffle(torch.cat([at, bt], 1))
    dyl = np.concatenate([np.asarray(dy, dtype=F64)[..., :half], np.asarray(dy, dtype=F64)[..., slot:slot + half]], -1)
    y.backward(torch.from_numpy(dyl).permute(0, 3, 1, 2).contiguous())
    yl = y.detach().permute(0, 2, 3, 1).numpy()
    yp = np.zeros(a.shape[:-1] + (2 * slot,))
    yp[..., :half], yp[..., slot:slot + half] = yl[..., :half], yl[..., half:]
    out = []
    for t in (at, bt):
        g = np.zeros(a.shape)
        g[..., :half] = t.grad.permute(0, 2, 3, 1).numpy()
        out.append(g)
    return yp, out[0], out[1]


# ---- the CPU op table ----------------------------------------------------------------------------------------------------------------------------
_np, _t, _v = M._np, M._t, M._v


class _DwBnLinear(torch.autograd.Function):
    """tests/_train_mobile._DwBn with no activation: ShuffleNetV2's linear depthwise stage."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running, momentum, eps, stride, rounding):
        xn, wn = _np(x), w.detach().numpy()[:, 0]
        wq = D.bf16(wn.astype(F32)) if rounding else wn
        z = D.dw_forward(xn, wq, stride, rounding)
        y, cache = M.bn_forward(z, gamma, beta, "none", running, momentum, eps, rounding)
        ctx.keep = (xn, wq, cache, stride, rounding)
        return _t(y)

    @staticmethod
    def backward(ctx, dy):
        xn, wq, cache, stride, rounding = ctx.keep
        g, dgamma, dbeta = D.bn_backward(_np(dy), cache, rounding)
        dx = D.dw_bwd_data(g, wq, xn.shape, stride, rounding)
        dw = D.dw_bwd_weight(xn, g, stride, rounding)["dw"]
        return (_t(dx), _v(dw)[:, None], _v(dgamma), _v(dbeta)) + (None,) * 5


class _Pool321(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rounding):
        xn = _np(x)
        y, idx = pool_forward(xn)
        ctx.keep = (idx, xn.shape, rounding)
        return _t(y)

    @staticmethod
    def backward(ctx, dy):
        idx, shape, rounding = ctx.keep
        return _t(pool_backward(_np(dy), idx, shape, rounding)), None


class _Shuffle2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, half):
        ctx.half = half
        return _t(shuffle_forward(_np(a), _np(b), half))

    @staticmethod
    def backward(ctx, dy):
        da, db = shuffle_backward(_np(dy), ctx.half)
        return _t(da), _t(db), None


def _three(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def cpu_ops(rounding):
    """The table of models/train.shuffle_ops on the CPU: tests/_train_pool.cpu_ops plus the five ops of the ShuffleNetV2 wiring; float64
    tensors in and out.  ``shuffle_unit_block`` is the composition on two slices of x."""
    def conv_bn_relu_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        return M._DenseBn.apply(x, w, gamma, beta, None, M._running(rm, rv), momentum, eps, stride, RELU, rounding)

    def dw_bn_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, act="relu6", momentum=0.1, eps=1e-5, training=True):
        assert act == "none"
        return _DwBnLinear.apply(x, w, gamma, beta, M._running(rm, rv), momentum, eps, stride, rounding)

    def max_pool_321(x):
        return _Pool321.apply(x, rounding)

    def channel_shuffle2(a, b, half):
        return _Shuffle2.apply(a, b, half)

    def shuffle_unit_block(x, half, w1, gamma1, beta1, rm1, rv1, wd, gamma2, beta2, rm2, rv2, w3, gamma3, beta3, rm3, rv3, *, momentum=0.1,
                           eps=1e-5):
        (m1, m2, m3), (e1, e2, e3) = _three(momentum), _three(eps)
        slot = x.shape[1] // 2
        y = conv_bn_relu_block(x[:, slot:], w1, gamma1, beta1, rm1, rv1, momentum=m1, eps=e1)
        y = dw_bn_block(y, wd, gamma2, beta2, rm2, rv2, act="none", momentum=m2, eps=e2)
        y = conv_bn_relu_block(y, w3, gamma3, beta3, rm3, rv3, momentum=m3, eps=e3)
        return channel_shuffle2(x[:, :slot], y, half)

    return SimpleNamespace(**vars(TP.cpu_ops(rounding)), conv_bn_relu_block=conv_bn_relu_block, dw_bn_block=dw_bn_block,
                           max_pool_321=max_pool_321, channel_shuffle2=channel_shuffle2, shuffle_unit_block=shuffle_unit_block)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
step_inputs, live_layers, randomise_bn = M.step_inputs, M.live_layers, M.randomise_bn


def training_model(seed=0, custom_bn=True):
    """YOLOv3TinyShuffle(n_class=2) in training mode: seeded weights, gamma, beta and running tensors away from their defaults and, with
    ``custom_bn``, a momentum and an eps that differ from layer to layer and from the defaults."""
    torch.manual_seed(seed)
    model = Y.YOLOv3TinyShuffle(**CTOR)
    randomise_bn(model, seed + 1)
    if custom_bn:
        for i, m in enumerate(b for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d)):
            m.momentum, m.eps = 0.05 + 0.01 * (i % 7), 1e-5 * (1 + i % 3)
    return model.train()


def reference_copy(model):
    return copy.deepcopy(model).double().train()


def reference_unit(unit, x):
    """torchvision's InvertedResidual.forward."""
    if unit.stride == 1:
        x1, x2 = x.chunk(2, dim=1)
        out = torch.cat((x1, unit.branch2(x2)), dim=1)
    else:
        out = torch.cat((unit.branch1(x), unit.branch2(x)), dim=1)
    return torch_channel_shuffle(out, 2)


def reference_forward(model, x):
    """[p1, p2] of ``model`` (a float64 copy in training mode) by torch alone: the model's own modules in torchvision's order (conv1,
    maxpool, stage2, stage3 | stage4, conv5), the heads as the reference orders them (ConvBlock = conv -> BatchNorm2d -> LeakyReLU(0.1))."""
    def encoder(seq, t):
        for m in seq:
            if isinstance(m, torch.nn.Sequential) and len(m) and hasattr(m[0], "branch2"):
                for unit in m:
                    t = reference_unit(unit, t)
            else:
                t = m(t)
        return t

    def block(b, t):
        return F.leaky_relu(b.sequence.batch_norm(b.sequence.conv(t)), 0.1)
    route1 = encoder(model.features.sequence1, x)
    route2 = encoder(model.features.sequence2, route1)
    up = F.interpolate(block(model.sequence_branch1_1.branch1_conv1, route2), scale_factor=2, mode="nearest")
    b1 = block(model.sequence_branch1_2.branch1_conv2, torch.cat([route1, up], 1))
    h1 = model.sequence_branch1_2.branch1_conv3(b1)
    h2 = model.sequence_branch2.branch2_conv2(block(model.sequence_branch2.branch2_conv1, route2))
    out = []
    for b, layer in zip((h1, h2), model.yolo_layers):
        bs, _, ny, nx = b.shape
        out.append(b.reshape(bs, layer.n_anchors, layer.n_classes + 5, ny, nx).permute(0, 1, 3, 4, 2).contiguous())
    return out


# ---- the eval trace ------------------------------------------------------------------------------------------------------------------------------
def eval_trace_nodes():
    """The node list (tests/test_train_wiring_cpu.node_list) of YOLOv3TinyShuffle's eval trace at 416, one image, as JSON data."""
    from test_train_wiring_cpu import node_list
    torch.manual_seed(0)
    model = Y.YOLOv3TinyShuffle(**CTOR).eval()
    M.randomise_bn(model, 1)
    for name, m in model.named_modules():
        m._trace_name = name
    rec = graph.Recorder(1, 3, TRACE_SIZE, TRACE_SIZE)
    model._trace(rec, rec.input)
    assert [layer for _, layer in rec.heads] == list(model.yolo_layers)
    return json.loads(json.dumps(node_list(rec)))
