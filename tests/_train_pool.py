"""Restatements of the max-pool layers of a training step of YOLOv3-tiny / LiteYOLOv3 (csrc/pool_train.hip,
yolo_bn_act_pool_fwd of csrc/batchnorm.hip, yolo_concat_upsample2_* of csrc/route.hip; include/yolo_hip.h) in numpy, the CPU op table of
tests/_train.py extended by them, and the golden configuration of the two models.

NHWC numpy arrays in and out, as in tests/_train.py; ``rounding=False`` keeps float64 (what has to equal torch's max_pool2d / interpolate /
cat under float64 autograd).

    pool_forward    stride 2: MaxPool2d(2, 2), tap 2i + j of the window at (oy, ox) is (2oy + i, 2ox + j); stride 1: MaxPool2d(2, 1,
                    padding=1, dilation=2), tap 2i + j of the window at (y, x) is (y - 1 + 2i, x - 1 + 2j), -inf outside.  idx: the tap of the
                    FIRST maximum among the in-bounds taps in row-major order
    pool_backward   stride 2: dx[p] = dy[q] where idx[q] names p in its own block, else 0.  stride 1: acc = 0; for q = p + (-1,-1), (-1,+1),
                    (+1,-1), (+1,+1): acc += dy[q] where q is in bounds and idx[q] == 3, 2, 1, 0; dx[p] = bf16(acc)
    bn_act_pool     t = bf16(act(f32(z) scale + shift)) per tap, then pool_forward(t, 2)
    catup_forward   cat([b, nearest_x2(a)]);  catup_backward  db = dy[..., :cb], da = bf16(((dy00 + dy01) + dy10) + dy11) of dy[..., cb:]
"""
from types import SimpleNamespace

import numpy as np
import torch

import _bn as N
import _cases as C
import _conv_bwd as B
import _train as T

F32, F64 = np.float32, np.float64

# ---- the golden configuration: tests/_train.py's input, seeds, targets and HYPER; every channel count but the 21-channel heads % 8 == 0 ----
MODELS = {"tiny": "train_tiny", "lite": "train_lite"}                      # family -> fixture name
CLASSES = {"tiny": "YOLOv3Tiny", "lite": "LiteYOLOv3"}
CTORS = {"tiny": dict(n_class=2, kernels_divider=4, anchors=C.TINY_ANCHORS), "lite": dict(n_class=2, kernels_divider=2, anchors=C.SPP_ANCHORS)}
HEADS = {"tiny": ("sequence_branch1_2.branch1_conv3.", "sequence_branch2.branch2_conv2."),
         "lite": ("seq_y1.conv2.", "seqy2_3.conv7.", "seqy3_2.conv2.")}
FIRST = {"tiny": ("sequence_1.conv1.", "sequence_1.conv2."), "lite": ("down1.", "down2.")}


def golden_inputs(family):
    """(x float32 [BS, 3, H, W], targets float32 [N_TARGETS, 6]) of the golden step (the targets are drawn for the family's anchors)."""
    import _loss as L
    from pytorch_yolo_amd.utils.synthetic import synth_images
    targets, _ = L.good_targets(T.TARGET_SEED, L.make_layers(CTORS[family]["anchors"], T.H, T.W), T.BS, 2, T.N_TARGETS)
    return synth_images(T.BS, T.H, T.W, seed=T.IMAGE_SEED), torch.from_numpy(np.asarray(targets, dtype=F32))


def stored_gradients(family, names):
    """The parameters whose gradient a fixture holds: every BN weight and bias, the first two conv weights and the head convs."""
    keep = FIRST[family] + HEADS[family]
    return [n for n in names if ".batch_norm." in n or n.startswith(keep)]


# ---- the pools, NHWC numpy ------------------------------------------------------------------------------------------------------------------
def _taps(x, stride):
    """[(candidate values, in-bounds mask)] of the four taps, each of the output map's shape."""
    n, h, w, c = x.shape
    if stride == 2:
        ho, wo = h // 2, w // 2
        return [(x[:, i:2 * ho:2, j:2 * wo:2], np.ones((1, ho, wo, 1), dtype=bool)) for i in (0, 1) for j in (0, 1)]
    assert stride == 1 and h >= 2 and w >= 2
    xp = np.full((n, h + 2, w + 2, c), -np.inf, dtype=x.dtype)
    xp[:, 1:1 + h, 1:1 + w] = x
    valid = np.zeros((h + 2, w + 2), dtype=bool)
    valid[1:1 + h, 1:1 + w] = True
    return [(xp[:, 2 * i:2 * i + h, 2 * j:2 * j + w], valid[2 * i:2 * i + h, 2 * j:2 * j + w][None, :, :, None]) for i in (0, 1) for j in (0, 1)]


def pool_forward(x, stride, tie="first"):
    """(y, idx uint8).  tie: "first" (the rule) or "last" (the fault injection: the last maximum wins)."""
    x = np.asarray(x)
    taps = _taps(x, stride)
    best = np.full(taps[0][0].shape, -np.inf, dtype=x.dtype)
    arg = np.full(best.shape, -1, dtype=np.int64)
    for k, (cand, ok) in enumerate(taps):
        take = ok & ((arg < 0) | ((cand > best) if tie == "first" else (cand >= best)))
        best, arg = np.where(take, cand, best), np.where(take, k, arg)
    assert arg.min() >= 0
    return best, arg.astype(np.uint8)


def pool_backward(dy, idx, shape, stride, rounding=True, drop=None):
    """dx of ``shape`` [n,h,w,c].  drop: the index of one stride-1 gather term that is left out (the fault injection)."""
    ft = F32 if rounding else F64
    dy, idx = np.asarray(dy).astype(ft), np.asarray(idx)
    n, h, w, c = shape
    if stride == 2:
        ho, wo = h // 2, w // 2
        dx = np.zeros(shape, dtype=ft)
        for k in range(4):
            dx[:, (k >> 1):2 * ho:2, (k & 1):2 * wo:2] = np.where(idx == k, dy, ft(0))
        return dx                                                          # a copy: bf16 values stay bf16 values
    d = np.zeros((n, h + 2, w + 2, c), dtype=ft)
    d[:, 1:1 + h, 1:1 + w] = dy
    ix = np.full((n, h + 2, w + 2, c), -1, dtype=np.int64)
    ix[:, 1:1 + h, 1:1 + w] = idx
    acc = np.zeros(shape, dtype=ft)
    for t in range(4):                                                     # the window centre q = p + (-1 + 2 (t >> 1), -1 + 2 (t & 1))
        if t == drop:
            continue
        sl = (slice(None), slice(2 * (t >> 1), 2 * (t >> 1) + h), slice(2 * (t & 1), 2 * (t & 1) + w))
        acc = acc + np.where(ix[sl] == 3 - t, d[sl], ft(0))
    return N.bf16(acc) if rounding else acc


def bn_act_pool(z, saved, rounding=True, pool_on_z=False):
    """(y, idx) of z [n,h,w,c] and saved [4, c]: the activated values pooled 2/2.  pool_on_z: the fault injection (the argmax is taken
    on z, the value is the activation at that tap)."""
    z = np.asarray(z)
    t = N.forward(z.reshape(-1, z.shape[3]), saved, "leaky", rounding).reshape(z.shape)
    if not pool_on_z:
        return pool_forward(t, 2)
    _, idx = pool_forward(z, 2)
    taps = np.stack([cand for cand, _ in _taps(t, 2)], 0)
    return np.take_along_axis(taps, idx[None].astype(np.int64), 0)[0], idx


def catup_forward(b, a):
    return np.concatenate([np.asarray(b), np.repeat(np.repeat(np.asarray(a), 2, 1), 2, 2)], 3)


def catup_backward(dy, cb, rounding=True):
    """(db, da) of dy [n,2h,2w,cb+ca]."""
    dy = np.asarray(dy)
    da, _ = T.upcat_backward(dy[..., cb:], dy.shape[3] - cb, rounding)                      # the same fixed 2x2 sum order
    return np.ascontiguousarray(dy[..., :cb]), da


# ---- the CPU op table -------------------------------------------------------------------------------------------------------------------
class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride, rounding):
        xn = T._nhwc(B.bf16(x, rounding))
        y, ctx.idx = pool_forward(xn, stride)
        ctx.keep = (xn.shape, stride, rounding)
        return T._nchw(y)

    @staticmethod
    def backward(ctx, dy):
        shape, stride, rounding = ctx.keep
        return T._nchw(pool_backward(T._nhwc(dy), ctx.idx, shape, stride, rounding)), None, None


class _ConvBnPool(torch.autograd.Function):
    """conv -> batch statistics over the unpooled z -> LeakyReLU(0.1) -> the pool; the backward expands dy, then is tests/_train._ConvBn's."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running, momentum, eps, pool_stride, rounding):
        x, k = B.bf16(x.detach(), rounding), w.shape[2]
        w = w.detach().to(torch.float64)
        z = B.bf16(B.forward(x, w, None, k, "none", rounding), rounding)
        zr = N._rows(z)
        rm, rv = running
        st = N.stats(zr, gamma.detach().numpy(), beta.detach().numpy(), eps, momentum, None if rm is None else rm.numpy(),
                     None if rv is None else rv.numpy(), rounding)
        if rm is not None:
            rm.copy_(torch.from_numpy(st["rm"].astype(F64)))
        if rv is not None:
            rv.copy_(torch.from_numpy(st["rv"].astype(F64)))
        full = T._nhwc(N._nchw(N.forward(zr, st["saved"], "leaky", rounding), z))
        y, idx = pool_forward(full, pool_stride)
        ctx.keep = (x, w, z, zr, st["saved"], k, rounding, idx, full.shape, pool_stride)
        return T._nchw(y)

    @staticmethod
    def backward(ctx, dy):
        x, w, z, zr, saved, k, rounding, idx, shape, pool_stride = ctx.keep
        ft = F32 if rounding else F64
        dfull = pool_backward(T._nhwc(dy), idx, shape, pool_stride, rounding)
        tr = N.backward_terms(dfull.reshape(-1, shape[3]), zr, saved, "leaky", rounding)
        c1, c2 = N.centre(tr, zr.shape[0], True, rounding)
        g = N._nchw(N.backward_apply(tr, saved, c1, c2, rounding), z)
        conv = B.grads(x, w, g, None, k, "none", rounding)
        return (conv["dx"], conv["dw"], T._vec(tr["G"], ft), T._vec(tr["B"], ft)) + (None,) * 5


class _Catup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, rounding):
        ctx.cb, ctx.rounding = b.shape[1], rounding
        return T._nchw(catup_forward(T._nhwc(B.bf16(b, rounding)), T._nhwc(B.bf16(a, rounding))))

    @staticmethod
    def backward(ctx, dy):
        db, da = catup_backward(T._nhwc(dy), ctx.cb, ctx.rounding)
        return T._nchw(da), T._nchw(db), None


def cpu_ops(rounding):
    """tests/_train.cpu_ops(rounding) plus max_pool, pool_bn_block and the up_first keyword of upsample_concat."""
    base = T.cpu_ops(rounding)

    def pool_bn_block(x, w, gamma, beta, rm=None, rv=None, *, pool_stride=2, momentum=0.1, eps=1e-5):
        running = (None if rm is None else rm.detach(), None if rv is None else rv.detach())
        return _ConvBnPool.apply(x, w, gamma, beta, running, momentum, eps, pool_stride, rounding)

    def upsample_concat(a, b, *, up_first=True):
        return base.upsample_concat(a, b) if up_first else _Catup.apply(a, b, rounding)

    table = dict(vars(base))
    table.update(max_pool=lambda x, *, stride=2: _Pool.apply(x, stride, rounding), pool_bn_block=pool_bn_block, upsample_concat=upsample_concat)
    return SimpleNamespace(**table)
