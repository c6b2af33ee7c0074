"""Restatements of the layers between the convs of a training step (csrc/route.hip, yolo_bn_act_add_fwd of
csrc/batchnorm.hip; include/yolo_hip.h) in numpy, a CPU op table for the models' training wiring, and the golden configuration.

The glue functions take and return NHWC numpy arrays (the device's layout).  With ``rounding`` every operation is the kernels': fp32
additions one by one in the documented order, one rounding to bf16 at the end; with ``rounding=False`` everything stays float64, the
form that has to equal torch's max_pool2d / interpolate / cat / add under float64 autograd (the sums are exact there).

    spp_forward     y = cat([maxpool5, maxpool9, maxpool13, x]); idx: the argmax of each window as (row offset) k + (column offset) inside
                    the window; the argmax is the FIRST maximum in row-major order (torch's rule)
    spp_backward    acc = 0; for k = 5, 9, 13: for the window centres q around p in row-major order: acc += dy_k[q] where idx_k[q] names p;
                    dx[p] = bf16(acc + dy_pass[p])
    upcat_forward   cat([nearest_x2(a), b]);   upcat_backward  da = bf16(((dy00 + dy01) + dy10) + dy11), db = dy[..., ca:]
    bn_act_add      a = f32(z) scale + shift; t = a > 0 ? a : 0.1f a; y_preadd = bf16(t); y = bf16(t + f32(residual))

``cpu_ops(rounding)`` is a table for ``pytorch_yolo_amd.models.train.forward_train``: float64 torch autograd Functions whose forward and
backward are these restatements and those of tests/_bn.py, tests/_conv_bwd.py and tests/_conv_down.py - with ``rounding`` every
rounding point of the device ops, without it plain float64 (what the goldens of tests/golden/make_golden_train.py are compared with).
"""
from types import SimpleNamespace

import numpy as np
import torch

import _bn as N
import _cases as C
import _conv_bwd as B
import _conv_down as D

F32, F64 = np.float32, np.float64
SPP_K = (5, 9, 13)
_R = 6

# ---- the golden configuration (the issue's: 3.9 M parameters, every cout a multiple of 8 except the 21-channel heads) -------------------
MODELS = {"spp": "train_spp", "yolov3": "train_yolov3"}                   # family -> fixture name
CTOR = dict(n_class=2, kernels_divider=4, anchors=C.SPP_ANCHORS)
BS, H, W = 2, 64, 96
WEIGHT_SEED, IMAGE_SEED, TARGET_SEED, N_TARGETS = 7, 3, 5, 8
HEADS = {"spp": ("branch1_2.conv2.", "branch2_3.conv7.", "branch3_2.conv7."),
         "yolov3": ("seq_y1.conv2.", "seqy2_3.conv7.", "seqy3_2.conv7.")}


def golden_inputs():
    """(x float32 [BS, 3, H, W], targets float32 [N_TARGETS, 6]) of the golden step."""
    import _loss as L
    from pytorch_yolo_amd.utils.synthetic import synth_images
    targets, _ = L.good_targets(TARGET_SEED, L.make_layers(C.SPP_ANCHORS, H, W), BS, CTOR["n_class"], N_TARGETS)
    return synth_images(BS, H, W, seed=IMAGE_SEED), torch.from_numpy(np.asarray(targets, dtype=F32))


def load_synthetic(model):
    from pytorch_yolo_amd.utils.synthetic import synth_state_dict
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=WEIGHT_SEED))
    return model


def stored_gradients(family, names):
    """The parameters whose gradient a fixture holds: every BN weight and bias, conv1, down1.conv0 and the head convs."""
    keep = ("conv1.", "down1.conv0.") + HEADS[family]
    return [n for n in names if ".batch_norm." in n or n.startswith(keep)]


def rel_err(got, want):
    """Largest |got - want| over the largest |want| of a tensor pair (float64)."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the glue, NHWC numpy -----------------------------------------------------------------------------------------------------------------
def _ft(rounding):
    return F32 if rounding else F64


def spp_forward(x, tie="first"):
    """(y [n,h,w,4c], idx uint8 [n,h,w,3c]).  tie: "first" (the rule) or "last" (the fault injection: the last maximum wins)."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    xp = np.full((n, h + 2 * _R, w + 2 * _R, c), -np.inf, dtype=x.dtype)
    xp[:, _R:_R + h, _R:_R + w] = x
    valid = np.zeros((h + 2 * _R, w + 2 * _R), dtype=bool)
    valid[_R:_R + h, _R:_R + w] = True
    outs, idxs = [], []
    for k in SPP_K:
        r = k // 2
        best, arg = np.full(x.shape, -np.inf, dtype=x.dtype), np.full(x.shape, -1, dtype=np.int64)
        for dh in range(-r, r + 1):
            for dw in range(-r, r + 1):
                sl = (slice(None), slice(_R + dh, _R + dh + h), slice(_R + dw, _R + dw + w))
                cand, ok = xp[sl], valid[sl[1:]][None, :, :, None]
                take = ok & ((arg < 0) | ((cand > best) if tie == "first" else (cand >= best)))
                best, arg = np.where(take, cand, best), np.where(take, (dh + r) * k + (dw + r), arg)
        outs.append(best), idxs.append(arg.astype(np.uint8))
    return np.concatenate(outs + [x], 3), np.concatenate(idxs, 3)


def spp_backward(dy, idx, rounding=True):
    """dx [n,h,w,c] of dy [n,h,w,4c] and idx [n,h,w,3c]."""
    ft = _ft(rounding)
    dy = np.asarray(dy)
    n, h, w, c4 = dy.shape
    c = c4 // 4
    acc = np.zeros((n, h, w, c), dtype=ft)
    for l, k in enumerate(SPP_K):
        r = k // 2
        d = np.zeros((n, h + 2 * _R, w + 2 * _R, c), dtype=ft)
        d[:, _R:_R + h, _R:_R + w] = dy[..., l * c:(l + 1) * c]
        ix = np.full((n, h + 2 * _R, w + 2 * _R, c), -1, dtype=np.int64)
        ix[:, _R:_R + h, _R:_R + w] = idx[..., l * c:(l + 1) * c]
        for dh in range(-r, r + 1):                                   # the window centre q = p + (dh, dw), row-major
            for dw in range(-r, r + 1):
                sl = (slice(None), slice(_R + dh, _R + dh + h), slice(_R + dw, _R + dw + w))
                acc = acc + np.where(ix[sl] == (r - dh) * k + (r - dw), d[sl], ft(0))
    acc = acc + dy[..., 3 * c:].astype(ft)
    return N.bf16(acc) if rounding else acc


def upcat_forward(a, b):
    return np.concatenate([np.repeat(np.repeat(np.asarray(a), 2, 1), 2, 2), np.asarray(b)], 3)


def upcat_backward(dy, ca, rounding=True, drop=None):
    """(da, db).  drop: the index of one 2x2 term that is left out (the fault injection)."""
    ft = _ft(rounding)
    d = np.asarray(dy)[..., :ca].astype(ft)
    terms = [d[:, 0::2, 0::2], d[:, 0::2, 1::2], d[:, 1::2, 0::2], d[:, 1::2, 1::2]]
    if drop is not None:
        terms.pop(drop)
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return (N.bf16(acc) if rounding else acc), np.ascontiguousarray(np.asarray(dy)[..., ca:])


def bn_act_add(z, saved, res, rounding=True, preadd_after_add=False):
    """(y, y_preadd) of z, res [M, C] and saved [4, C].  preadd_after_add: the fault injection (y_preadd taken after the add)."""
    ft = _ft(rounding)
    a = N.pre_act(z, saved, rounding)
    t = np.where(a > 0, a, ft(0.1) * a)
    s = t + np.asarray(res).astype(ft)
    pre = s if preadd_after_add else t
    return (N.bf16(s), N.bf16(pre)) if rounding else (s, pre)


# ---- the CPU op table ---------------------------------------------------------------------------------------------------------------------
def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).permute(0, 3, 1, 2).contiguous()


def _vec(a, ft):
    return torch.from_numpy(np.asarray(a).astype(ft).astype(F64))


class _ConvBn(torch.autograd.Function):
    """conv -> batch statistics -> LeakyReLU(0.1) [-> + residual], stride 1 or 2."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, running, momentum, eps, stride, rounding, want_preadd):
        x, k = B.bf16(x.detach(), rounding), w.shape[2]
        w = w.detach().to(torch.float64)
        zf = B.forward(x, w, None, k, "none", rounding) if stride == 1 else D.forward(x, w, None, "none", rounding)
        z = B.bf16(zf, rounding)
        zr = N._rows(z)
        rm, rv = running
        st = N.stats(zr, gamma.detach().numpy(), beta.detach().numpy(), eps, momentum, None if rm is None else rm.numpy(),
                     None if rv is None else rv.numpy(), rounding)
        if rm is not None:
            rm.copy_(torch.from_numpy(st["rm"].astype(F64)))
        if rv is not None:
            rv.copy_(torch.from_numpy(st["rv"].astype(F64)))
        ctx.keep = (x, w, z, zr, st["saved"], k, stride, rounding, residual is not None)
        ctx.set_materialize_grads(False)
        if residual is None:
            return N._nchw(N.forward(zr, st["saved"], "leaky", rounding), z)
        y, pre = bn_act_add(zr, st["saved"], N._rows(B.bf16(residual.detach(), rounding)), rounding)
        return (N._nchw(y, z), N._nchw(pre, z)) if want_preadd else N._nchw(y, z)

    @staticmethod
    def backward(ctx, dy, dpre=None):
        x, w, z, zr, saved, k, stride, rounding, has_res = ctx.keep
        if dy is None and dpre is None:
            return (None,) * 11
        tot = dy if dpre is None else dpre if dy is None else dy + dpre
        ft = _ft(rounding)
        tr = N.backward_terms(N._rows(tot), zr, saved, "leaky", rounding)
        c1, c2 = N.centre(tr, zr.shape[0], True, rounding)
        g = N._nchw(N.backward_apply(tr, saved, c1, c2, rounding), z)
        conv = B.grads(x, w, g, None, k, "none", rounding) if stride == 1 else D.grads(x, w, None, None, "none", rounding, g=g)
        return (conv["dx"], conv["dw"], _vec(tr["G"], ft), _vec(tr["B"], ft), dy if has_res else None) + (None,) * 6


class _Conv(torch.autograd.Function):
    """The plain head: conv + bias, no activation, a float32 result."""

    @staticmethod
    def forward(ctx, x, w, b, rounding):
        x, w, k = B.bf16(x.detach(), rounding), w.detach().to(torch.float64), w.shape[2]
        y = B.forward(x, w, None if b is None else b.detach(), k, "none", rounding)
        ctx.keep = (x, w, y, k, rounding)
        return y.to(torch.float32).to(torch.float64) if rounding else y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, k, rounding = ctx.keep
        gr = B.grads(x, w, dy, y, k, "none", rounding)
        return gr["dx"], gr["dw"], gr["db"], None


class _Spp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rounding):
        y, ctx.idx = spp_forward(_nhwc(B.bf16(x, rounding)))
        ctx.rounding = rounding
        return _nchw(y)

    @staticmethod
    def backward(ctx, dy):
        return _nchw(spp_backward(_nhwc(dy), ctx.idx, ctx.rounding)), None


class _Upcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, rounding):
        ctx.ca, ctx.rounding = a.shape[1], rounding
        return _nchw(upcat_forward(_nhwc(B.bf16(a, rounding)), _nhwc(B.bf16(b, rounding))))

    @staticmethod
    def backward(ctx, dy):
        da, db = upcat_backward(_nhwc(dy), ctx.ca, ctx.rounding)
        return _nchw(da), _nchw(db), None


def cpu_ops(rounding):
    """The op table of models/train.py on the CPU: float64 tensors in and out (with ``rounding`` they hold the device's bf16 / float32
    values)."""
    def running(rm, rv):
        return (None if rm is None else rm.detach(), None if rv is None else rv.detach())

    def conv_bn_block(x, w, gamma, beta, rm=None, rv=None, *, momentum=0.1, eps=1e-5):
        return _ConvBn.apply(x, w, gamma, beta, None, running(rm, rv), momentum, eps, 1, rounding, False)

    def down_bn_block(x, w, gamma, beta, rm=None, rv=None, *, momentum=0.1, eps=1e-5):
        return _ConvBn.apply(x, w, gamma, beta, None, running(rm, rv), momentum, eps, 2, rounding, False)

    def res_bn_block(x, w, gamma, beta, rm, rv, residual, *, want_preadd=False, momentum=0.1, eps=1e-5):
        return _ConvBn.apply(x, w, gamma, beta, residual, running(rm, rv), momentum, eps, 1, rounding, want_preadd)

    def conv_block(x, w, b=None, *, act="none", out_dtype=torch.float32):
        assert act == "none" and out_dtype == torch.float32
        return _Conv.apply(x, w, b, rounding)

    return SimpleNamespace(conv_block=conv_block, conv_bn_block=conv_bn_block, down_bn_block=down_bn_block, res_bn_block=res_bn_block,
                           spp_concat=lambda x: _Spp.apply(x, rounding), upsample_concat=lambda a, b: _Upcat.apply(a, b, rounding))
