"""Differentiable building blocks on the package's kernels.

``conv_block`` is ConvBlock.forward of the reference (models/yolo_base.py:19-44, BN folded; with ``act="none"`` and
``out_dtype=torch.float32`` the plain nn.Conv2d heads of models/yolov3_tiny.py:38,42) at stride 1, 1x1 or 3x3, in bf16 mode, WITH a
backward: the forward is the launch the models use (yolo_conv2d_fwd), the backward runs csrc/conv_bwd.hip.  The
models' eval forward stays inference-only: ``io, p = model(x)`` has no ``grad_fn``.

``conv_bn_block`` is the same ConvBlock with its BatchNorm2d NOT folded: conv -> batch norm on batch statistics -> LeakyReLU(0.1), the
layer as the reference trains it.  The conv and its two gradients are conv_block's launches; the statistics, the normalise-and-activate
pass and the batch-norm backward run csrc/batchnorm.hip.  With ``training=False`` the running statistics are frozen
numbers and the layer IS conv_block on the folded weights: that is what runs, with the fold written in torch so that autograd carries
the gradients on to weight, gamma and beta.

``down_block`` and ``down_bn_block`` are the same two contracts for the downsample, ConvBlock(3x3, stride 2, pad 1) - the five stride-2
layers of Darknet-53: the forward is again yolo_conv2d_fwd, the two gradients run csrc/conv_down_bwd.hip, the batch
norm is conv_bn_block's (yolo_bn_* take the n ho wo output pixels).

``res_bn_block``, ``spp_concat`` and ``upsample_concat`` are the layers between those convs in YOLOv3 / YOLOv3-SPP - the residual unit's
closing ConvBlock with its add, the SPP pyramid, the FPN's upsample + concat - with their backwards (csrc/route.hip, yolo_bn_act_add_fwd;
DESIGN.md 3.6f); models/train.py wires the training-mode forward of the two models from all seven ops.

``max_pool`` and ``pool_bn_block`` are the reference's MaxPool and ConvPoolBlock as they train - MaxPool2d(2, 2) and the form MaxPool(2, 1)
turns into, MaxPool2d(2, 1, padding=1, dilation=2) - and ``upsample_concat(..., up_first=False)`` is the concat in YOLOv3-tiny's order
(csrc/pool_train.hip, yolo_bn_act_pool_fwd, yolo_concat_upsample2_*): with them models/train.py wires YOLOv3-tiny and
LiteYOLOv3 too.
"""
from __future__ import annotations

import torch

from . import kernels as K
from ._lib import ACT_LEAKY01, ACT_NONE, DT_BF16, DT_F32

__all__ = ["conv_block", "conv_bn_block", "down_block", "down_bn_block", "res_bn_block", "spp_concat", "upsample_concat", "max_pool",
           "pool_bn_block"]

_ACTS = {"leaky": ACT_LEAKY01, "none": ACT_NONE}


def _desc(x, weight, act_id, out_f32, stride=1):
    n, c, h, w = x.shape
    cout, _, k, _ = weight.shape
    ct = K.roundup(cout, 4) if out_f32 else cout
    return K.conv_desc(n=n, h=h, w=w, cin=c, in_c_total=c, in_c_offset=0, cout=cout, out_c_total=ct, out_c_offset=0, ksize=k, stride=stride,
                       act=act_id, kpad=K.roundup(k * k * c, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_F32 if out_f32 else DT_BF16)


def _forward(x, weight, bias, act_id, out_f32, stride=1):
    """The forward launch on a device-packed weight.  x: bf16, NCHW-shaped, dense channels-last.  Returns the NCHW-shaped
    channels-last result (a view of the [n, ho, wo, out_c_total] buffer the kernel wrote) and the descriptor."""
    d = _desc(x, weight, act_id, out_f32, stride)
    with torch.cuda.device(x.device):
        packed, _, cout_pad = K.pack_conv_weight_dev(weight, d.cin)
        b = torch.zeros((cout_pad,), dtype=torch.float32, device=x.device)
        if bias is not None:
            b[:d.cout] = bias
        y = torch.empty((d.n, d.ho, d.wo, d.out_c_total), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
        K.conv2d(x, packed, b, y, d)
    return y[..., :d.cout].permute(0, 3, 1, 2), d


class _ConvBlockFunction(torch.autograd.Function):
    """_forward with a backward: prepare (g), then the weight / bias gradient only if one of them is wanted and the data gradient only
    if x wants one.  Every buffer is allocated per call and fully written by its kernel.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, weight, bias, act_id, out_f32):
        out, d = _forward(x, weight, None if bias is None else bias.detach(), act_id, out_f32)
        ctx.desc = d
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, out if act_id != ACT_NONE else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        dx = dw = db = None
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()                    # dense [n, h, w, cout]; no copy for a channels-last dy
            g = torch.empty((d.n, d.h, d.w, K.roundup(d.cout, 8)), dtype=torch.bfloat16, device=x.device)
            K.conv2d_bwd_prepare(dy, y, g, d)
            if need_w or need_b:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                db = torch.empty((d.cout,), dtype=torch.float32, device=x.device) if need_b else None
                ws = torch.empty((K.conv2d_bwd_workspace_bytes(d),), dtype=torch.uint8, device=x.device)
                K.conv2d_bwd_weight(x, g, dw, db, ws, d)
                if not need_w:
                    dw = None
            if need_x:
                packed_t, _, _ = K.pack_conv_weight_dev(weight, g.shape[3], transposed=True)
                buf = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
                K.conv2d_bwd_data(g, packed_t, buf, d)
                dx = buf.permute(0, 3, 1, 2)
        return dx, dw, db, None, None


def conv_block(x, weight, bias=None, *, act="leaky", out_dtype=torch.bfloat16, stride=1):
    """``act(conv2d(x, bf16(weight), padding=k // 2) + bias)`` at stride 1 on the device, differentiable once.

    x       [n, cin, h, w].  The zero-copy form is bfloat16, dense channels-last (the package's NHWC layout) with ``cin % 8 == 0``;
            any other dtype / layout / channel count is converted (and zero-padded to 8 channels) by torch operations, so torch
            differentiates the conversion and such an x gets a gradient of its own dtype and layout.
    weight  float32 [cout, cin, k, k] on the device, k = 1 or 3 (typically an nn.Parameter; rounded to bf16 for the product).
    bias    float32 [cout] or None.
    act     "leaky" (LeakyReLU(0.1)) or "none".
    out_dtype  torch.bfloat16 (``cout % 8 == 0``) or torch.float32 (the head form: any cout).
    Returns an NCHW-shaped channels-last tensor.  Under ``torch.no_grad()``, or when no input requires grad, only the forward runs and
    the result has no ``grad_fn``.  Gradients: x bf16 (rounded once), weight and bias float32; two runs give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError("conv_block: x must be [n, cin, h, w] and weight [cout, cin, k, k]")
    if stride != 1:
        raise ValueError(f"conv_block: stride {stride} unsupported (the backward covers stride 1)")
    if act not in _ACTS:
        raise ValueError(f"conv_block: act must be 'leaky' or 'none', not {act!r}")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"conv_block: out_dtype must be torch.bfloat16 or torch.float32, not {out_dtype}")
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"conv_block: kernel {k}x{k2} unsupported (1x1 or 3x3)")
    if x.shape[1] != cin:
        raise ValueError(f"conv_block: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError("conv_block: empty tensor")
    if weight.dtype != torch.float32 or (bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (cout,))):
        raise ValueError("conv_block: weight must be float32 [cout, cin, k, k] and bias float32 [cout]")
    if out_dtype == torch.bfloat16 and cout % 8:
        raise ValueError(f"conv_block: a bfloat16 output needs cout % 8 == 0 (cout {cout}); use out_dtype=torch.float32")
    if not (x.is_cuda and weight.is_cuda and (bias is None or bias.is_cuda)):
        raise RuntimeError("pytorch_yolo_amd.conv_block runs on a ROCm device only (no CPU fallback)")
    x, weight = _to_kernel_layout(x, weight)
    act_id, out_f32 = _ACTS[act], out_dtype == torch.float32
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _ConvBlockFunction.apply(x, weight, bias, act_id, out_f32)
    return _forward(x.detach(), weight.detach(), None if bias is None else bias.detach(), act_id, out_f32)[0]


def _bn_forward(x, weight, gamma, beta, running, momentum, eps, act_id, stride=1):
    """conv (act none, zero bias) -> batch statistics -> normalise and activate.  Returns the NCHW-shaped result, the conv's descriptor, the
    dense NHWC z and the saved [4, cout] vectors."""
    z, d = _forward(x, weight, None, ACT_NONE, False, stride)
    z = z.permute(0, 2, 3, 1)                                             # the dense [n, ho, wo, cout] buffer the conv wrote
    with torch.cuda.device(x.device):
        saved = torch.empty((4, d.cout), dtype=torch.float32, device=x.device)
        ws = torch.empty((K.bn_workspace_bytes(d.n * d.ho * d.wo, d.cout),), dtype=torch.uint8, device=x.device)
        K.bn_train_stats(z, gamma, beta, eps, momentum, running[0], running[1], saved, ws)
        y = torch.empty_like(z)
        K.bn_act_fwd(z, saved, y, act_id)
    return y.permute(0, 3, 1, 2), d, z, saved


class _ConvBnBlockFunction(torch.autograd.Function):
    """_bn_forward (training=True) with a backward: the batch-norm backward (g, dgamma, dbeta), then conv_block's weight and data gradients on g, each
    only where asked.  z and saved are kept, y is not.  ``running`` is a tuple, so autograd does not track the in-place update."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running, momentum, eps, act_id):
        out, d, z, saved = _bn_forward(x, weight, gamma.detach(), beta.detach(), running, momentum, eps, act_id)
        ctx.desc, ctx.act_id = d, act_id
        ctx.save_for_backward(x, weight, z, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, z, saved = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        dx = dw = dgamma = dbeta = g = None
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()                    # dense [n, h, w, cout]; no copy for a channels-last dy
            if need_x or need_w:
                g = torch.empty_like(z)
            if need_g:
                dgamma = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            if need_b:
                dbeta = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            ws = torch.empty((K.bn_workspace_bytes(d.n * d.h * d.w, d.cout),), dtype=torch.uint8, device=x.device)
            K.bn_act_bwd(dy, z, saved, ctx.act_id, True, g, dgamma, dbeta, ws)
            if need_w:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                ws = torch.empty((K.conv2d_bwd_workspace_bytes(d),), dtype=torch.uint8, device=x.device)
                K.conv2d_bwd_weight(x, g, dw, None, ws, d)
            if need_x:
                packed_t, _, _ = K.pack_conv_weight_dev(weight, d.cout, transposed=True)
                buf = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
                K.conv2d_bwd_data(g, packed_t, buf, d)
                dx = buf.permute(0, 3, 1, 2)
        return dx, dw, dgamma, dbeta, None, None, None, None


def _check_momentum_eps(name, momentum, eps):
    if momentum is None or isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum <= 1.0:
        raise ValueError(f"{name}: momentum must be a number in [0, 1], not {momentum!r} (the cumulative average is unsupported)")
    if not isinstance(eps, (int, float)) or not eps >= 0.0:
        raise ValueError(f"{name}: eps must be a non-negative number, not {eps!r}")


def _check_bn_vectors(name, cout, gamma, beta, running_mean, running_var, training):
    """The batch-norm vectors of ``name`` (conv_bn_block / down_bn_block): float32 [cout]; training=False needs both running tensors."""
    vectors = (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var))
    for what, t in vectors:
        if t is None and what.startswith("running"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (cout,):
            raise ValueError(f"{name}: {what} must be float32 [cout]")
    if not training and (running_mean is None or running_var is None):
        raise ValueError(f"{name}: training=False needs running_mean and running_var")
    return vectors


def _to_kernel_layout(x, weight):
    """The conversions of an op's x and weight, outside the Function so that torch differentiates them: cin zero-padded to a multiple of
    8, x bfloat16 and dense channels-last, weight contiguous."""
    cin = weight.shape[1]
    if cin % 8:
        padc = 8 - cin % 8
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, padc))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, padc))
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    if not x.permute(0, 2, 3, 1).is_contiguous():
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x, weight.contiguous()


def _running(name, running_mean, running_var):
    running = (None if running_mean is None else running_mean.detach(), None if running_var is None else running_var.detach())
    if any(t is not None and not t.is_contiguous() for t in running):
        raise ValueError(f"{name}: the running tensors must be contiguous (they are updated in place)")
    return running


def conv_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky",
                  stride=1):
    """``act(batch_norm(conv2d(x, bf16(weight), padding=k // 2)))`` at stride 1 on the device, differentiable once: the reference's
    ConvBlock (Conv2d(bias=False) -> BatchNorm2d -> LeakyReLU(0.1)) as it trains.

    x, weight   as in conv_block (the same conversions by torch outside the Function); ``cout % 8 == 0``.
    gamma, beta float32 [cout] on the device: BatchNorm2d's weight and bias.
    running_mean, running_var   float32 [cout] on the device or None.  ``training=True``: the batch's statistics normalise, and the
                running tensors that are given are updated in place (momentum; running_var takes the unbiased variance, as torch).
                ``training=False``: both are required, they normalise, and nothing is updated: the call is
                ``conv_block(x, weight * s, beta - running_mean * s, act=act)`` with ``s = gamma / sqrt(running_var + eps)`` folded by
                torch in float32 (one launch, one rounding of the result; autograd differentiates the fold).
                ``num_batches_tracked`` is the caller's, as with torch.nn.functional.batch_norm.
    momentum    a number in [0, 1]; None (torch's cumulative average) raises ValueError.
    act         "leaky" (LeakyReLU(0.1)) or "none".
    Returns an NCHW-shaped channels-last bfloat16 tensor.  Under ``torch.no_grad()``, or when no input requires grad, only the forward
    runs.  Gradients: x bf16, weight, gamma and beta float32, each computed only where asked; two runs give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError("conv_bn_block: x must be [n, cin, h, w] and weight [cout, cin, k, k]")
    if stride != 1:
        raise ValueError(f"conv_bn_block: stride {stride} unsupported (the backward covers stride 1)")
    if act not in _ACTS:
        raise ValueError(f"conv_bn_block: act must be 'leaky' or 'none', not {act!r}")
    _check_momentum_eps("conv_bn_block", momentum, eps)
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"conv_bn_block: kernel {k}x{k2} unsupported (1x1 or 3x3)")
    if x.shape[1] != cin:
        raise ValueError(f"conv_bn_block: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError("conv_bn_block: empty tensor")
    if cout % 8:
        raise ValueError(f"conv_bn_block: cout % 8 == 0 is required (cout {cout})")
    if weight.dtype != torch.float32:
        raise ValueError("conv_bn_block: weight must be float32 [cout, cin, k, k]")
    training = bool(training)
    vectors = _check_bn_vectors("conv_bn_block", cout, gamma, beta, running_mean, running_var, training)
    if training and x.shape[0] * x.shape[2] * x.shape[3] < 2:
        raise ValueError("conv_bn_block: expected more than 1 value per channel when training")
    if not (x.is_cuda and weight.is_cuda and all(t is None or t.is_cuda for _, t in vectors)):
        raise RuntimeError("pytorch_yolo_amd.conv_bn_block runs on a ROCm device only (no CPU fallback)")
    if not training:        # frozen statistics: the folded layer, as the models run it
        s = gamma / torch.sqrt(running_var.detach() + eps)
        return conv_block(x, weight * s.reshape(-1, 1, 1, 1), beta - running_mean.detach() * s, act=act)
    x, weight = _to_kernel_layout(x, weight)
    gamma, beta = gamma.contiguous(), beta.contiguous()
    running = _running("conv_bn_block", running_mean, running_var)
    act_id = _ACTS[act]
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or gamma.requires_grad or beta.requires_grad):
        return _ConvBnBlockFunction.apply(x, weight, gamma, beta, running, float(momentum), float(eps), act_id)
    return _bn_forward(x.detach(), weight.detach(), gamma.detach(), beta.detach(), running, float(momentum), float(eps), act_id)[0]


# ---- the residual unit's closing ConvBlock with the add fused in -------------------------------------------------------------------------
class _ResBnBlockFunction(torch.autograd.Function):
    """conv -> batch statistics -> normalise, activate and add the residual in one pass (yolo_bn_act_add_fwd).  The backward is
    conv_bn_block's on dy (+ the gradient of y_preadd where it was routed, summed in fp32 by torch); dy itself is the residual's."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, running, momentum, eps, want_preadd):
        z, d = _forward(x, weight, None, ACT_NONE, False)
        z = z.permute(0, 2, 3, 1)
        with torch.cuda.device(x.device):
            saved = torch.empty((4, d.cout), dtype=torch.float32, device=x.device)
            ws = torch.empty((K.bn_workspace_bytes(d.n * d.h * d.w, d.cout),), dtype=torch.uint8, device=x.device)
            K.bn_train_stats(z, gamma.detach(), beta.detach(), eps, momentum, running[0], running[1], saved, ws)
            y = torch.empty_like(z)
            pre = torch.empty_like(z) if want_preadd else None
            K.bn_act_add_fwd(z, saved, residual.detach().permute(0, 2, 3, 1), y, pre, ACT_LEAKY01)
        ctx.desc = d
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, weight, z, saved)
        y = y.permute(0, 3, 1, 2)
        return (y, pre.permute(0, 3, 1, 2)) if want_preadd else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dpre=None):
        x, weight, z, saved = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_g, need_b, need_r = ctx.needs_input_grad[:5]
        dx = dw = dgamma = dbeta = g = None
        if dy is None and dpre is None:
            return (None,) * 9
        dres = dy if need_r else None
        if dy is not None and dpre is not None:
            dy = dy.float() + dpre.float()                              # one fp32 sum: yolo_bn_act_bwd takes an fp32 dy
        elif dy is None:
            dy = dpre
        with torch.cuda.device(x.device):
            if need_x or need_w or need_g or need_b:
                dy = dy.permute(0, 2, 3, 1).contiguous()
                if need_x or need_w:
                    g = torch.empty_like(z)
                if need_g:
                    dgamma = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
                if need_b:
                    dbeta = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
                ws = torch.empty((K.bn_workspace_bytes(d.n * d.h * d.w, d.cout),), dtype=torch.uint8, device=x.device)
                K.bn_act_bwd(dy, z, saved, ACT_LEAKY01, True, g, dgamma, dbeta, ws)
            if need_w:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                ws = torch.empty((K.conv2d_bwd_workspace_bytes(d),), dtype=torch.uint8, device=x.device)
                K.conv2d_bwd_weight(x, g, dw, None, ws, d)
            if need_x:
                packed_t, _, _ = K.pack_conv_weight_dev(weight, d.cout, transposed=True)
                buf = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
                K.conv2d_bwd_data(g, packed_t, buf, d)
                dx = buf.permute(0, 3, 1, 2)
        return dx, dw, dgamma, dbeta, dres, None, None, None, None


def _dense_bf16(t):
    """t as bfloat16, dense channels-last, by torch operations (torch differentiates them)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    if not t.permute(0, 2, 3, 1).is_contiguous():
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def res_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, residual=None, *, want_preadd=False, training=True,
                 momentum=0.1, eps=1e-5):
    """``leaky(batch_norm(conv2d(x, bf16(weight), padding=k // 2))) + residual`` on the device, differentiable once: the closing ConvBlock
    of a Darknet-53 residual unit with its add (reference models/yolov3_spp.py:12-14,42-46), the add fused into the normalise-and-activate
    pass (yolo_bn_act_add_fwd).

    conv_bn_block's contract at stride 1 with LeakyReLU(0.1) and ``training=True`` (anything else raises ValueError).
    residual    [n, cout, h, w]; bfloat16 dense channels-last is taken as it is, anything else is converted by torch.
    want_preadd also return ``y_preadd = bf16(leaky(batch_norm(..)))``, the branch output before the add (what the reference routes to the
                FPN from the last unit of down3 / down4): ``(y, y_preadd)``; both carry gradients.
    Gradients: x bf16, weight, gamma and beta float32, residual the incoming gradient of y unchanged; each computed only where asked."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError("res_bn_block: x must be [n, cin, h, w] and weight [cout, cin, k, k]")
    if not training:
        raise ValueError("res_bn_block: training=True only (the frozen layer is the models' inference path)")
    _check_momentum_eps("res_bn_block", momentum, eps)
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"res_bn_block: kernel {k}x{k2} unsupported (1x1 or 3x3)")
    if x.shape[1] != cin:
        raise ValueError(f"res_bn_block: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError("res_bn_block: empty tensor")
    if cout % 8:
        raise ValueError(f"res_bn_block: cout % 8 == 0 is required (cout {cout})")
    if weight.dtype != torch.float32:
        raise ValueError("res_bn_block: weight must be float32 [cout, cin, k, k]")
    if not isinstance(residual, torch.Tensor) or tuple(residual.shape) != (x.shape[0], cout, x.shape[2], x.shape[3]):
        raise ValueError("res_bn_block: residual must be [n, cout, h, w]")
    vectors = _check_bn_vectors("res_bn_block", cout, gamma, beta, running_mean, running_var, True)
    if x.shape[0] * x.shape[2] * x.shape[3] < 2:
        raise ValueError("res_bn_block: expected more than 1 value per channel when training")
    if not (x.is_cuda and weight.is_cuda and residual.is_cuda and all(t is None or t.is_cuda for _, t in vectors)):
        raise RuntimeError("pytorch_yolo_amd.res_bn_block runs on a ROCm device only (no CPU fallback)")
    x, weight = _to_kernel_layout(x, weight)
    residual = _dense_bf16(residual)
    gamma, beta = gamma.contiguous(), beta.contiguous()
    running = _running("res_bn_block", running_mean, running_var)
    return _ResBnBlockFunction.apply(x, weight, gamma, beta, residual, running, float(momentum), float(eps), bool(want_preadd))


# ---- the SPP pyramid and the FPN's upsample + concat -------------------------------------------------------------------------------------
class _SppConcatFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xn = x.permute(0, 2, 3, 1)
        n, h, w, c = xn.shape
        with torch.cuda.device(x.device):
            y = torch.empty((n, h, w, 4 * c), dtype=torch.bfloat16, device=x.device)
            idx = torch.empty((n, h, w, 3 * c), dtype=torch.uint8, device=x.device)
            K.spp_train_fwd(xn, y, idx)
        ctx.save_for_backward(idx)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        n, h, w, c3 = idx.shape
        with torch.cuda.device(idx.device):
            dy = _dense_bf16(dy).permute(0, 2, 3, 1)
            dx = torch.empty((n, h, w, c3 // 3), dtype=torch.bfloat16, device=idx.device)
            K.spp_bwd(dy, idx, dx)
        return dx.permute(0, 3, 1, 2)


class _UpsampleConcatFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, up_first=True):
        an, bn = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)
        n, h, w, ca = an.shape
        ctx.dims = (n, h, w, ca, bn.shape[3])
        ctx.up_first = up_first
        with torch.cuda.device(a.device):
            y = torch.empty((n, 2 * h, 2 * w, ca + bn.shape[3]), dtype=torch.bfloat16, device=a.device)
            if up_first:
                K.upsample2_concat_fwd(an, bn, y)
            else:
                K.concat_upsample2_fwd(bn, an, y)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n, h, w, ca, cb = ctx.dims
        need_a, need_b = ctx.needs_input_grad[:2]
        da = db = None
        if not (need_a or need_b):
            return None, None, None
        with torch.cuda.device(dy.device):
            dy = _dense_bf16(dy).permute(0, 2, 3, 1)
            if need_a:
                da = torch.empty((n, h, w, ca), dtype=torch.bfloat16, device=dy.device)
            if need_b:
                db = torch.empty((n, 2 * h, 2 * w, cb), dtype=torch.bfloat16, device=dy.device)
            if ctx.up_first:
                K.upsample2_concat_bwd(dy, da, db, n=n, h=h, w=w, ca=ca, cb=cb)
            else:
                K.concat_upsample2_bwd(dy, db, da, n=n, h=h, w=w, cb=cb, ca=ca)
        return (None if da is None else da.permute(0, 3, 1, 2)), (None if db is None else db.permute(0, 3, 1, 2)), None


def _check_map(name, what, t):
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{name}: {what} must be [n, c, h, w]")
    if min(t.shape) < 1:
        raise ValueError(f"{name}: empty tensor")
    if t.shape[1] % 8:
        raise ValueError(f"{name}: {what} needs c % 8 == 0 (c {t.shape[1]})")


def spp_concat(x):
    """``cat([max_pool2d(x, 5, 1, 2), max_pool2d(x, 9, 1, 4), max_pool2d(x, 13, 1, 6), x], 1)`` on the device, differentiable once: the SPP
    pyramid of YOLOv3-SPP (reference models/yolov3_spp.py:75-77,129).  x [n, c, h, w], ``c % 8 == 0``, any h, w >= 1; bfloat16 dense
    channels-last is taken as it is, anything else is converted by torch.  Returns bfloat16 [n, 4c, h, w], channels-last.  The gradient
    of a window goes to its first maximum in row-major order (torch's rule), summed in fp32 in a fixed order and rounded once.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    _check_map("spp_concat", "x", x)
    if not x.is_cuda:
        raise RuntimeError("pytorch_yolo_amd.spp_concat runs on a ROCm device only (no CPU fallback)")
    return _SppConcatFunction.apply(_dense_bf16(x))


def upsample_concat(a, b, *, up_first=True):
    """``cat([interpolate(a, scale_factor=2, mode="nearest"), b], 1)`` on the device, differentiable once: the FPN's Upsample + Concat
    (reference models/yolo_layer.py:6-22).  a [n, ca, h, w], b [n, cb, 2h, 2w], ``ca % 8 == 0`` and ``cb % 8 == 0``; converted like
    spp_concat's x.  Returns bfloat16 [n, ca + cb, 2h, 2w], channels-last.  Gradients: a the fp32 sum of each 2x2 block rounded once, b
    the copy of its slice; each computed only where asked.  Errors as spp_concat.
    ``up_first=False`` gives ``cat([b, interpolate(a, ...)], 1)``, the order of YOLOv3-tiny (reference models/yolov3_tiny.py:73)."""
    _check_map("upsample_concat", "a", a)
    _check_map("upsample_concat", "b", b)
    if tuple(b.shape[0:1] + b.shape[2:]) != (a.shape[0], 2 * a.shape[2], 2 * a.shape[3]):
        raise ValueError(f"upsample_concat: b {tuple(b.shape)} must be [n, cb, 2h, 2w] of a {tuple(a.shape)}")
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("pytorch_yolo_amd.upsample_concat runs on a ROCm device only (no CPU fallback)")
    return _UpsampleConcatFunction.apply(_dense_bf16(a), _dense_bf16(b), bool(up_first))


# ---- the downsample: ConvBlock(3x3, stride 2, pad 1) ---------------------------------------------------------------------------------------
def _down_grads(x, weight, g, d, need_x, need_w, need_b):
    """The two gradients of the stride-2 conv ``d`` on the dense bf16 g [n, ho, wo, cout], each only where asked: (dx, dw, db)."""
    dx = dw = db = None
    if need_w or need_b:
        dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
        db = torch.empty((d.cout,), dtype=torch.float32, device=x.device) if need_b else None
        ws = torch.empty((K.conv2d_down_bwd_workspace_bytes(d),), dtype=torch.uint8, device=x.device)
        K.conv2d_down_bwd_weight(x, g, dw, db, ws, d)
        if not need_w:
            dw = None
    if need_x:
        packed_d = K.pack_conv_weight_down_dev(weight)
        buf = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
        K.conv2d_down_bwd_data(g, packed_d, buf, d)
        dx = buf.permute(0, 3, 1, 2)
    return dx, dw, db


class _DownBlockFunction(torch.autograd.Function):
    """_forward at stride 2 with a backward: prepare (g) on the stride-1 descriptor of the output map, then _down_grads."""

    @staticmethod
    def forward(ctx, x, weight, bias, act_id):
        out, d = _forward(x, weight, None if bias is None else bias.detach(), act_id, False, 2)
        ctx.desc = d
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, out if act_id != ACT_NONE else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()                    # dense [n, ho, wo, cout]; no copy for a channels-last dy
            g = torch.empty((d.n, d.ho, d.wo, d.cout), dtype=torch.bfloat16, device=x.device)
            od = K.conv_desc(n=d.n, h=d.ho, w=d.wo, cin=d.cout, in_c_total=d.cout, in_c_offset=0, cout=d.cout, out_c_total=d.cout,
                             out_c_offset=0, ksize=1, stride=1, act=d.act, kpad=K.roundup(d.cout, 64), cout_pad=d.cout_pad)
            K.conv2d_bwd_prepare(dy, y, g, od)
            dx, dw, db = _down_grads(x, weight, g, d, need_x, need_w, need_b)
        return dx, dw, db, None


class _DownBnBlockFunction(torch.autograd.Function):
    """_bn_forward at stride 2 (training=True) with a backward: conv_bn_block's batch-norm backward (g, dgamma, dbeta), then _down_grads."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running, momentum, eps, act_id):
        out, d, z, saved = _bn_forward(x, weight, gamma.detach(), beta.detach(), running, momentum, eps, act_id, 2)
        ctx.desc, ctx.act_id = d, act_id
        ctx.save_for_backward(x, weight, z, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, z, saved = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        dgamma = dbeta = g = None
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()
            if need_x or need_w:
                g = torch.empty_like(z)
            if need_g:
                dgamma = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            if need_b:
                dbeta = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            ws = torch.empty((K.bn_workspace_bytes(d.n * d.ho * d.wo, d.cout),), dtype=torch.uint8, device=x.device)
            K.bn_act_bwd(dy, z, saved, ctx.act_id, True, g, dgamma, dbeta, ws)
            dx, dw, _ = _down_grads(x, weight, g, d, need_x, need_w, False)
        return dx, dw, dgamma, dbeta, None, None, None, None


def _down_check(name, x, weight, act):
    """The argument checks the two downsample ops share (ValueError before any launch)."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{name}: x must be [n, cin, h, w] and weight [cout, cin, 3, 3]")
    if act not in _ACTS:
        raise ValueError(f"{name}: act must be 'leaky' or 'none', not {act!r}")
    cout, cin, k, k2 = weight.shape
    if k != 3 or k2 != 3:
        raise ValueError(f"{name}: kernel {k}x{k2} unsupported (the downsample is 3x3, stride 2, pad 1)")
    if x.shape[1] != cin:
        raise ValueError(f"{name}: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError(f"{name}: empty tensor")
    if cout % 8:
        raise ValueError(f"{name}: cout % 8 == 0 is required (cout {cout})")
    if weight.dtype != torch.float32:
        raise ValueError(f"{name}: weight must be float32 [cout, cin, 3, 3]")


def down_block(x, weight, bias=None, *, act="leaky"):
    """``act(conv2d(x, bf16(weight), stride=2, padding=1) + bias)`` on the device, differentiable once: conv_block's contract for the
    3x3 stride-2 downsample of Darknet-53 (ConvBlock(3x3, stride 2) with its BN folded).  The output map is
    ``((h - 1) // 2 + 1, (w - 1) // 2 + 1)``, torch's for even and odd maps.

    x       [n, cin, h, w]; zero-copy for bfloat16 dense channels-last with ``cin % 8 == 0``, otherwise converted by torch as in conv_block.
    weight  float32 [cout, cin, 3, 3] on the device, ``cout % 8 == 0``.      bias  float32 [cout] or None.
    act     "leaky" (LeakyReLU(0.1)) or "none".
    Returns an NCHW-shaped channels-last bfloat16 tensor.  Under ``torch.no_grad()``, or when no input requires grad, only the forward
    runs.  Gradients: x bf16 (rounded once), weight and bias float32, each computed only where asked; two runs give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    _down_check("down_block", x, weight, act)
    cout = weight.shape[0]
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (cout,)):
        raise ValueError("down_block: bias must be float32 [cout]")
    if not (x.is_cuda and weight.is_cuda and (bias is None or bias.is_cuda)):
        raise RuntimeError("pytorch_yolo_amd.down_block runs on a ROCm device only (no CPU fallback)")
    x, weight = _to_kernel_layout(x, weight)
    act_id = _ACTS[act]
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _DownBlockFunction.apply(x, weight, bias, act_id)
    return _forward(x.detach(), weight.detach(), None if bias is None else bias.detach(), act_id, False, 2)[0]


def down_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky"):
    """``act(batch_norm(conv2d(x, bf16(weight), stride=2, padding=1)))`` on the device, differentiable once: conv_bn_block's contract
    for the 3x3 stride-2 downsample (Conv2d(3x3, stride 2, bias=False) -> BatchNorm2d -> LeakyReLU(0.1)) as the reference trains it.

    Arguments, running statistics, ``training=False`` (down_block on the weights folded by torch) and errors are conv_bn_block's; the
    statistics run over the ``n ho wo`` output pixels."""
    _down_check("down_bn_block", x, weight, act)
    _check_momentum_eps("down_bn_block", momentum, eps)
    training = bool(training)
    vectors = _check_bn_vectors("down_bn_block", weight.shape[0], gamma, beta, running_mean, running_var, training)
    ho, wo = (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1
    if training and x.shape[0] * ho * wo < 2:
        raise ValueError("down_bn_block: expected more than 1 value per channel when training")
    if not (x.is_cuda and weight.is_cuda and all(t is None or t.is_cuda for _, t in vectors)):
        raise RuntimeError("pytorch_yolo_amd.down_bn_block runs on a ROCm device only (no CPU fallback)")
    if not training:        # frozen statistics: the folded layer
        s = gamma / torch.sqrt(running_var.detach() + eps)
        return down_block(x, weight * s.reshape(-1, 1, 1, 1), beta - running_mean.detach() * s, act=act)
    x, weight = _to_kernel_layout(x, weight)
    gamma, beta = gamma.contiguous(), beta.contiguous()
    running = _running("down_bn_block", running_mean, running_var)
    act_id = _ACTS[act]
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or gamma.requires_grad or beta.requires_grad):
        return _DownBnBlockFunction.apply(x, weight, gamma, beta, running, float(momentum), float(eps), act_id)
    return _bn_forward(x.detach(), weight.detach(), gamma.detach(), beta.detach(), running, float(momentum), float(eps), act_id, 2)[0]


# ---- the max-pools of YOLOv3-tiny / LiteYOLOv3: MaxPool and ConvPoolBlock as they train -----------------------------------
def _pool_forward(xn, stride):
    """The pool launch on the dense bf16 [n, h, w, c] xn: (y, idx), both dense NHWC."""
    n, h, w, c = xn.shape
    ho, wo = (h // 2, w // 2) if stride == 2 else (h, w)
    y = torch.empty((n, ho, wo, c), dtype=torch.bfloat16, device=xn.device)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=xn.device)
    K.maxpool_train_fwd(xn, y, idx, stride)
    return y, idx


def _pool_backward(dy, idx, shape, stride):
    """dy (NCHW-shaped, any layout / dtype) -> the dense bf16 [n, h, w, c] gradient of the pool's input."""
    dx = torch.empty(shape, dtype=torch.bfloat16, device=idx.device)
    K.maxpool_bwd(_dense_bf16(dy).permute(0, 2, 3, 1), idx, dx, stride)
    return dx


class _MaxPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride):
        xn = x.permute(0, 2, 3, 1)
        with torch.cuda.device(x.device):
            y, idx = _pool_forward(xn, stride)
        ctx.shape, ctx.stride = tuple(xn.shape), stride
        ctx.save_for_backward(idx)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        with torch.cuda.device(idx.device):
            dx = _pool_backward(dy, idx, ctx.shape, ctx.stride)
        return dx.permute(0, 3, 1, 2), None


def _check_pool(name, stride, h, w):
    if isinstance(stride, bool) or stride not in (1, 2):
        raise ValueError(f"{name}: pool stride must be 2 (MaxPool2d(2, 2)) or 1 (MaxPool2d(2, 1, padding=1, dilation=2)), not {stride!r}")
    if h < 2 or w < 2:
        raise ValueError(f"{name}: the pool needs a map of at least 2 x 2, got {h} x {w} (stride 2: empty output; stride 1: a window "
                         "would be all padding)")


def max_pool(x, *, stride=2):
    """The reference's MaxPool (models/yolo_base.py:60-66) on the device, differentiable once.  ``stride=2``: ``max_pool2d(x, 2, 2)``
    (floor: an odd last row or column is dropped); ``stride=1``: ``max_pool2d(x, 2, 1, padding=1, dilation=2)``, the form MaxPool(2, 1)
    turns into - the four diagonal neighbours, the output has the input's size.  x [n, c, h, w], ``c % 8 == 0``, h and w >= 2; bfloat16
    dense channels-last is taken as it is, anything else is converted by torch.  Returns bfloat16, channels-last.  The gradient of a window
    goes to its first maximum in row-major order (torch's rule); at stride 1 the up to four terms of a pixel are summed in fp32 in a fixed
    order and rounded once.  x must hold no NaN.  Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there
    is no CPU fallback)."""
    _check_map("max_pool", "x", x)
    _check_pool("max_pool", stride, x.shape[2], x.shape[3])
    if not x.is_cuda:
        raise RuntimeError("pytorch_yolo_amd.max_pool runs on a ROCm device only (no CPU fallback)")
    return _MaxPoolFunction.apply(_dense_bf16(x), int(stride))


def _pool_bn_forward(x, weight, gamma, beta, running, momentum, eps, act_id, pool_stride):
    """conv (act none) -> batch statistics over the unpooled z -> normalise, activate and pool: the fused pass at pool stride 2, the two
    separate launches at stride 1.  Returns the NCHW-shaped pooled result, the conv's descriptor, z, saved and idx."""
    z, d = _forward(x, weight, None, ACT_NONE, False)
    z = z.permute(0, 2, 3, 1)
    with torch.cuda.device(x.device):
        saved = torch.empty((4, d.cout), dtype=torch.float32, device=x.device)
        ws = torch.empty((K.bn_workspace_bytes(d.n * d.h * d.w, d.cout),), dtype=torch.uint8, device=x.device)
        K.bn_train_stats(z, gamma, beta, eps, momentum, running[0], running[1], saved, ws)
        if pool_stride == 2:
            y = torch.empty((d.n, d.h // 2, d.w // 2, d.cout), dtype=torch.bfloat16, device=x.device)
            idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
            K.bn_act_pool_fwd(z, saved, y, idx, act_id)
        else:
            full = torch.empty_like(z)
            K.bn_act_fwd(z, saved, full, act_id)
            y, idx = _pool_forward(full, 1)
    return y.permute(0, 3, 1, 2), d, z, saved, idx


class _PoolBnBlockFunction(torch.autograd.Function):
    """_pool_bn_forward with a backward: yolo_maxpool_bwd expands dy to a full-resolution bf16 map, which goes through conv_bn_block's
    backward (yolo_bn_act_bwd, then the conv's weight and data gradients), each only where asked.  x, weight, z, saved and idx are kept."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running, momentum, eps, act_id, pool_stride):
        out, d, z, saved, idx = _pool_bn_forward(x, weight, gamma.detach(), beta.detach(), running, momentum, eps, act_id, pool_stride)
        ctx.desc, ctx.act_id, ctx.pool_stride = d, act_id, pool_stride
        ctx.save_for_backward(x, weight, z, saved, idx)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, z, saved, idx = ctx.saved_tensors
        d = ctx.desc
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        dx = dw = dgamma = dbeta = g = None
        with torch.cuda.device(x.device):
            dfull = _pool_backward(dy, idx, tuple(z.shape), ctx.pool_stride)
            if need_x or need_w:
                g = torch.empty_like(z)
            if need_g:
                dgamma = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            if need_b:
                dbeta = torch.empty((d.cout,), dtype=torch.float32, device=x.device)
            ws = torch.empty((K.bn_workspace_bytes(d.n * d.h * d.w, d.cout),), dtype=torch.uint8, device=x.device)
            K.bn_act_bwd(dfull, z, saved, ctx.act_id, True, g, dgamma, dbeta, ws)
            if need_w:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                ws = torch.empty((K.conv2d_bwd_workspace_bytes(d),), dtype=torch.uint8, device=x.device)
                K.conv2d_bwd_weight(x, g, dw, None, ws, d)
            if need_x:
                packed_t, _, _ = K.pack_conv_weight_dev(weight, d.cout, transposed=True)
                buf = torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
                K.conv2d_bwd_data(g, packed_t, buf, d)
                dx = buf.permute(0, 3, 1, 2)
        return dx, dw, dgamma, dbeta, None, None, None, None, None


def pool_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, pool_stride=2, training=True, momentum=0.1, eps=1e-5,
                  act="leaky"):
    """``max_pool(act(batch_norm(conv2d(x, bf16(weight), padding=k // 2))), stride=pool_stride)`` on the device, differentiable once: the
    reference's ConvPoolBlock (models/yolo_base.py:69-80) as it trains.

    conv_bn_block's contract at stride 1 with ``training=True`` (anything else raises ValueError).  The conv, the batch statistics and the
    update of the running tensors run over the unpooled map.  ``pool_stride=2``: the normalise-and-activate pass pools as it goes
    (yolo_bn_act_pool_fwd; the full-resolution activation is never written); ``pool_stride=1``: yolo_bn_act_fwd, then the stride-1 pool.
    Both are max_pool's forms and rules, and the result is bit-equal to ``max_pool(conv_bn_block(...), stride=pool_stride)``.
    The backward expands the incoming gradient to the unpooled map (yolo_maxpool_bwd) and continues as conv_bn_block's.
    Gradients: x bf16, weight, gamma and beta float32, each computed only where asked; two runs give the same bits."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError("pool_bn_block: x must be [n, cin, h, w] and weight [cout, cin, k, k]")
    if not training:
        raise ValueError("pool_bn_block: training=True only (the frozen layer is the models' inference path)")
    if act not in _ACTS:
        raise ValueError(f"pool_bn_block: act must be 'leaky' or 'none', not {act!r}")
    _check_momentum_eps("pool_bn_block", momentum, eps)
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"pool_bn_block: kernel {k}x{k2} unsupported (1x1 or 3x3)")
    if x.shape[1] != cin:
        raise ValueError(f"pool_bn_block: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError("pool_bn_block: empty tensor")
    if cout % 8:
        raise ValueError(f"pool_bn_block: cout % 8 == 0 is required (cout {cout})")
    if weight.dtype != torch.float32:
        raise ValueError("pool_bn_block: weight must be float32 [cout, cin, k, k]")
    _check_pool("pool_bn_block", pool_stride, x.shape[2], x.shape[3])
    vectors = _check_bn_vectors("pool_bn_block", cout, gamma, beta, running_mean, running_var, True)
    if not (x.is_cuda and weight.is_cuda and all(t is None or t.is_cuda for _, t in vectors)):
        raise RuntimeError("pytorch_yolo_amd.pool_bn_block runs on a ROCm device only (no CPU fallback)")
    x, weight = _to_kernel_layout(x, weight)
    gamma, beta = gamma.contiguous(), beta.contiguous()
    running = _running("pool_bn_block", running_mean, running_var)
    act_id, pool_stride = _ACTS[act], int(pool_stride)
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or gamma.requires_grad or beta.requires_grad):
        return _PoolBnBlockFunction.apply(x, weight, gamma, beta, running, float(momentum), float(eps), act_id, pool_stride)
    return _pool_bn_forward(x.detach(), weight.detach(), gamma.detach(), beta.detach(), running, float(momentum), float(eps), act_id,
                            pool_stride)[0]
