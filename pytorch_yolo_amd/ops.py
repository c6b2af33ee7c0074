"""Differentiable building blocks on the package's kernels.

``conv_block`` is ConvBlock.forward of the reference (models/yolo_base.py:19-44, BN folded; with ``act="none"`` and
``out_dtype=torch.float32`` the plain nn.Conv2d heads of models/yolov3_tiny.py:38,42) at stride 1, 1x1 or 3x3, in bf16 mode, WITH a
backward: the forward is the launch the models use (yolo_conv2d_fwd), the backward runs csrc/conv_bwd.hip.  The
models' own forward stays inference-only: ``io, p = model(x)`` has no ``grad_fn``.
"""
from __future__ import annotations

import torch

from . import kernels as K
from ._lib import ACT_LEAKY01, ACT_NONE, DT_BF16, DT_F32

__all__ = ["conv_block"]

_ACTS = {"leaky": ACT_LEAKY01, "none": ACT_NONE}


def _desc(x, weight, act_id, out_f32):
    n, c, h, w = x.shape
    cout, _, k, _ = weight.shape
    ct = K.roundup(cout, 4) if out_f32 else cout
    return K.conv_desc(n=n, h=h, w=w, cin=c, in_c_total=c, in_c_offset=0, cout=cout, out_c_total=ct, out_c_offset=0, ksize=k, stride=1,
                       act=act_id, kpad=K.roundup(k * k * c, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_F32 if out_f32 else DT_BF16)


def _forward(x, weight, bias, act_id, out_f32):
    """The forward launch on a device-packed weight.  x: bf16, NCHW-shaped, dense channels-last.  Returns the NCHW-shaped
    channels-last result (a view of the [n, h, w, out_c_total] buffer the kernel wrote) and the descriptor."""
    d = _desc(x, weight, act_id, out_f32)
    with torch.cuda.device(x.device):
        packed, _, cout_pad = K.pack_conv_weight_dev(weight, d.cin)
        b = torch.zeros((cout_pad,), dtype=torch.float32, device=x.device)
        if bias is not None:
            b[:d.cout] = bias
        y = torch.empty((d.n, d.h, d.w, d.out_c_total), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
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
    # conversions outside the Function: torch differentiates them
    if cin % 8:
        padc = 8 - cin % 8
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, padc))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, padc))
    if x.dtype != torch.bfloat16:
        x = x.to(torch.bfloat16)
    if not x.permute(0, 2, 3, 1).is_contiguous():
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    weight = weight.contiguous()
    act_id, out_f32 = _ACTS[act], out_dtype == torch.float32
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _ConvBlockFunction.apply(x, weight, bias, act_id, out_f32)
    return _forward(x.detach(), weight.detach(), None if bias is None else bias.detach(), act_id, out_f32)[0]
