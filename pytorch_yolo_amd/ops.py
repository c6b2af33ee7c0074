"""Differentiable building blocks on the package's kernels: the layers of the reference as they train, each a once-differentiable
``autograd.Function`` on hand-written launches, with no CPU fallback.

The ops (contracts in their docstrings; the kernels in DESIGN.md 3.6c-g):
    conv_block, down_block          ConvBlock with its BN folded (and the plain nn.Conv2d heads), stride 1 (1x1, 3x3) / stride 2 (3x3)
    conv_bn_block, down_bn_block    the same ConvBlock with BatchNorm2d on batch statistics; ``training=False`` is the folded op above
    res_bn_block                    the closing ConvBlock of a residual unit with its add
    pool_bn_block, max_pool         ConvPoolBlock and MaxPool of YOLOv3-tiny / LiteYOLOv3
    spp_concat, upsample_concat     the SPP pyramid, the FPN's upsample + concat
    stem_block, fire_block, max_pool_ceil   SqueezeNet 1.1's unpadded stride-2 first layer, Fire module and MaxPool2d(3, 2, ceil_mode=True)
                                    (DESIGN.md 3.6i); ``conv_block(act="relu")`` is its plain conv
    conv_bn_relu6_block, dw_bn_block, project_bn_block   MobileNetV2's inverted residual: the dense ConvBNReLU (expand, first and last
                                    layer), the depthwise ConvBNReLU and the linear bottleneck with its add
    expand_dw_bn_block              the expand and the depthwise ConvBNReLU of an expanding inverted residual as one op: bit-equal to
                                    dw_bn_block(conv_bn_relu6_block(..)), the hidden activation never written
    conv_bn_relu_block, max_pool_321, channel_shuffle2, shuffle_unit_block   ShuffleNetV2: the dense ConvBNReLU, MaxPool2d(3, 2, 1), the
                                    channel shuffle in the two-slot layout and the stride-1 unit as one op, its halves read and its
                                    gradient written as channel views
models/train.py wires the training-mode forward of the models from them; the models' eval forward stays inference-only.

The structure - every launch has one owner.  The pieces:
    _forward        pack the weight, yolo_conv2d_fwd: the launch the models use, at either stride; ``into``: a channel view of a wider
                    buffer; ``in_offset``: the operand is a channel view of a wider x
    _conv_grads     the conv's weight / bias and data gradients on g, each only where asked; dispatches on the descriptor's stride and pad
                    (csrc/conv_bwd.hip, csrc/conv_down_bwd.hip) and is the only caller of those bindings; ``dx_into``: a channel view
    _stats          the batch statistics of a conv's output map: the only caller of bn_train_stats
    _conv_stats     _forward with act none, then _stats
    _bn_act         the normalise-and-activate launch: bn_act_fwd, or bn_clamp_fwd where the activation is a (lo, hi) clamp
    _bn_grads       the batch-norm + activation backward (g, dgamma, dbeta by need): the only caller of bn_act_bwd / bn_clamp_bwd
    _bn_forward     _conv_stats and the tail: _bn_act, bn_act_pool_fwd (pool stride 2) or _bn_act + the stride-1 pool
    _dw_pack        the depthwise weight rounded once to bf16, laid out [9, c]
    _dw_stats       the depthwise conv - dwconv3x3, or dwconv3x3_bnin_fwd on an operand that is normalised and clamped as it is loaded -
                    then _stats: the only caller of the two
    _dw_grads       the depthwise data and weight gradients on g, each only where asked: the only caller of dwconv3x3_bwd_data,
                    dwconv3x3_bwd_weight and dwconv3x3_bnin_bwd_weight
    _POOLS          the four window max-pools (csrc/pool_train.hip): per form the forward and the backward binding; the output maps are
                    kernels.POOL_OUT
The Functions, each ``plain`` forward / backward:
    _ConvFunction(stride, pad)          conv_block, down_block, stem_block:  _forward / conv2d_bwd_prepare, _conv_grads
    _ConvBnFunction(act, stride, pool_stride)   conv_bn_block, down_bn_block, pool_bn_block, conv_bn_relu6_block, conv_bn_relu_block and
                                        project_bn_block without a residual:  _bn_forward / [the pool's backward,] _bn_grads, _conv_grads
    _ResBnFunction(act)                 res_bn_block, project_bn_block with a residual:  _conv_stats, bn_act_add_fwd (leaky) or
                                        bn_add_rounded_fwd (none) / _bn_grads, _conv_grads; dy passes through to the residual
    _PoolFunction(form)                 max_pool (both strides), max_pool_ceil, max_pool_321, and - its ``plain`` and ``grad`` - the pool
                                        tail of _bn_forward and _ConvBnFunction
    _SppConcatFunction, _UpsampleConcatFunction, _ChannelShuffle2Function   the glue ops (csrc/route.hip, csrc/pointwise.hip,
                                        csrc/shuffle_train.hip)
    _FireFunction                       fire_block:  three _forward (the expands into one buffer) / fire_bwd_split, _conv_grads twice,
                                        fire_bwd_join, _conv_grads
    _DwBnFunction                       dw_bn_block:  _dw_forward (_dw_pack, _dw_stats, _bn_act) / _bn_grads, _dw_grads
    _ExpandDwBnFunction                 expand_dw_bn_block:  _conv_stats, _dw_pack, _dw_stats (bnin), _bn_act / _bn_grads, _dw_grads (bnin),
                                        _bn_grads, _conv_grads
    _ShuffleUnitFunction                shuffle_unit_block:  _conv_stats on slot 1 of x (``in_offset``), _bn_act, _dw_forward, _conv_stats,
                                        _bn_act, channel_shuffle2_fwd / channel_shuffle2_bwd, _bn_grads, _conv_grads, _bn_grads, _dw_grads,
                                        _bn_grads, _conv_grads into slot 1 of the dx buffer (``dx_into``)
The argument checks - every ValueError, then the RuntimeError, then the first allocation - and the dispatch:
    _check_conv, _check_bn, _check_dw, _check_map, _check_pool, _check_stride, _train_only, _need_device
    _conv_op, _bn_op, _fixed_bn_op, _res_op     the bodies the conv-bearing ops share;  _pool_op: the pool ops' tail
    _apply          Function.apply where a gradient can be asked for, the plain forward on detached inputs otherwise
tests/test_ops_trace_gpu.py pins every op's launch list (tests/golden/ops_trace.json).
"""
from __future__ import annotations

import torch

from . import kernels as K
from ._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU, DT_BF16, DT_F32

__all__ = ["conv_block", "conv_bn_block", "down_block", "down_bn_block", "res_bn_block", "spp_concat", "upsample_concat", "max_pool",
           "pool_bn_block", "stem_block", "fire_block", "max_pool_ceil", "conv_bn_relu6_block", "dw_bn_block", "project_bn_block",
           "expand_dw_bn_block", "conv_bn_relu_block", "max_pool_321", "channel_shuffle2", "shuffle_unit_block"]

_ACTS = {"leaky": ACT_LEAKY01, "none": ACT_NONE}
_ACTS_RELU = {**_ACTS, "relu": ACT_RELU}          # the ops without a batch norm at stride 1, and the unpadded first layer
_RELU6 = (0.0, 6.0)                               # an activation given as (lo, hi) is a clamp: bn_clamp_fwd / bn_clamp_bwd
_RELU = (0.0, float("inf"))                       # ReLU after a batch norm: the clamp without an upper bound
_ACTS_DW = {"relu6": _RELU6, "none": ACT_NONE}    # dw_bn_block

# The window max-pools, by the form that names their output map in kernels.POOL_OUT: (forward launch, backward launch, the arguments
# after the tensors).  The bindings are looked up when they are called, so a test can wrap them.
_MAXPOOL = (lambda *a: K.maxpool_train_fwd(*a), lambda *a: K.maxpool_bwd(*a))
_POOLS = {"2/2": _MAXPOOL + ((2,),),
          "2/1": _MAXPOOL + ((1,),),
          "3/2 ceil": (lambda *a: K.maxpool3s2_train_fwd(*a), lambda *a: K.maxpool3s2_bwd(*a), ()),
          "3/2/1": (lambda *a: K.maxpool3s2p1_train_fwd(*a), lambda *a: K.maxpool3s2p1_bwd(*a), ())}


# ---- the launches and their owners -------------------------------------------------------------------------------------------------------
def _desc(x, weight, act_id, out_f32, stride=1, pad=None, view=None, in_offset=None):
    """``in_offset``: the conv reads the channel view [in_offset, in_offset + weight's cin) of the wider x (None: x is the operand)."""
    n, ct_in, h, w = x.shape
    cout, _, k, _ = weight.shape
    c, in_off = (ct_in, 0) if in_offset is None else (weight.shape[1], in_offset)
    ct, off = view if view is not None else (K.roundup(cout, 4) if out_f32 else cout, 0)
    return K.conv_desc(n=n, h=h, w=w, cin=c, in_c_total=ct_in, in_c_offset=in_off, cout=cout, out_c_total=ct, out_c_offset=off, ksize=k, stride=stride,
                       act=act_id, kpad=K.roundup(k * k * c, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_F32 if out_f32 else DT_BF16,
                       pad=pad)


def _forward(x, weight, bias, act_id, out_f32, stride=1, pad=None, into=None, in_offset=None):
    """The forward launch on a device-packed weight.  x: bf16, NCHW-shaped, dense channels-last.  Returns the NCHW-shaped
    channels-last result (a view of the [n, ho, wo, out_c_total] buffer the kernel wrote) and the descriptor.  ``pad``: None is k // 2.
    ``into`` = (buffer [n, ho, wo, c_total], channel offset): the conv writes that channel view of a buffer the caller owns.
    ``in_offset``: the conv reads the channel view of x that starts there, cin = the weight's (addresses only: no copy of the view)."""
    d = _desc(x, weight, act_id, out_f32, stride, pad, None if into is None else (into[0].shape[3], into[1]), in_offset)
    with torch.cuda.device(x.device):
        packed, _, cout_pad = K.pack_conv_weight_dev(weight, d.cin)
        b = torch.zeros((cout_pad,), dtype=torch.float32, device=x.device)
        if bias is not None:
            b[:d.cout] = bias
        y = into[0] if into is not None else \
            torch.empty((d.n, d.ho, d.wo, d.out_c_total), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
        K.conv2d(x, packed, b, y, d)
    return y[..., d.out_c_offset:d.out_c_offset + d.cout].permute(0, 3, 1, 2), d


def _conv_grads(x, weight, g, d, need_x, need_w, need_b, dx_into=None):
    """The gradients of the conv ``d`` on the dense bf16 g [n, ho, wo, roundup(cout, 8)], each only where asked: (dx, dw, db).  Stride 1
    runs csrc/conv_bwd.hip, stride 2 csrc/conv_down_bwd.hip: the downsample's entries at pad 1, the unpadded first layer's (a weight
    gradient only) at pad 0.  Every buffer is allocated per call and fully written by its kernel.  Where ``d`` reads an input view (stride
    1), x is the wider buffer and ``dx_into`` the [n, h, w, in_c_total] buffer whose same view the data gradient writes: dx is that buffer."""
    down = d.stride == 2
    stem = down and d.pad == 0
    if stem and need_x:
        raise NotImplementedError("the unpadded stride-2 conv is a first layer: it has no data gradient")
    dx = dw = db = None
    if need_w or need_b:
        dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
        db = torch.empty((d.cout,), dtype=torch.float32, device=x.device) if need_b else None
        ws_bytes = K.conv2d_stem_bwd_workspace_bytes(d) if stem else K.conv2d_down_bwd_workspace_bytes(d) if down else \
            K.conv2d_bwd_workspace_bytes(d)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
        if stem:
            K.conv2d_stem_bwd_weight(x, g, dw, db, ws, d)
        elif down:
            K.conv2d_down_bwd_weight(x, g, dw, db, ws, d)
        else:
            K.conv2d_bwd_weight(x, g, dw, db, ws, d)
        if not need_w:
            dw = None
    if need_x:
        buf = dx_into if dx_into is not None else torch.empty((d.n, d.h, d.w, d.cin), dtype=torch.bfloat16, device=x.device)
        if down:
            K.conv2d_down_bwd_data(g, K.pack_conv_weight_down_dev(weight), buf, d)
        else:
            K.conv2d_bwd_data(g, K.pack_conv_weight_dev(weight, g.shape[3], transposed=True)[0], buf, d)
        dx = buf.permute(0, 3, 1, 2)
    return dx, dw, db


def _stats(z, gamma, beta, running, momentum, eps):
    """The batch statistics over the dense NHWC map z; the running tensors that are given are updated in place.  Returns the saved
    [4, c] vectors (mean, invstd, scale, shift)."""
    c = z.shape[3]
    with torch.cuda.device(z.device):
        saved = torch.empty((4, c), dtype=torch.float32, device=z.device)
        ws = torch.empty((K.bn_workspace_bytes(z.numel() // c, c),), dtype=torch.uint8, device=z.device)
        K.bn_train_stats(z, gamma, beta, eps, momentum, running[0], running[1], saved, ws)
    return saved


def _conv_stats(x, weight, gamma, beta, running, momentum, eps, stride=1, in_offset=None):
    """conv (act none, zero bias) -> _stats over its output map.  Returns the dense NHWC z the conv wrote, the conv's descriptor and the
    saved vectors."""
    z, d = _forward(x, weight, None, ACT_NONE, False, stride, in_offset=in_offset)
    z = z.permute(0, 2, 3, 1)
    return z, d, _stats(z, gamma, beta, running, momentum, eps)


def _bn_grads(dy, z, saved, act_id, need_x, need_w, need_g, need_b):
    """The batch-norm + activation backward of the NCHW-shaped dy (bf16 or fp32, any layout): (g, dgamma, dbeta), g - the conv
    gradients' operand - only if x or the weight needs it, dgamma and dbeta only where asked."""
    c = z.shape[3]
    dy = dy.permute(0, 2, 3, 1).contiguous()                            # dense [n, ho, wo, cout]; no copy for a channels-last dy
    g = torch.empty_like(z) if need_x or need_w else None
    dgamma = torch.empty((c,), dtype=torch.float32, device=z.device) if need_g else None
    dbeta = torch.empty((c,), dtype=torch.float32, device=z.device) if need_b else None
    ws = torch.empty((K.bn_workspace_bytes(z.numel() // c, c),), dtype=torch.uint8, device=z.device)
    if isinstance(act_id, tuple):
        K.bn_clamp_bwd(dy, z, saved, act_id[0], act_id[1], True, g, dgamma, dbeta, ws)
    else:
        K.bn_act_bwd(dy, z, saved, act_id, True, g, dgamma, dbeta, ws)
    return g, dgamma, dbeta


def _bn_act(z, saved, act_id):
    """y = bf16(act(f32(z) scale + shift)) in a new dense map; ``act_id``: an ACT_* value or a (lo, hi) clamp."""
    y = torch.empty_like(z)
    if isinstance(act_id, tuple):
        K.bn_clamp_fwd(z, saved, y, act_id[0], act_id[1])
    else:
        K.bn_act_fwd(z, saved, y, act_id)
    return y


def _bn_forward(x, weight, gamma, beta, running, momentum, eps, act_id, stride=1, pool_stride=0):
    """_conv_stats -> normalise and activate, and pool where ``pool_stride`` is not 0: the fused pass at pool stride 2, the two separate
    launches at pool stride 1.  Returns the NCHW-shaped result, the conv's descriptor, z, saved and the pool's idx (None without a pool)."""
    z, d, saved = _conv_stats(x, weight, gamma, beta, running, momentum, eps, stride)
    n, h, w, c = z.shape
    idx = None
    with torch.cuda.device(x.device):
        if pool_stride == 2:
            y = torch.empty((n,) + K.POOL_OUT["2/2"](h, w) + (c,), dtype=torch.bfloat16, device=x.device)
            idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
            K.bn_act_pool_fwd(z, saved, y, idx, act_id)
            y = y.permute(0, 3, 1, 2)
        else:
            y = _bn_act(z, saved, act_id).permute(0, 3, 1, 2)
            if pool_stride == 1:
                y, idx = _PoolFunction.plain(y, "2/1")
    return y, d, z, saved, idx


# ---- the Functions of a conv, a conv + batch norm, a conv + batch norm + residual, and a pool ------------------------------------------------
class _ConvFunction(torch.autograd.Function):
    """_forward with a backward: prepare (g = dy act'(y)), then _conv_grads.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, weight, bias, act_id, out_f32, stride, pad):
        out, d = _forward(x, weight, None if bias is None else bias.detach(), act_id, out_f32, stride, pad)
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
        od = d          # prepare reads y through the forward's output view; at stride 2 that is the stride-1 descriptor of the output map
        if d.stride == 2:
            od = K.conv_desc(n=d.n, h=d.ho, w=d.wo, cin=d.cout, in_c_total=d.cout, in_c_offset=0, cout=d.cout, out_c_total=d.cout,
                             out_c_offset=0, ksize=1, stride=1, act=d.act, kpad=K.roundup(d.cout, 64), cout_pad=d.cout_pad)
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()                    # dense [n, ho, wo, cout]; no copy for a channels-last dy
            g = torch.empty((d.n, d.ho, d.wo, K.roundup(d.cout, 8)), dtype=torch.bfloat16, device=x.device)
            K.conv2d_bwd_prepare(dy, y, g, od)
            dx, dw, db = _conv_grads(x, weight, g, d, need_x, need_w, need_b and ctx.has_bias)
        return dx, dw, db, None, None, None, None


class _PoolFunction(torch.autograd.Function):
    """A window max-pool of _POOLS on the dense bf16 NCHW-shaped x; the backward keeps the windows' tap numbers (uint8), not x."""

    @staticmethod
    def plain(x, form):
        """The forward launch: the NCHW-shaped result and idx (dense NHWC)."""
        launch, _, rest = _POOLS[form]
        xn = x.permute(0, 2, 3, 1)
        n, h, w, c = xn.shape
        with torch.cuda.device(x.device):
            y = torch.empty((n,) + K.POOL_OUT[form](h, w) + (c,), dtype=torch.bfloat16, device=x.device)
            idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
            launch(xn, y, idx, *rest)
        return y.permute(0, 3, 1, 2), idx

    @staticmethod
    def grad(dy, idx, shape, form):
        """The backward launch: dy (NCHW-shaped, any layout / dtype) -> the NCHW-shaped bf16 gradient of the pool's input [n, h, w, c]."""
        _, launch, rest = _POOLS[form]
        with torch.cuda.device(idx.device):
            dx = torch.empty(shape, dtype=torch.bfloat16, device=idx.device)
            launch(_dense_bf16(dy).permute(0, 2, 3, 1), idx, dx, *rest)
        return dx.permute(0, 3, 1, 2)

    @staticmethod
    def forward(ctx, x, form):
        y, idx = _PoolFunction.plain(x, form)
        ctx.shape, ctx.form = tuple(x.permute(0, 2, 3, 1).shape), form
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return _PoolFunction.grad(dy, ctx.saved_tensors[0], ctx.shape, ctx.form), None


class _ConvBnFunction(torch.autograd.Function):
    """_bn_forward (training=True) with a backward: through the pool where there is one (yolo_maxpool_bwd expands dy to the unpooled map),
    then _bn_grads and _conv_grads on its g.  x, weight, z, saved and idx are kept, y is not.  ``running`` is a tuple, so autograd does
    not track the in-place update."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running, momentum, eps, act_id, stride, pool_stride):
        out, d, z, saved, idx = _bn_forward(x, weight, gamma.detach(), beta.detach(), running, momentum, eps, act_id, stride, pool_stride)
        ctx.desc, ctx.act_id, ctx.pool_stride = d, act_id, pool_stride
        ctx.save_for_backward(x, weight, z, saved, idx)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, z, saved, idx = ctx.saved_tensors
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        with torch.cuda.device(x.device):
            if ctx.pool_stride:
                dy = _PoolFunction.grad(dy, idx, tuple(z.shape), f"2/{ctx.pool_stride}")
            g, dgamma, dbeta = _bn_grads(dy, z, saved, ctx.act_id, need_x, need_w, need_g, need_b)
            dx, dw, _ = _conv_grads(x, weight, g, ctx.desc, need_x, need_w, False)
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None


def _res_forward(x, weight, gamma, beta, residual, running, momentum, eps, act_id, want_preadd):
    """_conv_stats -> normalise, activate and add the residual in one pass: yolo_bn_act_add_fwd (leaky; ``want_preadd``: the value before
    the add is written too), or without an activation yolo_bn_add_rounded_fwd (the normalised value is rounded to bf16 before the add, as
    conv_bn_block(act="none") followed by a bf16 add would).  Returns the NCHW-shaped result - (y, y_preadd) with ``want_preadd`` - and
    what the backward keeps."""
    z, d, saved = _conv_stats(x, weight, gamma, beta, running, momentum, eps)
    with torch.cuda.device(x.device):
        y = torch.empty_like(z)
        pre = torch.empty_like(z) if want_preadd else None
        if act_id == ACT_NONE:
            K.bn_add_rounded_fwd(z, saved, residual.permute(0, 2, 3, 1), y)
        else:
            K.bn_act_add_fwd(z, saved, residual.permute(0, 2, 3, 1), y, pre, act_id)
    y = y.permute(0, 3, 1, 2)
    return ((y, pre.permute(0, 3, 1, 2)) if want_preadd else y), d, z, saved


class _ResBnFunction(torch.autograd.Function):
    """_res_forward with a backward: _ConvBnFunction's on dy (+ the gradient of y_preadd where it was routed, summed in fp32 by torch); dy
    itself is the residual's."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, running, momentum, eps, act_id, want_preadd):
        out, ctx.desc, z, saved = _res_forward(x, weight, gamma.detach(), beta.detach(), residual.detach(), running, momentum, eps, act_id,
                                               want_preadd)
        ctx.act_id = act_id
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, weight, z, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dpre=None):
        x, weight, z, saved = ctx.saved_tensors
        need_x, need_w, need_g, need_b, need_r = ctx.needs_input_grad[:5]
        dx = dw = dgamma = dbeta = None
        if dy is None and dpre is None:
            return (None,) * 10
        dres = dy if need_r else None
        if dy is not None and dpre is not None:
            dy = dy.float() + dpre.float()                              # one fp32 sum: yolo_bn_act_bwd takes an fp32 dy
        elif dy is None:
            dy = dpre
        if need_x or need_w or need_g or need_b:
            with torch.cuda.device(x.device):
                g, dgamma, dbeta = _bn_grads(dy, z, saved, ctx.act_id, need_x, need_w, need_g, need_b)
                dx, dw, _ = _conv_grads(x, weight, g, ctx.desc, need_x, need_w, False)
        return dx, dw, dgamma, dbeta, dres, None, None, None, None, None


# ---- the argument checks and the dispatch the ops share -----------------------------------------------------------------------------------
def _check_conv(name, x, weight, bias, act, ksizes, cout8, acts=_ACTS):
    """The ValueErrors of a conv-bearing op's x, weight, bias and act; ``ksizes``: the kernel sizes it takes; ``cout8``: cout % 8 == 0
    is required (every bfloat16 output); ``acts``: the activations it takes (_ACTS, or _ACTS_RELU where the backward has the ReLU slope)."""
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{name}: x must be [n, cin, h, w] and weight [cout, cin, k, k]")
    if act not in acts:
        names = [repr(a) for a in acts]
        raise ValueError(f"{name}: act must be {', '.join(names[:-1])} or {names[-1]}, not {act!r}")
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in ksizes:
        raise ValueError(f"{name}: kernel {k}x{k2} unsupported ({' or '.join(f'{s}x{s}' for s in ksizes)})")
    if x.shape[1] != cin:
        raise ValueError(f"{name}: x has {x.shape[1]} channels, weight expects {cin}")
    if min(x.shape) < 1 or cout < 1:
        raise ValueError(f"{name}: empty tensor")
    if cout8 and cout % 8:
        raise ValueError(f"{name}: a bfloat16 output needs cout % 8 == 0 (cout {cout})")
    if weight.dtype != torch.float32:
        raise ValueError(f"{name}: weight must be float32 [cout, cin, k, k]")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (cout,)):
        raise ValueError(f"{name}: bias must be float32 [cout]")


def _check_bn(name, x, weight, stride, gamma, beta, running_mean, running_var, training, momentum, eps):
    """The ValueErrors of a batch-norm op's own arguments, after _check_conv: momentum and eps, the float32 [cout] vectors (training=False
    needs both running tensors), more than one value per channel of the conv's output map, contiguous running tensors where they are
    updated.  Returns the detached (running_mean, running_var)."""
    if momentum is None or isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum <= 1.0:
        raise ValueError(f"{name}: momentum must be a number in [0, 1], not {momentum!r} (the cumulative average is unsupported)")
    if not isinstance(eps, (int, float)) or not eps >= 0.0:
        raise ValueError(f"{name}: eps must be a non-negative number, not {eps!r}")
    for what, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None and what.startswith("running"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (weight.shape[0],):
            raise ValueError(f"{name}: {what} must be float32 [cout]")
    running = (None if running_mean is None else running_mean.detach(), None if running_var is None else running_var.detach())
    if not training:
        if running_mean is None or running_var is None:
            raise ValueError(f"{name}: training=False needs running_mean and running_var")
        return running
    if x.shape[0] * ((x.shape[2] - 1) // stride + 1) * ((x.shape[3] - 1) // stride + 1) < 2:
        raise ValueError(f"{name}: expected more than 1 value per channel when training")
    if any(t is not None and not t.is_contiguous() for t in running):
        raise ValueError(f"{name}: the running tensors must be contiguous (they are updated in place)")
    return running


def _check_dw(name, w_dw, c, what, arg="w_dw", c8=False):
    """The ValueErrors of the 3x3 depthwise weight ``arg`` over ``c`` channels, which the op's docstring calls ``what``; ``c8``: the
    op's own ``c % 8 == 0`` check comes between the shape and the dtype (dw_bn_block, whose c is x's)."""
    if not isinstance(w_dw, torch.Tensor) or tuple(w_dw.shape) != (c, 1, 3, 3):
        raise ValueError(f"{name}: {arg} must be [{what}, 1, 3, 3] with {what} = {c} (a 3x3 depthwise conv), not "
                         f"{list(getattr(w_dw, 'shape', ()))}")
    if c8 and c % 8:
        raise ValueError(f"{name}: {what} % 8 == 0 is required ({what} {c})")
    if w_dw.dtype != torch.float32:
        raise ValueError(f"{name}: {arg} must be float32 [{what}, 1, 3, 3]")


def _check_stride(name, stride):
    if isinstance(stride, bool) or stride not in (1, 2):
        raise ValueError(f"{name}: stride {stride!r} unsupported (1 or 2)")


def _train_only(name, training):
    if not training:
        raise ValueError(f"{name}: training=True only (the frozen layer is the models' inference path)")


def _need_device(name, *tensors):
    if not all(t is None or t.is_cuda for t in tensors):
        raise RuntimeError(f"pytorch_yolo_amd.{name} runs on a ROCm device only (no CPU fallback)")


def _dense_bf16(t):
    """t as bfloat16, dense channels-last, by torch operations (torch differentiates them)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    if not t.permute(0, 2, 3, 1).is_contiguous():
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def _to_kernel_layout(x, weight):
    """The conversions of an op's x and weight, outside the Function so that torch differentiates them: cin zero-padded to a multiple of
    8, x bfloat16 and dense channels-last, weight contiguous."""
    cin = weight.shape[1]
    if cin % 8:
        padc = 8 - cin % 8
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, padc))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, padc))
    return _dense_bf16(x), weight.contiguous()


def _apply(function, plain, tensors, *rest):
    """``function.apply`` if grad is enabled and one of ``tensors`` requires grad; otherwise ``plain``, the forward the Function wraps, on
    the detached tensors: the result has no ``grad_fn``."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        return function.apply(*tensors, *rest)
    return plain(*(None if t is None else t.detach() for t in tensors), *rest)[0]


def _conv_op(name, ksizes, stride, x, weight, bias, act, out_dtype=torch.bfloat16, acts=_ACTS):
    """The body of conv_block and down_block, and of the batch-norm ops with ``training=False``."""
    _check_conv(name, x, weight, bias, act, ksizes, out_dtype == torch.bfloat16, acts)
    _need_device(name, x, weight, bias)
    x, weight = _to_kernel_layout(x, weight)
    return _apply(_ConvFunction, _forward, (x, weight, bias), acts[act], out_dtype == torch.float32, stride, None)


def _bn_op(name, ksizes, stride, pool_stride, x, weight, gamma, beta, running_mean, running_var, training, momentum, eps, act):
    """The body of the conv + batch-norm ops without a residual, after _check_conv.  ``act`` as given: a name of _ACTS, or the activation
    itself - an ACT_* value or a (lo, hi) clamp."""
    running = _check_bn(name, x, weight, stride, gamma, beta, running_mean, running_var, training, momentum, eps)
    _need_device(name, x, weight, gamma, beta, running_mean, running_var)
    if not training:        # frozen statistics: the folded layer, as the models run it
        s = gamma / torch.sqrt(running[1] + eps)
        return _conv_op(name, ksizes, stride, x, weight * s.reshape(-1, 1, 1, 1), beta - running[0] * s, act)
    x, weight = _to_kernel_layout(x, weight)
    return _apply(_ConvBnFunction, _bn_forward, (x, weight, gamma.contiguous(), beta.contiguous()), running, float(momentum), float(eps),
                  _ACTS.get(act, act), int(stride), pool_stride)


def _fixed_bn_op(name, act_id, ksizes, x, weight, gamma, beta, running_mean, running_var, stride, training, momentum, eps):
    """The conv + batch-norm ops whose activation is part of the layer (``act_id``: an ACT_* value or a clamp): ``ksizes`` at stride 1, 3x3
    at stride 2, training=True only."""
    _check_stride(name, stride)
    _check_conv(name, x, weight, None, "none", ksizes if stride == 1 else (3,), True)
    _train_only(name, training)
    return _bn_op(name, ksizes, stride, 0, x, weight, gamma, beta, running_mean, running_var, True, momentum, eps, act_id)


def _res_op(name, act_id, x, weight, gamma, beta, running_mean, running_var, residual, want_preadd, momentum, eps):
    """The body of the conv + batch-norm ops with a residual, after _check_conv and _train_only."""
    if not isinstance(residual, torch.Tensor) or tuple(residual.shape) != (x.shape[0], weight.shape[0], x.shape[2], x.shape[3]):
        raise ValueError(f"{name}: residual must be [n, cout, h, w]")
    running = _check_bn(name, x, weight, 1, gamma, beta, running_mean, running_var, True, momentum, eps)
    _need_device(name, x, weight, residual, gamma, beta, running_mean, running_var)
    x, weight = _to_kernel_layout(x, weight)
    return _apply(_ResBnFunction, _res_forward, (x, weight, gamma.contiguous(), beta.contiguous(), _dense_bf16(residual)), running,
                  float(momentum), float(eps), act_id, bool(want_preadd))


# ---- ConvBlock at stride 1 and the downsample, BN folded or on batch statistics --------------------------------------------------------------
def conv_block(x, weight, bias=None, *, act="leaky", out_dtype=torch.bfloat16, stride=1):
    """``act(conv2d(x, bf16(weight), padding=k // 2) + bias)`` at stride 1 on the device, differentiable once: ConvBlock.forward of the
    reference (models/yolo_base.py:19-44, BN folded); with ``act="none"`` and ``out_dtype=torch.float32`` the plain nn.Conv2d heads.

    x       [n, cin, h, w].  The zero-copy form is bfloat16, dense channels-last (the package's NHWC layout) with ``cin % 8 == 0``;
            any other dtype / layout / channel count is converted (and zero-padded to 8 channels) by torch operations, so torch
            differentiates the conversion and such an x gets a gradient of its own dtype and layout.
    weight  float32 [cout, cin, k, k] on the device, k = 1 or 3 (typically an nn.Parameter; rounded to bf16 for the product).
    bias    float32 [cout] or None.
    act     "leaky" (LeakyReLU(0.1)), "none" or "relu" (SqueezeNet's convs; the gradient at y == 0 is 0, torch's rule).
    out_dtype  torch.bfloat16 (``cout % 8 == 0``) or torch.float32 (the head form: any cout).
    Returns an NCHW-shaped channels-last tensor.  Under ``torch.no_grad()``, or when no input requires grad, only the forward runs and
    the result has no ``grad_fn``.  Gradients: x bf16 (rounded once), weight and bias float32, each computed only where asked; two runs
    give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    if stride != 1:
        raise ValueError(f"conv_block: stride {stride} unsupported (the backward covers stride 1)")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"conv_block: out_dtype must be torch.bfloat16 or torch.float32, not {out_dtype}")
    return _conv_op("conv_block", (1, 3), 1, x, weight, bias, act, out_dtype, _ACTS_RELU)


def down_block(x, weight, bias=None, *, act="leaky"):
    """``act(conv2d(x, bf16(weight), stride=2, padding=1) + bias)`` on the device, differentiable once: conv_block's contract for the
    3x3 stride-2 downsample of Darknet-53 (ConvBlock(3x3, stride 2) with its BN folded).  The output map is
    ``((h - 1) // 2 + 1, (w - 1) // 2 + 1)``, torch's for even and odd maps.

    x       [n, cin, h, w]; zero-copy for bfloat16 dense channels-last with ``cin % 8 == 0``, otherwise converted by torch as in conv_block.
    weight  float32 [cout, cin, 3, 3] on the device, ``cout % 8 == 0``.      bias  float32 [cout] or None.
    act     "leaky" (LeakyReLU(0.1)) or "none".
    Returns an NCHW-shaped channels-last bfloat16 tensor.  Grad modes, gradients and errors are conv_block's."""
    return _conv_op("down_block", (3,), 2, x, weight, bias, act)


def conv_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky",
                  stride=1):
    """``act(batch_norm(conv2d(x, bf16(weight), padding=k // 2)))`` at stride 1 on the device, differentiable once: the reference's
    ConvBlock (Conv2d(bias=False) -> BatchNorm2d -> LeakyReLU(0.1)) as it trains.

    x, weight   as in conv_block (the same conversions by torch outside the Function); ``cout % 8 == 0``.
    gamma, beta float32 [cout] on the device: BatchNorm2d's weight and bias.
    running_mean, running_var   float32 [cout] on the device or None.  ``training=True``: the batch's statistics normalise, and the
                running tensors that are given (contiguous) are updated in place (momentum; running_var takes the unbiased variance, as
                torch).  ``training=False``: both are required, they normalise, and nothing is updated: the call is
                ``conv_block(x, weight * s, beta - running_mean * s, act=act)`` with ``s = gamma / sqrt(running_var + eps)`` folded by
                torch in float32 (one launch, one rounding of the result; autograd differentiates the fold).
                ``num_batches_tracked`` is the caller's, as with torch.nn.functional.batch_norm.
    momentum    a number in [0, 1]; None (torch's cumulative average) raises ValueError.
    act         "leaky" (LeakyReLU(0.1)) or "none".
    Returns an NCHW-shaped channels-last bfloat16 tensor.  Under ``torch.no_grad()``, or when no input requires grad, only the forward
    runs.  Gradients: x bf16, weight, gamma and beta float32, each computed only where asked; two runs give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    if stride != 1:
        raise ValueError(f"conv_bn_block: stride {stride} unsupported (the backward covers stride 1)")
    _check_conv("conv_bn_block", x, weight, None, act, (1, 3), True)
    return _bn_op("conv_bn_block", (1, 3), 1, 0, x, weight, gamma, beta, running_mean, running_var, bool(training), momentum, eps, act)


def down_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky"):
    """``act(batch_norm(conv2d(x, bf16(weight), stride=2, padding=1)))`` on the device, differentiable once: conv_bn_block's contract
    for the 3x3 stride-2 downsample (Conv2d(3x3, stride 2, bias=False) -> BatchNorm2d -> LeakyReLU(0.1)) as the reference trains it.

    Arguments, running statistics, ``training=False`` (down_block on the weights folded by torch) and errors are conv_bn_block's; the
    statistics run over the ``n ho wo`` output pixels."""
    _check_conv("down_bn_block", x, weight, None, act, (3,), True)
    return _bn_op("down_bn_block", (3,), 2, 0, x, weight, gamma, beta, running_mean, running_var, bool(training), momentum, eps, act)


# ---- the residual unit's closing ConvBlock with the add fused in -------------------------------------------------------------------------
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
    _check_conv("res_bn_block", x, weight, None, "leaky", (1, 3), True)
    _train_only("res_bn_block", training)
    return _res_op("res_bn_block", ACT_LEAKY01, x, weight, gamma, beta, running_mean, running_var, residual, want_preadd, momentum, eps)


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
    _need_device("spp_concat", x)
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
    _need_device("upsample_concat", a, b)
    return _UpsampleConcatFunction.apply(_dense_bf16(a), _dense_bf16(b), bool(up_first))


# ---- the max-pools of YOLOv3-tiny / LiteYOLOv3: MaxPool and ConvPoolBlock as they train -----------------------------------
def _check_pool(name, stride, h, w):
    if isinstance(stride, bool) or stride not in (1, 2):
        raise ValueError(f"{name}: pool stride must be 2 (MaxPool2d(2, 2)) or 1 (MaxPool2d(2, 1, padding=1, dilation=2)), not {stride!r}")
    if h < 2 or w < 2:
        raise ValueError(f"{name}: the pool needs a map of at least 2 x 2, got {h} x {w} (stride 2: empty output; stride 1: a window "
                         "would be all padding)")


def _pool_op(name, form, x):
    """The tail of the pool ops, after their ValueErrors."""
    _need_device(name, x)
    return _apply(_PoolFunction, _PoolFunction.plain, (_dense_bf16(x),), form)


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
    return _pool_op("max_pool", f"2/{int(stride)}", x)


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
    _check_conv("pool_bn_block", x, weight, None, act, (1, 3), True)
    _train_only("pool_bn_block", training)
    _check_pool("pool_bn_block", pool_stride, x.shape[2], x.shape[3])
    return _bn_op("pool_bn_block", (1, 3), 1, int(pool_stride), x, weight, gamma, beta, running_mean, running_var, True, momentum, eps, act)


# ---- SqueezeNet 1.1 as it trains: the unpadded first layer, the ceil-mode pool and the Fire module ------------------------
def stem_block(x, weight, bias=None, *, act="relu"):
    """``act(conv2d(x, bf16(weight), stride=2, padding=0) + bias)`` on the device, differentiable once in weight and bias: features[0] of
    SqueezeNet 1.1 (Conv2d(3, 64, 3, stride=2) + ReLU).  The output map is ``((h - 3) // 2 + 1, (w - 3) // 2 + 1)``: an even map's last row
    and column are never read.  The forward is the launch the eval model runs for that layer.

    x       [n, cin, h, w], h and w >= 3; converted as in conv_block (3 channels are zero-padded to 8).  The op is a first layer: an x
            that requires grad raises NotImplementedError (there is no data gradient of the unpadded stride-2 conv).
    weight  float32 [cout, cin, 3, 3] on the device, ``cout % 8 == 0``.      bias  float32 [cout] or None.
    act     "relu", "leaky" (LeakyReLU(0.1)) or "none".
    Returns an NCHW-shaped channels-last bfloat16 tensor.  Gradients: weight and bias float32, each computed only where asked; two runs
    give the same bits.  Grad modes and errors are conv_block's."""
    _check_conv("stem_block", x, weight, bias, act, (3,), True, _ACTS_RELU)
    if x.shape[2] < 3 or x.shape[3] < 3:
        raise ValueError(f"stem_block: a {x.shape[2]} x {x.shape[3]} map has no unpadded 3x3 window")
    if x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("stem_block is a first layer: its input is the image and gets no gradient (x.requires_grad is set)")
    _need_device("stem_block", x, weight, bias)
    x, weight = _to_kernel_layout(x.detach(), weight)
    return _apply(_ConvFunction, _forward, (x, weight, bias), _ACTS_RELU[act], False, 2, 0)


def max_pool_ceil(x):
    """``max_pool2d(x, 3, 2, ceil_mode=True)`` on the device, differentiable once: the pool of SqueezeNet 1.1.  The output map is
    ``(ceil((h - 3) / 2) + 1, ceil((w - 3) / 2) + 1)`` = ``(h // 2, w // 2)``; on an even map the last window is partial (its taps beyond
    the map count as -inf).  x [n, c, h, w], ``c % 8 == 0``, h and w >= 2; bfloat16 dense channels-last is taken as it is, anything else
    is converted by torch.  Returns bfloat16, channels-last.  The gradient of a window goes to its first maximum in row-major order
    (torch's rule); the up to four terms of a pixel are summed in fp32 in row-major window order and rounded once.  x must hold no NaN.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    _check_map("max_pool_ceil", "x", x)
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(f"max_pool_ceil: the pool needs a map of at least 2 x 2, got {x.shape[2]} x {x.shape[3]}")
    return _pool_op("max_pool_ceil", "3/2 ceil", x)


def _fire_forward(x, sw, sb, w1, b1, w3, b3):
    """The three launches of a Fire module: the squeeze, then the two expands into the channel views of one [n, h, w, e1 + e3] buffer.
    Returns the NCHW-shaped result and what the backward keeps: the squeeze output and the three descriptors."""
    s, ds = _forward(x, sw, sb, ACT_RELU, False)
    e1, e3 = w1.shape[0], w3.shape[0]
    with torch.cuda.device(x.device):
        y = torch.empty((ds.n, ds.h, ds.w, e1 + e3), dtype=torch.bfloat16, device=x.device)
    _, d1 = _forward(s, w1, b1, ACT_RELU, False, into=(y, 0))
    _, d3 = _forward(s, w3, b3, ACT_RELU, False, into=(y, e1))
    return y.permute(0, 3, 1, 2), s, (ds, d1, d3)


class _FireFunction(torch.autograd.Function):
    """_fire_forward with a backward: fire_bwd_split (the concat's gradient through the expands' ReLU, as two dense operands), _conv_grads
    of the two expands, fire_bwd_join (their data gradients summed, through the squeeze's ReLU), _conv_grads of the squeeze.  x, the
    weights, the squeeze output and the result are kept."""

    @staticmethod
    def forward(ctx, x, sw, sb, w1, b1, w3, b3):
        out, s, ctx.descs = _fire_forward(x, sw, sb.detach(), w1, b1.detach(), w3, b3.detach())
        ctx.save_for_backward(x, sw, w1, w3, s, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, sw, w1, w3, s, out = ctx.saved_tensors
        ds, d1, d3 = ctx.descs
        need_x, need_sw, need_sb, need_w1, need_b1, need_w3, need_b3 = ctx.needs_input_grad
        need_s = need_x or need_sw or need_sb
        dx = dsw = dsb = dw1 = db1 = dw3 = db3 = None
        with torch.cuda.device(x.device):
            dy = dy.permute(0, 2, 3, 1).contiguous()                    # dense [n, h, w, e1 + e3]; no copy for a channels-last dy
            g1 = torch.empty((ds.n, ds.h, ds.w, d1.cout), dtype=torch.bfloat16, device=x.device)
            g3 = torch.empty((ds.n, ds.h, ds.w, d3.cout), dtype=torch.bfloat16, device=x.device)
            K.fire_bwd_split(dy, out.permute(0, 2, 3, 1), g1, g3)
            ds1, dw1, db1 = _conv_grads(s, w1, g1, d1, need_s, need_w1, need_b1)
            ds3, dw3, db3 = _conv_grads(s, w3, g3, d3, need_s, need_w3, need_b3)
            if need_s:
                gs = torch.empty((ds.n, ds.h, ds.w, ds.cout), dtype=torch.bfloat16, device=x.device)
                K.fire_bwd_join(ds1.permute(0, 2, 3, 1), ds3.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1), gs)
                dx, dsw, dsb = _conv_grads(x, sw, gs, ds, need_x, need_sw, need_sb)
        return dx, dsw, dsb, dw1, db1, dw3, db3


def fire_block(x, squeeze_w, squeeze_b, e1_w, e1_b, e3_w, e3_b):
    """SqueezeNet's Fire module on the device, differentiable once, as one op: ``s = relu(conv2d(x, squeeze_w) + squeeze_b)``, then
    ``cat([relu(conv2d(s, e1_w) + e1_b), relu(conv2d(s, e3_w, padding=1) + e3_b)], 1)`` - the two expand convs write the channel views of
    the result, so there is no concat copy.  Bit-equal, outputs and gradients, to three ``conv_block(act="relu")`` calls and ``torch.cat``.

    x           [n, cin, h, w]; converted as in conv_block.
    squeeze_w   float32 [sq, cin, 1, 1];  e1_w float32 [e1, sq, 1, 1];  e3_w float32 [e3, sq, 3, 3]; ``sq``, ``e1`` and ``e3`` multiples
                of 8 (anything else would misalign a channel view: ValueError).  The biases: float32 [sq], [e1], [e3].
    Returns bfloat16 [n, e1 + e3, h, w], channels-last.  The backward splits the incoming gradient through the expands' ReLU into the
    two convs' dense operands in one pass (yolo_fire_bwd_split), runs their weight and data gradients, adds the two data gradients through
    the squeeze's ReLU in one pass (yolo_fire_bwd_join) and runs the squeeze's gradients.  Gradients: x bf16, weights and biases float32,
    each computed only where asked (with nothing asked of x and the squeeze conv, no expand data gradient runs); two runs give the same
    bits.  Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    _check_conv("fire_block", x, squeeze_w, squeeze_b, "relu", (1,), True, _ACTS_RELU)
    for what, w, b, k in (("e1", e1_w, e1_b, 1), ("e3", e3_w, e3_b, 3)):
        if not isinstance(w, torch.Tensor) or w.dim() != 4 or tuple(w.shape[1:]) != (squeeze_w.shape[0], k, k) or w.shape[0] < 1:
            raise ValueError(f"fire_block: {what}_w must be [{what}, sq, {k}, {k}] with sq = {squeeze_w.shape[0]}")
        if w.shape[0] % 8:
            raise ValueError(f"fire_block: {what} % 8 == 0 is required (the expand convs write channel views of one map; {what} {w.shape[0]})")
        if w.dtype != torch.float32:
            raise ValueError(f"fire_block: {what}_w must be float32")
    for what, w, b in (("squeeze", squeeze_w, squeeze_b), ("e1", e1_w, e1_b), ("e3", e3_w, e3_b)):
        if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"fire_block: {what}_b must be float32 [{w.shape[0]}]")
    _need_device("fire_block", x, squeeze_w, squeeze_b, e1_w, e1_b, e3_w, e3_b)
    x, squeeze_w = _to_kernel_layout(x, squeeze_w)
    return _apply(_FireFunction, _fire_forward, (x, squeeze_w, squeeze_b, e1_w.contiguous(), e1_b, e3_w.contiguous(), e3_b))


# ---- MobileNetV2's inverted residual as it trains: ConvBNReLU dense and depthwise, the linear bottleneck ------------------
def conv_bn_relu6_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
    """``relu6(batch_norm(conv2d(x, bf16(weight), stride=stride, padding=k // 2)))`` on the device, differentiable once: torchvision's dense
    ConvBNReLU (Conv2d(bias=False) -> BatchNorm2d -> ReLU6) as it trains - 1x1 at stride 1 (an inverted residual's expand, the last
    layer), 3x3 at stride 1 or 2 (the first layer; its 3 input channels are zero-padded to 8 as in conv_block).

    conv_bn_block's contract (down_bn_block's at stride 2) with ``training=True`` (anything else raises ValueError): the same launches but
    for the two batch-norm passes, which clamp (yolo_bn_clamp_fwd / yolo_bn_clamp_bwd with lo 0, hi 6).  The gradient is 0 where the
    normalised value is <= 0 or >= 6 (torch's hardtanh rule).
    Gradients: x bf16, weight, gamma and beta float32, each computed only where asked; two runs give the same bits."""
    return _fixed_bn_op("conv_bn_relu6_block", _RELU6, (1, 3), x, weight, gamma, beta, running_mean, running_var, stride, training, momentum,
                        eps)


def _dw_pack(weight):
    """The depthwise weight [c, 1, 3, 3] rounded once to bf16 and laid out [9, c] (float32, tap-major)."""
    return weight.detach().to(torch.bfloat16).to(torch.float32).reshape(weight.shape[0], 9).t().contiguous()


def _dw_stats(operand, w9c, gamma, beta, running, momentum, eps, stride, bnin=None):
    """The depthwise conv (act none, zero bias) of the dense NHWC ``operand`` and _stats over its output map: z and saved.  ``bnin`` =
    (saved, (lo, hi)): the operand is the map before that batch norm and clamp, which the conv applies as it loads it
    (yolo_dwconv3x3_bnin_fwd; the padding is a zero of the transformed map)."""
    n, h, w, c = operand.shape
    with torch.cuda.device(operand.device):
        z = torch.empty((n, (h - 1) // stride + 1, (w - 1) // stride + 1, c), dtype=torch.bfloat16, device=operand.device)
        if bnin is None:
            K.dwconv3x3(operand, w9c, torch.zeros((c,), dtype=torch.float32, device=operand.device), z, n=n, h=h, w=w, c=c, in_view=(c, 0),
                        out_view=(c, 0), stride=stride, act=ACT_NONE)
        else:
            K.dwconv3x3_bnin_fwd(operand, bnin[0], bnin[1][0], bnin[1][1], w9c, z, stride)
    return z, _stats(z, gamma, beta, running, momentum, eps)


def _dw_grads(operand, g, w9c, stride, need_x, need_w, bnin=None):
    """The gradients of the depthwise conv of ``operand`` (dense NHWC; ``bnin`` as in _dw_stats) on the dense bf16 g, each only where
    asked: (the dense NHWC data gradient, the [c, 1, 3, 3] weight gradient).  Every buffer is allocated per call and fully written."""
    n, h, w, c = operand.shape
    dx = dw = None
    with torch.cuda.device(operand.device):
        if need_x:
            dx = torch.empty((n, h, w, c), dtype=torch.bfloat16, device=operand.device)
            K.dwconv3x3_bwd_data(g, w9c, dx, stride)
        if need_w:
            dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=operand.device)
            ws = torch.empty((K.dwconv3x3_bwd_weight_workspace_bytes(n, h, w, c, stride),), dtype=torch.uint8, device=operand.device)
            if bnin is None:
                K.dwconv3x3_bwd_weight(operand, g, dw, ws, stride)
            else:
                K.dwconv3x3_bnin_bwd_weight(operand, bnin[0], bnin[1][0], bnin[1][1], g, dw, ws, stride)
    return dx, dw


def _dw_forward(x, weight, gamma, beta, running, momentum, eps, act_id, stride):
    """_dw_pack, _dw_stats and the normalise-and-activate pass.  Returns the NCHW-shaped result and what the backward keeps: z, saved and
    the [9, c] weight."""
    w9c = _dw_pack(weight)
    z, saved = _dw_stats(x.permute(0, 2, 3, 1), w9c, gamma, beta, running, momentum, eps, stride)
    with torch.cuda.device(x.device):
        y = _bn_act(z, saved, act_id)
    return y.permute(0, 3, 1, 2), z, saved, w9c


class _DwBnFunction(torch.autograd.Function):
    """_dw_forward with a backward: _bn_grads, then _dw_grads on its g.  x, the [9, c] weight, z and saved are kept, y is not."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running, momentum, eps, act_id, stride):
        out, z, saved, w9c = _dw_forward(x, weight, gamma.detach(), beta.detach(), running, momentum, eps, act_id, stride)
        ctx.act_id, ctx.stride = act_id, stride
        ctx.save_for_backward(x, w9c, z, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w9c, z, saved = ctx.saved_tensors
        need_x, need_w, need_g, need_b = ctx.needs_input_grad[:4]
        with torch.cuda.device(x.device):
            g, dgamma, dbeta = _bn_grads(dy, z, saved, ctx.act_id, need_x, need_w, need_g, need_b)
            dx, dw = _dw_grads(x.permute(0, 2, 3, 1), g, w9c, ctx.stride, need_x, need_w)
        return (None if dx is None else dx.permute(0, 3, 1, 2)), dw, dgamma, dbeta, None, None, None, None, None


def dw_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, stride=1, act="relu6", momentum=0.1, eps=1e-5, training=True):
    """``act(batch_norm(conv2d(x, bf16(weight), stride=stride, padding=1, groups=c)))`` on the device, differentiable once: the depthwise
    ConvBNReLU of an inverted residual (Conv2d(c, c, 3, stride, 1, groups=c, bias=False) -> BatchNorm2d -> ReLU6) as it trains.

    x       [n, c, h, w], ``c % 8 == 0`` (a depthwise conv has no channel padding); bfloat16 dense channels-last is taken as it is,
            anything else is converted by torch.
    weight  float32 [c, 1, 3, 3] on the device; rounded to bf16 once for the products, in the forward and in the data gradient.
    stride  1 or 2; the output map is ``((h - 1) // stride + 1, (w - 1) // stride + 1)``.
    act     "relu6", or "none" (ShuffleNetV2's linear depthwise stage).
    gamma, beta, the running tensors, momentum and eps as in conv_bn_block; ``training=True`` only (anything else raises ValueError).
    Returns an NCHW-shaped channels-last bfloat16 tensor.  The forward conv is the launch the eval models run (yolo_dwconv3x3_fwd).
    Gradients: x bf16 (an fp32 chain in tap order, rounded once), weight float32 [c, 1, 3, 3] (float64 sums of exact products), gamma
    and beta float32, each computed only where asked; two runs give the same bits.
    Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    name = "dw_bn_block"
    if not isinstance(x, torch.Tensor) or not isinstance(weight, torch.Tensor) or x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{name}: x must be [n, c, h, w] and weight [c, 1, 3, 3]")
    if act not in _ACTS_DW:
        raise ValueError(f"{name}: act must be 'relu6' or 'none', not {act!r}")
    _check_stride(name, stride)
    if min(x.shape) < 1:
        raise ValueError(f"{name}: empty tensor")
    c = x.shape[1]
    _check_dw(name, weight, c, "c", arg="weight", c8=True)
    _train_only(name, training)
    running = _check_bn(name, x, weight, stride, gamma, beta, running_mean, running_var, True, momentum, eps)
    _need_device(name, x, weight, gamma, beta, running_mean, running_var)
    return _apply(_DwBnFunction, _dw_forward, (_dense_bf16(x), weight.contiguous(), gamma.contiguous(), beta.contiguous()), running,
                  float(momentum), float(eps), _ACTS_DW[act], int(stride))


def project_bn_block(x, weight, gamma, beta, running_mean=None, running_var=None, residual=None, *, momentum=0.1, eps=1e-5, training=True):
    """``batch_norm(conv2d(x, bf16(weight)))`` with a 1x1 weight and no activation, plus ``residual`` where one is given, on the device,
    differentiable once: the linear bottleneck that closes an inverted residual (Conv2d(hidden, cout, 1, bias=False) -> BatchNorm2d, and
    the block's ``x + conv(x)`` at stride 1 with cin == cout) as it trains.

    conv_bn_block's contract with a 1x1 weight, ``act="none"`` and ``training=True`` (anything else raises ValueError).
    residual    None, or [n, cout, h, w]: the add is fused into the normalise pass (yolo_bn_add_rounded_fwd): ``y = bf16(f32(bf16(a)) +
                f32(residual))`` with ``a`` the normalised fp32 value - bit-equal to ``conv_bn_block(act="none")`` followed by a bf16 add
                (one fp32 add, one rounding), in one launch.
                bfloat16 dense channels-last is taken as it is, anything else is converted by torch.
    Gradients: x bf16, weight, gamma and beta float32, residual the incoming gradient unchanged; each computed only where asked."""
    name = "project_bn_block"
    if residual is None:
        return _fixed_bn_op(name, ACT_NONE, (1,), x, weight, gamma, beta, running_mean, running_var, 1, training, momentum, eps)
    _check_conv(name, x, weight, None, "none", (1,), True)
    _train_only(name, training)
    return _res_op(name, ACT_NONE, x, weight, gamma, beta, running_mean, running_var, residual, False, momentum, eps)


# ---- the expand + depthwise pair of an expanding inverted residual as one op: the hidden activation is never written ------
def _expand_dw_forward(x, w_expand, gamma1, beta1, w_dw, gamma2, beta2, running1, running2, momentum1, eps1, momentum2, eps2, stride):
    """_conv_stats of the expand conv, the depthwise conv on its batch-normed and clamped output (_dw_stats with ``bnin``: the operand is
    transformed as it is loaded), and the normalise-and-clamp pass.  Returns the NCHW-shaped result and what the backward keeps: the
    expand conv's descriptor, z1, saved1, the [9, c] weight, z2 and saved2."""
    z1, d, saved1 = _conv_stats(x, w_expand, gamma1, beta1, running1, momentum1, eps1)
    w9c = _dw_pack(w_dw)
    z2, saved2 = _dw_stats(z1, w9c, gamma2, beta2, running2, momentum2, eps2, stride, bnin=(saved1, _RELU6))
    with torch.cuda.device(x.device):
        y = _bn_act(z2, saved2, _RELU6)
    return y.permute(0, 3, 1, 2), d, z1, saved1, w9c, z2, saved2


class _ExpandDwBnFunction(torch.autograd.Function):
    """_expand_dw_forward with a backward: _bn_grads on z2, _dw_grads (the weight gradient on the transformed z1:
    yolo_dwconv3x3_bnin_bwd_weight), _bn_grads (clamp) on z1, _conv_grads; each only where asked.  x, the expand weight, z1, saved1,
    the [9, c] weight, z2 and saved2 are kept; y1, the activation between the convs, is neither written nor kept."""

    @staticmethod
    def forward(ctx, x, w_expand, gamma1, beta1, w_dw, gamma2, beta2, running1, running2, momentum1, eps1, momentum2, eps2, stride):
        out, ctx.desc, z1, saved1, w9c, z2, saved2 = _expand_dw_forward(x, w_expand, gamma1.detach(), beta1.detach(), w_dw, gamma2.detach(),
                                                                        beta2.detach(), running1, running2, momentum1, eps1, momentum2,
                                                                        eps2, stride)
        ctx.stride = stride
        ctx.save_for_backward(x, w_expand, z1, saved1, w9c, z2, saved2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w_expand, z1, saved1, w9c, z2, saved2 = ctx.saved_tensors
        need_x, need_we, need_g1, need_b1, need_wd, need_g2, need_b2 = ctx.needs_input_grad[:7]
        need_y1 = need_x or need_we or need_g1 or need_b1               # what dw_bn_block's x would ask for
        dx = dwe = dgamma1 = dbeta1 = None
        with torch.cuda.device(x.device):
            g2, dgamma2, dbeta2 = _bn_grads(dy, z2, saved2, _RELU6, need_y1, need_wd, need_g2, need_b2)
            d1, dwd = _dw_grads(z1, g2, w9c, ctx.stride, need_y1, need_wd, bnin=(saved1, _RELU6))
            if need_y1:
                g1, dgamma1, dbeta1 = _bn_grads(d1.permute(0, 3, 1, 2), z1, saved1, _RELU6, need_x, need_we, need_g1, need_b1)
                dx, dwe, _ = _conv_grads(x, w_expand, g1, ctx.desc, need_x, need_we, False)
        return (dx, dwe, dgamma1, dbeta1, dwd, dgamma2, dbeta2) + (None,) * 7


def _pair(name, what, v):
    """``v`` as (the expand's, the depthwise's): a number for both, or a pair."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name}: {what} must be a number or a pair (expand's, depthwise's), not {v!r}")
        return v[0], v[1]
    return v, v


def expand_dw_bn_block(x, w_expand, gamma1, beta1, running_mean1, running_var1, w_dw, gamma2, beta2, running_mean2, running_var2, *,
                       stride=1, momentum=0.1, eps=1e-5, training=True):
    """``dw_bn_block(conv_bn_relu6_block(x, w_expand, gamma1, beta1, running_mean1, running_var1), w_dw, gamma2, beta2, running_mean2,
    running_var2, stride=stride)`` on the device as one op, differentiable once: the expand and the depthwise ConvBNReLU of an expanding
    inverted residual.  Bit-equal to that composition - the output, the seven gradients and the four running tensors.

    The hidden activation ``y1 = relu6(batch_norm(z1))`` between the two convs is never written: the depthwise conv reads the expand conv's
    output z1 and normalises and clamps it as it loads it (yolo_dwconv3x3_bnin_fwd; the padding is a zero of y1), and so does the depthwise
    weight gradient (yolo_dwconv3x3_bnin_bwd_weight).  One launch and one hidden map kept for the backward less than the composition.

    x           [n, cin, h, w]; converted as in conv_block.
    w_expand    float32 [hidden, cin, 1, 1], ``hidden % 8 == 0``.      w_dw  float32 [hidden, 1, 3, 3].
    gamma1, beta1, running_mean1, running_var1      the expand's BatchNorm2d, float32 [hidden]; the running tensors may be None.
    gamma2, beta2, running_mean2, running_var2      the depthwise's.
    stride      the depthwise conv's, 1 or 2.
    momentum, eps   a number for both batch norms, or a pair (the expand's, the depthwise's).
    ``training=True`` only (anything else raises ValueError).  Returns an NCHW-shaped channels-last bfloat16 tensor
    [n, hidden, ho, wo].  Gradients: x bf16, the weights, gammas and betas float32, each computed only where asked; two runs give the same
    bits.  Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU fallback)."""
    name = "expand_dw_bn_block"
    _check_conv(name, x, w_expand, None, "none", (1,), True)
    _check_stride(name, stride)
    _train_only(name, training)
    hidden = w_expand.shape[0]
    _check_dw(name, w_dw, hidden, "hidden")
    (momentum1, momentum2), (eps1, eps2) = _pair(name, "momentum", momentum), _pair(name, "eps", eps)
    running1 = _check_bn(name, x, w_expand, 1, gamma1, beta1, running_mean1, running_var1, True, momentum1, eps1)
    hidden_map = torch.empty((x.shape[0], hidden, x.shape[2], x.shape[3]), device="meta")        # (shape only: the depthwise conv's input)
    running2 = _check_bn(name, hidden_map, w_dw, stride, gamma2, beta2, running_mean2, running_var2, True, momentum2, eps2)
    _need_device(name, x, w_expand, gamma1, beta1, running_mean1, running_var1, w_dw, gamma2, beta2, running_mean2, running_var2)
    x, w_expand = _to_kernel_layout(x, w_expand)
    return _apply(_ExpandDwBnFunction, _expand_dw_forward,
                  (x, w_expand, gamma1.contiguous(), beta1.contiguous(), w_dw.contiguous(), gamma2.contiguous(), beta2.contiguous()),
                  running1, running2, float(momentum1), float(eps1), float(momentum2), float(eps2), int(stride))


# ---- ShuffleNetV2 as it trains: the dense ConvBNReLU, MaxPool2d(3, 2, 1), the channel shuffle and the stride-1 unit -------
def conv_bn_relu_block(x, weight, gamma, beta, running_mean=None, running_var=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
    """``relu(batch_norm(conv2d(x, bf16(weight), stride=stride, padding=k // 2)))`` on the device, differentiable once: ShuffleNetV2's dense
    Conv2d(bias=False) -> BatchNorm2d -> ReLU as it trains - 1x1 at stride 1 (the units' pointwise convs, conv5), 3x3 at stride 1 or 2
    (conv1; its 3 input channels are zero-padded to 8 as in conv_block).

    conv_bn_relu6_block's contract and launches with the clamp (0, +inf): yolo_bn_clamp_fwd / yolo_bn_clamp_bwd with lo 0 and hi +inf.
    The gradient is 0 where the normalised value is <= 0 (torch's rule for ReLU).
    Gradients: x bf16, weight, gamma and beta float32, each computed only where asked; two runs give the same bits."""
    return _fixed_bn_op("conv_bn_relu_block", _RELU, (1, 3), x, weight, gamma, beta, running_mean, running_var, stride, training, momentum, eps)


def max_pool_321(x):
    """``max_pool2d(x, 3, 2, padding=1)`` on the device, differentiable once: the pool of ShuffleNetV2.  The output map is
    ``((h - 1) // 2 + 1, (w - 1) // 2 + 1)``; the taps of a window that lie outside the map are no candidates (-inf, not 0: a map of
    negative values pools to negative values).  x [n, c, h, w], ``c % 8 == 0``, any h, w >= 1; bfloat16 dense channels-last is taken as it
    is, anything else is converted by torch.  Returns bfloat16, channels-last.  The backward keeps the windows' tap numbers (uint8), not
    x.  The gradient of a window goes to its first maximum in row-major order (torch's rule); the up to four terms of a pixel are summed
    in fp32 in row-major window order and rounded once.  x must hold no NaN.  Under ``torch.no_grad()``, or when x does not require
    grad, only the forward runs.  Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no CPU
    fallback)."""
    _check_map("max_pool_321", "x", x)
    return _pool_op("max_pool_321", "3/2/1", x)


def _shuffle2_forward(a, b, half):
    """The forward shuffle launch on two dense slot maps: the NCHW-shaped [n, 2 slot, h, w] result."""
    an, bn = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)
    n, h, w, slot = an.shape
    with torch.cuda.device(a.device):
        y = torch.empty((n, h, w, 2 * slot), dtype=torch.bfloat16, device=a.device)
        K.channel_shuffle2_fwd(an, bn, y, half, slot)
    return (y.permute(0, 3, 1, 2),)


class _ChannelShuffle2Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, half):
        ctx.half = half
        return _shuffle2_forward(a, b, half)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        need_a, need_b = ctx.needs_input_grad[:2]
        da = db = None
        if not (need_a or need_b):
            return None, None, None
        with torch.cuda.device(dy.device):
            dy = _dense_bf16(dy).permute(0, 2, 3, 1)
            n, h, w, c2 = dy.shape
            if need_a:
                da = torch.empty((n, h, w, c2 // 2), dtype=torch.bfloat16, device=dy.device)
            if need_b:
                db = torch.empty((n, h, w, c2 // 2), dtype=torch.bfloat16, device=dy.device)
            K.channel_shuffle2_bwd(dy, da, db, ctx.half, c2 // 2)
        return (None if da is None else da.permute(0, 3, 1, 2)), (None if db is None else db.permute(0, 3, 1, 2)), None


def _check_half(name, half, slot):
    if isinstance(half, bool) or not isinstance(half, int) or not 1 <= half <= slot:
        raise ValueError(f"{name}: half must be an integer in [1, slot] (slot {slot}), not {half!r}")


def channel_shuffle2(a, b, half):
    """ShuffleNetV2's ``channel_shuffle(cat(a, b), groups=2)`` on the device, differentiable once, in the two-slot layout of the eval
    trace: a and b [n, slot, h, w] hold ``half`` logical channels each in ``slot`` physical ones (``slot % 8 == 0``, zero beyond
    ``half``); the result [n, 2 slot, h, w] holds logical channel j = (a, b)[j % 2][j // 2] at physical ``(j // half) slot + j % half``,
    its pad channels zero.  bfloat16 dense channels-last maps are taken as they are, anything else is converted by torch.  The forward is
    the copy kernel the eval models run (yolo_channel_shuffle2_fwd), the backward its inverse (yolo_channel_shuffle2_bwd): a copy, the
    pad channels of both gradients written as zero; each gradient only where asked.  Wrong shapes raise ValueError before any launch; a
    CPU tensor raises RuntimeError (there is no CPU fallback)."""
    name = "channel_shuffle2"
    _check_map(name, "a", a)
    _check_map(name, "b", b)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{name}: a {tuple(a.shape)} and b {tuple(b.shape)} must have one shape [n, slot, h, w]")
    _check_half(name, half, a.shape[1])
    _need_device(name, a, b)
    return _apply(_ChannelShuffle2Function, _shuffle2_forward, (_dense_bf16(a), _dense_bf16(b)), int(half))


def _shuffle_unit_forward(x, w1, gamma1, beta1, w_dw, gamma2, beta2, w3, gamma3, beta3, half, running, momentum, eps):
    """The launches of a stride-1 unit on the two-slot map x: the first 1x1 conv reads slot 1 of x as an input view, its batch norm + ReLU,
    dw_bn_block's launches without an activation, the second 1x1 conv + batch norm + ReLU, and the shuffle with a = slot 0 of x read as a
    view.  Returns the NCHW-shaped result and what the backward keeps."""
    slot = w1.shape[0]
    z1, d1, saved1 = _conv_stats(x, w1, gamma1, beta1, running[0], momentum[0], eps[0], in_offset=slot)
    with torch.cuda.device(x.device):
        y1 = _bn_act(z1, saved1, _RELU)
    y2, z2, saved2, w9c = _dw_forward(y1.permute(0, 3, 1, 2), w_dw, gamma2, beta2, running[1], momentum[1], eps[1], ACT_NONE, 1)
    z3, d3, saved3 = _conv_stats(y2, w3, gamma3, beta3, running[2], momentum[2], eps[2])
    with torch.cuda.device(x.device):
        y3 = _bn_act(z3, saved3, _RELU)
        out = torch.empty((d1.n, d1.h, d1.w, 2 * slot), dtype=torch.bfloat16, device=x.device)
        K.channel_shuffle2_fwd(x.permute(0, 2, 3, 1), y3, out, half, slot)
    return out.permute(0, 3, 1, 2), (d1, d3), (z1, saved1, y1, w9c, z2, saved2, y2, z3, saved3)


class _ShuffleUnitFunction(torch.autograd.Function):
    """_shuffle_unit_forward with a backward: channel_shuffle2_bwd (da into slot 0 of the dx buffer, db dense), _bn_grads and _conv_grads of
    the second 1x1 conv, _bn_grads and _dw_grads of the depthwise conv, _bn_grads and _conv_grads of the first 1x1 conv, whose data gradient
    writes slot 1 of the dx buffer; each only where asked.  x, the weights, z and saved of the three layers and the two activations
    between them are kept; neither half of x is copied."""

    @staticmethod
    def forward(ctx, x, w1, gamma1, beta1, w_dw, gamma2, beta2, w3, gamma3, beta3, half, running, momentum, eps):
        out, ctx.descs, keep = _shuffle_unit_forward(x, w1, gamma1.detach(), beta1.detach(), w_dw, gamma2.detach(), beta2.detach(), w3,
                                                     gamma3.detach(), beta3.detach(), half, running, momentum, eps)
        ctx.half = half
        ctx.save_for_backward(x, w1, w3, *keep)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w1, w3, z1, saved1, y1, w9c, z2, saved2, y2, z3, saved3 = ctx.saved_tensors
        d1, d3 = ctx.descs
        need_x, need_w1, need_g1, need_b1, need_wd, need_g2, need_b2, need_w3, need_g3, need_b3 = ctx.needs_input_grad[:10]
        need_y1 = need_x or need_w1 or need_g1 or need_b1               # what dw_bn_block's x would ask for
        need_y2 = need_y1 or need_wd or need_g2 or need_b2              # what the second 1x1 conv's x would ask for
        need_y3 = need_y2 or need_w3 or need_g3 or need_b3
        dx = dw1 = dgamma1 = dbeta1 = dwd = dgamma2 = dbeta2 = dw3 = dgamma3 = dbeta3 = None
        if not (need_x or need_y3):
            return (None,) * 14
        slot = d1.cin
        with torch.cuda.device(x.device):
            dy = _dense_bf16(dy).permute(0, 2, 3, 1)
            n, h, w, _ = dy.shape
            dxb = torch.empty((n, h, w, 2 * slot), dtype=torch.bfloat16, device=x.device) if need_x else None
            db = torch.empty((n, h, w, slot), dtype=torch.bfloat16, device=x.device) if need_y3 else None
            K.channel_shuffle2_bwd(dy, dxb, db, ctx.half, slot)
            if need_y3:
                g3, dgamma3, dbeta3 = _bn_grads(db.permute(0, 3, 1, 2), z3, saved3, _RELU, need_y2, need_w3, need_g3, need_b3)
                dy2, dw3, _ = _conv_grads(y2, w3, g3, d3, need_y2, need_w3, False)
            if need_y2:
                g2, dgamma2, dbeta2 = _bn_grads(dy2, z2, saved2, ACT_NONE, need_y1, need_wd, need_g2, need_b2)
                dy1, dwd = _dw_grads(y1, g2, w9c, 1, need_y1, need_wd)
            if need_y1:
                g1, dgamma1, dbeta1 = _bn_grads(dy1.permute(0, 3, 1, 2), z1, saved1, _RELU, need_x, need_w1, need_g1, need_b1)
                _, dw1, _ = _conv_grads(x, w1, g1, d1, need_x, need_w1, False, dx_into=dxb)
            if need_x:
                dx = dxb.permute(0, 3, 1, 2)
        return (dx, dw1, dgamma1, dbeta1, dwd, dgamma2, dbeta2, dw3, dgamma3, dbeta3) + (None,) * 4


def _triple(name, what, v):
    """``v`` as (the first 1x1 conv's, the depthwise's, the second 1x1 conv's): a number for all three, or a triple."""
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise ValueError(f"{name}: {what} must be a number or a triple (first 1x1's, depthwise's, second 1x1's), not {v!r}")
        return tuple(v)
    return v, v, v


def shuffle_unit_block(x, half, w1, gamma1, beta1, running_mean1, running_var1, w_dw, gamma2, beta2, running_mean2, running_var2, w3, gamma3,
                       beta3, running_mean3, running_var3, *, momentum=0.1, eps=1e-5):
    """The stride-1 ShuffleNetV2 unit on the device as one op, differentiable once: with ``a, b = x[:, :slot], x[:, slot:]`` (``x.chunk(2)``
    in the two-slot layout of channel_shuffle2) it is ``channel_shuffle2(a, conv_bn_relu_block(dw_bn_block(conv_bn_relu_block(b, w1, ..),
    w_dw, .., act="none"), w3, ..), half)``, bit-equal to that composition - the output, the ten gradients and the six running tensors.

    Neither half of x is copied: the first 1x1 conv reads slot 1 of x as an input view of the conv descriptor, and the shuffle reads slot
    0 as a view.  In the backward the shuffle's inverse writes a's gradient straight into slot 0 of one [n, h, w, 2 slot] buffer and the
    first conv's data gradient writes slot 1 of it: every element of x's gradient is written by exactly one of the two, with no zero-fill
    and no add (autograd's slice backward fills two full maps with zeros and adds them).

    x       [n, 2 slot, h, w], ``slot % 8 == 0``: ``half`` logical channels in each slot, zero beyond; bfloat16 dense channels-last is
            taken as it is, anything else is converted by torch.
    half    an integer in [1, slot].
    w1, w3  float32 [slot, slot, 1, 1];  w_dw float32 [slot, 1, 3, 3].
    gamma, beta, running_mean, running_var (1: the first 1x1 conv's BatchNorm2d, 2: the depthwise's, 3: the second 1x1 conv's)
            float32 [slot]; the running tensors may be None, and those given are updated in place.
    momentum, eps   a number for the three batch norms, or a triple.
    Returns bfloat16 [n, 2 slot, h, w], channels-last.  Gradients: x bf16, the weights, gammas and betas float32, each computed only where
    asked; two runs give the same bits.  Wrong shapes raise ValueError before any launch; a CPU tensor raises RuntimeError (there is no
    CPU fallback)."""
    name = "shuffle_unit_block"
    _check_map(name, "x", x)
    if x.shape[1] % 16:
        raise ValueError(f"{name}: x needs two slots of a multiple of 8 channels (c {x.shape[1]})")
    slot = x.shape[1] // 2
    _check_half(name, half, slot)
    slot_map = torch.empty((x.shape[0], slot, x.shape[2], x.shape[3]), device="meta")            # (shape only: a conv's operand)
    for what, w_, k in (("w1", w1, 1), ("w3", w3, 1)):
        if not isinstance(w_, torch.Tensor) or tuple(w_.shape) != (slot, slot, k, k):
            raise ValueError(f"{name}: {what} must be [slot, slot, 1, 1] with slot = {slot}, not {list(getattr(w_, 'shape', ()))}")
        _check_conv(name, slot_map, w_, None, "none", (1,), True)
    _check_dw(name, w_dw, slot, "slot")
    momentum, eps = _triple(name, "momentum", momentum), _triple(name, "eps", eps)
    bns = ((w1, gamma1, beta1, running_mean1, running_var1), (w_dw, gamma2, beta2, running_mean2, running_var2),
           (w3, gamma3, beta3, running_mean3, running_var3))
    running = tuple(_check_bn(name, slot_map, w_, 1, g_, b_, rm, rv, True, momentum[i], eps[i]) for i, (w_, g_, b_, rm, rv) in enumerate(bns))
    _need_device(name, x, *(t for bn in bns for t in bn))
    return _apply(_ShuffleUnitFunction, _shuffle_unit_forward,
                  (_dense_bf16(x), w1.contiguous(), gamma1.contiguous(), beta1.contiguous(), w_dw.contiguous(), gamma2.contiguous(),
                   beta2.contiguous(), w3.contiguous(), gamma3.contiguous(), beta3.contiguous()),
                  int(half), running, tuple(float(m) for m in momentum), tuple(float(e) for e in eps))
