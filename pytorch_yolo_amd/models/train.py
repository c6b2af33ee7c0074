"""Training-mode forward of the Darknet-53 models (YOLOv3, YOLOv3-SPP), of the max-pool models (YOLOv3-tiny, LiteYOLOv3), of
YOLOv3-tiny/SqueezeNet, of YOLOv3-tiny/MobileNetV2 and of YOLOv3-tiny/ShuffleNetV2: the reference's ``model.train()(x)`` - batch-statistics BN, the raw ``p``
list with a ``grad_fn`` - wired from the differentiable ops of pytorch_yolo_amd.ops.

A model states its layer graph once, in ``_trace``.  For inference graph.Recorder records it; for training ``wiring`` (every trainable
class's ``_train_wiring``) runs the same ``_trace`` through a ``TrainTracer``, which has the Recorder's method names and runs each call at
once on tensors.  The tracer takes every op from a table, a namespace of functions: the default table runs the package's kernels; the
tests run the same wiring on the CPU with float64 torch restatements of the ops, which is how it is compared with the reference without a
GPU.  A table function has the signature of the op it stands for.  ``DEVICE_OPS`` holds the six functions the Darknet-53 models use;
``DEVICE_OPS_POOL`` adds ``max_pool`` and ``pool_bn_block`` and is the table ``forward_train`` runs by default (the ``up_first`` keyword
of ``upsample_concat`` goes through both).  ``DEVICE_OPS_FIRE`` adds ``stem_block``, ``fire_block``, ``max_pool_ceil`` and a ``concat``:
the table of YOLOv3-tiny/SqueezeNet, whose ``_trace`` runs through ``FireTracer`` - a model names its tracer class in ``_train_tracer``
and its default table in ``_train_ops``.  ``DEVICE_OPS_MOBILE`` (``mobile_ops()``) adds ``conv_bn_relu6_block``, ``dw_bn_block``,
``project_bn_block`` and ``expand_dw_bn_block`` to the pool table: the table of YOLOv3-tiny/MobileNetV2, whose ``_trace`` runs through
``MobileTracer``.  ``DEVICE_OPS_SHUFFLE`` (``shuffle_ops()``) adds ``conv_bn_relu_block``, ``dw_bn_block``, ``max_pool_321``,
``channel_shuffle2`` and ``shuffle_unit_block`` to the pool table: the table of YOLOv3-tiny/ShuffleNetV2, whose ``_trace`` runs through
``ShuffleTracer`` in the padded physical channel layout of the eval trace.

``forward_train(model, x)`` is the public entry for all classes.  ``model.train()(x)`` delegates to it for the classes whose
``_train_in_forward`` is True (YOLOv3, YOLOv3-SPP); YOLOv3-tiny and LiteYOLOv3 keep raising from the module call and train through the
function (DESIGN.md 3.6g says why: flipping their switch is a one-line change).  YOLOv3-tiny/MobileNetV2 is opt-in one step further: its
class sets ``_train_ops_by_name``, and it trains through ``forward_train(model, x, ops=DEVICE_OPS_MOBILE)`` only - without the table the
call raises what it raised before the class had a wiring.  YOLOv3-tiny/ShuffleNetV2 is opt-in the same way, through
``ops=DEVICE_OPS_SHUFFLE``.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
from torch import nn

from .. import graph
from .. import ops as _ops
from .yolo_base import ConvPoolBlock

DEVICE_OPS = SimpleNamespace(conv_block=_ops.conv_block, conv_bn_block=_ops.conv_bn_block, down_bn_block=_ops.down_bn_block,
                             res_bn_block=_ops.res_bn_block, spp_concat=_ops.spp_concat, upsample_concat=_ops.upsample_concat)
DEVICE_OPS_POOL = SimpleNamespace(**vars(DEVICE_OPS), max_pool=_ops.max_pool, pool_bn_block=_ops.pool_bn_block)


def _concat(xs):
    """cat of same-grid maps on the channels (YOLOv3-tiny/SqueezeNet's head concat [route1, b1]): torch's copy on channels-last bf16;
    autograd slices the gradient back."""
    return torch.cat(list(xs), 1)


DEVICE_OPS_FIRE = SimpleNamespace(**vars(DEVICE_OPS_POOL), stem_block=_ops.stem_block, fire_block=_ops.fire_block,
                                  max_pool_ceil=_ops.max_pool_ceil, concat=_concat)


def _composed_expand_dw(x, w_expand, gamma1, beta1, running_mean1, running_var1, w_dw, gamma2, beta2, running_mean2, running_var2, *,
                        stride=1, momentum=0.1, eps=1e-5, training=True):
    """``expand_dw_bn_block`` as the two ops it fuses: what ``mobile_ops(fused=False)`` puts under that name."""
    (m1, m2), (e1, e2) = (v if isinstance(v, (tuple, list)) else (v, v) for v in (momentum, eps))
    y1 = _ops.conv_bn_relu6_block(x, w_expand, gamma1, beta1, running_mean1, running_var1, momentum=m1, eps=e1, training=training)
    return _ops.dw_bn_block(y1, w_dw, gamma2, beta2, running_mean2, running_var2, stride=stride, momentum=m2, eps=e2, training=training)


def mobile_ops(fused=True):
    """The table of YOLOv3-tiny/MobileNetV2: the pool table's functions plus the three ops of an inverted residual and, under the name
    ``expand_dw_bn_block``, the fused expand + depthwise op - or, with ``fused=False``, the two-op composition it is bit-equal to (the
    form the timings and the tests compare it with)."""
    return SimpleNamespace(**vars(DEVICE_OPS_POOL), conv_bn_relu6_block=_ops.conv_bn_relu6_block, dw_bn_block=_ops.dw_bn_block,
                           project_bn_block=_ops.project_bn_block,
                           expand_dw_bn_block=_ops.expand_dw_bn_block if fused else _composed_expand_dw)


DEVICE_OPS_MOBILE = mobile_ops()


def _composed_shuffle_unit(x, half, w1, gamma1, beta1, running_mean1, running_var1, w_dw, gamma2, beta2, running_mean2, running_var2, w3,
                           gamma3, beta3, running_mean3, running_var3, *, momentum=0.1, eps=1e-5):
    """``shuffle_unit_block`` as the ops it fuses, on two torch slices of x: what ``shuffle_ops(fused=False)`` puts under that name."""
    (m1, m2, m3), (e1, e2, e3) = (tuple(v) if isinstance(v, (tuple, list)) else (v, v, v) for v in (momentum, eps))
    slot = x.shape[1] // 2
    y = _ops.conv_bn_relu_block(x[:, slot:], w1, gamma1, beta1, running_mean1, running_var1, momentum=m1, eps=e1)
    y = _ops.dw_bn_block(y, w_dw, gamma2, beta2, running_mean2, running_var2, act="none", momentum=m2, eps=e2)
    y = _ops.conv_bn_relu_block(y, w3, gamma3, beta3, running_mean3, running_var3, momentum=m3, eps=e3)
    return _ops.channel_shuffle2(x[:, :slot], y, half)


def shuffle_ops(fused=True):
    """The table of YOLOv3-tiny/ShuffleNetV2: the pool table's functions plus the dense ConvBNReLU, the depthwise stage, MaxPool2d(3, 2, 1),
    the channel shuffle and, under the name ``shuffle_unit_block``, the stride-1 unit as one op - or, with ``fused=False``, the composition
    on two slices of x it is bit-equal to (the form the timings and the tests compare it with)."""
    return SimpleNamespace(**vars(DEVICE_OPS_POOL), conv_bn_relu_block=_ops.conv_bn_relu_block, dw_bn_block=_ops.dw_bn_block,
                           max_pool_321=_ops.max_pool_321, channel_shuffle2=_ops.channel_shuffle2,
                           shuffle_unit_block=_ops.shuffle_unit_block if fused else _composed_shuffle_unit)


DEVICE_OPS_SHUFFLE = shuffle_ops()


def conv_bn(ops, block, x, residual=None, want_preadd=False, weight=None):
    """One ConvBlock as it trains (Conv2d(bias=False) -> BatchNorm2d on batch statistics -> LeakyReLU(0.1)), with the residual unit's add
    where ``residual`` is given.  momentum and eps are the BatchNorm2d's own; its running statistics are updated in place and
    num_batches_tracked counts the call.  A cout that is no multiple of 8 (the 3 (5 + nc) channels of a ConvBlock head) is padded by
    torch: zero weights, gamma 1, beta 0 and temporaries of the running tensors; the padded channels have z = 0 and give 0.  ``weight``
    stands in for the conv's own where the caller has laid it out for a physical channel space (ShuffleTracer.conv_block_mapped)."""
    conv, bn = block.sequence.conv, block.sequence.batch_norm
    kw = dict(momentum=bn.momentum, eps=bn.eps)
    with torch.no_grad():
        bn.num_batches_tracked += 1
    w, gamma, beta, rm, rv = conv.weight if weight is None else weight, bn.weight, bn.bias, bn.running_mean, bn.running_var
    if residual is not None:
        return ops.res_bn_block(x, w, gamma, beta, rm, rv, residual, want_preadd=want_preadd, **kw)
    if isinstance(block, ConvPoolBlock):        # (stride 1, cout % 8 == 0 in every model: ops.pool_bn_block checks)
        return ops.pool_bn_block(x, w, gamma, beta, rm, rv, pool_stride=block.pool.stride, **kw)
    if block.stride == 2:
        return ops.down_bn_block(x, w, gamma, beta, rm, rv, **kw)
    cout = w.shape[0]
    pad = -cout % 8
    if not pad:
        return ops.conv_bn_block(x, w, gamma, beta, rm, rv, **kw)
    w = nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, pad))
    gamma = torch.cat([gamma, gamma.new_ones(pad)])
    beta = torch.cat([beta, beta.new_zeros(pad)])
    rm_t, rv_t = torch.cat([rm.detach(), rm.new_zeros(pad)]), torch.cat([rv.detach(), rv.new_ones(pad)])
    y = ops.conv_bn_block(x, w, gamma, beta, rm_t, rv_t, **kw)[:, :cout]
    with torch.no_grad():
        rm.copy_(rm_t[:cout]), rv.copy_(rv_t[:cout])
    return y


class TrainTracer:
    """What a model's ``_trace`` drives in training mode: the method names of graph.Recorder that a trainable model uses, run at once on
    tensors through the op table ``ops``.  It has no ``conv``, ``dwconv``, ``se``, ``slice``, ``shuffle2``, ``concat`` or ``upsample2``: a
    class whose ``_trace`` needs one has no ``_train_wiring`` and is refused by ``forward_train`` before it gets here."""

    def __init__(self, ops, yolo_layers):
        self.ops, self.yolo_layers, self.branches = ops, tuple(yolo_layers), []

    def conv_block(self, block, x, residual=None, want_preadd=False, f32_out=False):
        """A ConvBlock (``conv_bn``; a ConvPoolBlock's pool is part of its op); ``f32_out``: the last layer of a head as float32."""
        y = conv_bn(self.ops, block, x, residual, want_preadd)
        return y.float() if f32_out and y.dtype == torch.bfloat16 else y    # (a table that works in float32 / float64 keeps its dtype)

    def plain_conv(self, conv, x):
        return self.ops.conv_block(x, conv.weight, conv.bias, act="none", out_dtype=torch.float32)

    def maxpool(self, x, size, stride):
        if (size, stride) != (2, 2):
            raise NotImplementedError(f"the training-mode forward has no stand-alone max-pool of size {size} / stride {stride} (2 / 2 only)")
        return self.ops.max_pool(x, stride=2)

    def spp_concat(self, x):
        return self.ops.spp_concat(x)

    def upsample_concat(self, a, b, up_first=True):
        # (no keyword where the upsampled map comes first: the tables of the Darknet-53 models take two arguments)
        return self.ops.upsample_concat(a, b) if up_first else self.ops.upsample_concat(a, b, up_first=False)

    def head(self, x, layer):
        if len(self.branches) >= len(self.yolo_layers) or layer is not self.yolo_layers[len(self.branches)]:
            raise RuntimeError(f"head {len(self.branches)} of the trace is not yolo_layers[{len(self.branches)}]: the heads are out of order")
        self.branches.append(x)


class FireTracer(TrainTracer):
    """TrainTracer plus what YOLOv3-tiny/SqueezeNet's ``_trace`` calls: graph.Recorder's ``stem_conv``, ``fire`` and ``concat``, and its
    ``maxpool`` with the geometry of MaxPool2d(3, 2, ceil_mode=True).  The ops take the modules' own parameters, so a gradient reaches
    them (the Recorder's side of the same methods packs detached copies)."""

    def stem_conv(self, conv, x):
        return self.ops.stem_block(x, conv.weight, conv.bias, act="relu")

    def fire(self, fire, x):
        return self.ops.fire_block(x, fire.squeeze.weight, fire.squeeze.bias, fire.expand1x1.weight, fire.expand1x1.bias,
                                   fire.expand3x3.weight, fire.expand3x3.bias)

    def maxpool(self, x, size, stride, pad=None, ceil_mode=False):
        if (size, stride, pad, ceil_mode) == (3, 2, 0, True):
            return self.ops.max_pool_ceil(x)
        if pad is not None or ceil_mode:
            raise NotImplementedError(f"the training-mode forward has no max-pool of size {size} / stride {stride} with pad {pad}, "
                                      f"ceil_mode {ceil_mode} (3 / 2 / 0 / True only)")
        return super().maxpool(x, size, stride)

    def concat(self, xs):
        return self.ops.concat(xs)


def _bn_args(bn):
    """A BatchNorm2d's tensors in an op's order; the call counts in num_batches_tracked, as conv_bn's does."""
    with torch.no_grad():
        bn.num_batches_tracked += 1
    return bn.weight, bn.bias, bn.running_mean, bn.running_var


class MobileTracer(TrainTracer):
    """TrainTracer plus what YOLOv3-tiny/MobileNetV2's ``_trace`` calls: graph.Recorder's ``conv_bn_relu6`` and ``inverted_residual``.  The
    ops take the modules' own parameters and each BatchNorm2d's own momentum and eps (the Recorder's side of the same methods folds
    detached copies)."""

    def conv_bn_relu6(self, module, x):
        conv, bn = module[0], module[1]
        kw = dict(stride=module.stride, momentum=bn.momentum, eps=bn.eps)
        if module.depthwise:
            return self.ops.dw_bn_block(x, conv.weight, *_bn_args(bn), **kw)
        return self.ops.conv_bn_relu6_block(x, conv.weight, *_bn_args(bn), **kw)

    def inverted_residual(self, block, x):
        layers = list(block.conv)
        if len(layers) == 4:                                             # the block expands: expand + depthwise as one op
            (ce, be, _), (cd, bd, _) = layers[0], layers[1]
            y = self.ops.expand_dw_bn_block(x, ce.weight, *_bn_args(be), cd.weight, *_bn_args(bd), stride=layers[1].stride,
                                            momentum=(be.momentum, bd.momentum), eps=(be.eps, bd.eps))
        else:
            y = self.conv_bn_relu6(layers[0], x)
        conv, bn = layers[-2], layers[-1]
        return self.ops.project_bn_block(y, conv.weight, *_bn_args(bn), residual=x if block.use_res_connect else None,
                                         momentum=bn.momentum, eps=bn.eps)


class _PhysBn:
    """A BatchNorm2d's tensors laid out for ``phys`` physical channels, logical channel i at ``rows[i]``: gamma 1 and beta 0 in the pad
    channels (built by torch operations that autograd differentiates), temporaries of the running tensors that ``store`` copies back.
    A pad channel's conv output is 0 in every pixel, so its normalised value is beta = 0.  The call counts in num_batches_tracked."""

    def __init__(self, bn, rows, phys):
        with torch.no_grad():
            bn.num_batches_tracked += 1
        self.bn, self.dense = bn, len(rows) == phys
        self.kw = dict(momentum=bn.momentum, eps=bn.eps)
        if self.dense:                                                   # (nothing to pad: the module's own tensors)
            self.args = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
            return
        self.idx = torch.as_tensor(rows, device=bn.weight.device)
        gamma = bn.weight.new_ones(phys).index_put((self.idx,), bn.weight)
        beta = bn.bias.new_zeros(phys).index_put((self.idx,), bn.bias)
        rm = bn.running_mean.new_zeros(phys).index_put((self.idx,), bn.running_mean.detach())
        rv = bn.running_var.new_ones(phys).index_put((self.idx,), bn.running_var.detach())
        self.args = (gamma, beta, rm, rv)

    def store(self):
        if not self.dense:
            with torch.no_grad():
                self.bn.running_mean.copy_(self.args[2][self.idx]), self.bn.running_var.copy_(self.args[3][self.idx])


def _phys_weight(w, out_rows, out_phys, in_cols=None, in_phys=None):
    """The logical weight [cout, cin, k, k] in physical channels: row o at ``out_rows[o]``, input channel i (dense convs) at
    ``in_cols[i]``, zero everywhere else - the training twin of graph.scatter_weight, by an index_put that autograd differentiates."""
    rows = torch.as_tensor(out_rows, device=w.device)
    if in_cols is None:                                                  # depthwise: [c, 1, 3, 3]
        if len(out_rows) == out_phys:
            return w
        return w.new_zeros((out_phys,) + tuple(w.shape[1:])).index_put((rows,), w)
    if (len(out_rows), len(in_cols)) == (out_phys, in_phys) and list(in_cols) == list(range(in_phys)):
        return w
    cols = torch.as_tensor(in_cols, device=w.device)
    return w.new_zeros((out_phys, in_phys) + tuple(w.shape[2:])).index_put((rows[:, None], cols[None, :]), w)


class ShuffleTracer(TrainTracer):
    """TrainTracer plus what YOLOv3-tiny/ShuffleNetV2's ``_trace`` calls: graph.Recorder's ``conv_bn_relu``, ``shuffle_unit`` and
    ``conv_block_mapped``, and its ``maxpool`` with the geometry of MaxPool2d(3, 2, 1).  It runs in the eval trace's physical layout -
    halves of 58 / 116 / 232 channels in slots of 64 / 128 / 256, conv1's 24 channels in 32: every layer's parameters are laid out for
    that space from the modules' own by torch operations (``_phys_weight``, ``_PhysBn``), so a gradient reaches the modules' parameters
    and the pad channels stay exactly 0 through every layer."""

    def _dense(self, conv, bn, x, in_map, out_phys):
        rows = list(range(conv.out_channels))
        p = _PhysBn(bn, rows, out_phys)
        y = self.ops.conv_bn_relu_block(x, _phys_weight(conv.weight, rows, out_phys, in_map, x.shape[1]), *p.args, stride=conv.stride[0], **p.kw)
        p.store()
        return y

    def _depthwise(self, conv, bn, x, rows):
        p = _PhysBn(bn, rows, x.shape[1])
        y = self.ops.dw_bn_block(x, _phys_weight(conv.weight, rows, x.shape[1]), *p.args, stride=conv.stride[0], act="none", **p.kw)
        p.store()
        return y

    def conv_bn_relu(self, module, x, in_map, out_phys):
        return self._dense(module[0], module[1], x, in_map, out_phys)

    def shuffle_unit(self, unit, x, in_map):
        h, hp = unit.bf, graph.shuffle_slot(unit.bf)
        rows, b2 = list(range(h)), unit.branch2
        out_map = rows + [hp + i for i in rows]
        if unit.stride > 1:                                              # both branches read the whole x: autograd adds their gradients
            b1 = unit.branch1
            a = self._dense(b1[2], b1[3], self._depthwise(b1[0], b1[1], x, in_map), in_map, hp)
            b = self._dense(b2[0], b2[1], x, in_map, hp)
            b = self._dense(b2[5], b2[6], self._depthwise(b2[3], b2[4], b, rows), rows, hp)
            return self.ops.channel_shuffle2(a, b, h), out_map
        bns = [_PhysBn(b2[i], rows, hp) for i in (1, 4, 6)]
        y = self.ops.shuffle_unit_block(x, h, _phys_weight(b2[0].weight, rows, hp, rows, hp), *bns[0].args,
                                        _phys_weight(b2[3].weight, rows, hp), *bns[1].args,
                                        _phys_weight(b2[5].weight, rows, hp, rows, hp), *bns[2].args,
                                        momentum=tuple(p.kw["momentum"] for p in bns), eps=tuple(p.kw["eps"] for p in bns))
        for p in bns:
            p.store()
        return y, out_map

    def conv_block_mapped(self, block, x, in_map):
        conv = block.sequence.conv
        w = _phys_weight(conv.weight, list(range(conv.out_channels)), conv.out_channels, in_map, x.shape[1])
        return conv_bn(self.ops, block, x, weight=w)

    def maxpool(self, x, size, stride, pad=None, ceil_mode=False):
        if (size, stride, ceil_mode) == (3, 2, False) and pad in (1, None):
            return self.ops.max_pool_321(x)
        if pad is not None or ceil_mode:
            raise NotImplementedError(f"the training-mode forward has no max-pool of size {size} / stride {stride} with pad {pad}, "
                                      f"ceil_mode {ceil_mode} (3 / 2 / 1 / False only)")
        return super().maxpool(x, size, stride)


def wiring(model, ops, x):
    """``model._train_wiring``: the raw head maps [bs, 3 (5 + nc), ny, nx] of ``model._trace`` run on the ops of a table, through the
    tracer class the model names (``_train_tracer``; TrainTracer without one)."""
    g = getattr(model, "_train_tracer", TrainTracer)(ops, model.yolo_layers)
    model._trace(g, x)
    return tuple(g.branches)


def forward_train(model, x, ops=None):
    """``[p1, p2, p3]`` (``[p1, p2]`` for YOLOv3-tiny), each ``[bs, 3, ny, nx, 5 + nc]`` contiguous with a grad_fn, as the reference's
    training-mode forward returns.  With the default table: float32 on the device; x float32 NCHW, H and W multiples of 32 (YOLOv3-tiny:
    at least 64), bf16 mode, BN not fused.  YOLOv3-tiny/MobileNetV2 and YOLOv3-tiny/ShuffleNetV2 have no default: ``ops=DEVICE_OPS_MOBILE``
    / ``ops=DEVICE_OPS_SHUFFLE`` runs them on the device under the same checks, ``ops=None`` raises NotImplementedError (DESIGN.md 3.6k,
    3.6l)."""
    by_name = getattr(model, "_train_ops_by_name", False)                # the class trains only with its table named by the caller
    if not hasattr(model, "_train_wiring") or (by_name and ops is None):
        raise NotImplementedError(
            "training-mode forward (batch-statistics BN, raw p list) is outside the inference hot path; "
            "call .eval() first")
    if model.precision != "bf16":
        raise NotImplementedError(f"the training-mode forward runs in bf16 mode only (model.precision is {model.precision!r})")
    if any(getattr(m, "is_fused", False) for m in model.modules()):
        raise NotImplementedError("the training-mode forward needs the BatchNorm2d layers: this model was fuse()d")
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != model.in_channels or x.shape[0] < 1:
        raise ValueError(f"expected input [bs,{model.in_channels},H,W], got {tuple(getattr(x, 'shape', ()))}")
    if x.shape[2] % 32 or x.shape[3] % 32 or min(x.shape[2:]) < 32:
        raise ValueError(f"the training-mode forward needs H and W to be multiples of 32, got {tuple(x.shape[2:])}")
    min_size = getattr(model, "_train_min_size", 32)
    if min(x.shape[2:]) < min_size:
        raise ValueError(f"the training-mode forward of {type(model).__name__} needs H and W of at least {min_size}, got "
                         f"{tuple(x.shape[2:])}: on a smaller input its stride-1 max-pool sees a 1x1 map, whose window is all padding "
                         "(the reference itself returns -inf there)")
    if ops is None or (by_name and ops is model._train_ops):
        if x.dtype != torch.float32:
            raise ValueError(f"the training-mode forward takes a float32 NCHW batch, got {x.dtype}")
        if not x.is_cuda:
            raise RuntimeError("pytorch_yolo_amd runs on a ROCm device only: move the input to cuda "
                               "(there is no CPU fallback)")
        ops = getattr(model, "_train_ops", DEVICE_OPS_POOL)
    branches = model._train_wiring(ops, x)
    img_size = max(x.shape[-2:])
    out = []
    for b, layer in zip(branches, model.yolo_layers):
        bs, _, ny, nx = b.shape
        layer._sync_grid_attrs(ny, nx, img_size, b.device)
        out.append(b.reshape(bs, layer.n_anchors, layer.n_classes + 5, ny, nx).permute(0, 1, 3, 4, 2).contiguous())
    # the kernels updated the running statistics through raw pointers: torch's version counters did not move, so a cached eval plan
    # would keep its stale folded weights
    model.invalidate()
    return out
