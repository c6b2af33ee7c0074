"""The symbolic layer graph a model records once per (batch, H, W): ``Recorder`` and the ``Sym`` / ``Node`` / ``Buf`` records.

A model's ``_trace`` method reads like the reference's ``_forward_encoder``; every call appends one ``Node``.  ``Node.attrs`` holds
what the recorder wrote (weights, stride, activation, padding, name, pool geometry) and nothing else: what the planner decides
lives in its own records (planner.Launch), where a tensor lives in ``Sym.buf`` / ``Sym.c_offset``."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import kernels as K
from .utils.torch_utils import fold_conv_bn


SHUFFLE_SLOT = 32     # ShuffleNetV2's slot granule: 8 channels would do for the views; 32 keeps every 1x1 / 3x3 conv on the LDS-DMA fast path


def shuffle_slot(half: int) -> int:
    """Physical channels of the slot that holds ``half`` logical channels of a ShuffleNetV2 unit (58 / 116 / 232 -> 64 / 128 / 256)."""
    return K.roundup(half, SHUFFLE_SLOT)


def _fold(conv, bn):
    return fold_conv_bn(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def scatter_weight(wb, out_map, out_phys, in_map=None, in_phys=None):
    """Logical folded (weight OIHW, bias) -> the same conv in physical channels: row o goes to out_map[o], input channel i (full convs
    only) to in_map[i]; everything else is zero."""
    w, b = wb
    cout, cin, k, _ = w.shape
    if in_map is None:                                      # depthwise: [c, 1, 3, 3]
        wp = torch.zeros((out_phys, 1, k, k), dtype=torch.float32)
        wp[out_map] = w
    else:
        wp = torch.zeros((out_phys, in_phys, k, k), dtype=torch.float32)
        wp[torch.as_tensor(out_map)[:, None], torch.as_tensor(in_map)[None, :]] = w
    bp = torch.zeros(out_phys, dtype=torch.float32)
    bp[out_map] = b
    return wp, bp


@dataclass(eq=False)
class Sym:
    """A logical NHWC activation."""
    n: int
    h: int
    w: int
    c: int
    producer: Optional["Node"] = None
    slot: int = 0                      # 0 main output, 1 pre-add output
    f32: bool = False
    # placement (filled by the planner)
    buf: Optional["Buf"] = None
    c_offset: int = 0
    consumers: List["Node"] = field(default_factory=list)

    @property
    def shape(self):
        """(n, c, h, w): what the tensor in its place has under models/train.TrainTracer, so a ``_trace`` can ask either for its channels."""
        return self.n, self.c, self.h, self.w


@dataclass(eq=False)
class Buf:
    n: int
    h: int
    w: int
    c_total: int
    f32: bool = False
    tensor: Optional[torch.Tensor] = None


@dataclass(eq=False)
class Node:
    kind: str                          # input | conv | dwconv | pool | spp | up | cat | head
    srcs: List[Sym]
    outs: List[Sym]
    attrs: dict


class Recorder:
    def __init__(self, n, c_in, h, w):
        self.nodes: List[Node] = []
        self.c_in = c_in
        x = Sym(n, h, w, K.roundup(c_in, 8))
        self.input = x
        self._add("input", [], [x])
        self.heads = []

    def _add(self, kind, srcs, outs, **attrs):
        node = Node(kind, list(srcs), list(outs), attrs)
        for o in outs:
            o.producer = node
        for s in srcs:
            s.consumers.append(node)
        self.nodes.append(node)
        return node

    # weight = (w_oihw f32, bias f32) already BN-folded; act in {'leaky','relu6','none'}
    @staticmethod
    def tf_same(size: int, k: int, stride: int):
        """TensorFlow "same" padding as efficientnet_pytorch 0.2.0's Conv2dSamePadding computes it: output ceil(size / stride),
        total pad max((out - 1) stride + k - size, 0), the odd one BELOW / RIGHT.  Returns (out, leading pad)."""
        out = -(-size // stride)
        return out, max((out - 1) * stride + k - size, 0) // 2

    def conv(self, x: Sym, weight, stride=1, act="leaky", residual: Sym = None, want_preadd=False, f32_out=False, pad=None,
             name=None, tf_same=False):
        w, _ = weight
        cout, cin_w, k, _ = w.shape
        if cin_w > x.c:
            raise RuntimeError(f"conv expects {cin_w} input channels, tensor has {x.c}")
        same = (k - 1) // 2
        pad = same if pad is None else pad
        ho, wo = (x.h + 2 * pad - k) // stride + 1, (x.w + 2 * pad - k) // stride + 1
        if tf_same:
            (ho, pad), (wo, pad_w) = self.tf_same(x.h, k, stride), self.tf_same(x.w, k, stride)
            if pad != pad_w:
                raise RuntimeError("tf_same conv: the two axes need different leading pads (one odd, one even size): not supported")
        if not f32_out and cout % 8:
            raise RuntimeError(f"internal conv width {cout} is not a multiple of 8 (unsupported kernels_divider)")
        y = Sym(x.n, ho, wo, cout, f32=f32_out)
        outs = [y]
        if want_preadd:
            outs.append(Sym(x.n, ho, wo, cout, slot=1))
        srcs = [x] + ([residual] if residual is not None else [])
        self._add("conv", srcs, outs, weight=weight, stride=stride, act=act, has_res=residual is not None, name=name)
        if pad != same:
            self.nodes[-1].attrs["pad"] = pad            # (SqueezeNet's unpadded first conv; no fused form takes it)
        return (y, outs[1]) if want_preadd else y

    # The three methods below and maxpool / spp_concat / head are the vocabulary a trainable model's ``_trace`` keeps to:
    # models/train.TrainTracer has the same names and runs them on tensors, so one ``_trace`` is both wirings.
    def conv_block(self, block, x: Sym, **kw):
        """A ConvBlock (conv + folded BN + LeakyReLU) and, where the block has one, its max-pool (ConvPoolBlock)."""
        y = self.conv(x, block.folded(), stride=block.stride, act="leaky", name=getattr(block, "_trace_name", None), **kw)
        pool = getattr(block, "pool", None)
        return y if pool is None else self.maxpool(y, pool.size, pool.stride)

    def plain_conv(self, conv, x: Sym):
        """A biased ``nn.Conv2d(C, 3 (5 + nc), 1)`` without BN or activation, float32 out: the last layer of a plain head."""
        return self.conv(x, (conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()), stride=1,
                         act="none", f32_out=True, name=getattr(conv, "_trace_name", None))

    def upsample_concat(self, a: Sym, b: Sym, up_first=True):
        """cat([nearest_x2(a), b]), or cat([b, nearest_x2(a)]) with ``up_first=False``."""
        up = self.upsample2(a)
        return self.concat([up, b] if up_first else [b, up])

    # SqueezeNet 1.1's two layers (models/yolov3_tiny_squeeze.py); with maxpool(3, 2, pad=0, ceil_mode=True) and concat they are what
    # models/train.FireTracer adds to the trainable vocabulary.
    def stem_conv(self, conv, x: Sym):
        """features[0]: a biased ``nn.Conv2d(cin, cout, 3, stride=2)`` WITHOUT padding, the ReLU that follows folded in."""
        return self.conv(x, (conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()), stride=2, act="relu", pad=0)

    def fire(self, fire, x: Sym):
        """A Fire module: squeeze 1x1 + ReLU -> cat(expand 1x1 + ReLU, expand 3x3 (pad 1) + ReLU).  The squeeze tensor (16 / 32 / 48 / 64
        channels) is kept in a multiple of 32 physical channels (zero weight rows and biases, zero input columns in the expand convs):
        the expand convs then take the LDS-DMA fast path."""
        pad = torch.nn.functional.pad

        def wb(conv):
            return conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()
        sq, sp = fire.squeeze.out_channels, -(-fire.squeeze.out_channels // 32) * 32
        w, b = wb(fire.squeeze)
        s = self.conv(x, (pad(w, (0, 0, 0, 0, 0, 0, 0, sp - sq)), pad(b, (0, sp - sq))), act="relu")

        def widen(conv):
            w_, b_ = wb(conv)
            return pad(w_, (0, 0, 0, 0, 0, sp - sq)), b_
        return self.concat([self.conv(s, widen(fire.expand1x1), act="relu"), self.conv(s, widen(fire.expand3x3), act="relu")])

    # MobileNetV2's two layers (models/yolov3_tiny_mobilenet.py); they are what models/train.MobileTracer adds to the trainable vocabulary.
    def conv_bn_relu6(self, module, x: Sym):
        """torchvision's ConvBNReLU (Conv2d(bias=False) -> BatchNorm2d -> ReLU6) with its BN folded: dense or depthwise."""
        conv, bn = module[0], module[1]
        w = fold_conv_bn(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        if module.depthwise:
            return self.dwconv(x, w, stride=module.stride, act="relu6")
        return self.conv(x, w, stride=module.stride, act="relu6")

    def inverted_residual(self, block, x: Sym):
        """An inverted residual: [expand 1x1 ->] depthwise 3x3 -> the linear bottleneck (no activation) with the block's add."""
        y = x
        for m in list(block.conv)[:-2]:
            y = self.conv_bn_relu6(m, y)
        conv, bn = block.conv[-2], block.conv[-1]
        proj = fold_conv_bn(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        return self.conv(y, proj, stride=1, act="none", residual=x if block.use_res_connect else None)

    # ShuffleNetV2's layers (models/yolov3_tiny_shuffle.py) in the padded physical space of that module's docstring; with
    # maxpool(3, 2) they are what models/train.ShuffleTracer adds to the trainable vocabulary.  ``in_map[i]`` is the physical channel of
    # x that holds logical input channel i.
    def conv_bn_relu(self, module, x: Sym, in_map, out_phys):
        """Conv2d(bias=False) -> BatchNorm2d -> ReLU with its BN folded, dense: the cout logical outputs in [0, cout) of ``out_phys``."""
        conv, bn = module[0], module[1]
        in_phys = len(in_map) if x is self.input else x.c               # (the first layer's weight keeps the image's channel count)
        w = scatter_weight(_fold(conv, bn), list(range(conv.out_channels)), out_phys, in_map, in_phys)
        return self.conv(x, w, stride=conv.stride[0], act="relu")

    def shuffle_unit(self, unit, x: Sym, in_map):
        """A ShuffleNetV2 unit: at stride 1 ``shuffle(cat(x1, branch2(x2)))`` with ``x.chunk(2)`` as the two slot views of x, at stride 2
        ``shuffle(cat(branch1(x), branch2(x)))``.  Returns (y, the map of y): two slots of ``shuffle_slot(half)`` channels."""
        h, hp = unit.bf, shuffle_slot(unit.bf)
        rows = list(range(h))

        def branch2(t, t_map):
            b2 = unit.branch2
            u = self.conv(t, scatter_weight(_fold(b2[0], b2[1]), rows, hp, t_map, t.c), act="relu")
            v = self.dwconv(u, scatter_weight(_fold(b2[3], b2[4]), rows, hp), stride=unit.stride, act="none")
            return self.conv(v, scatter_weight(_fold(b2[5], b2[6]), rows, hp, rows, hp), act="relu")
        if unit.stride > 1:
            b1 = unit.branch1
            t = self.dwconv(x, scatter_weight(_fold(b1[0], b1[1]), in_map, x.c), stride=unit.stride, act="none")
            a = self.conv(t, scatter_weight(_fold(b1[2], b1[3]), rows, hp, in_map, x.c), act="relu")
            b = branch2(x, in_map)
        else:
            a = self.slice(x, 0, hp)                                     # x.chunk(2): the two slots
            b = branch2(self.slice(x, hp, hp), rows)
        return self.shuffle2(a, b, h), rows + [hp + i for i in rows]

    def conv_block_mapped(self, block, x: Sym, in_map):
        """A ConvBlock whose logical input channels sit at ``in_map`` of a wider physical x (the head conv on cat(route1, up))."""
        cout = block.out_channels
        return self.conv(x, scatter_weight(block.folded(), list(range(cout)), cout, in_map, x.c), act="leaky")

    def dwconv(self, x: Sym, weight, stride=1, act="relu6", tf_same=False):
        """Depthwise k x k conv.  Default: 3x3 / pad 1 (MobileNetV2).  ``tf_same``: k = 3 or 5 with TensorFlow "same" padding
        (EfficientNet-B0's MBConvBlock._depthwise_conv) - the general kernel, which also takes the swish activation."""
        w, _ = weight                                   # [c,1,k,k]
        k = w.shape[2]
        if not tf_same:
            if k != 3:
                raise RuntimeError("dwconv: only 3x3 with torch-style pad 1; pass tf_same=True for k = 5")
            ho, wo = (x.h - 1) // stride + 1, (x.w - 1) // stride + 1
            y = Sym(x.n, ho, wo, x.c)
            self._add("dwconv", [x], [y], weight=weight, stride=stride, act=act)
            return y
        (ho, pad), (wo, pad_w) = self.tf_same(x.h, k, stride), self.tf_same(x.w, k, stride)
        if pad != pad_w:
            raise RuntimeError("tf_same dwconv: the two axes need different leading pads: not supported")
        y = Sym(x.n, ho, wo, x.c)
        self._add("dwconv", [x], [y], weight=weight, stride=stride, act=act, ksize=k, pad=pad)
        return y

    def se(self, x: Sym, w1, b1, w2, b2):
        """Squeeze-and-excitation: y = x * sigmoid(W2 swish(W1 mean_hw(x) + b1) + b2) (efficientnet_pytorch MBConvBlock).
        w1: [sq, c] (or [sq, c, 1, 1]), w2: [c, sq]."""
        y = Sym(x.n, x.h, x.w, x.c)
        self._add("se", [x], [y], w1=w1, b1=b1, w2=w2, b2=b2)
        return y

    def maxpool(self, x: Sym, size, stride, pad=None, ceil_mode=False):
        # reference MaxPool: (2,1) -> pad 1, dilation 2 (models/yolo_base.py:60-66)
        if size == 2 and stride == 1:
            pad, dil = 1, 2
        else:
            pad, dil = ((size - 1) // 2 if pad is None else pad), 1

        def out(n):                                       # torch.nn.MaxPool2d output size incl. ceil_mode
            span = n + 2 * pad - dil * (size - 1) - 1
            o = (-(-span // stride) if ceil_mode else span // stride) + 1
            return o - 1 if ceil_mode and (o - 1) * stride >= n + pad else o
        ho, wo = out(x.h), out(x.w)
        y = Sym(x.n, ho, wo, x.c)
        self._add("pool", [x], [y], size=size, stride=stride, pad=pad, dil=dil)
        return y

    def spp_concat(self, x: Sym):
        y = Sym(x.n, x.h, x.w, 4 * x.c)
        self._add("spp", [x], [y])
        return y

    def upsample2(self, x: Sym):
        y = Sym(x.n, 2 * x.h, 2 * x.w, x.c)
        self._add("up", [x], [y])
        return y

    def concat(self, xs: List[Sym]):
        y = Sym(xs[0].n, xs[0].h, xs[0].w, sum(x.c for x in xs))
        self._add("cat", xs, [y])
        return y

    def slice(self, x: Sym, offset: int, c: int):
        """Channel view [offset, offset + c) of ``x`` (8-channel aligned): no launch, the consumers read the view."""
        if offset % 8 or c % 8 or offset + c > x.c:
            raise RuntimeError("slice: views are 8-channel aligned")
        y = Sym(x.n, x.h, x.w, c)
        self._add("slice", [x], [y], offset=offset)
        return y

    def shuffle2(self, a: Sym, b: Sym, half: int):
        """ShuffleNetV2's ``channel_shuffle(cat(a, b), groups=2)`` for two tensors of ``half`` logical channels each,
        every one held in a slot of a.c == b.c >= half physical channels (zero beyond ``half``): logical channel j of the
        result is (a, b)[j % 2][j // 2]; the result keeps the two-slot layout (logical [0, half) in slot 0, [half, 2 half)
        in slot 1)."""
        if a.c != b.c or half > a.c or (a.h, a.w) != (b.h, b.w):
            raise RuntimeError("shuffle2: mismatched halves")
        y = Sym(a.n, a.h, a.w, 2 * a.c)
        self._add("shuffle", [a, b], [y], half=half)
        return y

    def head(self, x: Sym, yolo_layer):
        self.heads.append((x, yolo_layer))
        self._add("head", [x], [])

