"""YOLOv3-tiny head on a ShuffleNetV2 x1.0 encoder — host mirror of reference models/yolov3_tiny_shuffle.py
(SURVEY.md 8f rank 4).

The reference takes the encoder from torchvision (``shufflenet_v2_x1_0(True)``, yolov3_tiny_shuffle.py:3,13-47), which
is not installed here and whose pretrained weights need a download.  The encoder below restates the published
ShuffleNetV2 x1.0 (Ma et al. 2018; torchvision layer order and ``state_dict`` key names
``features.sequence1.{0,2,3}...`` / ``features.sequence2.{0,1}...``) with random initialisation; load real weights with
``load_state_dict``.  The split (conv1, maxpool, stage2, stage3 | stage4, conv5) and the tiny-style head follow the
reference (:28-35, :58-69).

On the device the stage widths 116 / 232 / 464 split into halves of 58 / 116 / 232 channels, and 58 and 116 are not
multiples of the 8-channel (16-byte) granule of the NHWC views.  The trace therefore runs in a padded physical space:
a unit's output keeps its two halves in two slots of 64 / 128 / 256 physical channels (multiples of 32, which also
keeps every conv on the fast LDS-DMA path); the weights recorded for every
conv are the logical ones scattered into that space (zero rows, columns and biases for the pad channels, which ReLU
and the linear depthwise stage keep at zero), the stride-1 split ``x.chunk(2)`` is two channel views, and
``channel_shuffle(cat(a, b), 2)`` is one copy kernel (``yolo_channel_shuffle2_fwd``).  graph.Recorder's ``conv_bn_relu``,
``shuffle_unit`` and ``conv_block_mapped`` hold that layout; models/train.ShuffleTracer has the same names and trains the
model in it.
"""
from __future__ import annotations

from torch import nn

from .. import engine
from ..graph import shuffle_slot
from ..utils.torch_utils import fold_conv_bn
from . import train as T
from .yolo_base import ConvBlock, YOLOBase
from .yolo_layer import Concat, Upsample

_STAGES = ((4, 116), (8, 232), (4, 464))


def _folded(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    return fold_conv_bn(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


class _ConvBNReLU(nn.Sequential):
    def __init__(self, cin, cout, k, stride):
        super().__init__(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class _MaxPool321(nn.MaxPool2d):
    pass


class InvertedResidual(nn.Module):
    """torchvision.models.shufflenetv2.InvertedResidual: children ``branch1`` / ``branch2`` with the same indices."""

    def __init__(self, inp, oup, stride):
        super().__init__()
        self.stride, bf = stride, oup // 2
        if stride > 1:
            self.branch1 = nn.Sequential(nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False), nn.BatchNorm2d(inp),
                                         nn.Conv2d(inp, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))
        else:
            self.branch1 = nn.Sequential()
        cin2 = inp if stride > 1 else bf
        self.branch2 = nn.Sequential(nn.Conv2d(cin2, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True),
                                     nn.Conv2d(bf, bf, 3, stride, 1, groups=bf, bias=False), nn.BatchNorm2d(bf),
                                     nn.Conv2d(bf, bf, 1, 1, 0, bias=False), nn.BatchNorm2d(bf), nn.ReLU(inplace=True))
        self.bf = bf

    def _trace(self, g, x, in_map):
        """x: the physical tensor, in_map[i] = physical channel of logical input channel i.  Returns (y, map of y)."""
        return g.shuffle_unit(self, x, in_map)


class ShuffleEncoder(nn.Module):
    """sequence1 = (conv1, maxpool, stage2, stage3) -> 232 ch @/16, sequence2 = (stage4, conv5) -> 1024 ch @/32
    (yolov3_tiny_shuffle.py:13-47)."""

    def __init__(self, in_channels=3):
        super().__init__()
        stages, inp = [], 24
        for rep, oup in _STAGES:
            stages.append(nn.Sequential(*[InvertedResidual(inp if u == 0 else oup, oup, 2 if u == 0 else 1) for u in range(rep)]))
            inp = oup
        self.sequence1 = nn.Sequential(_ConvBNReLU(in_channels, 24, 3, 2), _MaxPool321(3, 2, 1), stages[0], stages[1])
        self.sequence2 = nn.Sequential(stages[2], _ConvBNReLU(464, 1024, 1, 1))

    @property
    def out_channels(self):
        return 232, 1024

    def _trace(self, g, x):
        """Returns (route1 physical tensor, its channel map, route2)."""
        c1 = self.sequence1[0]
        cmap = list(range(24))
        x = g.conv_bn_relu(c1, x, list(range(c1[0].in_channels)), shuffle_slot(24))    # 24 real channels in a 32-channel tensor
        x = g.maxpool(x, 3, 2)
        for stage in (self.sequence1[2], self.sequence1[3]):
            for unit in stage:
                x, cmap = unit._trace(g, x, cmap)
        route1, map1 = x, cmap
        for unit in self.sequence2[0]:
            x, cmap = unit._trace(g, x, cmap)
        route2 = g.conv_bn_relu(self.sequence2[1], x, cmap, 1024)
        return route1, map1, route2


class YOLOv3TinyShuffle(YOLOBase):
    # trains through pytorch_yolo_amd.forward_train(model, x, ops=DEVICE_OPS_SHUFFLE) only: with ops=None forward_train keeps raising what
    # it raised before the class had a wiring, and so does model.train()(x) (the flip is the one-line follow-up of 3.6k)
    _train_in_forward = False
    _train_ops_by_name = True         # the caller names the table: forward_train(model, x) without one refuses this class
    _train_tracer = T.ShuffleTracer   # conv_bn_relu, shuffle_unit and conv_block_mapped beside TrainTracer's vocabulary
    _train_ops = T.DEVICE_OPS_SHUFFLE
    _train_wiring = T.wiring          # training runs the same _trace on the ops of a table (models/train.py)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        kd = self.kernels_divider
        wd = lambda c: max(8, c // kd)
        out = self.yolo_layer_input_size
        self.features = ShuffleEncoder(in_channels=self.in_channels)
        f1, f2 = self.features.out_channels

        b11 = nn.Sequential()
        b11.add_module("branch1_conv1", ConvBlock(f2, wd(128), size=1))
        b11.add_module("branch1_upsample", Upsample(2))
        self.sequence_branch1_1 = b11

        b12 = nn.Sequential()
        b12.add_module("branch1_concat", Concat(1))
        b12.add_module("branch1_conv2", ConvBlock(f1 + wd(128), wd(128)))
        b12.add_module("branch1_conv3", nn.Conv2d(wd(128), out, kernel_size=1))
        self.sequence_branch1_2 = b12

        b2 = nn.Sequential()
        b2.add_module("branch2_conv1", ConvBlock(f2, wd(128)))
        b2.add_module("branch2_conv2", nn.Conv2d(wd(128), out, kernel_size=1))
        self.sequence_branch2 = b2

        self.yolo1, self.yolo2 = self._create_yolo_layers()

    @property
    def yolo_layers(self):
        return self.yolo1, self.yolo2

    def _trace(self, g: engine.Recorder, x):
        """Reference _forward_encoder + forward (yolov3_tiny_shuffle.py:79-110)."""
        route1, map1, route2 = self.features._trace(g, x)
        b = self.sequence_branch1_1.branch1_conv1._trace(g, route2)
        cat = g.upsample_concat(b, route1, up_first=False)               # [x_route1, x_branch1] (:83)
        n_route1, n_up = cat.shape[1] - b.shape[1], b.shape[1]           # (physical channels of the two parts)
        cmap = map1 + [n_route1 + i for i in range(n_up)]
        b1 = g.conv_block_mapped(self.sequence_branch1_2.branch1_conv2, cat, cmap)   # its weights see 232 + 128 logical channels
        g.head(g.plain_conv(self.sequence_branch1_2.branch1_conv3, b1), self.yolo1)
        b2 = self.sequence_branch2.branch2_conv1._trace(g, route2)
        g.head(g.plain_conv(self.sequence_branch2.branch2_conv2, b2), self.yolo2)
