"""The dense conv kernels one full-size training step of YOLOv3-tiny/MobileNetV2 selects, in the style of
tests/_train_fire_families.py: the step is recorded on ``meta`` tensors through the model's own wiring, every dense conv call becomes the
descriptors ops._desc / yolo_conv2d_bwd_data build, and every (role, family) the step selects is in tests/_train_families.FAMILY_CASES,
in tests/_train_fire_families.FIRE_FAMILY_CASES, or has a case in MOBILE_FAMILY_CASES below (tests/test_train_mobile_cpu.py keeps that
complete, tests/test_train_mobile_gpu.py launches the cases).  The depthwise convs are not dense convs: their kernels have one form each
(tests/_dw_train.CASES).

What differs from the other configurations: the 1x1 convs of the inverted residuals - expands with K = 16 ... 160 and 96 ... 960 output
channels, linear bottlenecks with K = 32 ... 960 and 16 ... 320 output channels, on maps from 208 x 208 down to 13 x 13 -, the 3x3
stride-2 first layer with 32 output channels and the 320 -> 1280 last layer.
"""
import collections
from types import SimpleNamespace

import torch

import _dw_train as D
import _train_families as TF
import _train_fire_families as FF

BF16, F32 = torch.bfloat16, torch.float32
CONFIG = ("YOLOv3TinyMobile", 416, 32)          # class, input size, batch: full width, nc = 80


def recording_meta_ops(calls):
    """tests/_train_families.recording_meta_ops plus the four functions of DEVICE_OPS_MOBILE.  A dense conv records (kind, x shape, weight
    shape, stride, x requires a gradient); the fused op records its expand conv; a depthwise conv records ("dw", x shape, weight shape,
    stride, True), which enumerate_step leaves out."""
    base = TF.recording_meta_ops(calls)

    def out(x, c, h, w):
        return torch.empty((x.shape[0], c, h, w), dtype=BF16, device="meta")

    def conv_bn_relu6_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        calls.append(("relu6", tuple(x.shape), tuple(w.shape), stride, len(calls) > 0))
        return out(x, w.shape[0], *D.out_hw(x.shape[2], x.shape[3], stride))

    def dw_bn_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, act="relu6", momentum=0.1, eps=1e-5, training=True):
        calls.append(("dw", tuple(x.shape), tuple(w.shape), stride, True))
        return out(x, x.shape[1], *D.out_hw(x.shape[2], x.shape[3], stride))

    def project_bn_block(x, w, gamma, beta, rm=None, rv=None, residual=None, *, momentum=0.1, eps=1e-5, training=True):
        calls.append(("project", tuple(x.shape), tuple(w.shape), 1, True))
        return out(x, w.shape[0], x.shape[2], x.shape[3])

    def expand_dw_bn_block(x, we, gamma1, beta1, rm1, rv1, wd, gamma2, beta2, rm2, rv2, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        calls.append(("expand", tuple(x.shape), tuple(we.shape), 1, True))
        calls.append(("dw", (x.shape[0], we.shape[0]) + tuple(x.shape[2:]), tuple(wd.shape), stride, True))
        return out(x, we.shape[0], *D.out_hw(x.shape[2], x.shape[3], stride))

    return SimpleNamespace(**vars(base), conv_bn_relu6_block=conv_bn_relu6_block, dw_bn_block=dw_bn_block, project_bn_block=project_bn_block,
                           expand_dw_bn_block=expand_dw_bn_block)


def record_step():
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    cls, size, bs = CONFIG
    model = getattr(Y, cls)(n_class=80).to("meta").train()
    calls = []
    p = MT.forward_train(model, torch.empty((bs, 3, size, size), dtype=F32, device="meta"), ops=recording_meta_ops(calls))
    assert len(p) == 2 and all(t.shape[0] == bs and t.shape[-1] == 85 for t in p)
    return calls


def enumerate_step():
    """Counter of (role, family) over the dense conv calls of the step, the calls as [(kind, (n, h, w, cin, cout, k), stride, {role:
    family})], and the depthwise calls as [(n, h, w, c, stride)]."""
    count, rows, dws = collections.Counter(), [], []
    for kind, xs, ws, stride, need_dx in record_step():
        n, cin, h, w = xs
        if kind == "dw":
            dws.append((n, h, w, cin, stride))
            continue
        cout, _, k, _ = ws
        p = TF.picks_of(TF.forward_desc(n, h, w, cin, cout, k, stride, kind == "head"), need_dx)
        count.update(p.items())
        rows.append((kind, (n, h, w, cin, cout, k), stride, p))
    return count, rows, dws


def known(key):
    return key in TF.FAMILY_CASES or key in TF.OTHER_FAMILIES or key in FF.FIRE_FAMILY_CASES or key in FF.OTHER_FAMILIES


# ---- the cases of the (role, family) pairs that the two sibling tables do not hold -----------------------------------------------------------
# A case is TF._c's dict; the sibling's rule for a new one: the cheapest layer with the step's own (cin, cout, k) that selects the family, on
# a 5 x 7 map where it can, with more than one pixel tile and a partial last one (TF.partial_and_two_k_steps where the layer's K allows two
# steps).  On 256 compute units enumerate_step() selects no (role, family) outside the two sibling tables and their OTHER_FAMILIES - the
# 1x1 convs of the inverted residuals land in the igemm and stream1x1 families the Darknet and SqueezeNet steps already use -, so the
# table is empty; tests/test_train_mobile_cpu.py fails when a change of the dispatch rule makes that untrue.
MOBILE_FAMILY_CASES = {}
CASES = list({id(c): c for c in MOBILE_FAMILY_CASES.values()}.values())
