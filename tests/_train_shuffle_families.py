"""The dense conv kernels one full-size training step of YOLOv3-tiny/ShuffleNetV2 selects, in the style of
tests/_train_mobile_families.py: the step is recorded on ``meta`` tensors through the model's own wiring, every dense conv call becomes the
descriptors ops._desc / yolo_conv2d_bwd_data build, and every (role, family) the step selects is in tests/_train_families.FAMILY_CASES, in
tests/_train_fire_families.FIRE_FAMILY_CASES, in their OTHER_FAMILIES, or has a case in SHUFFLE_FAMILY_CASES below
(tests/test_train_shuffle_cpu.py keeps that complete, tests/test_train_shuffle_gpu.py launches the cases).  The depthwise convs are not dense
convs: their kernels have one form each (tests/_dw_train.CASES).

What differs from the other configurations: the step runs in the padded physical space of the eval trace - 1x1 convs with 64 / 128 / 256
output channels on maps from 52 x 52 down to 13 x 13, K = 32 ... 512 -, and the first 1x1 conv of a fused stride-1 unit reads slot 1 of
its two-slot input as a channel view: its descriptor has ``in_c_total = 2 slot`` and ``in_c_offset = slot``, and its data gradient writes
that view.
"""
import collections
from types import SimpleNamespace

import torch

import _dw_train as D
import _train_families as TF
import _train_fire_families as FF

BF16, F32 = torch.bfloat16, torch.float32
CONFIG = ("YOLOv3TinyShuffle", 416, 32)          # class, input size, batch: full width, nc = 80


def recording_meta_ops(calls):
    """tests/_train_families.recording_meta_ops plus the five functions of DEVICE_OPS_SHUFFLE.  A dense conv records (kind, x shape, weight
    shape, stride, x requires a gradient[, (channels of the input buffer, offset of the view)]); the fused unit records its two 1x1
    convs, the first with its input view; a depthwise conv records ("dw", ...), which enumerate_step keeps apart."""
    base = TF.recording_meta_ops(calls)

    def out(x, c, h, w):
        return torch.empty((x.shape[0], c, h, w), dtype=BF16, device="meta")

    def conv_bn_relu_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, momentum=0.1, eps=1e-5, training=True):
        calls.append(("relu", tuple(x.shape), tuple(w.shape), stride, len(calls) > 0))
        return out(x, w.shape[0], *D.out_hw(x.shape[2], x.shape[3], stride))

    def dw_bn_block(x, w, gamma, beta, rm=None, rv=None, *, stride=1, act="relu6", momentum=0.1, eps=1e-5, training=True):
        assert act == "none"
        calls.append(("dw", tuple(x.shape), tuple(w.shape), stride, True))
        return out(x, x.shape[1], *D.out_hw(x.shape[2], x.shape[3], stride))

    def max_pool_321(x):
        calls.append(("pool321", tuple(x.shape), (), 2, True))
        return out(x, x.shape[1], *D.out_hw(x.shape[2], x.shape[3], 2))

    def channel_shuffle2(a, b, half):
        assert a.shape == b.shape
        calls.append(("shuffle", tuple(a.shape), (), 1, True))
        return out(a, 2 * a.shape[1], a.shape[2], a.shape[3])

    def shuffle_unit_block(x, half, w1, gamma1, beta1, rm1, rv1, wd, gamma2, beta2, rm2, rv2, w3, gamma3, beta3, rm3, rv3, *, momentum=0.1,
                           eps=1e-5):
        n, c2, h, w = x.shape
        slot = c2 // 2
        calls.append(("unit_pw1", (n, slot, h, w), tuple(w1.shape), 1, True, (c2, slot)))
        calls.append(("dw", (n, slot, h, w), tuple(wd.shape), 1, True))
        calls.append(("unit_pw2", (n, slot, h, w), tuple(w3.shape), 1, True))
        return out(x, c2, h, w)

    return SimpleNamespace(**vars(base), conv_bn_relu_block=conv_bn_relu_block, dw_bn_block=dw_bn_block, max_pool_321=max_pool_321,
                           channel_shuffle2=channel_shuffle2, shuffle_unit_block=shuffle_unit_block)


def record_step(size=None, bs=None, n_class=80):
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    cls, size0, bs0 = CONFIG
    size, bs = size or size0, bs or bs0
    model = getattr(Y, cls)(n_class=n_class).to("meta").train()
    calls = []
    p = MT.forward_train(model, torch.empty((bs, 3, size, size), dtype=F32, device="meta"), ops=recording_meta_ops(calls))
    assert len(p) == 2 and all(t.shape[0] == bs and t.shape[-1] == 5 + n_class for t in p)
    return calls, p


def call_desc(call):
    """ops._desc of a recorded dense conv call: tests/_train_families.forward_desc, with the input view where the call has one."""
    kind, xs, ws, stride, need_dx = call[:5]
    n, cin, h, w = xs
    d = TF.forward_desc(n, h, w, cin, ws[0], ws[2], stride, kind == "head")
    if len(call) > 5:
        d.in_c_total, d.in_c_offset = call[5]
    return d


def enumerate_step():
    """Counter of (role, family) over the dense conv calls of the step, the calls as [(kind, (n, h, w, cin, cout, k), stride, {role:
    family}, input view or None)], and the other calls as [(kind, x shape, stride)]."""
    count, rows, others = collections.Counter(), [], []
    for call in record_step()[0]:
        kind, xs, ws, stride, need_dx = call[:5]
        n, cin, h, w = xs
        if kind in ("dw", "pool321", "shuffle"):
            others.append((kind, (n, h, w, cin), stride))
            continue
        p = TF.picks_of(call_desc(call), need_dx)
        count.update(p.items())
        rows.append((kind, (n, h, w, cin, ws[0], ws[2]), stride, p, call[5] if len(call) > 5 else None))
    return count, rows, others


def known(key):
    return key in TF.FAMILY_CASES or key in TF.OTHER_FAMILIES or key in FF.FIRE_FAMILY_CASES or key in FF.OTHER_FAMILIES


# ---- the cases of the (role, family) pairs that the sibling tables do not hold -----------------------------------------------------------------
# A case is TF._c's dict; the siblings' rule for a new one: the cheapest layer with the step's own (cin, cout, k) that selects the family, on
# a 5 x 7 map where it can, with more than one pixel tile and a partial last one.  tests/test_train_shuffle_cpu.py fails when the step
# selects a pair that neither a sibling table nor this one holds.
# On 256 compute units the step selects one pair outside them: the 128 -> 128 1x1 convs of stage 3's first unit on the 52 x 52 map take the
# streaming 1x1 kernel with K = 128, forward and data gradient (the layer is its own transpose).  The cheapest map that keeps the family is
# _STREAM64's of tests/_train_families.py: 0.66 GMAC, 40341 pixels = 504 strips of 80 and one of 21.
_STREAM128 = TF._c(3, 113, 119, 128, 128, 1)
SHUFFLE_FAMILY_CASES = {
    ("forward", "stream1x1p<128 couts,K 128,80 px>"): _STREAM128,
    ("dgrad", "stream1x1p<128 couts,K 128,80 px>"): _STREAM128,
}
CASES = list({id(c): c for c in SHUFFLE_FAMILY_CASES.values()}.values())
