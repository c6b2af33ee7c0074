"""The conv kernels one full-size training step of YOLOv3-tiny/SqueezeNet selects, in the style of
tests/_train_families.py: the step is recorded on ``meta`` tensors, every conv call becomes the descriptors ops._desc / ops._fire_forward /
yolo_conv2d_bwd_data build, and every (role, family) the step selects is either in tests/_train_families.FAMILY_CASES already or has a
case in FIRE_FAMILY_CASES below (tests/test_train_fire_cpu.py keeps that complete, tests/test_train_fire_gpu.py launches the cases).

What differs from the four configurations of tests/_train_families.py: the convs carry a bias and ReLU (neither changes a pick), the
first layer is the unpadded stride-2 conv (forward and weight gradient only: its input is the image), a Fire module's expand convs
write channel views of the concat map, and the squeeze tensors are 16 to 64 channels wide - a data gradient with 16 ... 64 output
channels, and forwards with K = 16 ... 64 (1x1) and 144 ... 576 (3x3).
"""
import collections
from types import SimpleNamespace

import torch

import _train_families as TF

BF16, F32 = torch.bfloat16, torch.float32
CONFIG = ("YOLOv3TinySqueeze", 416, 32)          # class, input size, batch: full width, nc = 80


def recording_meta_ops(calls):
    """tests/_train_families.recording_meta_ops plus the four functions of DEVICE_OPS_FIRE.  A Fire module records its three convs:
    (kind, x shape, weight shape, stride, x requires a gradient[, (channels of the output buffer, offset)])."""
    base = TF.recording_meta_ops(calls)

    def out(x, c, h, w):
        return torch.empty((x.shape[0], c, h, w), dtype=BF16, device="meta")

    def stem_block(x, w, b=None, *, act="relu"):
        calls.append(("stem", tuple(x.shape), tuple(w.shape), 2, False))
        return out(x, w.shape[0], (x.shape[2] - 3) // 2 + 1, (x.shape[3] - 3) // 2 + 1)

    def fire_block(x, sw, sb, w1, b1, w3, b3):
        n, _, h, w = x.shape
        s = (n, sw.shape[0], h, w)
        total = w1.shape[0] + w3.shape[0]
        calls.append(("fire_squeeze", tuple(x.shape), tuple(sw.shape), 1, True))
        calls.append(("fire_e1", s, tuple(w1.shape), 1, True, (total, 0)))
        calls.append(("fire_e3", s, tuple(w3.shape), 1, True, (total, w1.shape[0])))
        return out(x, total, h, w)

    table = dict(vars(base))
    table.update(stem_block=stem_block, fire_block=fire_block, max_pool_ceil=lambda x: out(x, x.shape[1], x.shape[2] // 2, x.shape[3] // 2),
                 concat=lambda xs: out(xs[0], sum(t.shape[1] for t in xs), xs[0].shape[2], xs[0].shape[3]))
    return SimpleNamespace(**table)


def record_step():
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    cls, size, bs = CONFIG
    model = getattr(Y, cls)(n_class=80).to("meta").train()
    calls = []
    p = MT.forward_train(model, torch.empty((bs, 3, size, size), dtype=F32, device="meta"), ops=recording_meta_ops(calls))
    assert len(p) == 2 and all(t.shape[0] == bs and t.shape[-1] == 85 for t in p)
    return calls


def call_desc(call):
    """The forward descriptor of a recorded call: TF.forward_desc (act none; the act changes no pick), the stem with pad 0, an expand
    conv with its channel view of the concat map."""
    from pytorch_yolo_amd import kernels as K
    kind, xs, ws, stride = call[:4]
    n, cin, h, w = xs
    cout, _, k, _ = ws
    d = TF.forward_desc(n, h, w, cin, cout, k, stride, kind == "head")
    if kind == "stem":
        d = K.conv_desc(n=d.n, h=d.h, w=d.w, cin=d.cin, in_c_total=d.cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=3,
                        stride=2, act=d.act, kpad=d.kpad, cout_pad=d.cout_pad, pad=0)
    if len(call) > 5:
        d.out_c_total, d.out_c_offset = call[5]
    return d


def picks_of(call):
    """{role: family} of one recorded call."""
    from pytorch_yolo_amd import kernels as K
    d = call_desc(call)
    if call[0] == "stem":
        return {"forward": TF.family(K.conv2d_pick(d)), "wgrad": TF.family(K.conv2d_stem_bwd_pick(d))}
    return TF.picks_of(d, call[4])


def enumerate_step():
    """Counter of (role, family) over the conv calls of the step, and the calls as [(kind, (n, h, w, cin, cout, k), stride, {role: family})]."""
    count, rows = collections.Counter(), []
    for call in record_step():
        n, cin, h, w = call[1]
        cout, _, k, _ = call[2]
        p = picks_of(call)
        count.update(p.items())
        rows.append((call[0], (n, h, w, cin, cout, k), call[3], p))
    return count, rows


# ---- the cases of the (role, family) pairs that tests/_train_families.FAMILY_CASES does not hold ----------------------------------------------
# A case is TF._c's dict: a tests/_conv_bwd.py case (act none, plain views), the stride and the tuning words.  FIRE_FAMILY_CASES is filled
# from what enumerate_step() selects on 256 compute units; tests/test_train_fire_cpu.py asserts that nothing is missing.
_M32, _G = TF._M32, TF._G
# The cheapest layer with the step's own (cin, cout, k) that selects the family, by multiply-accumulates, on maps of h x (h + 2) pixels
# with more than one pixel tile and a partial last one (TF.partial_and_two_k_steps; the 1x1 64 -> 256 expand has one 64-channel K step
# whatever the map, and takes its 128x256 tile only from 16,920 pixels on: 0.28 GMAC).
_SQ48_DGRAD = TF._c(4, 5, 7, 256, 48, 1)          # the squeeze 256 -> 48: its data gradient has K = 48, two 32-channel steps
_E1_DGRAD64 = TF._c(2, 5, 7, 64, 256, 1)          # the expand 64 -> 256: its data gradient has 64 output channels
_E1_192 = TF._c(4, 5, 7, 48, 192, 1)
_E3_192 = TF._c(4, 5, 7, 48, 192, 3)              # K = 432: no whole 32-channel chunks per tap
_E1_256 = TF._c(8, 45, 47, 64, 256, 1)            # 0.28
_E3_64 = TF._c(8, 5, 7, 16, 64, 3)                # K = 144
_SQ64 = TF._c(2, 5, 7, 384, 64, 1)

FIRE_FAMILY_CASES = {
    ("dgrad", _M32 % "128x128,2x2 waves,BK32,3 stages"): _SQ48_DGRAD,
    ("dgrad", _G % "64x64,2x2 waves,BK64,4 stages"): _E1_DGRAD64,
    ("forward", _M32 % "128x128,2x2 waves,BK32,3 stages"): _E1_192,
    ("forward", _M32 % "128x128,2x2 waves,BK32,3 stages,generic"): _E3_192,
    ("forward", _G % "128x256,2x8 waves,BK64,3 stages"): _E1_256,
    ("forward", _M32 % "256x64,4x1 waves,BK32,2 stages,generic"): _E3_64,
    ("forward", _G % "64x64,2x2 waves,BK64,4 stages"): _SQ64,
}
CASES = list({id(c): c for c in FIRE_FAMILY_CASES.values()}.values())
# the weight gradient of the unpadded first layer: launched by the stem_block tests of tests/test_train_fire_gpu.py (one of them splits)
OTHER_FAMILIES = TF.OTHER_FAMILIES | {("wgrad", "wgrad<64x128,BK64,tr_b16,s2,p0>")}
