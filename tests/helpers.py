"""Test helpers shared by CPU and GPU suites."""
import os

import numpy as np
import torch

import _cases as C
from pytorch_yolo_amd import LiteYOLOv3, YOLOv3, YOLOv3SPP, YOLOv3Tiny
from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILY = {"spp": YOLOv3SPP, "tiny": YOLOv3Tiny, "yolov3": YOLOv3, "lite": LiteYOLOv3}


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


GOLDEN_THREADS = 8      # torch.set_num_threads() of tests/golden/make_golden.py: the CPU convs sum in a thread-count-dependent order


def arith_fingerprint() -> str:
    """SHA-256 of the bits of seeded fp32 conv / batch-norm / activation / decode ops on this CPU at GOLDEN_THREADS threads: the
    torch CPU arithmetic the oracle runs on, and no oracle code."""
    import hashlib
    import torch.nn.functional as F
    before = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    g = torch.Generator().manual_seed(20261016)
    h = hashlib.sha256()
    try:
        with torch.no_grad():
            for n, cin, cout, hw, k, s in ((1, 3, 32, 64, 3, 1), (2, 32, 64, 40, 3, 2), (1, 64, 128, 20, 3, 1), (2, 128, 64, 26, 1, 1),
                                           (1, 256, 512, 13, 3, 1), (1, 512, 255, 10, 1, 1), (4, 64, 64, 16, 3, 1)):
                x = torch.rand(n, cin, hw, hw, generator=g) - 0.5
                w = (torch.rand(cout, cin, k, k, generator=g) - 0.5) / (cin * k * k) ** 0.5
                y = F.conv2d(x, w, torch.rand(cout, generator=g) - 0.5, stride=s, padding=k // 2)
                y = F.batch_norm(y, torch.rand(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) + 0.5,
                                 torch.rand(cout, generator=g), eps=1e-5)
                h.update(y.numpy().tobytes())
                h.update(F.leaky_relu(y, 0.1).numpy().tobytes())
            v = torch.linspace(-30.0, 30.0, 100003)
            for t in (torch.sigmoid(v), torch.exp(v), F.interpolate(v.view(1, 1, 1, -1), scale_factor=2, mode="nearest"),
                      F.max_pool2d(v[:100000].view(1, 1, 100, 1000), 5, 1, 2)):
                h.update(t.numpy().tobytes())
            io = (torch.rand(2, 3, 13, 13, 85, generator=g) - 0.5) * 20.0      # strided column slices, as in the YOLO decode
            io[..., 0:2] = torch.sigmoid(io[..., 0:2])
            io[..., 2:4] = torch.exp(io[..., 2:4]) * torch.rand(1, 3, 1, 1, 2, generator=g)
            io[..., 4:] = torch.sigmoid(io[..., 4:])
            io[..., :4] *= 32.0
            h.update(io.numpy().tobytes())
    finally:
        torch.set_num_threads(before)
    return h.hexdigest()


_GOLDEN_ARITH = []


def golden_arithmetic() -> bool:
    """True when this CPU computes like the host that recorded the goldens (tests/golden/host_arithmetic.json): the oracle tests then
    require bit-equality with them.  Elsewhere the reference itself would give other bits, and they use bounds measured for that."""
    if not _GOLDEN_ARITH:
        import json
        with open(os.path.join(GOLDEN, "host_arithmetic.json")) as f:
            want = json.load(f)["fingerprint"]
        _GOLDEN_ARITH.append(arith_fingerprint() == want)
    return _GOLDEN_ARITH[0]


def build_case(case):
    """(product model in eval mode with seeded weights, state_dict, input x) for a MODEL/FULL case tuple."""
    family, kw, bs, h, w, wseed, xseed = case
    model = FAMILY[family](**kw).eval()
    sd = synth_state_dict(model.state_dict(), wseed, n_class=kw["n_class"])
    model.load_state_dict(sd)
    return model, sd, synth_images(bs, h, w, xseed)


def oracle_forward(case, sd, x):
    from oracle import models as om
    family, kw = case[0], case[1]
    fwd = {"spp": om.spp_forward, "tiny": om.tiny_forward, "yolov3": om.yolov3_forward, "lite": om.lite_forward}[family]
    with torch.no_grad():
        return fwd(sd, x, kw["anchors"], kw["n_class"])


def build_separable_case():
    """(product YOLOv3-SPP in eval mode, state_dict, x) of tests/_cases.py::SEPARABLE: seeded weights with the head BN arrays
    the golden stores (calibrated by make_golden.py from the reference's own raw head outputs), the seeded patch image."""
    sep = C.SEPARABLE
    g = load_golden("full_spp_640_separable")
    model = YOLOv3SPP(n_class=80, kernels_divider=1, anchors=C.SPP_ANCHORS).eval()
    sd = synth_state_dict(model.state_dict(), sep["weight_seed"], n_class=80)
    for k, h in enumerate(C.SEPARABLE_HEADS):
        sd[h + ".sequence.batch_norm.weight"] = torch.from_numpy(g[f"head_bn_weight_{k}"].copy())
        sd[h + ".sequence.batch_norm.bias"] = torch.from_numpy(g[f"head_bn_bias_{k}"].copy())
    model.load_state_dict(sd)
    return model, sd, torch.from_numpy(C.patch_image(sep["image_seed"], sep["n_patches"])), g


def build_rule_case(seed: int):
    """(product YOLOv3-SPP in eval mode, state_dict, x, golden) of one rule-selected case (tests/_cases.py::RULE, RULE_SEEDS): seeded
    weights with the head BN arrays the golden stores (calibrated by make_golden.py from the reference's own raw head outputs)."""
    rule = C.RULE
    g = load_golden(f"full_spp_640_rule_{seed}")
    model = YOLOv3SPP(n_class=80, kernels_divider=1, anchors=C.SPP_ANCHORS).eval()
    sd = synth_state_dict(model.state_dict(), rule["weight_seed"], n_class=80)
    for k, h in enumerate(C.SEPARABLE_HEADS):
        sd[h + ".sequence.batch_norm.weight"] = torch.from_numpy(g[f"head_bn_weight_{k}"].copy())
        sd[h + ".sequence.batch_norm.bias"] = torch.from_numpy(g[f"head_bn_bias_{k}"].copy())
    model.load_state_dict(sd)
    return model, sd, torch.from_numpy(C.patch_image(seed, rule["n_patches"])), g


def box_iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter + 1e-16)


def strict_share(da, db, iou_min=0.9, dconf=0.03):
    """Share of the detections [n, 7] in ``da`` that have a partner in ``db``: same class, IoU >= iou_min, |dconf| <= dconf."""
    if da is None or len(da) == 0:
        return 1.0
    if db is None or len(db) == 0:
        return 0.0
    return sum(any(int(r[6]) == int(q[6]) and abs(float(r[4]) - float(q[4])) <= dconf and box_iou(r[:4], q[:4]) >= iou_min
                   for q in db) for r in da) / len(da)
