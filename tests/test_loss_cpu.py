"""CPU-only checks of the validation loss (compute_loss / build_targets, csrc/loss.hip): the numpy restatement of tests/_loss.py against
the reference's own answers (tests/golden/loss.npz, captured by tests/golden/make_golden_loss.py), the conditions on the generated
inputs, the three C entry points (declared, exported, argument errors without a device), the host-side refusals of the Python entry
points, and the reference's box helpers (bbox_iou, wh_iou, xyxy2xywh), which are plain tensor code and run here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _loss as L
from helpers import load_golden
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_loss_workspace_bytes", "yolo_build_targets_fwd", "yolo_loss_fwd")


def golden_assignment(g, name, nl):
    return [{k: g[f"{name}_L{i}_{k}"] for k in ("b", "a", "gj", "gi", "tcls", "txy", "twh")} for i in range(nl)]


@pytest.mark.parametrize("name", list(L.CASES))
def test_restatement_vs_golden(name):
    g = load_golden("loss")
    layers, p, targets, cw, nc, bs = L.case_inputs(name)
    assert np.array_equal(targets, g[f"{name}_targets"]), "the target generator drifted"
    for i, t in enumerate(p):
        assert float(t.astype(np.float64).sum()) == float(g[f"{name}_p{i}_sum"]), f"the generator of p drifted (layer {i})"
    items, asg, n_bad = L.compute_loss(p, targets, layers, L.HYPER, nc, cw)
    assert n_bad == 0
    worst = L.assert_assignment(asg, golden_assignment(g, name, len(layers)), f"case {name}: restatement vs reference", txy_exact=False)
    print(f"[loss] case {name}: restatement vs reference, largest relative twh difference {worst:.3e}")
    L.assert_items(items, g[f"{name}_items"], f"case {name}: restatement vs reference")
    if name == "E":
        assert items[0] == items[1] == items[3] == 0.0 and items[2] == items[4] > 0


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_input_conditions(name):
    layers, _, targets, _, nc, bs = L.case_inputs(name)
    L.assert_conditions(L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc), f"case {name}")
    # the generator's fixed targets: 1 repeats 0 (a duplicate cell wherever 0 is kept), 3 fits no anchor
    assert np.array_equal(targets[1, [0, 2, 3, 4, 5]], targets[0, [0, 2, 3, 4, 5]])
    asg = L.build_targets(layers, targets, L.HYPER["iou_thresh"], bs, nc)
    assert not any(A["kept"][3] for A in asg) and any(A["kept"][0] and A["kept"][1] for A in asg)


@pytest.mark.parametrize("geometry", list(L.SWEEP_SEEDS))
def test_sweep_inputs_satisfy_the_conditions(geometry):
    for k in range(len(L.SWEEP_SEEDS[geometry])):
        layers, _, targets, _, nc, bs, seed = L.sweep_inputs(geometry, k)
        L.assert_conditions(L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc), f"sweep {geometry}{k} (seed {seed})")


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "utils/utils.py:99-197" in text
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # no new struct, no changed meaning
    assert [_lib.load().yolo_abi_sizeof(i) for i in range(5)] == [ctypes.sizeof(_lib.YoloConvDesc), ctypes.sizeof(_lib.YoloOp),
                                                                 ctypes.sizeof(_lib.YoloMbconvDesc), ctypes.sizeof(_lib.YoloPipeStep), -1]
    import pytorch_yolo_amd as pkg
    from pytorch_yolo_amd.utils import utils as U
    for name in ("compute_loss", "build_targets", "wh_iou", "bbox_iou", "xyxy2xywh"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(U, name)


def test_workspace_bytes_monotone():
    base = dict(geom=[(3, 4, 6), (3, 8, 12)], bs=2, nt=40)
    n0 = K.loss_workspace_bytes(**base)
    assert n0 > 0
    # records: 48 bytes per (layer, target); tconf: one byte per row; one float64 partial per workgroup
    assert n0 >= 2 * 40 * 4 * K.LOSS_REC_WORDS + 2 * 3 * (4 * 6 + 8 * 12)
    bigger = [dict(base, bs=64), dict(base, nt=4000), dict(base, geom=base["geom"] + [(3, 16, 24)]), dict(base, geom=[(8, 4, 6), (3, 8, 12)]),
              dict(base, geom=[(3, 40, 6), (3, 8, 12)]), dict(base, geom=[(3, 4, 60), (3, 8, 12)])]
    for kw in bigger:
        assert K.loss_workspace_bytes(**kw) > n0, kw
    for kw in (dict(base, bs=3), dict(base, nt=41), dict(base, geom=[(3, 4, 7), (3, 8, 12)])):
        assert K.loss_workspace_bytes(**kw) >= n0, kw
    assert K.loss_workspace_bytes(base["geom"], 2, 0) == K.loss_workspace_bytes(base["geom"], 2, 1) > 0      # nt == 0 is legal


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_argument_errors_without_a_device():
    """Every bad-argument path returns before any launch: fake non-null pointers are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    av = (ctypes.c_float * 32)(*([1.0] * 32))
    gains = (ctypes.c_float * 4)(1, 1, 1, 1)
    heads = (ctypes.c_void_p * 5)(*([0x1000] * 5))
    geo = dict(nl=2, na=_i32(3, 3, 3, 3, 3), ny=_i32(2, 4, 8, 16, 32), nx=_i32(3, 6, 12, 24, 48))
    big = 1 << 30

    def loss(p=heads, targets=fake, nt=4, nl=None, na=None, ny=None, nx=None, anchors=av, bs=2, nc=3, g=gains, ws=fake, ws_bytes=big,
             out=fake, status=fake):
        pick = lambda v, k: geo[k] if v is None else v
        return lib.yolo_loss_fwd(p, targets, nt, pick(nl, "nl"), pick(na, "na"), pick(ny, "ny"), pick(nx, "nx"), anchors, bs, nc, 0.2, g, None,
                                 ws, ws_bytes, out, status, None)

    def targets(t=fake, nt=4, nl=None, na=None, anchors=av, bs=2, nc=3, ws=fake, ws_bytes=big):
        return lib.yolo_build_targets_fwd(t, nt, geo["nl"] if nl is None else nl, geo["na"] if na is None else na, geo["ny"], geo["nx"],
                                          anchors, bs, nc, 0.2, ws, ws_bytes, None)

    def expect(rc, code, pattern):
        msg = lib.yolo_last_error().decode()
        assert rc == code and re.search(pattern, msg), (rc, msg)

    none_f = ctypes.POINTER(ctypes.c_float)()
    none_i = ctypes.POINTER(ctypes.c_int32)()
    none_p = ctypes.POINTER(ctypes.c_void_p)()
    for call in (lambda: loss(p=none_p), lambda: loss(targets=None), lambda: loss(anchors=none_f), lambda: loss(g=none_f), lambda: loss(ws=None),
                 lambda: loss(out=None), lambda: loss(status=None), lambda: targets(t=None), lambda: targets(anchors=none_f),
                 lambda: targets(ws=None)):
        expect(call(), -1, "null pointer")
    expect(loss(na=none_i), -1, "null geometry")
    expect(loss(p=(ctypes.c_void_p * 5)(0x1000, 0, 0, 0, 0)), -1, "null head tensor of layer 1")
    for bad_nl in (0, 5):
        expect(loss(nl=bad_nl), -1, rf"{bad_nl} YOLO layers not in \[1, 4\]")
        expect(targets(nl=bad_nl), -1, rf"{bad_nl} YOLO layers not in \[1, 4\]")
        assert lib.yolo_loss_workspace_bytes(bad_nl, geo["na"], geo["ny"], geo["nx"], 2, 4) == 0
    expect(loss(na=_i32(3, 9)), -1, r"layer 1 has 9 anchors, not in \[1, 8\]")
    expect(targets(na=_i32(9, 3)), -1, r"layer 0 has 9 anchors")
    expect(loss(nt=-1), -1, "negative target count -1")
    expect(targets(nt=-1), -1, "negative target count -1")
    expect(loss(bs=0), -1, "bad batch size")
    need = lib.yolo_loss_workspace_bytes(2, geo["na"], geo["ny"], geo["nx"], 2, 4)
    assert need == K.loss_workspace_bytes([(3, 2, 3), (3, 4, 6)], 2, 4)
    expect(loss(ws_bytes=need - 1), -3, rf"workspace {need - 1} < {need} bytes")
    expect(targets(ws_bytes=need - 1), -3, rf"workspace {need - 1} < {need} bytes")
    with pytest.raises(RuntimeError, match="YOLO layers not in"):
        K.loss_workspace_bytes([(3, 2, 2)] * 5, 1, 1)


def test_compute_loss_refusals_on_the_host():
    from pytorch_yolo_amd.utils.utils import build_targets, compute_loss
    layers, p, targets, _, nc, bs = L.case_inputs("A")
    pt = [torch.from_numpy(t) for t in p]
    tt = torch.from_numpy(targets)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only \\(no CPU fallback\\)"):
        compute_loss(pt, tt, L.namespace_model(layers, nc))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_targets(L.namespace_model(layers, nc), tt)
    for hyper in (None, {k: v for k, v in L.HYPER.items() if k != "wh_loss"}):
        for call in (lambda m: compute_loss(pt, tt, m), lambda m: build_targets(m, tt)):
            with pytest.raises(ValueError) as e:
                call(L.namespace_model(layers, nc, hyper=hyper))
            assert all(k in str(e.value) for k in L.HYPER_KEYS)
    sig = inspect.signature(compute_loss)
    assert list(sig.parameters) == ["p", "targets", "model", "class_weight", "check"]
    assert sig.parameters["class_weight"].default is None and sig.parameters["check"].default is True
    assert list(inspect.signature(build_targets).parameters)[:2] == ["model", "targets"]
    # a model that has not run forward: the mirror's YOLOLayer still holds the int 0 where the grid attributes go
    from pytorch_yolo_amd import YOLOv3Tiny
    import _cases as C
    model = YOLOv3Tiny(n_class=3, kernels_divider=8, anchors=C.TINY_ANCHORS, hyper_params=dict(L.HYPER)).eval()
    with pytest.raises(RuntimeError, match="run the model"):
        build_targets(model, tt)


def test_box_helpers_vs_golden():
    from pytorch_yolo_amd.utils.utils import bbox_iou, wh_iou, xywh2xyxy, xyxy2xywh
    g = load_golden("loss")
    box = torch.from_numpy(g["box_xyxy"].copy())
    xywh = xyxy2xywh(box)
    assert xywh.dtype == torch.float32 and np.array_equal(xywh.numpy(), g["xyxy2xywh"])
    assert np.array_equal(xyxy2xywh(g["box_xyxy"].copy()), g["xyxy2xywh"])                     # the numpy branch of the reference
    assert np.array_equal(torch.stack([bbox_iou(b, box) for b in box]).numpy(), g["bbox_iou_xyxy"])
    assert np.array_equal(torch.stack([bbox_iou(b, xywh, x1y1x2y2=False) for b in xywh]).numpy(), g["bbox_iou_xywh"])
    assert np.array_equal(torch.stack([wh_iou(b, xywh[:, 2:4]) for b in xywh[:, 2:4]]).numpy(), g["wh_iou"])
    assert list(inspect.signature(bbox_iou).parameters) == ["box1", "box2", "x1y1x2y2"] and inspect.signature(bbox_iou).parameters["x1y1x2y2"].default is True
    assert list(inspect.signature(wh_iou).parameters) == ["box1", "box2"] and list(inspect.signature(xyxy2xywh).parameters) == ["x"]
    # known answers: a box with itself, a nested box, disjoint boxes; the round trip through xywh2xyxy
    iou = g["bbox_iou_xyxy"]
    assert abs(iou[0, 0] - 1.0) < 1e-6 and iou[0, 4] == 0.0 and abs(iou[5, 2] - 18 * 18 / 40000.0) < 1e-7
    assert np.allclose(xywh2xyxy(xywh).numpy(), g["box_xyxy"], rtol=0, atol=1e-4)
    # the layer_ious of the restatement is wh_iou
    layers, _, targets, _, _, _ = L.case_inputs("A")
    for Ly in layers:
        gwh = torch.from_numpy(targets[:, 4:6] * np.asarray([Ly["nx"], Ly["ny"]], dtype=np.float32))
        want = torch.stack([wh_iou(x, gwh) for x in torch.from_numpy(Ly["anchor_vec"])]).numpy()
        assert np.array_equal(L.layer_ious(Ly, targets), want)


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def detect(self, imgs, conf, nms, nms_style="MERGE"):
        self.calls.append((tuple(imgs.shape), conf, nms, nms_style))
        return [None] * imgs.shape[0]


def test_predict_dataset_default_is_unchanged():
    from pytorch_yolo_amd.utils.utils import predict_dataset
    params = inspect.signature(predict_dataset).parameters
    assert list(params)[-1] == "loss" and params["loss"].default is False
    model = _StubModel().train()
    batches = [(torch.zeros(2, 3, 32, 32), torch.zeros(0, 6), ["a", "b"], [(32, 32)] * 2), (torch.zeros(1, 3, 32, 32), None, ["c"], [(32, 32)])]
    data = predict_dataset(model, batches, 0.3, 0.4)
    assert isinstance(data, dict) and data == {}
    assert model.calls == [((2, 3, 32, 32), 0.3, 0.4, "MERGE"), ((1, 3, 32, 32), 0.3, 0.4, "MERGE")] and model.training
