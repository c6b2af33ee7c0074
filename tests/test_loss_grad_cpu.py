"""CPU-only checks of the gradient of compute_loss (yolo_loss_bwd, csrc/loss.hip): the float64 restatement of tests/_loss_grad.py against
the reference's own ``loss.backward()`` (tests/golden/loss_grad.npz, captured by tests/golden/make_golden_loss_grad.py), the new C
entry point (declared, exported, argument errors without a device), the workspace size (unchanged) and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _loss as L
import _loss_grad as LG
from helpers import load_golden
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(L.CASES))
def test_restatement_vs_golden(name):
    gold = load_golden("loss_grad")
    layers, p, targets, cw, nc, bs = L.case_inputs(name)
    assert np.array_equal(gold[f"{name}_items"], load_golden("loss")[f"{name}_items"]), "captured from another call than loss.npz"
    want, asg = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw)
    ref = LG.golden_grads(gold, name, [t.shape for t in p], asg)
    ref_err = LG.golden_ref_err(gold, name, len(layers))
    errs = LG.assert_grads(ref, want, f"case {name}: reference vs restatement", ref_err)
    assert np.allclose(errs, ref_err, rtol=1e-4, atol=1e-12), "the restatement drifted from the one the golden file was captured with"
    assert float(ref_err.max()) <= 7.9e-7                                      # the reference's own error, far below the bar
    for i, (g, w, A) in enumerate(zip(ref, want, asg)):
        assert [a.shape for a in (g, w)] == [p[i].shape] * 2 and w.dtype == np.float64
        assert np.array_equal(g != 0, w != 0), f"case {name} layer {i}: the zero patterns differ"
        LG.assert_structure(g, A, f"case {name} layer {i}: reference")
        LG.assert_structure(w.astype(np.float32), A, f"case {name} layer {i}: restatement")
    if name == "E":
        assert all(not g[..., :4].any() and not g[..., 5:].any() for g in want)


def test_restatement_vs_float64_autograd():
    """The restatement against float64 torch autograd of the loss written out with torch.nn.functional (cases A, B, C: nc > 1,
    nc == 1, weighted), with an upstream gradient of -3."""
    F = torch.nn.functional
    for name in ("A", "B", "C"):
        layers, p, targets, cw, nc, bs = L.case_inputs(name)
        want, asg = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw, G=-3.0)
        gain = {k: float(L.F32(bs * L.HYPER[k])) for k in ("xy_loss", "wh_loss", "cls_loss", "conf_loss")}
        total = 0.0
        pt = [torch.from_numpy(t).double().requires_grad_() for t in p]
        for x, A in zip(pt, asg):
            assert len(A["b"])
            tconf = torch.zeros(x.shape[:4], dtype=torch.float64)
            idx = tuple(torch.from_numpy(A[k]) for k in ("b", "a", "gj", "gi"))
            tconf[idx] = 1.0
            pi = x[idx]
            tc = torch.from_numpy(A["tcls"])
            if nc > 1:
                cls = F.cross_entropy(pi[:, 5:], tc, weight=None if cw is None else torch.from_numpy(cw).double())
            else:
                cls = F.binary_cross_entropy_with_logits(pi[:, 5], tc.double())
            total = (total + gain["xy_loss"] * F.mse_loss(torch.sigmoid(pi[:, 0:2]), torch.from_numpy(A["txy"]).double())
                     + gain["wh_loss"] * F.mse_loss(pi[:, 2:4], torch.from_numpy(A["twh"]).double()) + gain["cls_loss"] * cls
                     + gain["conf_loss"] * F.binary_cross_entropy_with_logits(x[..., 4], tconf))
        (-3.0 * total).backward()
        for i, (x, w) in enumerate(zip(pt, want)):
            assert np.allclose(x.grad.numpy(), w, rtol=1e-11, atol=1e-14), f"case {name} layer {i}"


def test_group_errors_measure():
    g64 = np.zeros((1, 1, 2, 2, 8))
    g64[..., 4] = 0.5
    g64[0, 0, 0, 0, 0] = 2.0
    g = g64.copy()
    g[0, 0, 1, 1, 1] = 1e-3                          # an xy element off by 1e-3 where the group's largest is 2.0
    assert np.allclose(LG.group_errors(g, g64), [5e-4, 0, 0, 0])
    with pytest.raises(AssertionError, match="xy differs by 5.000e-04"):
        LG.assert_grads([g], [g64], "measure")
    g[0, 0, 1, 1, 1] = 0.0
    g[0, 0, 0, 0, 6] = 1e-30                         # a class group that must be all zero
    assert LG.group_errors(g, g64)[3] == np.inf
    with pytest.raises(AssertionError, match="class differs"):
        LG.assert_grads([g], [g64], "measure")


def test_symbol_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert declared.count("yolo_loss_bwd") == 1 and "yolo_loss_bwd" in _lib.SIGNATURES and hasattr(lib, "yolo_loss_bwd")
    fwd, bwd = _lib.SIGNATURES["yolo_loss_fwd"], _lib.SIGNATURES["yolo_loss_bwd"]
    assert bwd[0] is fwd[0] and bwd[1][:15] == fwd[1][:15] and len(bwd[1]) == len(fwd[1])      # out, status -> grad_loss, grad_p
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2                            # additive: no struct, no new version
    import pytorch_yolo_amd as pkg
    from pytorch_yolo_amd.utils import utils as U
    assert "loss_grad_raw" in pkg.__all__ and pkg.loss_grad_raw is U.loss_grad_raw and "loss_bwd" in K.__all__
    assert list(inspect.signature(U.loss_grad_raw).parameters) == ["p", "targets", "model", "class_weight", "grad_loss", "workspace", "out"]
    assert all(v.default is None for k, v in inspect.signature(U.loss_grad_raw).parameters.items() if k not in ("p", "targets", "model"))
    assert list(inspect.signature(U.compute_loss).parameters) == ["p", "targets", "model", "class_weight", "check"]


def test_workspace_bytes_unchanged():
    """The gradient needs no more scratch than the forward, and the forward's sizes are what they were: records (48 bytes per layer
    and target), the tconf map (a byte per row, each layer on a 256-byte boundary), a float64 partial per 1024 rows, four float64 terms
    per record - each part rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256

    def expected(geom, bs, nt):
        nl, nt1 = len(geom), max(nt, 1)
        rows = [bs * na * ny * nx for na, ny, nx in geom]
        return (up(nl * nt1 * 48) + sum(up(r) for r in rows) + up(8 * sum((r + 1023) // 1024 for r in rows)) + up(nl * nt1 * 32))

    base = dict(geom=[(3, 4, 6), (3, 8, 12)], bs=2, nt=40)
    for kw in (base, dict(base, bs=64), dict(base, nt=4000), dict(base, nt=0), dict(base, nt=1), dict(base, nt=41), dict(base, bs=3),
               dict(base, geom=base["geom"] + [(3, 16, 24)]), dict(base, geom=[(8, 4, 6), (3, 8, 12)]), dict(base, geom=[(3, 40, 6), (3, 8, 12)]),
               dict(base, geom=[(3, 4, 60), (3, 8, 12)]), dict(base, geom=[(3, 4, 7), (3, 8, 12)]), dict(geom=[(3, 2, 3), (3, 4, 6)], bs=2, nt=4)):
        assert K.loss_workspace_bytes(**kw) == expected(**kw), kw
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "yolo_loss_bwd_workspace_bytes")


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_argument_errors_without_a_device():
    """Every bad-argument path returns before any launch: fake non-null pointers are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    av = (ctypes.c_float * 32)(*([1.0] * 32))
    gains = (ctypes.c_float * 4)(1, 1, 1, 1)
    heads = (ctypes.c_void_p * 5)(*([0x1000] * 5))
    grads = (ctypes.c_void_p * 5)(*([0x2000] * 5))
    geo = dict(nl=2, na=_i32(3, 3, 3, 3, 3), ny=_i32(2, 4, 8, 16, 32), nx=_i32(3, 6, 12, 24, 48))
    big = 1 << 30

    def bwd(p=heads, targets=fake, nt=4, nl=None, na=None, anchors=av, bs=2, nc=3, g=gains, ws=fake, ws_bytes=big, grad_loss=fake,
            grad_p=grads):
        return lib.yolo_loss_bwd(p, targets, nt, geo["nl"] if nl is None else nl, geo["na"] if na is None else na, geo["ny"], geo["nx"],
                                 anchors, bs, nc, 0.2, g, None, ws, ws_bytes, grad_loss, grad_p, None)

    def expect(rc, code, pattern):
        msg = lib.yolo_last_error().decode()
        assert rc == code and re.search(pattern, msg), (rc, msg)

    none_f = ctypes.POINTER(ctypes.c_float)()
    none_p = ctypes.POINTER(ctypes.c_void_p)()
    expect(bwd(grad_p=none_p), -1, "loss_bwd: null grad_p")
    expect(bwd(grad_loss=None), -1, "loss_bwd: null grad_loss")
    for call in (lambda: bwd(p=none_p), lambda: bwd(targets=None), lambda: bwd(anchors=none_f), lambda: bwd(g=none_f), lambda: bwd(ws=None)):
        expect(call(), -1, "loss_bwd: null pointer")
    expect(bwd(p=(ctypes.c_void_p * 5)(0x1000, 0, 0, 0, 0)), -1, "null head tensor of layer 1")
    expect(bwd(grad_p=(ctypes.c_void_p * 5)(0x2000, 0, 0, 0, 0)), -1, "null gradient tensor of layer 1")
    expect(bwd(grad_p=(ctypes.c_void_p * 5)(0x2000, 0x2004, 0, 0, 0)), -1, "gradient tensor of layer 1 is not 16-byte aligned")
    for bad_nl in (0, 5):
        expect(bwd(nl=bad_nl), -1, rf"{bad_nl} YOLO layers not in \[1, 4\]")
    expect(bwd(na=_i32(3, 9)), -1, r"layer 1 has 9 anchors, not in \[1, 8\]")
    expect(bwd(nt=-1), -1, "negative target count -1")
    expect(bwd(bs=0), -1, "bad batch size")
    need = lib.yolo_loss_workspace_bytes(2, geo["na"], geo["ny"], geo["nx"], 2, 4)
    expect(bwd(ws_bytes=need - 1), -3, rf"loss_bwd: workspace {need - 1} < {need} bytes")


def test_host_side_refusals():
    from pytorch_yolo_amd.utils.utils import compute_loss, loss_grad_raw
    layers, p, targets, _, nc, bs = L.case_inputs("A")
    tt = torch.from_numpy(targets)
    for pt in ([torch.from_numpy(t) for t in p], [torch.from_numpy(t).requires_grad_() for t in p]):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only \\(no CPU fallback\\)"):
            compute_loss(pt, tt, L.namespace_model(layers, nc))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss_grad_raw(pt, tt, L.namespace_model(layers, nc))
        with pytest.raises(ValueError) as e:
            compute_loss(pt, tt, L.namespace_model(layers, nc, hyper=None))
        assert all(k in str(e.value) for k in L.HYPER_KEYS)
        with pytest.raises(ValueError):
            loss_grad_raw(pt, tt, L.namespace_model(layers, nc, hyper=None))
