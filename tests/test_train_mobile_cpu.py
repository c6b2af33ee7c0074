"""CPU tests of the training-mode forward of YOLOv3-tiny/MobileNetV2 and of the fused expand + depthwise op.

  exports; the argument checks of the two new C entries without a GPU (dummy pointers, never dereferenced: every check fires before a
    launch); the op's ValueErrors, which come before the "no CPU fallback" RuntimeError; the new weight-gradient entry asks for the
    workspace tests/_dw_train.PICKS pins for the old one;
  the table DEVICE_OPS_MOBILE, its CPU mirror, the class attributes and the tracer's vocabulary; what keeps raising;
  the eval recorder's node list did not move: tests/golden/mobile_trace_nodes.json was recorded (make_golden_mobile_trace.py) on the
    commit whose ConvBNReLU._trace and InvertedResidual._trace still called Recorder.conv / dwconv themselves;
  the restated fused op (tests/_train_mobile.py) with the rounding off against float64 autograd of conv1x1 -> F.batch_norm(training=True)
    -> F.hardtanh(0, 6) -> depthwise conv -> F.batch_norm(training=True) -> F.hardtanh(0, 6) on tests/_dw_train.SMALL_CASES, to 1e-11
    (3.6j's bound for the same restatements); the padding taken as clamp(shift) has to break the comparison;
  the wiring leg: forward_train(YOLOv3TinyMobile, ops=<CPU float64 table>) at 96 x 128, batch 2, from the gradient of the restated loss,
    against a float64 deep copy of the model run by torch alone in oracle.mobilenet's layer order;
  the dense conv picks of a full-size step all have a case.

The reference takes MobileNetV2 from torchvision, which is not available here; oracle/mobilenet.py says so in its header: PARITY
UNPINNED.  The wiring leg therefore pins the wiring and the ops against torch's autograd of the model's own modules, not against a
recorded step of torchvision's encoder.

Wiring leg, measured (largest |got - want| / largest |want| per tensor - per module for the parameter gradients -, the worst over all
tensors): 1.02e-13 (p 4.5e-14, gradients 1.02e-13, running tensors 9.7e-15); the test asserts ten times that, WIRING_BOUND = 1.02e-12,
for BLAS and summation-order differences between machines."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _dw_train as D
import _loss as L
import _loss_grad as LG
import _train as T
import _train_families as TF
import _train_fire_families as FF
import _train_mobile as M
import _train_mobile_families as MF
import _train_pool as TP
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib, graph
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_dwconv3x3_bnin_fwd", "yolo_dwconv3x3_bnin_bwd_weight")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG, E_WORKSPACE = -1, -3
INF, NAN = float("inf"), float("nan")
AUTOGRAD_BOUND = 1e-11
WIRING_MEASURED = 1.02e-13     # the worst relative error of the wiring leg as measured (the module's header)
WIRING_BOUND = 10 * WIRING_MEASURED


# ---- exports, tables, class attributes --------------------------------------------------------------------------------------------------------
def test_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name[5:] in K.__all__ and callable(getattr(K, name[5:]))
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    assert "expand_dw_bn_block" in Y.__all__ and "expand_dw_bn_block" in Y.ops.__all__ and Y.expand_dw_bn_block is Y.ops.expand_dw_bn_block
    assert "DEVICE_OPS_MOBILE" in Y.__all__ and Y.DEVICE_OPS_MOBILE is MT.DEVICE_OPS_MOBILE


def test_tables_and_class_attributes():
    mobile, pool = vars(MT.DEVICE_OPS_MOBILE), vars(MT.DEVICE_OPS_POOL)
    assert set(mobile) == set(pool) | set(M.NEW_OPS) == set(vars(M.cpu_ops(False))) == set(vars(MF.recording_meta_ops([])))
    assert all(mobile[k] is v for k, v in pool.items()) and all(mobile[k] is getattr(Y, k) for k in M.NEW_OPS)
    fused, composed = vars(MT.mobile_ops()), vars(MT.mobile_ops(fused=False))
    assert all(fused[k] is mobile[k] for k in mobile) and set(composed) == set(mobile)
    assert composed["expand_dw_bn_block"] is not Y.expand_dw_bn_block and all(composed[k] is mobile[k] for k in mobile if k != "expand_dw_bn_block")
    # the three existing tables are untouched
    assert set(pool) == set(vars(MT.DEVICE_OPS)) | {"max_pool", "pool_bn_block"}
    assert set(vars(MT.DEVICE_OPS_FIRE)) == set(pool) | {"stem_block", "fire_block", "max_pool_ceil", "concat"}
    cls = Y.YOLOv3TinyMobile
    assert callable(cls._train_wiring) and cls._train_in_forward is False and cls._train_ops is MT.DEVICE_OPS_MOBILE
    assert cls._train_ops_by_name is True and cls._train_tracer is MT.MobileTracer and issubclass(MT.MobileTracer, MT.TrainTracer)
    assert not hasattr(cls, "_train_min_size")                                  # 32: there is no stride-1 pool
    assert {n for n in vars(MT.MobileTracer) if not n.startswith("_")} == {"conv_bn_relu6", "inverted_residual"}
    assert all(hasattr(graph.Recorder, n) for n in ("conv_bn_relu6", "inverted_residual"))
    assert not any(getattr(c, "_train_ops_by_name", False) for c in (Y.YOLOv3, Y.YOLOv3SPP, Y.YOLOv3Tiny, Y.LiteYOLOv3, Y.YOLOv3TinySqueeze))


# ---- the C entries refuse before any launch ---------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def _refused(fn, args, cases):
    for kw, msg in cases:
        rc, err = _rc(fn, *[kw.get(k, v) for k, v in args])
        assert rc == E_ARG and err.startswith(fn[5:]) and msg in err, (fn, kw, rc, err)


SHAPE = ((dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-1), "empty"), (dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"),
         (dict(stride=3), "stride 3"), (dict(stride=0), "stride 0"), (dict(h=1 << 21), "out of range"))
BOUNDS = ((dict(lo=6.0), "clamp bounds"), (dict(lo=7.0), "clamp bounds"), (dict(lo=NAN), "clamp bounds"), (dict(hi=NAN), "clamp bounds"),
          (dict(lo=-INF), "clamp bounds"), (dict(lo=INF, hi=INF), "clamp bounds"), (dict(hi=-INF), "clamp bounds"))


def test_forward_entry_argument_checks():
    args = (("zin", P), ("saved", P), ("lo", 0.0), ("hi", 6.0), ("wt", P), ("z", P), ("n", 2), ("h", 6), ("w", 5), ("c", 16), ("stride", 2), ("s", None))
    _refused("yolo_dwconv3x3_bnin_fwd", args, SHAPE + BOUNDS + (
        (dict(zin=None), "null"), (dict(saved=None), "null"), (dict(wt=None), "null"), (dict(z=None), "null"), (dict(zin=P + 8), "misaligned"),
        (dict(saved=P + 4), "misaligned"), (dict(wt=P + 4), "misaligned"), (dict(z=P + 2), "misaligned")))
    # hi = +inf is ReLU: past the bounds check, the next refusal is the null pointer
    rc, err = _rc("yolo_dwconv3x3_bnin_fwd", *[dict(hi=INF, z=None).get(k, v) for k, v in args])
    assert rc == E_ARG and "null" in err


def test_weight_entry_argument_checks_and_workspace():
    args = (("zin", P), ("saved", P), ("lo", 0.0), ("hi", 6.0), ("g", P), ("dw", P), ("ws", P), ("ws_bytes", 1 << 30), ("n", 2), ("h", 6), ("w", 5),
            ("c", 16), ("stride", 2), ("s", None))
    fn = "yolo_dwconv3x3_bnin_bwd_weight"
    _refused(fn, args, SHAPE + BOUNDS + (
        (dict(zin=None), "null"), (dict(saved=None), "null"), (dict(g=None), "null"), (dict(dw=None), "null"), (dict(ws=None), "null"),
        (dict(zin=P + 8), "misaligned"), (dict(saved=P + 4), "misaligned"), (dict(g=P + 8), "misaligned"), (dict(ws=P + 8), "misaligned"),
        (dict(dw=P + 2), "misaligned")))
    # the split rule, the workspace size and the pick string are the old entry's: the sizes tests/_dw_train.PICKS pins, one byte short
    for case, (pick, nbytes) in zip(D.CASES, D.PICKS):
        n, h, w, c, stride = case
        assert K.dwconv3x3_bwd_weight_pick(*case) == pick and K.dwconv3x3_bwd_weight_workspace_bytes(*case) == nbytes
        over = dict(ws_bytes=nbytes - 1, n=n, h=h, w=w, c=c, stride=stride)
        rc, err = _rc(fn, *[over.get(k, v) for k, v in args])
        assert rc == E_WORKSPACE and err.startswith(fn[5:]) and f"workspace {nbytes - 1} < {nbytes} bytes" in err, (case, rc, err)
        old = [dict(over, x=P).get(k, v) for k, v in (("x", P),) + args[4:]]
        rc, err = _rc("yolo_dwconv3x3_bwd_weight", *old)
        assert rc == E_WORKSPACE and f"workspace {nbytes - 1} < {nbytes} bytes" in err, (case, rc, err)
    try:
        for (i, share), want in D.SPLIT_PICKS.items():
            K.set_launch_cus(share)
            n, h, w, c, stride = D.CASES[i]
            need = D.parse_pick(want)["splits"] * 9 * c * 8
            rc, err = _rc(fn, *[dict(ws_bytes=need - 1, n=n, h=h, w=w, c=c, stride=stride).get(k, v) for k, v in args])
            assert rc == E_WORKSPACE and f"workspace {need - 1} < {need} bytes" in err, (i, share, err)
    finally:
        K.set_launch_cus(256)


# ---- the op refuses -------------------------------------------------------------------------------------------------------------------------
def _op_args(cin=8, hidden=16, h=4, w=4):
    return [torch.zeros(2, cin, h, w), torch.zeros(hidden, cin, 1, 1), torch.ones(hidden), torch.zeros(hidden), None, None,
            torch.zeros(hidden, 1, 3, 3), torch.ones(hidden), torch.zeros(hidden), None, None]


def test_op_argument_checks():
    """Every ValueError comes before the "no CPU fallback" RuntimeError."""
    bad = [(1, torch.zeros(16, 8, 3, 3), {}), (1, torch.zeros(12, 8, 1, 1), {}), (1, torch.zeros(16, 4, 1, 1), {}), (1, torch.zeros(16, 8, 1, 1).double(), {}),
           (0, torch.zeros(8, 4, 4), {}), (6, torch.zeros(16, 1, 5, 5), {}), (6, torch.zeros(8, 1, 3, 3), {}), (6, torch.zeros(16, 1, 3, 3).double(), {}),
           (6, None, {}), (2, torch.ones(8), {}), (3, torch.zeros(16).double(), {}), (7, torch.ones(8), {}), (8, None, {}), (4, torch.zeros(8), {}),
           (9, torch.zeros(16).double(), {}), (None, None, dict(stride=3)), (None, None, dict(stride=True)), (None, None, dict(training=False)),
           (None, None, dict(momentum=None)), (None, None, dict(momentum=(0.1, None))), (None, None, dict(momentum=(0.1, 0.2, 0.3))),
           (None, None, dict(eps=-1.0)), (None, None, dict(eps=(1e-5, -1.0))), (None, None, dict(momentum=(2.0, 0.1)))]
    for i, t, kw in bad:
        args = _op_args()
        if i is not None:
            args[i] = t
        with pytest.raises(ValueError, match="expand_dw_bn_block"):
            Y.expand_dw_bn_block(*args, **kw)
    one = _op_args(h=1, w=1)
    one[0] = one[0][:1]
    with pytest.raises(ValueError, match="more than 1 value"):
        Y.expand_dw_bn_block(*one)
    with pytest.raises(ValueError, match="more than 1 value"):                  # the depthwise conv's output map: 2 x 2 at stride 2 -> 1 x 1
        args = _op_args(h=2, w=2)
        args[0] = args[0][:1]
        Y.expand_dw_bn_block(*args, stride=2)
    for kw in ({}, dict(stride=2), dict(momentum=(0.1, 0.2), eps=(1e-5, 1e-3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Y.expand_dw_bn_block(*_op_args(), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MT.mobile_ops(fused=False).expand_dw_bn_block(*_op_args())


def test_what_keeps_raising():
    model = Y.YOLOv3TinyMobile(**M.CTOR).train()
    x = torch.zeros((2, 3, 64, 96))
    with pytest.raises(NotImplementedError, match="training-mode forward") as e1:
        Y.forward_train(model, x)
    with pytest.raises(NotImplementedError, match="training-mode forward") as e2:
        model(x)
    with pytest.raises(NotImplementedError, match="training-mode forward") as e3:
        Y.forward_train(model, "not a tensor")                                  # before any other check
    shuffle = Y.YOLOv3TinyShuffle(n_class=2).train()                            # a class without a wiring: the same text
    with pytest.raises(NotImplementedError) as e4:
        Y.forward_train(shuffle, x)
    assert str(e1.value) == str(e2.value) == str(e3.value) == str(e4.value) and "eval" in str(e1.value)
    for call in (lambda: model.detect(x), lambda: next(model.detect_stream([x]))):
        with pytest.raises(NotImplementedError, match="eval"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.forward_train(model, x, ops=Y.DEVICE_OPS_MOBILE)
    with pytest.raises(ValueError, match="multiples of 32"):
        Y.forward_train(model, torch.zeros((2, 3, 64, 100)), ops=Y.DEVICE_OPS_MOBILE)
    with pytest.raises(ValueError, match="float32"):
        Y.forward_train(model, x.double(), ops=Y.DEVICE_OPS_MOBILE)
    model.precision = "fp16"
    with pytest.raises(NotImplementedError, match="bf16 mode"):
        Y.forward_train(model, x, ops=Y.DEVICE_OPS_MOBILE)
    fused = Y.YOLOv3TinyMobile(**M.CTOR)
    fused.fuse()
    with pytest.raises(NotImplementedError, match="fuse"):
        Y.forward_train(fused.train(), x, ops=Y.DEVICE_OPS_MOBILE)
    # the minimum input is 32: one pixel on the coarse grid, two values per channel with two images
    p = Y.forward_train(Y.YOLOv3TinyMobile(**M.CTOR).double().train(), torch.zeros((2, 3, 32, 32), dtype=F64), ops=MF.recording_meta_ops([]))
    assert [tuple(t.shape) for t in p] == [(2, 3, 2, 2, 7), (2, 3, 1, 1, 7)]


# ---- the eval trace did not move ---------------------------------------------------------------------------------------------------------------
def test_eval_trace_equals_the_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "mobile_trace_nodes.json")) as f:
        want = json.load(f)
    got = M.eval_trace_nodes()
    kinds = [n[0] for n in got[:-1]]
    assert kinds.count("dwconv") == 17 and kinds.count("conv") == 1 + 16 + 17 + 1 + 5 and kinds.count("head") == 2 and len(got) == len(want) == 63
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"node {i}"


# ---- the restated fused op against float64 autograd ----------------------------------------------------------------------------------------------
def _rel(got, want):
    got, want = (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (got, want))
    return float(np.abs(got.astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1.0)


def fused_operands(case, cin=8, seed=0):
    n, h, w, c, stride = case
    gen = torch.Generator().manual_seed(500 + seed)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=F64)
    x, we, wd = rnd(n, cin, h, w), rnd(c, cin, 1, 1) / cin ** 0.5, rnd(c, 1, 3, 3) / 3
    x = x - x.mean((0, 2, 3), keepdim=True)          # the expand conv's output has mean 0 in every channel: shift = beta1, positive below
    g1, b1 = 1.5 + torch.rand(c, generator=gen, dtype=F64), 2.0 + 2.0 * torch.rand(c, generator=gen, dtype=F64)
    g2, b2 = 1.5 + torch.rand(c, generator=gen, dtype=F64), 3.0 + rnd(c)
    ho, wo = D.out_hw(h, w, stride)
    return [x, we, g1, b1, wd, g2, b2], [0.1 * rnd(c), 0.5 + torch.rand(c, generator=gen, dtype=F64), 0.1 * rnd(c), 0.5 + torch.rand(c, generator=gen, dtype=F64)], rnd(n, c, ho, wo)


def run_fused(table, operands, running, dy, stride):
    leaves = [t.clone().requires_grad_() for t in operands]
    run = [t.clone() for t in running]
    x, we, g1, b1, wd, g2, b2 = leaves
    y = table.expand_dw_bn_block(x, we, g1, b1, run[0], run[1], wd, g2, b2, run[2], run[3], stride=stride, momentum=(0.1, 0.3), eps=(1e-5, 1e-3))
    y.backward(dy)
    return [y] + [t.grad for t in leaves] + run


def torch_fused(operands, running, dy, stride):
    leaves = [t.clone().requires_grad_() for t in operands]
    run = [t.clone() for t in running]
    x, we, g1, b1, wd, g2, b2 = leaves
    y1 = F.hardtanh(F.batch_norm(F.conv2d(x, we), run[0], run[1], g1, b1, True, 0.1, 1e-5), 0.0, 6.0)
    z2 = F.conv2d(y1, wd, None, stride, 1, 1, wd.shape[0])
    y = F.hardtanh(F.batch_norm(z2, run[2], run[3], g2, b2, True, 0.3, 1e-3), 0.0, 6.0)
    y.backward(dy)
    shift = b1 - F.conv2d(x, we).mean((0, 2, 3)) * g1 / torch.sqrt(F.conv2d(x, we).var((0, 2, 3), unbiased=False) + 1e-5)
    return [y] + [t.grad for t in leaves] + run, shift.detach(), y1.detach()


@pytest.mark.parametrize("case", D.SMALL_CASES, ids=D.case_id)
def test_restated_fused_op_equals_autograd(case):
    """The output, the seven gradients and the four running tensors of the restated fused op with the rounding off against float64
    autograd; with the padding taken as clamp(shift), on operands whose shifts are all positive, the comparison breaks."""
    operands, running, dy = fused_operands(case)
    want, shift, y1 = torch_fused(operands, running, dy, case[4])
    got = run_fused(M.cpu_ops(False), operands, running, dy, case[4])
    names = ("y",) + ("dx", "dw_expand", "dgamma1", "dbeta1", "dw_dw", "dgamma2", "dbeta2") + ("rm1", "rv1", "rm2", "rv2")
    errs = {name: _rel(g, w) for name, g, w in zip(names, got, want)}
    assert max(errs.values()) <= AUTOGRAD_BOUND, errs
    assert all(bool(w.any()) for w in want[1:8]) and bool((shift > 0).all())
    if case[1] * case[2] >= 30:
        assert bool((y1 == 0).any()) and bool((y1 == 6).any())                   # both bounds of the inner clamp are active
    # the fault: on the conv itself in every case; through the op where the output map has more than one pixel (a constant added to
    # the one pixel of a channel is removed by the batch norm that follows)
    z1 = F.conv2d(operands[0], operands[1]).permute(0, 2, 3, 1).numpy()
    saved1 = M.N.stats(z1.reshape(-1, case[3]), operands[2].numpy(), operands[3].numpy(), 1e-5, 0.1, None, None, False)["saved"]
    assert np.allclose(saved1[3], shift.numpy(), rtol=1e-12, atol=0)
    wd = operands[4].numpy()[:, 0]
    z2, z2_bad = M.fused_forward(z1, saved1, wd, case[4], rounding=False), M.fused_forward(z1, saved1, wd, case[4], rounding=False, inject="pad")
    assert z2.shape == z2_bad.shape and _rel(z2_bad, z2) > 1e-2, "the injected padding fault does not show in the conv"
    ho, wo = D.out_hw(case[1], case[2], case[4])
    if ho * wo > 1:
        bad = run_fused(M.cpu_ops(False, inject="pad"), operands, running, dy, case[4])
        assert _rel(bad[0], want[0]) > 1e-3 and _rel(bad[5], want[5]) > 1e-3, "the injected padding fault does not show in the op"


def test_composed_table_is_the_same_function_in_float64():
    """dw_bn_block(conv_bn_relu6_block(..)) of the CPU table equals its fused op: the restatements state one function twice."""
    case = D.SMALL_CASES[3]
    operands, running, dy = fused_operands(case, seed=1)
    table = M.cpu_ops(False)
    fused = run_fused(table, operands, running, dy, case[4])
    leaves = [t.clone().requires_grad_() for t in operands]
    run = [t.clone() for t in running]
    x, we, g1, b1, wd, g2, b2 = leaves
    y1 = table.conv_bn_relu6_block(x, we, g1, b1, run[0], run[1], momentum=0.1, eps=1e-5)
    y = table.dw_bn_block(y1, wd, g2, b2, run[2], run[3], stride=case[4], momentum=0.3, eps=1e-3)
    y.backward(dy)
    for a, b in zip(fused, [y] + [t.grad for t in leaves] + run):
        assert _rel(a, b) <= 1e-14


# ---- the wiring against torch -----------------------------------------------------------------------------------------------------------------------
def test_wiring_against_float64_autograd():
    """forward_train on the CPU float64 table against torch's autograd of a float64 deep copy of the model, its own nn.Sequential children
    run in oracle.mobilenet's layer order (tests/_train_mobile.reference_forward): the two p, every parameter gradient from the gradient
    of the restated loss (tests/_loss_grad.py, evaluated once on the wiring's p and handed to both sides), every running tensor and every
    num_batches_tracked.  Every BatchNorm2d has a momentum and an eps of its own.  Fails before the class had a ``_train_wiring``.

    Measured: worst relative error 1.02e-13 = WIRING_MEASURED (the module's header has the parts); the bound is ten times that."""
    model = M.training_model().double()
    ref = M.reference_copy(model)
    x, targets = M.step_inputs(2, 96, 128)
    x = x.double()
    p = Y.forward_train(model, x, ops=M.cpu_ops(False))
    ranges = []
    want = M.reference_forward(ref, x, ranges)
    assert len(ranges) == 1 + 16 + 17 + 1 and len(p) == 2
    for numel, lo, hi in ranges:
        assert numel < 1000 or (lo == 0.0 and hi == 6.0), (numel, lo, hi)      # both clamp bounds are active in every sizeable layer
    assert sum(numel >= 1000 for numel, _, _ in ranges) >= 30
    dp, _ = LG.loss_grad([t.detach().numpy().astype(np.float32) for t in p], targets.numpy(), M.live_layers(model), L.HYPER, 2)
    dp = [torch.from_numpy(g) for g in dp]
    assert all(bool(g.any()) for g in dp)
    torch.autograd.backward(p, dp)
    torch.autograd.backward(want, dp)
    worst = {}
    for got, w, grid in zip(p, want, ((6, 8), (3, 4))):
        assert got.dtype == F64 and got.is_contiguous() and got.grad_fn is not None and tuple(got.shape) == (2, 3) + grid + (7,)
        worst["p"] = max(worst.get("p", 0.0), T.rel_err(got.detach().numpy(), w.detach().numpy()))
    params, ref_params = dict(model.named_parameters()), dict(ref.named_parameters())
    assert len(params) == 3 * 52 + 3 * 3 + 2 * 2
    # A gradient's error is taken over the parameters of its module (a BatchNorm2d's weight and bias, sums over the same terms): the
    # beta of a linear bottleneck's BatchNorm2d adds a per-channel constant to a map that only reaches 1x1 convs followed by a batch
    # norm on batch statistics, which removes it - its true gradient is 0 and both sides hold rounding noise of 1e-17 there.
    modules = {}
    for n, t in params.items():
        assert t.grad is not None and bool(t.grad.any()) and ref_params[n].grad is not None, n
        diff, size = modules.setdefault(n.rsplit(".", 1)[0], [0.0, 0.0])
        modules[n.rsplit(".", 1)[0]] = [max(diff, float((t.grad - ref_params[n].grad).abs().max())), max(size, float(ref_params[n].grad.abs().max()))]
    assert len(modules) == 2 * 52 + 2 * 3 + 2
    worst["grad"] = max(diff / size for diff, size in modules.values())
    sd, ref_sd = model.state_dict(), ref.state_dict()
    fresh = M.training_model().state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref_sd[k]) == 1, k
        elif "running" in k:
            assert not np.array_equal(v.numpy(), fresh[k].double().numpy()), k
            worst["running"] = max(worst.get("running", 0.0), T.rel_err(v.numpy(), ref_sd[k].numpy()))
    print("wiring leg, mobile: worst relative error  " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"  (bound {WIRING_BOUND:.1e})")
    assert max(worst.values()) <= WIRING_BOUND, worst
    assert model._plans == {}


def test_rounding_table_runs_the_same_wiring():
    model = M.training_model().double()
    x, _ = M.step_inputs(2, 64, 96)
    p = Y.forward_train(model, x.double(), ops=M.cpu_ops(True))
    for t in p:
        a = t.detach().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.isfinite(a).all() and a.any()
    sum(t.sum() for t in p).backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())


# ---- the conv picks of a full-size step -----------------------------------------------------------------------------------------------------------
def test_every_conv_family_of_the_step_has_a_case():
    """One training step of full-width YOLOv3TinyMobile at 416 x 32 on meta tensors: every (role, family) its dense conv calls select is
    in tests/_train_families.FAMILY_CASES or tests/_train_fire_families.FIRE_FAMILY_CASES (launched by their GPU tests), in their
    OTHER_FAMILIES (the weight gradients and the stride-2 data gradient), or has a case in MOBILE_FAMILY_CASES that picks it."""
    count, rows, dws = MF.enumerate_step()
    kinds = [r[0] for r in rows]
    assert kinds.count("relu6") == 2 and kinds.count("expand") == 16 and kinds.count("project") == 17 and kinds.count("bn") == 3
    assert kinds.count("head") == 2 and len(rows) == 40 and len(dws) == 17
    assert rows[0][1] == (32, 416, 416, 3, 32, 3) and rows[0][2] == 2 and "dgrad_s2" not in rows[0][3]
    assert rows[2][1] == (32, 208, 208, 16, 96, 1) and dws[1] == (32, 208, 208, 96, 2) and rows[-1][1] == (32, 13, 13, 64, 255, 1)
    missing = [k for k in count if not MF.known(k) and k not in MF.MOBILE_FAMILY_CASES]
    assert not missing, missing
    for (role, fam), c in MF.MOBILE_FAMILY_CASES.items():
        assert (role, fam) in count and not MF.known((role, fam)), (role, fam)   # nothing stale, nothing doubled
        assert TF.case_picks(c)[role] == fam, (role, fam, TF.case_picks(c))
    assert len(MF.CASES) == len({id(c) for c in MF.MOBILE_FAMILY_CASES.values()})
    # the depthwise shapes of the step are inside what the entries take, and the two largest split their weight gradient
    for n, h, w, c, stride in dws:
        assert K.dwconv3x3_bwd_weight_workspace_bytes(n, h, w, c, stride) > 0
    assert D.parse_pick(K.dwconv3x3_bwd_weight_pick(*dws[1]))["splits"] > 1
