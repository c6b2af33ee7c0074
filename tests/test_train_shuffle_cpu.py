"""CPU tests of the training-mode forward of YOLOv3-tiny/ShuffleNetV2 and of its ops.

  exports; the argument checks of the three new C entries without a GPU (dummy pointers, never dereferenced: every check fires before a
    launch); every op's ValueErrors, which come before the "no CPU fallback" RuntimeError;
  the table DEVICE_OPS_SHUFFLE, its CPU mirror, the class attributes and the tracer's vocabulary; what keeps raising;
  the eval recorder's node list did not move: tests/golden/shuffle_trace_nodes.json was recorded (make_golden_shuffle_trace.py) on the
    commit whose InvertedResidual._trace, ShuffleEncoder._trace and the head still called Recorder.conv / dwconv / slice / shuffle2;
  the numpy restatements of MaxPool2d(3, 2, 1) and of the shuffle's inverse (tests/_train_shuffle.py) against torch float64 -
    F.max_pool2d(3, 2, 1) under autograd, the view / transpose channel_shuffle under autograd - on integer maps in [-3, 3] (ties in every
    window: torch's first-maximum rule decides) and on an all-negative map, exactly;
  the wiring leg: forward_train(YOLOv3TinyShuffle, ops=<CPU float64 table>) at 64 x 96, batch 2, from the gradient of the restated loss,
    against a float64 deep copy of the model run by torch alone in torchvision's unit order;
  the dense conv picks of a full-size step all have a case, and the fused unit's first conv is recorded with its input view.

The reference takes ShuffleNetV2 from torchvision, which is not available here.  The wiring leg therefore pins the wiring and the ops
against torch's autograd of the model's own modules in torchvision's published unit order (a stride-1 unit is cat(x1, branch2(x2)), a
stride-2 unit cat(branch1(x), branch2(x)), then channel_shuffle), not against a recorded step of torchvision's encoder.

Wiring leg, measured (largest |got - want| / largest |want| per tensor - per module for the parameter gradients -, the worst over all
tensors): 5.31e-13 (p 1.3e-13, gradients 5.31e-13, running tensors 1.7e-14); the test asserts ten times that, WIRING_BOUND = 5.31e-12,
for BLAS and summation-order differences between machines: both sides are float64 and differ in summation order only."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import _loss as L
import _loss_grad as LG
import _train as T
import _train_families as TF
import _train_shuffle as S
import _train_shuffle_families as SF
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib, graph
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_maxpool3s2p1_train_fwd", "yolo_maxpool3s2p1_bwd", "yolo_channel_shuffle2_bwd")
NEW_OPS = ("conv_bn_relu_block", "max_pool_321", "channel_shuffle2", "shuffle_unit_block")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG = -1
WIRING_MEASURED = 5.31e-13     # the worst relative error of the wiring leg as measured (the module's header)
WIRING_BOUND = 10 * WIRING_MEASURED
assert WIRING_BOUND <= 1e-9


# ---- exports, tables, class attributes --------------------------------------------------------------------------------------------------------
def test_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name[5:] in K.__all__ and callable(getattr(K, name[5:]))
    assert "channel_shuffle2_fwd" in K.__all__ and callable(K.channel_shuffle2_fwd)
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    for name in NEW_OPS:
        assert name in Y.__all__ and name in Y.ops.__all__ and getattr(Y, name) is getattr(Y.ops, name), name
    assert "DEVICE_OPS_SHUFFLE" in Y.__all__ and Y.DEVICE_OPS_SHUFFLE is MT.DEVICE_OPS_SHUFFLE


def test_tables_and_class_attributes():
    shuffle, pool = vars(MT.DEVICE_OPS_SHUFFLE), vars(MT.DEVICE_OPS_POOL)
    assert set(shuffle) == set(pool) | set(S.NEW_OPS) == set(vars(S.cpu_ops(False))) == set(vars(SF.recording_meta_ops([])))
    assert all(shuffle[k] is v for k, v in pool.items()) and all(shuffle[k] is getattr(Y, k) for k in S.NEW_OPS)
    fused, composed = vars(MT.shuffle_ops()), vars(MT.shuffle_ops(fused=False))
    assert all(fused[k] is shuffle[k] for k in shuffle) and set(composed) == set(shuffle)
    assert composed["shuffle_unit_block"] is not Y.shuffle_unit_block
    assert all(composed[k] is shuffle[k] for k in shuffle if k != "shuffle_unit_block")
    # the existing tables are untouched
    assert set(pool) == set(vars(MT.DEVICE_OPS)) | {"max_pool", "pool_bn_block"}
    assert set(vars(MT.DEVICE_OPS_FIRE)) == set(pool) | {"stem_block", "fire_block", "max_pool_ceil", "concat"}
    assert set(vars(MT.DEVICE_OPS_MOBILE)) == set(pool) | {"conv_bn_relu6_block", "dw_bn_block", "project_bn_block", "expand_dw_bn_block"}
    cls = Y.YOLOv3TinyShuffle
    assert callable(cls._train_wiring) and cls._train_in_forward is False and cls._train_ops is MT.DEVICE_OPS_SHUFFLE
    assert cls._train_ops_by_name is True and cls._train_tracer is MT.ShuffleTracer and issubclass(MT.ShuffleTracer, MT.TrainTracer)
    assert not hasattr(cls, "_train_min_size")                                  # 32: there is no stride-1 pool
    assert {n for n in vars(MT.ShuffleTracer) if not n.startswith("_")} == {"conv_bn_relu", "shuffle_unit", "conv_block_mapped", "maxpool"}
    assert all(hasattr(graph.Recorder, n) for n in ("conv_bn_relu", "shuffle_unit", "conv_block_mapped", "upsample_concat"))
    # TrainTracer's own refusal stands; the subclass takes (3, 2) with pad 1 or None in floor mode and nothing else new
    g = MT.ShuffleTracer(S.cpu_ops(False), ())
    x = torch.zeros((1, 8, 5, 7), dtype=F64)
    assert tuple(g.maxpool(x, 3, 2).shape) == tuple(g.maxpool(x, 3, 2, pad=1).shape) == (1, 8, 3, 4)
    for args, kw in (((3, 2), dict(ceil_mode=True)), ((3, 2), dict(pad=0)), ((3, 1), {}), ((5, 2), dict(pad=2))):
        with pytest.raises(NotImplementedError, match="max-pool"):
            g.maxpool(x, *args, **kw)
    with pytest.raises(NotImplementedError, match="2 / 2 only"):
        MT.TrainTracer(S.cpu_ops(False), ()).maxpool(x, 3, 2)


# ---- the C entries refuse before any launch ---------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def _refused(fn, args, cases):
    for kw, msg in cases:
        rc, err = _rc(fn, *[kw.get(k, v) for k, v in args])
        assert rc == E_ARG and err.startswith(fn[5:]) and msg in err, (fn, kw, rc, err)


@pytest.mark.parametrize("fn,ptrs", [("yolo_maxpool3s2p1_train_fwd", ("x", "y", "idx")), ("yolo_maxpool3s2p1_bwd", ("dy", "idx", "dx"))])
def test_pool_entry_argument_checks(fn, ptrs):
    args = tuple((p, P) for p in ptrs) + (("n", 2), ("h", 5), ("w", 7), ("c", 16), ("s", None))
    maps = [p for p in ptrs if p != "idx"]
    _refused(fn, args, (
        (dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-1), "empty"), (dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"),
        (dict(h=1 << 21), "out of range"), ({ptrs[0]: None}, "null"), ({ptrs[1]: None}, "null"), ({ptrs[2]: None}, "null"),
        ({maps[0]: P + 8}, "misaligned"), ({maps[1]: P + 2}, "misaligned"), (dict(idx=P + 4), "misaligned")))


def test_shuffle_entry_argument_checks():
    args = (("dy", P), ("da", P), ("db", P), ("n", 2), ("h", 3), ("w", 5), ("half", 58), ("c_slot", 64), ("dy_ct", 128), ("dy_co", 0),
            ("da_ct", 128), ("da_co", 0), ("db_ct", 64), ("db_co", 0), ("s", None))
    _refused("yolo_channel_shuffle2_bwd", args, (
        (dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-2), "empty"), (dict(half=0), "logical channels"), (dict(half=65), "logical channels"),
        (dict(c_slot=60), "logical channels"), (dict(c_slot=0), "logical channels"), (dict(dy_ct=120), "view of dy"), (dict(dy_co=8), "view of dy"),
        (dict(dy_co=-1), "view of dy"), (dict(da_ct=60), "views of da / db"), (dict(da_co=68), "views of da / db"), (dict(da_co=4, da_ct=132), "views of da / db"),
        (dict(db_co=8), "views of da / db"), (dict(db_ct=68, db_co=4), "views of da / db"), (dict(h=1 << 21), "out of range"),
        (dict(dy=None), "null"), (dict(da=None, db=None), "null"), (dict(da=P + 8), "misaligned"), (dict(db=P + 2), "misaligned"), (dict(dy=P + 1), "misaligned")))
    # one missing output is allowed, any half >= 1 and an unaligned view of dy are taken: past every check the next refusal is the null dy
    for kw in (dict(da=None), dict(db=None), dict(half=1), dict(half=3, c_slot=8, dy_ct=19, dy_co=3, da_ct=8, db_ct=8)):
        rc, err = _rc("yolo_channel_shuffle2_bwd", *[dict(kw, dy=None).get(k, v) for k, v in args])
        assert rc == E_ARG and "null" in err, (kw, err)


# ---- the ops refuse ---------------------------------------------------------------------------------------------------------------------------
def _unit_args(slot=8, h=4, w=4):
    bn = lambda: [torch.ones(slot), torch.zeros(slot), None, None]
    return [torch.zeros(2, 2 * slot, h, w), 5, torch.zeros(slot, slot, 1, 1)] + bn() + [torch.zeros(slot, 1, 3, 3)] + bn() + \
        [torch.zeros(slot, slot, 1, 1)] + bn()


def test_op_argument_checks():
    """Every ValueError comes before the "no CPU fallback" RuntimeError."""
    x, w, v = torch.zeros(2, 8, 4, 4), torch.zeros(16, 8, 1, 1), torch.ones(16)
    for args, kw in (((x, torch.zeros(16, 8, 5, 5), v, v), {}), ((x, torch.zeros(12, 8, 1, 1), torch.ones(12), torch.ones(12)), {}),
                     ((x, torch.zeros(16, 4, 1, 1), v, v), {}), ((x, w.double(), v, v), {}), ((x[0], w, v, v), {}), ((x, w, v[:8], v), {}),
                     ((x, w, v, v.double()), {}), ((x, w, v, v), dict(stride=3)), ((x, w, v, v), dict(stride=True)), ((x, w, v, v), dict(stride=2)),
                     ((x, w, v, v), dict(training=False)), ((x, w, v, v), dict(momentum=None)), ((x, w, v, v), dict(eps=-1.0)),
                     ((x[:1, :, :1, :1], w, v, v), {})):
        with pytest.raises(ValueError, match="conv_bn_relu_block"):
            Y.conv_bn_relu_block(*args, **kw)
    for kw in ({}, dict(momentum=0.3, eps=1e-3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Y.conv_bn_relu_block(x, w, v, v, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.conv_bn_relu_block(torch.zeros(2, 3, 8, 8), torch.zeros(16, 3, 3, 3), v, v, stride=2)
    # conv_bn_block(act="relu") keeps raising: the ReLU layer is an op of its own
    with pytest.raises(ValueError, match="act must be"):
        Y.conv_bn_block(x, w, v, v, act="relu")

    for bad in (torch.zeros(2, 8, 4), torch.zeros(2, 12, 4, 4), torch.zeros(0, 8, 4, 4), "x"):
        with pytest.raises(ValueError, match="max_pool_321"):
            Y.max_pool_321(bad)
    for ok in (x, torch.zeros(1, 8, 1, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Y.max_pool_321(ok)

    for a, b, half in ((x, x[:, :, :3], 5), (x, torch.zeros(2, 16, 4, 4), 5), (x, x, 0), (x, x, 9), (x, x, True), (x, x, 2.0),
                       (torch.zeros(2, 12, 4, 4), torch.zeros(2, 12, 4, 4), 5), (x[0], x[0], 5)):
        with pytest.raises(ValueError, match="channel_shuffle2"):
            Y.channel_shuffle2(a, b, half)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.channel_shuffle2(x, x, 8)

    bad = [(0, torch.zeros(2, 8, 4, 4)), (0, torch.zeros(2, 24, 4, 4)), (0, torch.zeros(2, 16, 4)), (1, 0), (1, 9), (1, True), (2, torch.zeros(8, 8, 3, 3)),
           (2, torch.zeros(16, 8, 1, 1)), (2, torch.zeros(8, 8, 1, 1).double()), (2, None), (7, torch.zeros(8, 1, 5, 5)), (7, torch.zeros(16, 1, 3, 3)),
           (7, torch.zeros(8, 1, 3, 3).double()), (12, torch.zeros(8, 16, 1, 1)), (3, torch.ones(16)), (4, torch.zeros(8).double()), (8, None),
           (9, torch.zeros(4)), (13, torch.ones(8).double()), (14, torch.zeros(16)), (5, torch.zeros(16)), (16, torch.zeros(8).double())]
    for i, t in bad:
        args = _unit_args()
        args[i] = t
        with pytest.raises(ValueError, match="shuffle_unit_block"):
            Y.shuffle_unit_block(*args)
    for kw in (dict(momentum=None), dict(momentum=(0.1, 0.2)), dict(momentum=(0.1, None, 0.1)), dict(eps=-1.0), dict(eps=(1e-5, 1e-5, -1.0)),
               dict(momentum=(0.1, 0.2, 2.0))):
        with pytest.raises(ValueError, match="shuffle_unit_block"):
            Y.shuffle_unit_block(*_unit_args(), **kw)
    one = _unit_args(h=1, w=1)
    one[0] = one[0][:1]
    with pytest.raises(ValueError, match="more than 1 value"):
        Y.shuffle_unit_block(*one)
    for table in (MT.shuffle_ops(), MT.shuffle_ops(fused=False)):
        for kw in ({}, dict(momentum=(0.1, 0.2, 0.3), eps=(1e-5, 1e-3, 1e-4))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                table.shuffle_unit_block(*_unit_args(), **kw)


def test_what_keeps_raising():
    model = Y.YOLOv3TinyShuffle(**S.CTOR).train()
    x = torch.zeros((2, 3, 64, 96))
    with pytest.raises(NotImplementedError, match="training-mode forward") as e1:
        Y.forward_train(model, x)
    with pytest.raises(NotImplementedError, match="training-mode forward") as e2:
        model(x)
    with pytest.raises(NotImplementedError, match="training-mode forward") as e3:
        Y.forward_train(model, "not a tensor")                                  # before any other check
    mobile = Y.YOLOv3TinyMobile(n_class=2).train()                              # the other opt-in class: the same text
    with pytest.raises(NotImplementedError) as e4:
        Y.forward_train(mobile, x)
    efficient = Y.YOLOv3TinyEfficient(n_class=2).train()                        # a class without a wiring: the same text
    with pytest.raises(NotImplementedError) as e5:
        Y.forward_train(efficient, x, ops=Y.DEVICE_OPS_SHUFFLE)
    assert str(e1.value) == str(e2.value) == str(e3.value) == str(e4.value) == str(e5.value) and "eval" in str(e1.value)
    for call in (lambda: model.detect(x), lambda: next(model.detect_stream([x]))):
        with pytest.raises(NotImplementedError, match="eval"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.forward_train(model, x, ops=Y.DEVICE_OPS_SHUFFLE)
    with pytest.raises(ValueError, match="multiples of 32"):
        Y.forward_train(model, torch.zeros((2, 3, 64, 100)), ops=Y.DEVICE_OPS_SHUFFLE)
    with pytest.raises(ValueError, match="float32"):
        Y.forward_train(model, x.double(), ops=Y.DEVICE_OPS_SHUFFLE)
    with pytest.raises(ValueError, match="expected input"):
        Y.forward_train(model, x[:, :2], ops=Y.DEVICE_OPS_SHUFFLE)
    model.precision = "fp16"
    with pytest.raises(NotImplementedError, match="bf16 mode"):
        Y.forward_train(model, x, ops=Y.DEVICE_OPS_SHUFFLE)
    # the minimum input is 32: one pixel on the coarse grid, two values per channel with two images
    calls = []
    p = Y.forward_train(Y.YOLOv3TinyShuffle(**S.CTOR).double().train(), torch.zeros((2, 3, 32, 32), dtype=F64), ops=SF.recording_meta_ops(calls))
    assert [tuple(t.shape) for t in p] == [(2, 3, 2, 2, 7), (2, 3, 1, 1, 7)]
    assert [c[0] for c in calls].count("unit_pw1") == 13


# ---- the eval trace did not move ---------------------------------------------------------------------------------------------------------------
def test_eval_trace_equals_the_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "shuffle_trace_nodes.json")) as f:
        want = json.load(f)
    got = S.eval_trace_nodes()
    kinds = [n[0] for n in got[:-1]]
    assert kinds.count("shuffle") == 16 and kinds.count("slice") == 2 * 13 and kinds.count("dwconv") == 16 + 3 and kinds.count("pool") == 1
    assert kinds.count("conv") == 2 + 2 * 16 + 3 + 3 + 2 and kinds.count("head") == 2 and len(got) == len(want) == 110
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"node {i}"


# ---- the restatements against torch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["integer", "negative"])
@pytest.mark.parametrize("case", S.POOL_CASES, ids=S.case_id)
def test_restated_pool_equals_torch(case, kind):
    x = (S.pool_integer_map if kind == "integer" else S.pool_negative_map)(case)
    dy = S.pool_integer_dy(case)
    y, idx = S.pool_forward(x)
    y64, dx64 = S.torch_pool(x, dy)
    assert y.shape == (case[0],) + S.pool_out(case[1], case[2]) + (case[3],) and np.array_equal(y, y64) and idx.max() <= 8
    for rounding in (True, False):
        assert np.array_equal(S.pool_backward(dy, idx, case, rounding), dx64), rounding
    if kind == "negative":
        assert (y < 0).all()
    elif y.size >= 100:
        # ties: some window's maximum sits in more than one tap, and the first one was taken
        n, h, w, c = case
        later = 0
        for oy, ox in np.ndindex(*S.pool_out(h, w)):
            for k in range(9):
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                if 0 <= iy < h and 0 <= ix < w:
                    tie = (x[:, iy, ix] == y[:, oy, ox])
                    assert (idx[:, oy, ox][tie] <= k).all()
                    later += int((tie & (idx[:, oy, ox] < k)).sum())
        assert later > 0


@pytest.mark.parametrize("half,slot", S.SHUFFLE_CASES, ids=lambda v: str(v))
def test_restated_shuffle_equals_torch(half, slot):
    rng = np.random.default_rng(5200 + half)
    a, b = (rng.integers(-3, 4, S.SHUFFLE_MAP + (slot,)).astype(np.float64) for _ in range(2))
    a[..., half:], b[..., half:] = 0, 0
    dy = rng.integers(-7, 8, S.SHUFFLE_MAP + (2 * slot,)).astype(np.float64)
    dy_pad = dy.copy()
    dy_pad[..., half:slot], dy_pad[..., slot + half:] = np.nan, np.nan         # never read
    y64, da64, db64 = S.torch_shuffle(a, b, dy, half)
    assert np.array_equal(S.shuffle_forward(a, b, half), y64)
    da, db = S.shuffle_backward(dy_pad, half)
    assert np.array_equal(da, da64) and np.array_equal(db, db64) and not da[..., half:].any() and not db[..., half:].any()
    # the inverse: shuffling the two gradients gives dy back on the live channels
    back = S.shuffle_forward(da, db, half)
    assert np.array_equal(back[..., :half], dy[..., :half]) and np.array_equal(back[..., slot:slot + half], dy[..., slot:slot + half])


# ---- the wiring against torch -----------------------------------------------------------------------------------------------------------------------
def test_wiring_against_float64_autograd():
    """forward_train on the CPU float64 table against torch's autograd of a float64 deep copy of the model, its own modules run in
    torchvision's unit order (tests/_train_shuffle.reference_forward): the two p, every parameter gradient from the gradient of the
    restated loss (tests/_loss_grad.py, evaluated once on the wiring's p and handed to both sides), every running tensor and every
    num_batches_tracked.  Every BatchNorm2d has a momentum and an eps of its own.  Fails before the class had a ``_train_wiring``.

    Measured: worst relative error 5.31e-13 = WIRING_MEASURED (the module's header has the parts); the bound is ten times that."""
    model = S.training_model().double()
    ref = S.reference_copy(model)
    x, targets = S.step_inputs(2, 64, 96)
    x = x.double()
    p = Y.forward_train(model, x, ops=S.cpu_ops(False))
    want = S.reference_forward(ref, x)
    assert len(p) == 2
    dp, _ = LG.loss_grad([t.detach().numpy().astype(np.float32) for t in p], targets.numpy(), S.live_layers(model), L.HYPER, 2)
    dp = [torch.from_numpy(g) for g in dp]
    assert all(bool(g.any()) for g in dp)
    torch.autograd.backward(p, dp)
    torch.autograd.backward(want, dp)
    worst = {}
    for got, w, grid in zip(p, want, ((4, 6), (2, 3))):
        assert got.dtype == F64 and got.is_contiguous() and got.grad_fn is not None and tuple(got.shape) == (2, 3) + grid + (7,)
        worst["p"] = max(worst.get("p", 0.0), T.rel_err(got.detach().numpy(), w.detach().numpy()))
    params, ref_params = dict(model.named_parameters()), dict(ref.named_parameters())
    n_bn = 2 + 13 * 3 + 3 * 5 + 3                       # conv1, conv5; three per stride-1 unit, five per stride-2 unit; three ConvBlocks
    assert len(params) == 3 * n_bn + 2 * 2 and sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules()) == n_bn
    # a gradient's error is taken over the parameters of its module (a BatchNorm2d's weight and bias: sums over the same terms)
    modules = {}
    for n, t in params.items():
        assert t.grad is not None and bool(t.grad.any()) and ref_params[n].grad is not None, n
        diff, size = modules.setdefault(n.rsplit(".", 1)[0], [0.0, 0.0])
        modules[n.rsplit(".", 1)[0]] = [max(diff, float((t.grad - ref_params[n].grad).abs().max())), max(size, float(ref_params[n].grad.abs().max()))]
    assert len(modules) == 2 * n_bn + 2
    worst["grad"] = max(diff / size for diff, size in modules.values())
    sd, ref_sd = model.state_dict(), ref.state_dict()
    fresh = S.training_model().state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref_sd[k]) == 1, k
        elif "running" in k:
            assert not np.array_equal(v.numpy(), fresh[k].double().numpy()), k
            worst["running"] = max(worst.get("running", 0.0), T.rel_err(v.numpy(), ref_sd[k].numpy()))
    print("wiring leg, shuffle: worst relative error  " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"  (bound {WIRING_BOUND:.1e})")
    assert max(worst.values()) <= WIRING_BOUND, worst
    assert model._plans == {}


def test_pad_channels_stay_zero():
    """The tracer's physical layout: every map between the layers holds exact zeros in its pad channels, forward and backward, and the
    fused unit of the CPU table and the two-slice composition are one function."""
    model = S.training_model().double()
    x, _ = S.step_inputs(2, 64, 96)
    seen = []
    table = S.cpu_ops(False)
    inner = table.shuffle_unit_block

    def unit(xu, half, *args, **kw):
        xu.retain_grad()
        seen.append((xu, half))
        return inner(xu, half, *args, **kw)
    table.shuffle_unit_block = unit
    p = Y.forward_train(model, x.double(), ops=table)
    sum(t.square().sum() for t in p).backward()
    assert [(t.shape[1], h) for t, h in seen] == [(128, 58)] * 3 + [(256, 116)] * 7 + [(512, 232)] * 3
    for t, half in seen:
        slot = t.shape[1] // 2
        for m in (t.detach(), t.grad):
            assert bool(m[:, :half].any()) and not bool(m[:, half:slot].any()) and not bool(m[:, slot + half:].any())


# ---- the conv picks of a full-size step -----------------------------------------------------------------------------------------------------------
def test_every_conv_family_of_the_step_has_a_case():
    """One training step of full-width YOLOv3TinyShuffle at 416 x 32 on meta tensors: every (role, family) its dense conv calls select is in
    tests/_train_families.FAMILY_CASES or tests/_train_fire_families.FIRE_FAMILY_CASES (launched by their GPU tests), in their
    OTHER_FAMILIES, or has a case in SHUFFLE_FAMILY_CASES that picks it.  The fused unit's first conv is recorded with its input view, and
    the view names the kernels the dense descriptor names."""
    count, rows, others = SF.enumerate_step()
    kinds = [r[0] for r in rows]
    assert kinds.count("relu") == 2 + 3 * 3 and kinds.count("unit_pw1") == kinds.count("unit_pw2") == 13 and kinds.count("bn") == 3
    assert kinds.count("head") == 2 and len(rows) == 42
    assert [o[0] for o in others].count("dw") == 13 + 6 and [o[0] for o in others].count("shuffle") == 3 and others[0] == ("pool321", (32, 208, 208, 32), 2)
    assert rows[0][1] == (32, 416, 416, 3, 32, 3) and rows[0][2] == 2 and "dgrad_s2" not in rows[0][3]
    assert rows[-1][1] == (32, 13, 13, 128, 255, 1)
    views = [r for r in rows if r[4] is not None]
    assert [r[0] for r in views] == ["unit_pw1"] * 13
    assert [(r[1][1], r[1][3], r[4]) for r in views] == [(52, 64, (128, 64))] * 3 + [(26, 128, (256, 128))] * 7 + [(13, 256, (512, 256))] * 3
    for r in views:
        n, h, w, cin, cout, k = r[1]
        dense = TF.forward_desc(n, h, w, cin, cout, k)
        assert TF.picks_of(dense) == r[3], r[1]                                 # a view changes addresses only
    missing = [k for k in count if not SF.known(k) and k not in SF.SHUFFLE_FAMILY_CASES]
    assert not missing, missing
    for (role, fam), c in SF.SHUFFLE_FAMILY_CASES.items():
        assert (role, fam) in count and not SF.known((role, fam)), (role, fam)   # nothing stale, nothing doubled
        assert TF.case_picks(c)[role] == fam, (role, fam, TF.case_picks(c))
        n, h, w, cin, cout, k = c["case"][:6]
        assert TF.partial_and_two_k_steps(fam, n, h, w, k * k * (cin if role == "forward" else cout)), (role, fam)
    assert len(SF.CASES) == len({id(c) for c in SF.SHUFFLE_FAMILY_CASES.values()})
    for kind, (n, h, w, c), stride in others:
        if kind == "dw":
            assert K.dwconv3x3_bwd_weight_workspace_bytes(n, h, w, c, stride) > 0
