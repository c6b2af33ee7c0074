"""CPU tests of the max-pool ops and of the training-mode forward of YOLOv3-tiny / LiteYOLOv3.

  restatements (tests/_train_pool.py) against torch autograd of max_pool2d(2, 2), max_pool2d(2, 1, padding=1, dilation=2), interpolate and
    cat in float64, on inputs drawn from five bf16 values so that ties are everywhere: forward, idx's effect and backward equal;
  fault injections into the restatements, each of which has to break its comparison;
  the wiring leg: the models' own ``_train_wiring`` on the CPU float64 op table with the rounding off, started from the reference's loss
    gradient, against the reference's float64 training step (tests/golden/train_tiny.npz, train_lite.npz);
  exports, argument checks of the C entries without a GPU, the ops' ValueErrors, and what keeps raising.

Wiring leg, measured (largest |got - want| / largest |want| per tensor, the worst over all tensors): YOLOv3-tiny 3.28e-13, LiteYOLOv3
1.17e-12; the bound is WIRING_BOUND = 4.5e-10 of tests/test_train_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _train as T
import _train_pool as TP
import helpers
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd.models import train as MT
from test_train_cpu import WIRING_BOUND, nchw, nhwc, tied

F64 = torch.float64
POOL_MAPS = [(2, 2, 3, 8, 2), (2, 6, 4, 8, 2), (2, 7, 5, 8, 2), (2, 2, 3, 8, 1), (2, 7, 5, 8, 1)]        # (n, h, w, c, stride)


def torch_pool(x, stride, dy):
    xt = nchw(x).requires_grad_()
    y = F.max_pool2d(xt, 2, 2) if stride == 2 else F.max_pool2d(xt, 2, 1, padding=1, dilation=2)
    y.backward(nchw(dy))
    return nhwc(y), nhwc(xt.grad)


def out_shape(n, h, w, c, stride):
    return (n, h // 2, w // 2, c) if stride == 2 else (n, h, w, c)


@pytest.mark.parametrize("case", POOL_MAPS, ids=lambda s: "%dx%dx%d_c%d_s%d" % s)
def test_pool_restatement_equals_autograd(case):
    n, h, w, c, stride = case
    x, dy = tied((n, h, w, c), 1), tied(out_shape(*case), 2) + 3.0                   # no zero gradient: every window shows in dx
    y, idx = TP.pool_forward(x, stride)
    want_y, want_dx = torch_pool(x, stride, dy)
    assert y.shape == out_shape(*case) and idx.shape == y.shape and idx.dtype == np.uint8 and idx.max() <= 3
    assert np.array_equal(y, want_y)
    assert np.array_equal(TP.pool_backward(dy, idx, x.shape, stride, rounding=False), want_dx)
    # with the rounding points: the same values rounded once (sums of at most four small values: exact in fp32)
    assert np.array_equal(TP.pool_backward(dy.astype(np.float32), idx, x.shape, stride), T.N.bf16(want_dx.astype(np.float32)))
    if stride == 2 and h % 2:
        assert not want_dx[:, h - 1].any() and not want_dx[:, :, w - 1].any()      # the dropped row and column get 0
    assert len(np.unique(idx)) == 4


def test_all_ones_sends_the_gradient_to_the_first_in_bounds_tap():
    x = np.ones((1, 4, 4, 8))
    _, idx2 = TP.pool_forward(x, 2)
    _, idx1 = TP.pool_forward(x, 1)
    assert (idx2 == 0).all()
    assert idx1[0, 0, 0, 0] == 3 and idx1[0, 0, 1, 0] == 2 and idx1[0, 1, 0, 0] == 1 and idx1[0, 1, 1, 0] == 0
    for stride, idx in ((2, idx2), (1, idx1)):
        dy = np.ones(idx.shape)
        assert np.array_equal(TP.pool_backward(dy, idx, x.shape, stride, rounding=False), torch_pool(x, stride, dy)[1])


def test_concat_upsample_restatement_equals_autograd():
    n, h, w, ca, cb = 2, 3, 5, 8, 24
    a, b, dy = tied((n, h, w, ca), 3), tied((n, 2 * h, 2 * w, cb), 4), tied((n, 2 * h, 2 * w, ca + cb), 5)
    at, bt = nchw(a).requires_grad_(), nchw(b).requires_grad_()
    y = torch.cat([bt, F.interpolate(at, scale_factor=2, mode="nearest")], 1)
    y.backward(nchw(dy))
    assert np.array_equal(TP.catup_forward(b, a), nhwc(y))
    db, da = TP.catup_backward(dy, cb, rounding=False)
    assert np.array_equal(da, nhwc(at.grad)) and np.array_equal(db, nhwc(bt.grad))
    assert not np.array_equal(TP.catup_forward(b, a), T.upcat_forward(a, b))          # the order matters


def _pool_bn_case(seed=6, shape=(2, 6, 4, 8)):
    rng = np.random.default_rng(seed)
    z = T.N.bf16(rng.standard_normal(shape).astype(np.float32))
    gamma, beta = rng.uniform(0.5, 1.5, shape[3]).astype(np.float32), (0.5 * rng.standard_normal(shape[3])).astype(np.float32)
    gamma[::2] *= -1.0                                                            # negative gamma: the activation reverses the order of z
    return z, gamma, beta


def test_bn_act_pool_restatement_equals_autograd():
    z, gamma, beta = _pool_bn_case()
    c = z.shape[3]
    st = T.N.stats(z.reshape(-1, c), gamma, beta, rounding=False)
    y, idx = TP.bn_act_pool(z.astype(np.float64), st["saved"], rounding=False)
    zt = nchw(z.astype(np.float64))
    act = F.leaky_relu(F.batch_norm(zt, None, None, torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), True,
                                    T.N.MOMENTUM, T.N.EPS), 0.1)
    want, want_idx = F.max_pool2d(act, 2, 2, return_indices=True)
    assert np.abs(y - nhwc(want)).max() < 1e-12
    # torch's flat index h w_full + x -> the tap 2i + j
    wi = nhwc(want_idx)
    assert np.array_equal(idx, ((wi // z.shape[2]) % 2 * 2 + (wi % z.shape[2]) % 2).astype(np.uint8))
    # the rounding points: bit-equal to the two separate passes
    saved = T.N.stats(z.reshape(-1, c), gamma, beta)["saved"]
    y32, idx32 = TP.bn_act_pool(z, saved)
    full = T.N.forward(z.reshape(-1, c), saved).reshape(z.shape)
    y2, idx2 = TP.pool_forward(full, 2)
    assert np.array_equal(y32, y2) and np.array_equal(idx32, idx2) and np.array_equal(y32, T.N.bf16(y32))


# ---- fault injections ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [POOL_MAPS[2], POOL_MAPS[4]], ids=["stride2", "stride1"])
def test_injected_last_maximum_breaks_the_comparison(case):
    n, h, w, c, stride = case
    x, dy = tied((n, h, w, c), 1), tied(out_shape(*case), 2) + 3.0
    y, idx = TP.pool_forward(x, stride, tie="last")
    want_y, want_dx = torch_pool(x, stride, dy)
    assert np.array_equal(y, want_y)                                              # the values agree, the routing does not
    assert not np.array_equal(TP.pool_backward(dy, idx, x.shape, stride, rounding=False), want_dx)


@pytest.mark.parametrize("drop", range(4))
def test_injected_dropped_gather_term_breaks_the_comparison(drop):
    n, h, w, c, stride = POOL_MAPS[4]
    x, dy = tied((n, h, w, c), 1), tied((n, h, w, c), 2) + 3.0
    _, idx = TP.pool_forward(x, 1)
    want = torch_pool(x, 1, dy)[1]
    assert np.array_equal(TP.pool_backward(dy, idx, x.shape, 1, rounding=False), want)
    assert not np.array_equal(TP.pool_backward(dy, idx, x.shape, 1, rounding=False, drop=drop), want)


def test_injected_pool_on_z_breaks_the_comparison():
    z, gamma, beta = _pool_bn_case()
    saved = T.N.stats(z.reshape(-1, z.shape[3]), gamma, beta)["saved"]
    y, idx = TP.bn_act_pool(z, saved)
    y2, idx2 = TP.bn_act_pool(z, saved, pool_on_z=True)
    neg, pos = slice(0, None, 2), slice(1, None, 2)
    assert not np.array_equal(y[..., neg], y2[..., neg]) and not np.array_equal(idx[..., neg], idx2[..., neg])
    assert np.array_equal(y[..., pos], y2[..., pos])                              # a positive gamma keeps the order: the values agree there


# ---- the wiring leg -----------------------------------------------------------------------------------------------------------------------
def cpu_step(family, rounding=False):
    """The training forward of the package's model on the CPU table: (model, p, targets)."""
    model = T.load_synthetic(getattr(Y, TP.CLASSES[family])(**TP.CTORS[family])).double().train()
    x, targets = TP.golden_inputs(family)
    p = Y.forward_train(model, x.double(), ops=TP.cpu_ops(rounding))
    return model, p, targets


@pytest.mark.parametrize("family", list(TP.MODELS))
def test_wiring_against_the_reference_step(family):
    gold = helpers.load_golden(TP.MODELS[family])
    model, p, _ = cpu_step(family)
    assert len(p) == len(model.yolo_layers) == (2 if family == "tiny" else 3)
    worst = 0.0
    for i, t in enumerate(p):
        assert t.dtype == F64 and t.is_contiguous() and t.grad_fn is not None and tuple(t.shape) == gold[f"p{i}"].shape
        worst = max(worst, T.rel_err(t.detach().numpy(), gold[f"p{i}"]))
    assert min(tuple(t.shape[2:4]) for t in p) == (2, 3)                                    # the smallest map the stride-1 pool takes
    torch.autograd.backward(p, [torch.from_numpy(gold[f"gp{i}"].copy()) for i in range(len(p))])
    params = dict(model.named_parameters())
    names = TP.stored_gradients(family, list(params))
    assert len(names) > 20 and sorted("grad/" + n for n in names) == sorted(k for k in gold.files if k.startswith("grad/"))
    for n, t in params.items():
        assert t.grad is not None and bool(t.grad.any()), n
    for n in names:
        worst = max(worst, T.rel_err(params[n].grad.numpy(), gold["grad/" + n]))
    for n, m in model.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert int(m.num_batches_tracked) == 1, n
            worst = max(worst, T.rel_err(m.running_mean.numpy(), gold["rm/" + n]), T.rel_err(m.running_var.numpy(), gold["rv/" + n]))
    print(f"wiring leg, {family}: worst relative error {worst:.3e} (bound {WIRING_BOUND:.1e})")
    assert worst <= WIRING_BOUND, worst
    assert model._plans == {}


def test_rounding_table_runs_the_same_wiring():
    """The wiring on the table WITH the rounding points runs: p holds finite float32 values, every BN layer counted one batch."""
    gold = helpers.load_golden(TP.MODELS["tiny"])
    model, p, _ = cpu_step("tiny", rounding=True)
    for i, t in enumerate(p):
        a = t.detach().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.isfinite(a).all()
        print(f"rounding-point model vs float64 reference, p{i}: relative L2 {np.linalg.norm(a - gold[f'p{i}']) / np.linalg.norm(gold[f'p{i}']):.3f}")
        assert not np.array_equal(a, gold[f"p{i}"])
    assert all(int(m.num_batches_tracked) == 1 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))


# ---- exports, argument checks, what keeps raising ----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("yolo_maxpool_train_fwd", "yolo_maxpool_bwd", "yolo_bn_act_pool_fwd", "yolo_concat_upsample2_fwd", "yolo_concat_upsample2_bwd")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG = -1


def test_exports():
    import os
    import re
    from pytorch_yolo_amd import kernels as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name[5:] in K.__all__ and callable(getattr(K, name[5:]))
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    for name in ("max_pool", "pool_bn_block", "forward_train", "upsample_concat"):
        assert name in Y.__all__ and callable(getattr(Y, name))
    assert Y.forward_train is MT.forward_train
    # the pool table: the six functions of DEVICE_OPS (the same objects) plus the two new ones, mirrored by the CPU table
    assert set(vars(MT.DEVICE_OPS_POOL)) == set(vars(MT.DEVICE_OPS)) | {"max_pool", "pool_bn_block"} == set(vars(TP.cpu_ops(False)))
    assert all(getattr(MT.DEVICE_OPS_POOL, k) is v for k, v in vars(MT.DEVICE_OPS).items())
    assert MT.DEVICE_OPS_POOL.max_pool is Y.max_pool and MT.DEVICE_OPS_POOL.pool_bn_block is Y.pool_bn_block
    for cls in (Y.YOLOv3Tiny, Y.LiteYOLOv3):
        assert callable(cls._train_wiring) and cls._train_in_forward is False
    for cls in (Y.YOLOv3, Y.YOLOv3SPP):
        assert cls._train_in_forward is True


def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def test_entry_argument_checks():
    """Every new entry refuses, before any launch (dummy pointers, no GPU): c % 8, a stride of 3, a 1-row map at stride 1, an empty
    stride-2 output, an empty shape, a null or misaligned pointer."""
    for fn in ("yolo_maxpool_train_fwd", "yolo_maxpool_bwd"):
        call = lambda **kw: _rc(fn, *[kw.get(k, v) for k, v in (
            ("a", P), ("b", P), ("c_", P), ("n", 2), ("h", 6), ("w", 4), ("c", 8), ("stride", 2), ("s", None))])
        out_ptr = "b" if fn.endswith("fwd") else "c_"                            # y / dx: 16 bytes; idx: 8
        idx_ptr = "c_" if fn.endswith("fwd") else "b"
        for kw, msg in ((dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"), (dict(stride=3), "stride"), (dict(stride=0), "stride"),
                        (dict(stride=1, h=1), "stride-1"), (dict(stride=1, w=1), "stride-1"), (dict(h=1), "empty output"), (dict(w=1), "empty output"),
                        (dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-1), "empty"),
                        (dict(a=None), "null"), (dict(b=None), "null"), (dict(c_=None), "null"), (dict(a=P + 8), "misaligned"),
                        ({out_ptr: P + 8}, "misaligned"), ({idx_ptr: P + 4}, "misaligned")):
            rc, err = call(**kw)
            assert rc == E_ARG and msg in err, (fn, kw, rc, err)
    call = lambda **kw: _rc("yolo_bn_act_pool_fwd", *[kw.get(k, v) for k, v in (
        ("z", P), ("saved", P), ("y", P), ("idx", P), ("n", 2), ("h", 6), ("w", 4), ("c", 16), ("act", _lib.ACT_LEAKY01), ("s", None))])
    for kw, msg in ((dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"), (dict(n=0), "empty"), (dict(h=1), "empty output"), (dict(w=1), "empty output"),
                    (dict(act=_lib.ACT_RELU6), "act"), (dict(z=None), "null"), (dict(saved=None), "null"), (dict(y=None), "null"), (dict(idx=None), "null"),
                    (dict(z=P + 8), "misaligned"), (dict(saved=P + 4), "misaligned"), (dict(y=P + 2), "misaligned"), (dict(idx=P + 4), "misaligned")):
        rc, err = call(**kw)
        assert rc == E_ARG and msg in err, (kw, rc, err)
    for fn in ("yolo_concat_upsample2_fwd", "yolo_concat_upsample2_bwd"):
        call = lambda **kw: _rc(fn, *[kw.get(k, v) for k, v in (
            ("a", P), ("b", P), ("c_", P), ("n", 2), ("h", 3), ("w", 5), ("cb", 24), ("ca", 8), ("s", None))])
        for kw, msg in ((dict(ca=12), "multiples of 8"), (dict(cb=0), "multiples of 8"), (dict(n=0), "empty"), (dict(h=0), "empty"),
                        (dict(a=None), "null"), (dict(a=P + 8), "misaligned"), (dict(b=P + 2), "misaligned"), (dict(c_=P + 8), "misaligned")):
            rc, err = call(**kw)
            assert rc == E_ARG and msg in err, (fn, kw, rc, err)
    assert _rc("yolo_concat_upsample2_fwd", P, None, P, 2, 3, 5, 24, 8, None)[0] == E_ARG
    assert _rc("yolo_concat_upsample2_bwd", P, None, None, 2, 3, 5, 24, 8, None)[0] == E_ARG          # neither gradient wanted


def test_op_argument_checks():
    """The ops' own checks: ValueError for shapes, strides and dtypes, RuntimeError for CPU tensors (no fallback)."""
    x, w = torch.zeros(2, 8, 4, 4), torch.zeros(16, 8, 3, 3)
    ga, be, rm, rv = torch.ones(16), torch.zeros(16), torch.zeros(16), torch.ones(16)
    for bad, kw in ((x[0], {}), (x[:, :4], {}), (x[:0], {}), (None, {}), (x, dict(stride=3)), (x, dict(stride=True)), (x[:, :, :1], dict(stride=1)),
                    (x[:, :, :, :1], dict(stride=2))):
        with pytest.raises(ValueError, match="max_pool"):
            Y.max_pool(bad, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.max_pool(x)
    for args, kw in (((x, w, ga, be, rm, rv), dict(training=False)), ((x, w, ga, be, rm, rv), dict(pool_stride=3)),
                     ((x[:, :, :1], w, ga, be, rm, rv), dict(pool_stride=1)), ((x[:, :, :, :1], w, ga, be, rm, rv), {}),
                     ((x, w, ga, be, rm, rv), dict(momentum=None)), ((x, w, ga, be, rm, rv), dict(act="relu")),
                     ((x, w[:12], ga[:12], be[:12], rm[:12], rv[:12]), {}), ((x, w, ga[:8], be, rm, rv), {}), ((x, w.double(), ga, be, rm, rv), {}),
                     ((x[:, :4], w, ga, be, rm, rv), {}), ((x, torch.zeros(16, 8, 5, 5), ga, be, rm, rv), {}), ((x[0], w, ga, be, rm, rv), {})):
        with pytest.raises(ValueError, match="pool_bn_block"):
            Y.pool_bn_block(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.pool_bn_block(x, w, ga, be, rm, rv)
    b = torch.zeros(2, 24, 8, 8)
    for a_, b_ in ((x, b[:, :, :4]), (x, b[:1]), (x[:, :4], b), (x, b[:, :20])):
        with pytest.raises(ValueError, match="upsample_concat"):
            Y.upsample_concat(a_, b_, up_first=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.upsample_concat(x, b, up_first=False)


def test_forward_train_checks_and_what_keeps_raising():
    """forward_train: no CPU fallback; YOLOv3-tiny below 64 raises a ValueError that says why; fp16 mode and a fused model raise.  The
    module call in training mode keeps raising for the two classes (their switch is off)."""
    tiny = Y.YOLOv3Tiny(**TP.CTORS["tiny"]).train()
    lite = Y.LiteYOLOv3(**TP.CTORS["lite"]).train()
    x = torch.zeros(1, 3, 64, 64)
    for model in (tiny, lite):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Y.forward_train(model, x)
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            model(x)
        with pytest.raises(ValueError, match="multiples of 32"):
            Y.forward_train(model, torch.zeros(1, 3, 64, 72))
        with pytest.raises(ValueError):
            Y.forward_train(model, x.double())
    with pytest.raises(ValueError, match="1x1 map"):
        Y.forward_train(tiny, torch.zeros(1, 3, 32, 64))
    with pytest.raises(ValueError, match="1x1 map"):
        Y.forward_train(tiny, torch.zeros(1, 3, 32, 64).double(), ops=TP.cpu_ops(False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.forward_train(lite, torch.zeros(1, 3, 32, 64))                          # LiteYOLOv3 has no stride-1 pool: 32 passes the shape checks
    tiny.precision = "fp16"
    with pytest.raises(NotImplementedError, match="bf16 mode only"):
        Y.forward_train(tiny, x)
    fused = Y.LiteYOLOv3(**TP.CTORS["lite"])
    fused.fuse()
    with pytest.raises(NotImplementedError, match="fuse"):
        Y.forward_train(fused.train(), x)
    with pytest.raises(NotImplementedError, match="training-mode forward"):
        Y.forward_train(Y.YOLOv3TinyMobile(n_class=2, anchors=TP.CTORS["tiny"]["anchors"]).train(), x)
    # YOLOv3-SPP behaves as before through both routes
    spp = Y.YOLOv3SPP(**T.CTOR).train()
    for call in (lambda: spp(x), lambda: Y.forward_train(spp, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
