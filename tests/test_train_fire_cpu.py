"""CPU tests of the ops and of the training-mode forward of YOLOv3-tiny/SqueezeNet.

  exports and the argument checks of the new C entries without a GPU (dummy pointers, never dereferenced), the ops' ValueErrors in the
    order the header of ops.py states, and what keeps raising;
  the float64 restatements of tests/_train_fire.py with the rounding off against torch float64 autograd of F.relu(F.conv2d(..)) at
    stride 1 and at stride 2 without padding, F.max_pool2d(x, 3, 2, ceil_mode=True) on maps with ties (exact, partial last window, the
    minimum) and oracle.squeezenet._fire; fault injections into the pool restatement, each of which has to break its comparison;
  the wiring leg: forward_train(YOLOv3TinySqueeze) on the CPU float64 table against autograd of a restatement built from
    oracle.squeezenet.squeezenet_routes and the head with F.batch_norm(training=True);
  the eval recorder's node list did not move; the conv picks of a full-size step all have a case.

The reference's own class takes its encoder from torchvision and downloads its weights; neither is available, and oracle/squeezenet.py
says so in its header: PARITY UNPINNED - the encoder restates the published SqueezeNet 1.1 and is checked against itself.  The wiring leg
therefore pins the wiring and the ops against torch's autograd of that restatement, not against a recorded reference step.

Wiring leg, measured (largest |got - want| / largest |want| per tensor, the worst over all tensors): 4.5e-15; the bound is WIRING_BOUND =
4.5e-10 of tests/test_train_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_bwd as B
import _train as T
import _train_families as TF
import _train_fire as FR
import _train_fire_families as FF
import pytorch_yolo_amd as Y
from oracle.squeezenet import _fire
from pytorch_yolo_amd import _lib, graph
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT
from test_train_cpu import WIRING_BOUND, nchw, nhwc, tied
from test_train_wiring_cpu import node_list

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_maxpool3s2_train_fwd", "yolo_maxpool3s2_bwd", "yolo_fire_bwd_split", "yolo_fire_bwd_join",
               "yolo_conv2d_stem_bwd_workspace_bytes", "yolo_conv2d_stem_bwd_pick", "yolo_conv2d_stem_bwd_weight")
NEW_OPS = ("stem_block", "fire_block", "max_pool_ceil")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG = -1
CONV_BOUND = 1e-11          # tests/test_conv_bwd_cpu.py's, tests/test_conv_down_cpu.py's: relative, against float64 autograd


# ---- exports ------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name[5:] in K.__all__ and callable(getattr(K, name[5:]))
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    for name in NEW_OPS:
        assert name in Y.__all__ and name in Y.ops.__all__ and callable(getattr(Y, name))
    # the three tables: the pool table's functions (the same objects) plus the three ops plus a concat, mirrored by the CPU table
    fire, pool = vars(MT.DEVICE_OPS_FIRE), vars(MT.DEVICE_OPS_POOL)
    assert set(fire) == set(pool) | set(NEW_OPS) | {"concat"} == set(vars(FR.cpu_ops(False))) == set(vars(FF.recording_meta_ops([])))
    assert all(fire[k] is v for k, v in pool.items()) and all(fire[k] is getattr(Y, k) for k in NEW_OPS)
    assert set(pool) == set(vars(MT.DEVICE_OPS)) | {"max_pool", "pool_bn_block"}
    cls = Y.YOLOv3TinySqueeze
    assert callable(cls._train_wiring) and cls._train_in_forward is False and cls._train_ops is MT.DEVICE_OPS_FIRE
    assert cls._train_tracer is MT.FireTracer and issubclass(MT.FireTracer, MT.TrainTracer)
    assert {n for n in vars(MT.FireTracer) if not n.startswith("_")} == {"stem_conv", "fire", "maxpool", "concat"}
    assert all(hasattr(graph.Recorder, n) for n in ("stem_conv", "fire", "maxpool", "concat"))


# ---- the C entries refuse before any launch ---------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def _refused(fn, args, cases):
    for kw, msg in cases:
        rc, err = _rc(fn, *[kw.get(k, v) for k, v in args])
        assert rc == E_ARG and err.startswith(fn[5:]) and msg in err, (fn, kw, rc, err)


def test_pool_entry_argument_checks():
    for fn in ("yolo_maxpool3s2_train_fwd", "yolo_maxpool3s2_bwd"):
        args = (("a", P), ("b", P), ("c_", P), ("n", 2), ("h", 6), ("w", 4), ("c", 8), ("s", None))
        out_ptr, idx_ptr = ("b", "c_") if fn.endswith("fwd") else ("c_", "b")        # y / dx: 16 bytes; idx: 8
        _refused(fn, args, ((dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"), (dict(h=1), "h >= 2"), (dict(w=1), "h >= 2"),
                            (dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-1), "empty"), (dict(a=None), "null"), (dict(b=None), "null"),
                            (dict(c_=None), "null"), (dict(a=P + 8), "misaligned"), ({out_ptr: P + 8}, "misaligned"), ({idx_ptr: P + 4}, "misaligned"),
                            (dict(h=1 << 21), "out of range")))


def test_fire_entry_argument_checks():
    split = (("dy", P), ("dt", _lib.DT_BF16), ("y", P), ("g1", P), ("g3", P), ("pixels", 70), ("e1", 64), ("e3", 64), ("s", None))
    _refused("yolo_fire_bwd_split", split, ((dict(e1=12), "e1 12"), (dict(e3=0), "e3 0"), (dict(e3=20), "e3 20"), (dict(pixels=0), "empty"),
                                            (dict(dt=_lib.DT_F16), "dy_dtype"), (dict(dt=7), "dy_dtype"), (dict(dy=None), "null"), (dict(y=None), "null"),
                                            (dict(g1=None), "null"), (dict(g3=None), "null"), (dict(dy=P + 8), "misaligned"), (dict(g3=P + 2), "misaligned"),
                                            (dict(pixels=1 << 40), "out of range")))
    join = (("d1", P), ("d3", P), ("sa", P), ("gs", P), ("pixels", 70), ("sq", 16), ("s", None))
    _refused("yolo_fire_bwd_join", join, ((dict(sq=12), "sq 12"), (dict(sq=0), "sq 0"), (dict(pixels=0), "empty"), (dict(pixels=-3), "empty"),
                                          (dict(d1=None), "null"), (dict(d3=None), "null"), (dict(sa=None), "null"), (dict(gs=None), "null"),
                                          (dict(d3=P + 8), "misaligned"), (dict(gs=P + 4), "misaligned")))


def stem_desc(n=2, h=17, w=19, cin=8, cout=64, **over):
    kw = dict(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=3, stride=2,
              act=_lib.ACT_RELU, kpad=K.roundup(9 * cin, 64), cout_pad=K.roundup(cout, 128), pad=0)
    kw.update(over)
    return K.conv_desc(**kw)


def test_stem_entries_refuse_what_they_do_not_cover():
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    for what, over in (("stride", dict(stride=1)), ("ksize", dict(ksize=1, kpad=64)), ("pad", dict(pad=1)), ("upsample", dict(upsample2x=1)),
                       ("residual", dict(res=(64, 0))), ("pre-add", dict(aux=(64, 0))), ("f32 output", dict(out_dtype=_lib.DT_F32)),
                       ("act", dict(act=_lib.ACT_RELU6)), ("act", dict(act=_lib.ACT_SWISH)), ("cin", dict(cin=4, in_c_total=4)),
                       ("cout", dict(cout=12, out_c_total=12)), ("view", dict(in_c_total=28, in_c_offset=4)), ("map", dict(h=2)), ("empty", dict(n=0))):
        d = stem_desc(**over)
        assert lib.yolo_conv2d_stem_bwd_pick(C.byref(d), buf, 256) == E_ARG, what
        assert lib.yolo_last_error().decode().startswith("conv2d_stem_bwd_pick"), what
        assert lib.yolo_conv2d_stem_bwd_workspace_bytes(C.byref(d)) == 0, what
        assert lib.yolo_conv2d_stem_bwd_weight(P, P, P, None, P, 1 << 30, C.byref(d), None) == E_ARG, what
    d = stem_desc()
    d.ho += 1                                                                    # the "one more row" output of a padded conv
    assert lib.yolo_conv2d_stem_bwd_pick(C.byref(d), buf, 256) == E_ARG
    d = stem_desc()
    for kw in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None), dict(x=P + 8), dict(g=P + 8), dict(ws=P + 8), dict(dw=P + 2)):
        a = dict(dict(x=P, g=P, dw=P, ws=P), **kw)
        assert lib.yolo_conv2d_stem_bwd_weight(a["x"], a["g"], a["dw"], None, a["ws"], 1 << 30, C.byref(d), None) == E_ARG, kw
    assert lib.yolo_conv2d_stem_bwd_weight(P, P, P, None, P, 16, C.byref(d), None) == -3                      # YOLO_E_WORKSPACE
    # the pad-1 entries still refuse pad 0, the stride-1 entries now take ReLU
    assert lib.yolo_conv2d_down_bwd_pick(C.byref(d), buf, 256) == E_ARG and "pad 0" in lib.yolo_last_error().decode()
    relu = B.fwd_desc(B.CASES[0], act=_lib.ACT_RELU)
    assert lib.yolo_conv2d_bwd_pick(C.byref(relu), buf, 256) == 0 and buf.value.decode() == K.conv2d_bwd_pick(B.fwd_desc(B.CASES[0]))
    assert K.conv2d_bwd_workspace_bytes(relu) == K.conv2d_bwd_workspace_bytes(B.fwd_desc(B.CASES[0]))
    down = K.conv_desc(n=2, h=8, w=8, cin=8, in_c_total=8, in_c_offset=0, cout=16, out_c_total=16, out_c_offset=0, ksize=3, stride=2,
                       act=_lib.ACT_RELU, kpad=128, cout_pad=128)
    assert lib.yolo_conv2d_down_bwd_pick(C.byref(down), buf, 256) == E_ARG and "act" in lib.yolo_last_error().decode()


def test_stem_pick_and_workspace():
    """The split rule of yolo_conv2d_down_bwd_weight on the output pixels; the full-size layer (32 x 416 x 416 -> 207 x 207) splits."""
    for n, h, w, cin, cout in ((2, 17, 19, 8, 64), (2, 18, 20, 8, 64), (2, 9, 11, 8, 16), (4, 67, 69, 8, 64), (32, 416, 416, 8, 64)):
        d = stem_desc(n, h, w, cin, cout)
        m = re.fullmatch(r"wgrad<(\d+)x128,BK64,tr_b16,s2,p0> grid (\d+)x(\d+) splits (\d+)", K.conv2d_stem_bwd_pick(d))
        assert m, K.conv2d_stem_bwd_pick(d)
        tm, tn, tmm, splits = (int(v) for v in m.groups())
        assert (d.ho, d.wo) == ((h - 3) // 2 + 1, (w - 3) // 2 + 1) and tm == 64 and tn == 1 and tmm == 1
        steps = -(-n * d.ho * d.wo // 64)
        assert 1 <= splits <= max(1, steps // 8) and K.conv2d_stem_bwd_workspace_bytes(d) == 4 * splits * cout * (9 * cin + 1)
        # the same pixels through the pad-1 entry's rule: a padded map with the same output size
        same = K.conv_desc(n=n, h=2 * d.ho, w=2 * d.wo, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0,
                           ksize=3, stride=2, act=_lib.ACT_NONE, kpad=d.kpad, cout_pad=d.cout_pad)
        assert K.conv2d_down_bwd_pick(same).split(";")[0].replace(",s2>", ",s2,p0>") == K.conv2d_stem_bwd_pick(d)
    assert splits == 64 and int(K.conv2d_stem_bwd_pick(stem_desc(4, 67, 69)).rsplit(" ", 1)[1]) >= 2


# ---- the ops' argument checks -------------------------------------------------------------------------------------------------------------------
def _fire_args(cin=8, sq=8, e1=8, e3=16):
    return [torch.zeros((1, cin, 4, 4), dtype=torch.bfloat16), torch.zeros((sq, cin, 1, 1)), torch.zeros(sq), torch.zeros((e1, sq, 1, 1)),
            torch.zeros(e1), torch.zeros((e3, sq, 3, 3)), torch.zeros(e3)]


def test_op_argument_checks():
    """Every ValueError, then the no-CPU-fallback RuntimeError: a bad argument on CPU tensors raises ValueError, a good call RuntimeError."""
    x, w = torch.zeros((1, 8, 5, 5), dtype=torch.bfloat16), torch.zeros((8, 8, 3, 3))
    with pytest.raises(ValueError, match="'leaky', 'none' or 'relu'"):
        Y.conv_block(x, w, act="relu6")
    with pytest.raises(ValueError, match="'leaky' or 'none'"):
        Y.down_block(x, w, act="relu")
    with pytest.raises(ValueError, match="'leaky' or 'none'"):
        Y.conv_bn_block(x, w, torch.ones(8), torch.zeros(8), act="relu")
    with pytest.raises(ValueError):
        Y.pool_bn_block(x, w, torch.ones(8), torch.zeros(8), act="relu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.conv_block(x, w, act="relu")
    # stem_block
    for bad_x, bad_w, kw in ((x, torch.zeros((8, 8, 1, 1)), {}), (x, torch.zeros((8, 8, 5, 5)), {}), (x, torch.zeros((8, 16, 3, 3)), {}),
                             (x[0], w, {}), (x, w, dict(act="relu6")), (x, torch.zeros((12, 8, 3, 3)), {}), (x, w.double(), {}),
                             (x[:, :, :2], w, {}), (x[:, :, :, :2], w, {})):
        with pytest.raises(ValueError, match="stem_block"):
            Y.stem_block(bad_x, bad_w, **kw)
    with pytest.raises(ValueError, match="bias"):
        Y.stem_block(x, w, torch.zeros(7))
    with pytest.raises(NotImplementedError, match="first layer"):
        Y.stem_block(x.float().requires_grad_(), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.stem_block(x, w, torch.zeros(8))
    # max_pool_ceil
    for bad in (x[0], x[:, :4], x[:, :, :1], x[:, :, :, :1], x[:, :, :0]):
        with pytest.raises(ValueError, match="max_pool_ceil"):
            Y.max_pool_ceil(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.max_pool_ceil(x[:, :, :2, :2])
    # fire_block: sq, e1, e3 % 8, shapes, dtypes
    for i, bad in ((1, torch.zeros((12, 8, 1, 1))), (1, torch.zeros((8, 8, 3, 3))), (1, torch.zeros((8, 16, 1, 1))), (2, torch.zeros(7)),
                   (3, torch.zeros((12, 8, 1, 1))), (3, torch.zeros((8, 8, 3, 3))), (3, torch.zeros((8, 16, 1, 1))), (3, torch.zeros((8, 8, 1, 1)).double()),
                   (4, torch.zeros(9)), (4, None), (5, torch.zeros((20, 8, 3, 3))), (5, torch.zeros((16, 8, 1, 1))), (6, torch.zeros(16).double()),
                   (0, torch.zeros((8, 4, 4)))):
        args = _fire_args()
        args[i] = bad
        with pytest.raises(ValueError, match="fire_block"):
            Y.fire_block(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.fire_block(*_fire_args())


def test_what_keeps_raising():
    model = Y.YOLOv3TinySqueeze(**FR.CTOR).train()
    x = torch.zeros((2, 3, 64, 96))
    with pytest.raises(NotImplementedError, match="forward_train"):
        model(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.forward_train(model, x)
    with pytest.raises(ValueError, match="multiples of 32"):
        Y.forward_train(model, torch.zeros((2, 3, 64, 100)))
    with pytest.raises(ValueError, match="float32"):
        Y.forward_train(model, x.double())
    model.precision = "fp16"
    with pytest.raises(NotImplementedError, match="bf16 mode"):
        Y.forward_train(model, x)
    # the classes without a wiring are refused as before
    with pytest.raises(NotImplementedError, match="eval"):
        Y.forward_train(Y.YOLOv3TinyMobile(n_class=2).train(), x)
    # the tracer: the base class still has no 3 / 2 pool; the subclass takes SqueezeNet's and nothing else with a pad or ceil mode
    meta = torch.empty((1, 8, 8, 8), dtype=torch.bfloat16, device="meta")
    table = FF.recording_meta_ops([])
    with pytest.raises(NotImplementedError):
        MT.TrainTracer(table, model.yolo_layers).maxpool(meta, 3, 2)
    g = MT.FireTracer(table, model.yolo_layers)
    assert g.maxpool(meta, 3, 2, pad=0, ceil_mode=True).shape == (1, 8, 4, 4) and g.maxpool(meta, 2, 2).shape == (1, 8, 4, 4)
    for args, kw in (((3, 2), {}), ((3, 2), dict(pad=1, ceil_mode=True)), ((3, 2), dict(pad=0)), ((2, 2), dict(ceil_mode=True)), ((2, 1), {})):
        with pytest.raises(NotImplementedError):
            g.maxpool(meta, *args, **kw)


# ---- restatements against float64 autograd ------------------------------------------------------------------------------------------------------
def _rel(got, want):
    return T.rel_err(got.detach().numpy(), want.detach().numpy())


@pytest.mark.parametrize("case", [c for c in B.CASES if c[0] * c[1] * c[2] < 2000], ids=B.case_id)
def test_relu_conv_restatement_equals_autograd(case):
    """relu_forward / relu_grads with the rounding off against autograd of F.relu(F.conv2d(..)): the stride-1 cases of tests/_conv_bwd.py
    with the act swapped."""
    n, h, w_, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
    y = F.relu(F.conv2d(xa, wa, ba, padding=k // 2))
    y.backward(dy)
    got_y = FR.relu_forward(x, w, b, rounding=False)
    r = FR.relu_grads(x, w, dy, got_y, rounding=False)
    assert _rel(got_y, y) <= CONV_BOUND and float((y == 0).double().mean()) > 0.2
    assert max(_rel(r["dw"], wa.grad), _rel(r["db"], ba.grad), _rel(r["dx"], xa.grad)) <= CONV_BOUND
    # with the rounding points g is dy where y > 0 and 0 elsewhere, as a bf16 value
    g = FR.relu_upstream(dy, got_y)
    assert torch.equal(g, torch.where(got_y > 0, B.bf16(dy), torch.zeros_like(dy)))


STEM_CASES = [(2, 17, 19, 3, 64), (2, 18, 20, 3, 64), (2, 9, 11, 8, 16)]


@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "%dx%dx%d_%dto%d" % c)
def test_stem_restatement_equals_autograd(case):
    n, h, w_, cin, cout = case
    gen = torch.Generator().manual_seed(31)
    x, w, b = (torch.randn(s, generator=gen, dtype=F64) for s in ((n, cin, h, w_), (cout, cin, 3, 3), (cout,)))
    wa, ba = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.relu(F.conv2d(x, wa, ba, stride=2))
    dy = torch.randn(y.shape, generator=gen, dtype=F64)
    y.backward(dy)
    got_y = FR.relu_forward(x, w, b, rounding=False, stride=2, pad=0)
    r = FR.stem_grads(x, w, dy, got_y, rounding=False)
    assert tuple(y.shape[2:]) == ((h - 3) // 2 + 1, (w_ - 3) // 2 + 1)
    assert max(_rel(got_y, y), _rel(r["dw"], wa.grad), _rel(r["db"], ba.grad)) <= CONV_BOUND
    assert float(r["dw_terms"].min()) == float(r["dw_terms"].max()) == n * y.shape[2] * y.shape[3]        # pad 0: every tap of every window is inside
    if h % 2 == 0:                                                                 # the unread last row and column
        x2 = x.clone()
        x2[:, :, h - 1], x2[:, :, :, w_ - 1] = 7.0, -7.0
        assert torch.equal(FR.stem_grads(x2, w, dy, got_y, rounding=False)["dw"], r["dw"])


POOL_MAPS = [(2, 7, 9, 8), (2, 8, 10, 8), (2, 2, 3, 8), (2, 3, 2, 24), (1, 4, 5, 8)]          # exact; a partial last window both ways; the minimum


def torch_pool3(x, dy):
    xt = nchw(x).requires_grad_()
    y, where = F.max_pool2d(xt, 3, 2, ceil_mode=True, return_indices=True)
    y.backward(nchw(dy))
    return nhwc(y), nhwc(xt.grad), nhwc(where)


def torch_tap(where, w):
    """torch's flat index h w_full + x of a window's maximum -> the tap 3i + j inside the window at (oy, ox)."""
    n, ho, wo, c = where.shape
    oy, ox = np.arange(ho)[None, :, None, None], np.arange(wo)[None, None, :, None]
    return (3 * (where // w - 2 * oy) + (where % w - 2 * ox)).astype(np.uint8)


@pytest.mark.parametrize("case", POOL_MAPS, ids=lambda s: "%dx%dx%d_c%d" % s)
def test_pool_restatement_equals_autograd(case):
    n, h, w, c = case
    x = tied(case, 1)
    y, idx = FR.pool3_forward(x)
    dy = tied(y.shape, 2) + 3.0                                                  # no zero gradient: every window shows in dx
    want_y, want_dx, where = torch_pool3(x, dy)
    assert y.shape == (n, FR.pool3_out(h), FR.pool3_out(w), c) == want_y.shape and idx.dtype == np.uint8 and idx.max() <= 8
    assert np.array_equal(y, want_y) and np.array_equal(idx, torch_tap(where, w))
    assert np.array_equal(FR.pool3_backward(dy, idx, x.shape, rounding=False), want_dx)
    # with the rounding points: the same values rounded once (sums of at most four small values: exact in fp32)
    assert np.array_equal(FR.pool3_backward(dy.astype(np.float32), idx, x.shape), T.N.bf16(want_dx.astype(np.float32)))
    if h >= 7:
        assert len(np.unique(idx)) == 9 and (want_dx > dy.max()).any()           # every tap wins somewhere; some pixel sums two windows


def test_all_ones_sends_the_gradient_to_the_first_tap():
    x = np.ones((1, 6, 6, 8))
    y, idx = FR.pool3_forward(x)
    assert (idx == 0).all() and y.shape == (1, 3, 3, 8)
    dy = np.ones(idx.shape)
    dx = FR.pool3_backward(dy, idx, x.shape, rounding=False)
    assert np.array_equal(dx, torch_pool3(x, dy)[1]) and dx.sum() == dy.sum() and (dx[0, ::2, ::2] == 1).all()


def test_injected_pool_faults_break_the_comparison():
    n, h, w, c = POOL_MAPS[1]
    x = tied(POOL_MAPS[1], 1)
    y, idx = FR.pool3_forward(x)
    dy = tied(y.shape, 2) + 3.0
    want_y, want_dx, _ = torch_pool3(x, dy)
    y_last, idx_last = FR.pool3_forward(x, tie="last")
    assert np.array_equal(y_last, want_y)                                        # the values agree, the routing does not
    assert not np.array_equal(FR.pool3_backward(dy, idx_last, x.shape, rounding=False), want_dx)
    for drop in range(4):
        assert not np.array_equal(FR.pool3_backward(dy, idx, x.shape, rounding=False, drop=drop), want_dx), drop


FIRE_CASES = [(2, 5, 7, 64, 16, 64), (2, 5, 7, 256, 48, 192), (1, 13, 15, 64, 16, 64)]


def fire_operands(case, seed=0):
    """x, dy ~ N(0, 1) as bf16 values, the six parameters (weights ~ N(0, 1 / fan_in), biases ~ N(0, 1/4)), float64."""
    n, h, w, cin, sq, e = case
    gen = torch.Generator().manual_seed(5000 + seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    x, dy = rn(n, cin, h, w).to(torch.bfloat16).to(F64), rn(n, 2 * e, h, w).to(torch.bfloat16).to(F64)
    p = [(rn(sq, cin, 1, 1) / cin ** 0.5).to(F64), (rn(sq) * 0.5).to(F64), (rn(e, sq, 1, 1) / sq ** 0.5).to(F64), (rn(e) * 0.5).to(F64),
         (rn(e, sq, 3, 3) / (9 * sq) ** 0.5).to(F64), (rn(e) * 0.5).to(F64)]
    return x, p, dy


@pytest.mark.parametrize("case", FIRE_CASES, ids=lambda c: "%dx%dx%d_%d_%d_%d" % c)
def test_fire_restatement_equals_autograd(case):
    x, p, dy = fire_operands(case)
    xa = x.clone().requires_grad_()
    pa = [t.clone().requires_grad_() for t in p]
    y = _fire(dict(zip(("f." + k for k in FR.FIRE_KEYS), pa)), "f", xa)
    y.backward(dy)
    r = FR.fire_restated(x, p, dy, rounding=False)
    got = [r["rs"]["dw"], r["rs"]["db"], r["r1"]["dw"], r["r1"]["db"], r["r3"]["dw"], r["r3"]["db"]]
    assert _rel(r["y"], y) <= CONV_BOUND and _rel(r["rs"]["dx"], xa.grad) <= CONV_BOUND
    assert max(_rel(g, t.grad) for g, t in zip(got, pa)) <= CONV_BOUND
    assert 0.2 < float((r["s"] == 0).double().mean()) < 0.8 and 0.2 < float((y == 0).double().mean()) < 0.8
    # the CPU table's Function is the same restatement under autograd
    xa2, pa2 = x.clone().requires_grad_(), [t.clone().requires_grad_() for t in p]
    FR.cpu_ops(False).fire_block(xa2, *pa2).backward(dy)
    assert torch.equal(xa2.grad, r["rs"]["dx"]) and all(torch.equal(t.grad, g) for t, g in zip(pa2, got))


# ---- the wiring leg -------------------------------------------------------------------------------------------------------------------------------
def test_wiring_against_float64_autograd():
    """forward_train on the CPU float64 table against autograd of the restatement from oracle.squeezenet.squeezenet_routes and the head
    with F.batch_norm(training=True): outputs, every parameter gradient from a fixed scalar loss, the running statistics and
    num_batches_tracked.  (oracle/squeezenet.py: PARITY UNPINNED - the reference's encoder is torchvision's and is not available; both
    sides here restate the published SqueezeNet 1.1.)  Fails with NotImplementedError before the class had a ``_train_wiring``."""
    model = T.load_synthetic(Y.YOLOv3TinySqueeze(**FR.CTOR)).double().train()
    x = FR.golden_inputs(model)[0].double()
    assert tuple(x.shape) == (2, 3, 64, 96)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    p = Y.forward_train(model, x, ops=FR.cpu_ops(False))
    gen = torch.Generator().manual_seed(77)
    r = [torch.randn(t.shape, generator=gen, dtype=F64) for t in p]
    sum((t * w).sum() for t, w in zip(p, r)).backward()
    # the reference
    ref = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd0.items()}
    b1, b2, stats = FR.reference_step(ref, x)
    want = [b.reshape(2, 3, 7, *b.shape[2:]).permute(0, 1, 3, 4, 2) for b in (b1, b2)]
    sum((t * w).sum() for t, w in zip(want, r)).backward()
    assert len(p) == 2 and all(tuple(t.shape) == (2, 3, 3, 5, 7) for t in p)     # 64 x 96 -> 31 x 47 -> 15 x 23 -> 7 x 11 -> 3 x 5
    worst = 0.0
    for got, w in zip(p, want):
        assert got.dtype == F64 and got.is_contiguous() and got.grad_fn is not None
        worst = max(worst, _rel(got, w))
    params = dict(model.named_parameters())
    assert len(params) == 2 + 8 * 6 + 3 * 3 + 2 * 2
    for n, t in params.items():
        assert t.grad is not None and bool(t.grad.any()) and ref[n].grad is not None, n
        worst = max(worst, _rel(t.grad, ref[n].grad))
    bns = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert len(bns) == 3
    for n, m in bns.items():
        prefix = n[:-len(".sequence.batch_norm")]
        mean, var = stats[prefix]
        assert int(m.num_batches_tracked) == 1, n
        worst = max(worst, _rel(m.running_mean, 0.9 * sd0[n + ".running_mean"] + 0.1 * mean),
                    _rel(m.running_var, 0.9 * sd0[n + ".running_var"] + 0.1 * var))
    print(f"wiring leg, squeeze: worst relative error {worst:.3e} (bound {WIRING_BOUND:.1e})")
    assert worst <= WIRING_BOUND, worst
    assert model._plans == {}


def test_rounding_table_runs_the_same_wiring():
    model = T.load_synthetic(Y.YOLOv3TinySqueeze(**FR.CTOR)).double().train()
    p = Y.forward_train(model, FR.golden_inputs(model)[0].double(), ops=FR.cpu_ops(True))
    for t in p:
        a = t.detach().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.isfinite(a).all() and a.any()
    sum(t.sum() for t in p).backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in model.parameters())


# ---- the recorder side did not move ---------------------------------------------------------------------------------------------------------------
class DirectRecorder(graph.Recorder):
    """stem_conv and fire written out as the direct calls the model's ``_trace`` made before the two methods existed."""

    @staticmethod
    def _wb(conv):
        return conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()

    def stem_conv(self, conv, x):
        return self.conv(x, self._wb(conv), stride=2, act="relu", pad=0)

    def fire(self, fire, x):
        sq, sp = fire.squeeze.out_channels, -(-fire.squeeze.out_channels // 32) * 32
        w, b = self._wb(fire.squeeze)
        s = self.conv(x, (F.pad(w, (0, 0, 0, 0, 0, 0, 0, sp - sq)), F.pad(b, (0, sp - sq))), act="relu")

        def widen(conv):
            w_, b_ = self._wb(conv)
            return F.pad(w_, (0, 0, 0, 0, 0, sp - sq)), b_
        return self.concat([self.conv(s, widen(fire.expand1x1), act="relu"), self.conv(s, widen(fire.expand3x3), act="relu")])


def test_recorder_methods_record_the_direct_nodes():
    torch.manual_seed(0)
    model = Y.YOLOv3TinySqueeze(**FR.CTOR).eval()
    for name, m in model.named_modules():
        m._trace_name = name
    lists = []
    for kind in (graph.Recorder, DirectRecorder):
        rec = kind(2, 3, 64, 96)
        model._trace(rec, rec.input)
        lists.append(node_list(rec))
    kinds = [n[0] for n in lists[0][:-1]]
    assert kinds.count("conv") == 1 + 8 * 3 + 5 and kinds.count("pool") == 3 and kinds.count("cat") == 9 and kinds.count("head") == 2
    squeeze = [n for n in lists[0][:-1] if n[0] == "conv"][1]
    assert squeeze[2][0][4] == 32                                                # the 16-channel squeeze tensor in 32 physical channels
    pools = [dict(n[3]) for n in lists[0][:-1] if n[0] == "pool"]
    assert all(a == dict(size=3, stride=2, pad=0, dil=1) for a in pools)
    assert lists[0] == lists[1]
    assert [layer for _, layer in rec.heads] == list(model.yolo_layers)


# ---- the conv picks of a full-size step ---------------------------------------------------------------------------------------------------------
def test_every_conv_family_of_the_step_has_a_case():
    """One training step of full-width YOLOv3TinySqueeze at 416 x 32 on meta tensors: every (role, family) its conv calls select is in
    tests/_train_families.FAMILY_CASES (launched by tests/test_train_families_gpu.py), in OTHER_FAMILIES (the weight gradients), or has
    a case in FIRE_FAMILY_CASES that picks it (launched by tests/test_train_fire_gpu.py)."""
    count, rows = FF.enumerate_step()
    kinds = [r[0] for r in rows]
    assert kinds.count("stem") == 1 and kinds.count("fire_squeeze") == kinds.count("fire_e1") == kinds.count("fire_e3") == 8
    assert kinds.count("bn") == 3 and kinds.count("head") == 2 and len(rows) == 30
    assert rows[0][1] == (32, 416, 416, 3, 64, 3) and rows[1][1] == (32, 103, 103, 64, 16, 1) and rows[-1][1] == (32, 25, 25, 128, 255, 1)
    missing = [k for k in count if k not in TF.FAMILY_CASES and k not in FF.OTHER_FAMILIES and k not in FF.FIRE_FAMILY_CASES]
    assert not missing, missing
    for (role, fam), c in FF.FIRE_FAMILY_CASES.items():
        assert (role, fam) in count and (role, fam) not in TF.FAMILY_CASES, (role, fam)     # nothing stale, nothing doubled
        assert TF.case_picks(c)[role] == fam, (role, fam, TF.case_picks(c))
        assert c["knobs"] == (-1, 0, 0)
    assert len(FF.CASES) == len(FF.FIRE_FAMILY_CASES) == 7
