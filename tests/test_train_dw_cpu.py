"""CPU tests of the training ops of MobileNetV2's inverted residual: conv_bn_relu6_block, dw_bn_block, project_bn_block
and the C entries behind them (the clamp entries of csrc/batchnorm.hip, csrc/dw_train.hip).

  exports; the argument checks of the new C entries without a GPU (dummy pointers, never dereferenced: every check fires before a
    launch); the ops' ValueErrors, which come before the "no CPU fallback" RuntimeError; the pinned pick strings of the weight gradient;
  the numpy restatements of tests/_dw_train.py with the rounding off against torch float64 autograd of F.conv2d(groups=c) ->
    F.batch_norm(training=True) -> F.hardtanh(0, 6), and of x + batch_norm(conv1x1(..)) for the projection, to 1e-11 relative;
  fault injections into the restatements, each of which has to break its comparison: the data gradient with the wrong parity at stride
    2, a dropped split partial of the weight gradient, the slope taken as 1 at a == 6;
  an inverted residual composed from the restated ops, at stride 1 with the residual and at stride 2 without it, against float64
    autograd of the same block in oracle.mobilenet's layer order with F.batch_norm(training=True): outputs, all parameter gradients
    and running statistics to 1e-10.

The reference takes MobileNetV2 from torchvision, which is not available here; oracle/mobilenet.py says so in its header: PARITY
UNPINNED.  The composed block is therefore checked against torch's autograd of the published layer order restated in this file, not
against a recorded step of torchvision's InvertedResidual."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn as N
import _dw_train as D
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_bn_clamp_fwd", "yolo_bn_clamp_bwd", "yolo_bn_add_rounded_fwd", "yolo_dwconv3x3_bwd_data", "yolo_dwconv3x3_bwd_weight_workspace_bytes",
               "yolo_dwconv3x3_bwd_weight_pick", "yolo_dwconv3x3_bwd_weight")
NEW_OPS = ("conv_bn_relu6_block", "dw_bn_block", "project_bn_block")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG, E_WORKSPACE = -1, -3
INF, NAN = float("inf"), float("nan")
AUTOGRAD_BOUND = 1e-11
BLOCK_BOUND = 1e-10


def test_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name[5:] in K.__all__ and callable(getattr(K, name[5:]))
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    for name in NEW_OPS:
        assert name in Y.__all__ and name in Y.ops.__all__ and getattr(Y, name) is getattr(Y.ops, name)


# ---- the C entries refuse before any launch ---------------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def _refused(fn, args, cases):
    for kw, msg in cases:
        rc, err = _rc(fn, *[kw.get(k, v) for k, v in args])
        assert rc == E_ARG and err.startswith(fn[5:]) and msg in err, (fn, kw, rc, err)


def test_clamp_entry_argument_checks():
    bounds = ((dict(lo=6.0), "clamp bounds"), (dict(lo=7.0), "clamp bounds"), (dict(lo=NAN), "clamp bounds"), (dict(hi=NAN), "clamp bounds"),
              (dict(lo=-INF), "clamp bounds"), (dict(lo=INF, hi=INF), "clamp bounds"), (dict(hi=-INF), "clamp bounds"))
    fwd = (("z", P), ("saved", P), ("y", P), ("pixels", 100), ("c", 16), ("lo", 0.0), ("hi", 6.0), ("s", None))
    _refused("yolo_bn_clamp_fwd", fwd, bounds + ((dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"), (dict(pixels=0), "pixels"),
                                                 (dict(z=None), "null"), (dict(saved=None), "null"), (dict(y=None), "null"),
                                                 (dict(z=P + 8), "misaligned"), (dict(y=P + 2), "misaligned"), (dict(saved=P + 4), "misaligned")))
    bwd = (("dy", P), ("dy_dtype", _lib.DT_BF16), ("z", P), ("saved", P), ("pixels", 100), ("c", 16), ("lo", 0.0), ("hi", 6.0),
           ("batch_stats", 1), ("g", P), ("dgamma", P), ("dbeta", P), ("ws", P), ("ws_bytes", 1 << 20), ("s", None))
    _refused("yolo_bn_clamp_bwd", bwd, bounds + ((dict(c=12), "multiple of 8"), (dict(dy_dtype=_lib.DT_F16), "dy_dtype"),
                                                 (dict(pixels=1), "more than one value"), (dict(batch_stats=2), "batch_stats"),
                                                 (dict(dy=None), "null"), (dict(z=None), "null"), (dict(saved=None), "null"), (dict(ws=None), "null"),
                                                 (dict(dy=P + 8), "misaligned"), (dict(g=P + 8), "misaligned"), (dict(dgamma=P + 2), "misaligned")))
    rc, err = _rc("yolo_bn_clamp_bwd", *[dict(ws_bytes=K.bn_workspace_bytes(100, 16) - 1).get(k, v) for k, v in bwd])
    assert rc == E_WORKSPACE and err.startswith("bn_clamp_bwd") and "workspace" in err
    # hi = +inf is ReLU: past the bounds check, the next refusal is the null pointer
    rc, err = _rc("yolo_bn_clamp_fwd", *[dict(hi=INF, z=None).get(k, v) for k, v in fwd])
    assert rc == E_ARG and "null" in err


def test_add_rounded_entry_argument_checks():
    args = (("z", P), ("saved", P), ("res", P), ("y", P), ("pixels", 100), ("c", 16), ("s", None))
    _refused("yolo_bn_add_rounded_fwd", args, ((dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"), (dict(pixels=0), "pixels"),
                                               (dict(z=None), "null"), (dict(saved=None), "null"), (dict(res=None), "null"), (dict(y=None), "null"),
                                               (dict(z=P + 8), "misaligned"), (dict(res=P + 8), "misaligned"), (dict(y=P + 2), "misaligned"),
                                               (dict(saved=P + 4), "misaligned")))


def test_depthwise_entry_argument_checks():
    shape = ((dict(n=0), "empty"), (dict(h=0), "empty"), (dict(w=-1), "empty"), (dict(c=12), "multiple of 8"), (dict(c=0), "multiple of 8"),
             (dict(stride=3), "stride 3"), (dict(stride=0), "stride 0"), (dict(h=1 << 21), "out of range"))
    data = (("g", P), ("wt", P), ("dx", P), ("n", 2), ("h", 6), ("w", 5), ("c", 16), ("stride", 2), ("s", None))
    _refused("yolo_dwconv3x3_bwd_data", data, shape + ((dict(g=None), "null"), (dict(wt=None), "null"), (dict(dx=None), "null"),
                                                        (dict(g=P + 8), "misaligned"), (dict(dx=P + 2), "misaligned"), (dict(wt=P + 4), "misaligned")))
    weight = (("x", P), ("g", P), ("dw", P), ("ws", P), ("ws_bytes", 1 << 20), ("n", 2), ("h", 6), ("w", 5), ("c", 16), ("stride", 2), ("s", None))
    _refused("yolo_dwconv3x3_bwd_weight", weight, shape + ((dict(x=None), "null"), (dict(g=None), "null"), (dict(dw=None), "null"),
                                                            (dict(ws=None), "null"), (dict(x=P + 8), "misaligned"), (dict(g=P + 8), "misaligned"),
                                                            (dict(ws=P + 8), "misaligned"), (dict(dw=P + 2), "misaligned")))
    need = K.dwconv3x3_bwd_weight_workspace_bytes(2, 6, 5, 16, 2)
    rc, err = _rc("yolo_dwconv3x3_bwd_weight", *[dict(ws_bytes=need - 1).get(k, v) for k, v in weight])
    assert rc == E_WORKSPACE and err.startswith("dwconv3x3_bwd_weight") and "workspace" in err
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    for bad in ((0, 6, 5, 16, 2), (2, 6, 5, 12, 2), (2, 6, 5, 16, 3)):
        assert lib.yolo_dwconv3x3_bwd_weight_workspace_bytes(*bad) == 0 and lib.yolo_last_error().decode().startswith("dwconv3x3_bwd_weight_workspace_bytes")
        assert lib.yolo_dwconv3x3_bwd_weight_pick(*bad, buf, 128) == E_ARG
    assert lib.yolo_dwconv3x3_bwd_weight_pick(2, 6, 5, 16, 2, None, 128) == E_ARG


def test_picks_and_workspace_sizes_are_pinned():
    """The split rule of the weight gradient on the eight cases at the default 256 compute units, and the split cases under two other
    shares.  The workspace is splits x 9 x C doubles; no split is empty and the splits cover the output pixels once."""
    for case, (pick, nbytes) in zip(D.CASES, D.PICKS):
        n, h, w, c, stride = case
        assert K.dwconv3x3_bwd_weight_pick(*case) == pick and K.dwconv3x3_bwd_weight_workspace_bytes(*case) == nbytes, \
            (case, K.dwconv3x3_bwd_weight_pick(*case), K.dwconv3x3_bwd_weight_workspace_bytes(*case))
        p = D.parse_pick(pick)
        ho, wo = D.out_hw(h, w, stride)
        m = n * ho * wo
        assert nbytes == p["splits"] * 9 * c * 8 and p["stride"] == stride
        assert p["width"] == min(c // 8, 256) and p["rows"] == 256 // p["width"] and p["tiles"] == -(-(c // 8) // 256)
        ranges = D.split_ranges(m, pick)
        assert ranges[0][0] == 0 and ranges[-1][1] == m and all(a < b for a, b in ranges)
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))
        assert (p["splits"] - 1) * p["passes"] + p["last"] == -(-m // p["rows"]) and 1 <= p["last"] <= p["passes"]
    for i in D.SPLIT_CASES:
        assert D.parse_pick(D.PICKS[i][0])["splits"] >= 3
    assert D.parse_pick(D.PICKS[5][0])["width"] == 17 and D.parse_pick(D.PICKS[5][0])["passes"] > 1
    try:
        for (i, share), want in D.SPLIT_PICKS.items():
            K.set_launch_cus(share)
            assert K.dwconv3x3_bwd_weight_pick(*D.CASES[i]) == want, (i, share)
    finally:
        K.set_launch_cus(256)
    assert all(D.SPLIT_PICKS[(i, 8)] != D.PICKS[i][0] for i in D.SPLIT_CASES)
    assert K.dwconv3x3_bwd_weight_pick(*D.CASES[6]) == D.PICKS[6][0]


# ---- the ops refuse ---------------------------------------------------------------------------------------------------------------------
def test_op_argument_checks():
    """Every ValueError comes before the "no CPU fallback" RuntimeError."""
    x, ga, be = torch.zeros(2, 16, 4, 4), torch.ones(16), torch.zeros(16)
    wd = torch.zeros(16, 1, 3, 3)
    for args, kw in (((x, torch.zeros(16, 2, 3, 3), ga, be), {}), ((x, torch.zeros(16, 1, 5, 5), ga, be), {}), ((x, wd, ga, be), dict(stride=3)),
                     ((x[:, :12], wd[:12], ga[:12], be[:12]), {}), ((x, wd, ga, be), dict(training=False)), ((x, wd, ga, be), dict(momentum=None)),
                     ((x, wd, ga, be), dict(act="leaky")), ((x, wd, ga, be), dict(act="relu")), ((x, wd.double(), ga, be), {}),
                     ((x, wd, ga[:8], be), {}), ((x, wd[:8], ga, be), {}), ((x[0], wd, ga, be), {}), ((x[:1, :, :1, :1], wd, ga, be), {}),
                     ((x, wd, ga, be), dict(eps=-1.0)), ((x, wd, ga, be, torch.zeros(8)), {})):
        with pytest.raises(ValueError, match="dw_bn_block"):
            Y.dw_bn_block(*args, **kw)
    w1, w3 = torch.zeros(16, 16, 1, 1), torch.zeros(16, 16, 3, 3)
    for args, kw in (((x, w3, ga, be), dict(stride=3)), ((x, w1, ga, be), dict(stride=2)), ((x, torch.zeros(16, 16, 5, 5), ga, be), {}),
                     ((x, w1[:12], ga[:12], be[:12]), {}), ((x, w1, ga, be), dict(training=False)), ((x, w1, ga, be), dict(momentum=None)),
                     ((x, w1[:, :8], ga, be), {}), ((x, w1, ga, be.double()), {}), ((x[:1, :, :1, :1], w1, ga, be), {})):
        with pytest.raises(ValueError, match="conv_bn_relu6_block"):
            Y.conv_bn_relu6_block(*args, **kw)
    res = torch.zeros(2, 16, 4, 4)
    for args, kw in (((x, w3, ga, be), {}), ((x, w1[:12], ga[:12], be[:12]), {}), ((x, w1, ga, be), dict(training=False)),
                     ((x, w1, ga, be), dict(momentum=None)), ((x, w1, ga, be, None, None, res[:, :8]), {}), ((x, w1, ga, be, None, None, res[:, :, :2]), {}),
                     ((x, w1, ga, be, None, None, "x"), {}), ((x, w1, ga[:8], be), {})):
        with pytest.raises(ValueError, match="project_bn_block"):
            Y.project_bn_block(*args, **kw)
    for call in (lambda: Y.dw_bn_block(x, wd, ga, be), lambda: Y.dw_bn_block(x, wd, ga, be, stride=2, act="none"),
                 lambda: Y.conv_bn_relu6_block(x, w1, ga, be), lambda: Y.conv_bn_relu6_block(x[:, :3], w3[:, :3], ga, be, stride=2),
                 lambda: Y.project_bn_block(x, w1, ga, be), lambda: Y.project_bn_block(x, w1, ga, be, residual=res)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # what the existing ops keep refusing
    for call in (lambda: Y.conv_bn_block(x, w1, ga, be, act="relu6"), lambda: Y.conv_block(x, w1, act="relu6"),
                 lambda: Y.down_bn_block(x, w3, ga, be, act="relu6")):
        with pytest.raises(ValueError):
            call()


# ---- the restatements with the rounding off against float64 autograd -------------------------------------------------------------------
def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=F64) - want).max()) / max(float(np.abs(want).max()), 1.0)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=F64))).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _operands64(case, seed=0):
    """float64 operands with an asymmetric weight: x, w [c, 3, 3], gamma, beta, rm, rv, dy."""
    n, h, wd, c, stride = case
    ho, wo = D.out_hw(h, wd, stride)
    rng = np.random.default_rng(100 + seed)
    return (rng.standard_normal((n, h, wd, c)), rng.standard_normal((c, 3, 3)) / 3.0, rng.uniform(1.5, 2.5, c), 3.0 + rng.standard_normal(c),
            rng.standard_normal(c), rng.uniform(0.5, 2.0, c), rng.standard_normal((n, ho, wo, c)))


def _torch_dw_bn(x, w, gamma, beta, rm, rv, dy, stride, act):
    xt, wt = _nchw(x).requires_grad_(), torch.from_numpy(w.copy()).unsqueeze(1).requires_grad_()
    gt, bt = torch.from_numpy(gamma.copy()).requires_grad_(), torch.from_numpy(beta.copy()).requires_grad_()
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    y = F.batch_norm(F.conv2d(xt, wt, None, stride, 1, 1, wt.shape[0]), rmt, rvt, gt, bt, True, N.MOMENTUM, N.EPS)
    if act != "none":
        y = F.hardtanh(y, 0.0, 6.0)
    y.backward(_nchw(dy))
    return dict(y=_nhwc(y), dx=_nhwc(xt.grad), dw=wt.grad[:, 0].numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy(), rm=rmt.numpy(), rv=rvt.numpy())


def _restated_dw_bn(x, w, gamma, beta, rm, rv, dy, stride, act, inject=None):
    z = D.dw_forward(x, w, stride, False)
    y, cache = D.bn_forward(z, gamma, beta, D.RELU6 if act != "none" else "none", rm, rv, False)
    g, dgamma, dbeta = D.bn_backward(dy, cache, False)
    return dict(y=y, dx=D.dw_bwd_data(g, w, x.shape, stride, False, inject), dw=D.dw_bwd_weight(x, g, stride, False)["dw"], dgamma=dgamma,
                dbeta=dbeta, rm=cache["rm"], rv=cache["rv"], g=g)


@pytest.mark.parametrize("act", ["relu6", "none"])
@pytest.mark.parametrize("case", D.SMALL_CASES, ids=D.case_id)
def test_depthwise_restatement_equals_torch_float64(case, act):
    """conv2d(groups=c) -> batch_norm(training=True) -> hardtanh(0, 6): output, running statistics and the gradients of x, the weight,
    gamma and beta.  gamma is ~2 and beta ~3, so that both bounds of the clamp are met by a share of the values."""
    ops = _operands64(case)
    want = _torch_dw_bn(*ops, case[4], act)
    got = _restated_dw_bn(*ops, case[4], act)
    for name in want:
        assert _rel(got[name], want[name]) <= AUTOGRAD_BOUND, name
        assert np.abs(want[name]).max() > 0, name
    assert got["dw"].shape == (case[3], 3, 3) and got["dx"].shape == ops[0].shape
    if act == "relu6" and case[1] * case[2] > 4:
        assert 0.02 < float((want["y"] == 0).mean()) and 0.02 < float((want["y"] == 6).mean())


def test_a_flipped_tap_shows():
    """The weights are asymmetric: the restatement with the weight flipped is far from autograd, in z and in dx."""
    case = D.SMALL_CASES[2]
    x, w, gamma, beta, rm, rv, dy = _operands64(case)
    z, dx, dw = D.torch_dw_reference(x, w, dy, case[4])
    assert _rel(D.dw_forward(x, w, case[4], False), z) <= AUTOGRAD_BOUND and _rel(D.dw_bwd_data(dy, w, x.shape, case[4], False), dx) <= AUTOGRAD_BOUND
    assert _rel(D.dw_bwd_weight(x, dy, case[4], False)["dw"], dw) <= AUTOGRAD_BOUND
    for flipped in (w[:, ::-1], w[:, :, ::-1], w.transpose(0, 2, 1)):
        assert _rel(D.dw_forward(x, flipped, case[4], False), z) > 0.05 and _rel(D.dw_bwd_data(dy, flipped, x.shape, case[4], False), dx) > 0.05


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
def test_projection_restatement_equals_torch_float64(residual):
    """x + batch_norm(conv1x1(x)) (and without the add): output, running statistics and every gradient; the residual's is dy."""
    rng = np.random.default_rng(11)
    n, h, wd, cin, cout = 2, 5, 3, 24, 16
    x, w = rng.standard_normal((n, h, wd, cin)), rng.standard_normal((cout, cin)) / 5.0
    r, dy = rng.standard_normal((n, h, wd, cout)), rng.standard_normal((n, h, wd, cout))
    gamma, beta, rm, rv = rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout), rng.standard_normal(cout), rng.uniform(0.5, 2.0, cout)
    xt, wt = _nchw(x).requires_grad_(), torch.from_numpy(w.copy()).reshape(cout, cin, 1, 1).requires_grad_()
    rt = _nchw(r).requires_grad_()
    gt, bt = torch.from_numpy(gamma.copy()).requires_grad_(), torch.from_numpy(beta.copy()).requires_grad_()
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    y = F.batch_norm(F.conv2d(xt, wt), rmt, rvt, gt, bt, True, N.MOMENTUM, N.EPS)
    y = rt + y if residual else y
    y.backward(_nchw(dy))
    z = D.pw_forward(x, w, False)
    y3, cache = D.bn_forward(z, gamma, beta, "none", rm, rv, False)
    g, dgamma, dbeta = D.bn_backward(dy, cache, False)
    dx, dw = D.pw_backward(x, w, g, False)
    for name, got, want in (("y", y3 + r if residual else y3, _nhwc(y)), ("dx", dx, _nhwc(xt.grad)), ("dw", dw, wt.grad[:, :, 0, 0].numpy()),
                            ("dgamma", dgamma, gt.grad.numpy()), ("dbeta", dbeta, bt.grad.numpy()), ("rm", cache["rm"], rmt.numpy()),
                            ("rv", cache["rv"], rvt.numpy())):
        assert _rel(got, want) <= AUTOGRAD_BOUND and np.abs(want).max() > 0, name
    if residual:
        assert np.array_equal(_nhwc(rt.grad), dy)


# ---- fault injections that must fail --------------------------------------------------------------------------------------------------------
def test_wrong_parity_at_stride_2_fails():
    for case in (D.SMALL_CASES[2], D.SMALL_CASES[3]):
        x, w, gamma, beta, rm, rv, dy = _operands64(case)
        _, dx, _ = D.torch_dw_reference(x, w, dy, 2)
        assert _rel(D.dw_bwd_data(dy, w, x.shape, 2, False), dx) <= AUTOGRAD_BOUND
        assert _rel(D.dw_bwd_data(dy, w, x.shape, 2, False, inject="parity"), dx) > 0.05
    xi, wi, gi = D.integer_operands(D.CASES[1])
    _, dxi, _ = D.torch_dw_reference(xi, wi, gi, 2)
    assert np.array_equal(D.dw_bwd_data(gi, wi, xi.shape, 2), dxi) and not np.array_equal(D.dw_bwd_data(gi, wi, xi.shape, 2, inject="parity"), dxi)


@pytest.mark.parametrize("i", D.SPLIT_CASES)
def test_dropped_split_partial_fails(i):
    """Leaving out any one split's output pixels moves the weight gradient of every channel by far more than its bound, on the random
    operands and (bit-exactly seen) on the integer ones."""
    case = D.CASES[i]
    n, h, w, c, stride = case
    ho, wo = D.out_hw(h, w, stride)
    ranges = D.split_ranges(n * ho * wo, D.PICKS[i][0])
    x, wt, g = D.random_operands(case)
    xi, wi, gi = D.integer_operands(case)
    full, fulli = D.dw_bwd_weight(x, g, stride), D.dw_bwd_weight(xi, gi, stride)
    _, _, dwi = D.torch_dw_reference(xi, wi, gi, stride)
    assert np.array_equal(fulli["dw"], dwi) and float(fulli["A"].max()) < 2 ** 24
    bound = D.dw_weight_bound(full)
    assert N.ratio(full["dw"], full["S"], bound) <= 1.0
    for a, b in (ranges[0], ranges[len(ranges) // 2], ranges[-1]):
        dropped = D.dw_bwd_weight(x, g, stride, drop=(a, b))
        assert float((np.abs(dropped["dw"].astype(F64) - full["S"]) / bound).max()) > 100.0, (a, b)
        assert not np.array_equal(D.dw_bwd_weight(xi, gi, stride, drop=(a, b))["dw"], dwi), (a, b)


def test_slope_of_one_at_the_upper_bound_fails():
    """On operands that hit a == 0 and a == 6 the restated ga equals torch's hardtanh backward (zero at both bounds); with the slope
    taken as 1 at a == 6 it does not, and dbeta and g move.  lo = 0, hi = +inf is torch's ReLU rule at a == 0."""
    case = N.CASES[1]
    z, dy, saved = D.clamp_edge_operands(case)
    a = torch.from_numpy((z + saved[3]).astype(F64)).requires_grad_()
    assert bool((a == 0).any()) and bool((a == 6).any()) and bool((a == 5).any()) and bool((a == 1).any()) and bool((a > 6).any()) and bool((a < 0).any())
    y = F.hardtanh(a, 0.0, 6.0)
    y.backward(torch.from_numpy(dy.astype(F64)))
    assert np.array_equal(D.clamp_forward(z, saved), y.detach().numpy())
    good, bad = D.clamp_terms(dy, z, saved), D.clamp_terms(dy, z, saved, inject="hi")
    assert np.array_equal(good["ga"], a.grad.numpy()) and not np.array_equal(bad["ga"], a.grad.numpy())
    assert not np.array_equal(good["B"], bad["B"]) and 0.1 < good["clamped"] < 0.9
    c1, c2 = N.centre(good, z.shape[0], True)
    assert not np.array_equal(N.backward_apply(good, saved, c1, c2), N.backward_apply(bad, saved, *N.centre(bad, z.shape[0], True)))
    a0 = torch.from_numpy((z + saved[3]).astype(F64)).requires_grad_()
    F.relu(a0).backward(torch.from_numpy(dy.astype(F64)))
    relu = D.clamp_terms(dy, z, saved, 0.0, np.inf)
    assert np.array_equal(relu["ga"], a0.grad.numpy()) and np.array_equal(D.clamp_forward(z, saved, 0.0, np.inf), F.relu(a0).detach().numpy())


def test_rounding_points():
    """With rounding on: z, y, g and dx are bf16 values, dw float32; on integer operands every restated value equals float64 autograd."""
    case = D.CASES[2]
    x, w, g = D.random_operands(case)
    z, dx, dw = D.dw_forward(x, w, 2), D.dw_bwd_data(g, w, x.shape, 2), D.dw_bwd_weight(x, g, 2)["dw"]
    assert np.array_equal(D.bf16(z), z) and np.array_equal(D.bf16(dx), dx) and dw.dtype == np.float32 and z.dtype == np.float32
    zr, dxr, dwr = D.torch_dw_reference(x, w, g, 2)
    assert 0 < _rel(z, zr) < 2.0 ** -7 and 0 < _rel(dx, dxr) < 2.0 ** -7 and _rel(dw, dwr) < 2.0 ** -22
    for c in D.CASES[:6]:
        xi, wi, gi = D.integer_operands(c)
        zi, dxi, dwi = D.torch_dw_reference(xi, wi, gi, c[4])
        assert np.array_equal(D.dw_forward(xi, wi, c[4]), zi) and np.array_equal(D.dw_bwd_data(gi, wi, xi.shape, c[4]), dxi)
        assert np.array_equal(D.dw_bwd_weight(xi, gi, c[4])["dw"], dwi) and float(np.abs(dxi).max()) < 256


# ---- a composed inverted residual ---------------------------------------------------------------------------------------------------------
def _block_params(rng, cin, hid, cout):
    p = dict(w_exp=rng.standard_normal((hid, cin)) / cin ** 0.5, w_dw=rng.standard_normal((hid, 3, 3)) / 3.0,
             w_proj=rng.standard_normal((cout, hid)) / hid ** 0.5)
    for i, c in ((1, hid), (2, hid), (3, cout)):
        p["g%d" % i], p["b%d" % i] = rng.uniform(0.5, 1.5, c), (3.0 if i < 3 else 0.0) + rng.standard_normal(c)
        p["rm%d" % i], p["rv%d" % i] = rng.standard_normal(c), rng.uniform(0.5, 2.0, c)
    return p


def _torch_block(x, p, stride, residual, dy):
    """The block in oracle.mobilenet._inverted_residual's layer order (1x1 expand BN ReLU6 -> dw3x3 BN ReLU6 -> 1x1 BN, + identity) with
    F.batch_norm(training=True), under float64 autograd."""
    t = {k: torch.from_numpy(np.asarray(v, dtype=F64).copy()) for k, v in p.items()}
    for k in t:
        if not k.startswith("r"):
            t[k].requires_grad_()
    bn = lambda v, i: F.batch_norm(v, t["rm%d" % i], t["rv%d" % i], t["g%d" % i], t["b%d" % i], True, N.MOMENTUM, N.EPS)
    xt = _nchw(x).requires_grad_()
    hid = t["w_dw"].shape[0]
    y = F.relu6(bn(F.conv2d(xt, t["w_exp"].reshape(hid, -1, 1, 1)), 1))
    y = F.relu6(bn(F.conv2d(y, t["w_dw"].unsqueeze(1), None, stride, 1, 1, hid), 2))
    y = bn(F.conv2d(y, t["w_proj"].reshape(t["w_proj"].shape[0], hid, 1, 1)), 3)
    y = xt + y if residual else y
    y.backward(_nchw(dy))
    out = {k: (v.grad if v.requires_grad else v).numpy() for k, v in t.items()}
    out.update(y=_nhwc(y), dx=_nhwc(xt.grad))
    return out


@pytest.mark.parametrize("stride,residual", [(1, True), (2, False)], ids=["s1_residual", "s2"])
def test_composed_inverted_residual_equals_float64_autograd(stride, residual):
    """The restated ops composed - expand, depthwise, projection (with x as the residual at stride 1) - against autograd of the same
    block: the output, the gradients of x and of all nine parameters, and the six running tensors, to 1e-10.  PARITY UNPINNED (see the
    module docstring): the block restates the published layer order; torchvision's InvertedResidual is not available."""
    rng = np.random.default_rng(21 + stride)
    n, h, wd, cin, hid = 2, 7, 6, 16, 96
    cout = cin if residual else 24
    ho, wo = D.out_hw(h, wd, stride)
    x, dy, p = rng.standard_normal((n, h, wd, cin)), rng.standard_normal((n, ho, wo, cout)), _block_params(rng, cin, hid, cout)
    want = _torch_block(x, p, stride, residual, dy)
    got = D.inverted_residual(x, p, stride, residual, dy, rounding=False)
    assert set(got) == set(want)
    worst = 0.0
    for name in sorted(want):
        e = _rel(got[name], want[name])
        worst = max(worst, e)
        assert e <= BLOCK_BOUND and np.abs(want[name]).max() > 0, (name, e)
        assert not name.startswith("r") or not np.allclose(want[name], p[name])          # the running statistics moved
    print(f"composed inverted residual stride {stride}: largest |got - want| / max(largest |want|, 1) = {worst:.2e}")
    rounded = D.inverted_residual(D.bf16(x.astype(np.float32)), p, stride, residual, D.bf16(dy.astype(np.float32)), rounding=True)
    for name in ("w_exp", "w_dw", "w_proj", "g1", "b1", "g2", "b2", "g3", "b3"):
        # With the rounding points on, the distance is a rounding-sized one, not a wrong term's (order one).  Its ceiling: bf16 roundings
        # (2^-9 each, <= 2^-6 if a handful add up) and the clamp decisions they flip - a value within 2^-8 |a| <= 0.024 of a bound, at a
        # density of <= 0.2 per unit of a and two bounds a share p <= 0.02 of the elements, changes ga by all of dy: sqrt(p) of a
        # gradient's norm per clamp layer, two layers -> 2^-6 + 2 sqrt(0.02) <= 0.3.
        e = float(np.linalg.norm(rounded[name].astype(F64) - want[name]) / np.linalg.norm(want[name]))
        print(f"  with the rounding points, relative L2 of d{name} against float64 autograd: {e:.3e}")
        assert 0 < e < 0.3, (name, e)
