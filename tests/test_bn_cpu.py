"""CPU tests of the training-mode batch norm (csrc/batchnorm.hip, pytorch_yolo_amd.ops.conv_bn_block): the C ABI table, the argument
checks that need no GPU (dummy pointers that are never dereferenced: every check fires before a launch), the split rule, the numpy
restatement of tests/_bn.py against torch under float64 autograd, and the guards of the generators the GPU tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _bn as N
import pytorch_yolo_amd
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.ops import conv_bn_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_bn_workspace_bytes", "yolo_bn_pick", "yolo_bn_train_stats", "yolo_bn_eval_stats", "yolo_bn_act_fwd", "yolo_bn_act_bwd")
P = 4096          # a dummy pointer: 16-byte aligned, never dereferenced
E_ARG, E_WORKSPACE = -1, -3


def test_abi_table_and_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # additive: no struct, no new version
    assert "models/yolo_base.py:19-44" in text[text.index("training-mode ConvBlock"):text.index("yolo_bn_workspace_bytes(long long")]
    for name in ("bn_workspace_bytes", "bn_pick", "bn_train_stats", "bn_eval_stats", "bn_act_fwd", "bn_act_bwd"):
        assert name in K.__all__ and callable(getattr(K, name))
    assert "conv_bn_block" in pytorch_yolo_amd.__all__ and pytorch_yolo_amd.conv_bn_block is conv_bn_block
    assert "conv_block" in pytorch_yolo_amd.__all__


def test_picks_and_workspace_sizes_are_pinned():
    """The split rule on the six cases at the default 256 compute units, and the split case under two other shares.  The workspace is
    2 C floats (c1 | c2) and splits x 2 x C doubles; no split is empty and the splits cover the rows once."""
    for case, (pick, nbytes) in zip(N.CASES, N.PICKS):
        m, c = N.rows_of(case), case[3]
        assert K.bn_pick(m, c) == pick and K.bn_workspace_bytes(m, c) == nbytes, (case, K.bn_pick(m, c), K.bn_workspace_bytes(m, c))
        p = N.parse_pick(pick)
        assert nbytes == 8 * c + p["splits"] * 2 * c * 8
        assert p["width"] == min(c // 8, 256) and p["rows"] == 256 // p["width"] and p["tiles"] == -(-(c // 8) // 256)
        ranges = N.split_ranges(m, pick)
        assert ranges[0][0] == 0 and ranges[-1][1] == m and all(a < b for a, b in ranges)
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))
        assert (p["splits"] - 1) * p["passes"] + p["last"] == -(-m // p["rows"]) and 1 <= p["last"] <= p["passes"]
    split = N.parse_pick(N.PICKS[N.SPLIT_CASE][0])
    m, c = N.rows_of(N.CASES[N.SPLIT_CASE]), N.CASES[N.SPLIT_CASE][3]
    assert split["splits"] >= 3 and split["last"] < split["passes"] and m % split["rows"]        # ragged last split, ragged last pass
    assert N.parse_pick(N.PICKS[4][0])["tiles"] == 2 and N.CASES[4][3] // 8 % 256 == 1             # the second tile is one chunk wide
    try:
        for share in N.CU_SHARES:
            old = K.set_launch_cus(share)
            assert K.bn_pick(m, c) == N.SPLIT_PICKS[share]
            K.set_launch_cus(old)
    finally:
        K.set_launch_cus(256)
    assert N.SPLIT_PICKS[8] != N.SPLIT_PICKS[64]
    assert K.bn_pick(m, c) == N.PICKS[N.SPLIT_CASE][0]


def _rc(fn, *args):
    rc = getattr(_lib.load(), fn)(*args)
    return rc, _lib.load().yolo_last_error().decode()


def test_entry_argument_checks():
    """Every entry refuses, before any launch: c % 8, an act other than none / LeakyReLU(0.1), pixels < 2 with batch statistics, a null
    or misaligned pointer, a small workspace."""
    lib = _lib.load()
    big = 1 << 20
    assert lib.yolo_bn_workspace_bytes(100, 12) == 0 and "multiple of 8" in lib.yolo_last_error().decode()
    assert lib.yolo_bn_workspace_bytes(0, 8) == 0 and lib.yolo_bn_workspace_bytes(100, 0) == 0
    buf = ctypes.create_string_buffer(64)
    assert lib.yolo_bn_pick(100, 12, buf, 64) == E_ARG and lib.yolo_bn_pick(100, 8, None, 64) == E_ARG
    train = lambda **kw: _rc("yolo_bn_train_stats", *[kw.get(k, v) for k, v in (
        ("z", P), ("pixels", 100), ("c", 16), ("gamma", P), ("beta", P), ("eps", 1e-5), ("momentum", 0.1), ("rm", None), ("rv", None),
        ("saved", P), ("ws", P), ("ws_bytes", big), ("s", None))])
    for kw, msg in ((dict(c=12), "multiple of 8"), (dict(pixels=1), "more than one value"), (dict(z=None), "null"), (dict(gamma=None), "null"),
                    (dict(beta=None), "null"), (dict(saved=None), "null"), (dict(ws=None), "null"), (dict(z=P + 8), "misaligned"),
                    (dict(saved=P + 4), "misaligned"), (dict(ws=P + 8), "misaligned"), (dict(rm=P + 2), "misaligned"), (dict(momentum=1.5), "momentum"),
                    (dict(eps=-1.0), "eps")):
        rc, err = train(**kw)
        assert rc == E_ARG and msg in err, (kw, rc, err)
    rc, err = train(ws_bytes=K.bn_workspace_bytes(100, 16) - 1)
    assert rc == E_WORKSPACE and "workspace" in err
    ev = lambda **kw: _rc("yolo_bn_eval_stats", *[kw.get(k, v) for k, v in (
        ("gamma", P), ("beta", P), ("rm", P), ("rv", P), ("c", 16), ("eps", 1e-5), ("saved", P), ("s", None))])
    for kw, msg in ((dict(c=20), "multiple of 8"), (dict(rm=None), "null"), (dict(rv=None), "null"), (dict(gamma=None), "null"),
                    (dict(saved=None), "null"), (dict(saved=P + 8), "misaligned"), (dict(beta=P + 1), "misaligned")):
        rc, err = ev(**kw)
        assert rc == E_ARG and msg in err, (kw, rc, err)
    fwd = lambda **kw: _rc("yolo_bn_act_fwd", *[kw.get(k, v) for k, v in (
        ("z", P), ("saved", P), ("y", P), ("pixels", 100), ("c", 16), ("act", _lib.ACT_LEAKY01), ("s", None))])
    for kw, msg in ((dict(c=4), "multiple of 8"), (dict(act=_lib.ACT_RELU6), "act"), (dict(act=_lib.ACT_SWISH), "act"), (dict(z=None), "null"),
                    (dict(y=None), "null"), (dict(saved=None), "null"), (dict(y=P + 2), "misaligned"), (dict(pixels=0), "pixels")):
        rc, err = fwd(**kw)
        assert rc == E_ARG and msg in err, (kw, rc, err)
    bwd = lambda **kw: _rc("yolo_bn_act_bwd", *[kw.get(k, v) for k, v in (
        ("dy", P), ("dy_dtype", _lib.DT_BF16), ("z", P), ("saved", P), ("pixels", 100), ("c", 16), ("act", _lib.ACT_LEAKY01), ("batch_stats", 1),
        ("g", P), ("dgamma", P), ("dbeta", P), ("ws", P), ("ws_bytes", big), ("s", None))])
    for kw, msg in ((dict(c=12), "multiple of 8"), (dict(act=_lib.ACT_RELU), "act"), (dict(dy_dtype=_lib.DT_F16), "dy_dtype"),
                    (dict(pixels=1), "more than one value"), (dict(batch_stats=2), "batch_stats"), (dict(dy=None), "null"), (dict(z=None), "null"),
                    (dict(saved=None), "null"), (dict(ws=None), "null"), (dict(dy=P + 8), "misaligned"), (dict(g=P + 8), "misaligned"),
                    (dict(dgamma=P + 2), "misaligned")):
        rc, err = bwd(**kw)
        assert rc == E_ARG and msg in err, (kw, rc, err)
    rc, err = bwd(ws_bytes=8 * 16)
    assert rc == E_WORKSPACE and "workspace" in err


def test_conv_bn_block_argument_checks():
    """The op's own checks: ValueError for shapes, dtypes, stride, act, momentum; RuntimeError for CPU tensors (no fallback)."""
    x, w = torch.zeros(2, 8, 4, 4), torch.zeros(16, 8, 3, 3)
    ga, be, rm, rv = torch.ones(16), torch.zeros(16), torch.zeros(16), torch.ones(16)
    for args, kw in (((x, w, ga, be), dict(stride=2)), ((x, w, ga, be), dict(act="relu")), ((x, w, ga, be), dict(momentum=None)),
                     ((x, w, ga, be), dict(momentum=2.0)), ((x, w, ga, be), dict(eps=-1.0)), ((x, w[:12], ga[:12], be[:12]), {}),
                     ((x, w, ga[:8], be), {}), ((x, w, ga, be.double()), {}), ((x, w, ga, be, rm[:8]), {}), ((x, w, ga, be, rm, rv.half()), {}),
                     ((x, w, ga, be), dict(training=False)), ((x, w, ga, be, rm), dict(training=False)), ((x[:, :4], w, ga, be), {}),
                     ((x, torch.zeros(16, 8, 5, 5), ga, be), {}), ((x, w.double(), ga, be), {}), ((x[0], w, ga, be), {}),
                     ((x[:1, :, :1, :1], w, ga, be), {}), ((x, w, None, be), {})):
        with pytest.raises(ValueError, match="conv_bn_block"):
            conv_bn_block(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv_bn_block(x, w, ga, be, rm, rv)
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # one value per channel passes the checks with running statistics
        conv_bn_block(x[:1, :, :1, :1], w, ga, be, rm, rv, training=False)


@pytest.mark.parametrize("training", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("act", ["leaky", "none"])
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_restatement_equals_torch_float64(case, act, training):
    """Rounding off, the restatement equals F.batch_norm + leaky_relu under float64 autograd to 1e-10 relative: output, the updated running
    statistics (biased variance inside, unbiased in running_var) and the gradients of input, gamma and beta.  Both sides are float64 and
    differ in summation order only: 2 10^4 terms x 2^-53 is below the margin."""
    z, dy, gamma, beta, rm, rv = N.random_operands(case, torch.float32)
    want = N.torch_reference(z, dy, gamma, beta, rm, rv, training, act)
    got = N.restated_block(z, dy, gamma, beta, rm, rv, training, act, rounding=False)
    for name in ("y", "dz", "dgamma", "dbeta", "rm", "rv"):
        scale = max(float(np.abs(want[name]).max()), 1.0)
        assert float(np.abs(got[name] - want[name]).max()) <= 1e-10 * scale, name
        assert np.abs(want[name]).max() > 0
    if training:
        m = z.shape[0]
        assert not np.allclose(want["rm"], rm) and not np.allclose(want["rv"], rv)
        st = N.stats(z, gamma, beta, rm=rm, rv=rv, rounding=False)
        assert np.allclose(st["rv"], 0.9 * rv.astype(np.float64) + 0.1 * st["var64"] * m / (m - 1), rtol=1e-14)
    else:
        assert np.array_equal(want["rm"], rm.astype(np.float64)) and np.array_equal(got["rm"], rm)


def test_rounding_points():
    """With rounding on: the saved vectors are float32, y and g bf16 values, the slope at a == 0 is 0.1, and eval mode centres nothing."""
    case = N.CASES[1]
    z, dy, gamma, beta, rm, rv = N.random_operands(case)
    r = N.restated_block(z, dy, gamma, beta, rm, rv, True, "leaky")
    assert r["saved"].dtype == np.float32 and r["rm"].dtype == np.float32 and r["rv"].dtype == np.float32
    assert np.array_equal(N.bf16(r["y"]), r["y"]) and np.array_equal(N.bf16(r["dz"]), r["dz"])
    a = N.pre_act(z, r["saved"])
    assert a.dtype == np.float32 and np.array_equal(r["y"], N.bf16(np.where(a > 0, a, np.float32(0.1) * a)))
    saved = r["saved"].copy()
    saved[2], saved[3] = 0.0, 0.0                                            # a == 0 everywhere: the slope is the package's 0.1
    t = N.backward_terms(dy, z, saved)
    assert np.array_equal(t["ga"], dy * np.float32(0.1)) and t["nonpositive"] == 1.0
    e = N.restated_block(z, dy, gamma, beta, rm, rv, False, "leaky")
    assert not e["c1"].any() and not e["c2"].any() and np.array_equal(e["rm"], rm) and np.array_equal(e["rv"], rv)
    assert r["c1"].any() and r["c2"].any()


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_exact_generator_guards(case):
    """What makes the exact GPU test a test: z holds odd integers in [-7, 7] with two distinct values per channel, S1 and S2 are
    integers far below 2^53, and leaving out ONE row - or one split's partial - changes var of EVERY channel."""
    z, gamma, beta, rm, rv = N.exact_operands(case)
    m, c = z.shape
    st = N.stats(z, gamma, beta, rm=rm, rv=rv)
    assert np.array_equal(st["s1"], np.round(st["s1"])) and float(st["s2"].max()) <= 49 * m < 2 ** 53 and float(st["s2"].min()) >= m
    assert bool((st["var"] > 0).all())
    for row in (0, m // 2, m - 1):
        dropped = N.stats(z, gamma, beta, drop=(row, row + 1))
        assert bool((dropped["var"] != st["var"]).all()), row
    ranges = N.split_ranges(m, K.bn_pick(m, c))
    for a, b in ranges[:1] + ranges[-1:] if len(ranges) > 1 else []:
        dropped = N.stats(z, gamma, beta, drop=(a, b))
        assert bool((dropped["var"] != st["var"]).all()), (a, b)


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_random_generator_guards(case):
    """The random operands cancel in S2 / M - mean^2 (some channel has mean^2 above 4 var) and at least 15 % of a is non-positive."""
    z, dy, gamma, beta, rm, rv = N.random_operands(case)
    st = N.stats(z, gamma, beta)
    assert float((st["mean64"] ** 2 / st["var64"]).max()) > 4.0
    for saved in (st["saved"], N.eval_saved(gamma, beta, rm, rv)):
        assert N.backward_terms(dy, z, saved)["nonpositive"] >= 0.15


def test_chain_restatement_equals_float64_autograd():
    """The two conv_bn_block layers and the head: with rounding off the restated chain equals float64 autograd of conv -> batch_norm(
    training=True) -> leaky_relu to 1e-9 relative in every parameter gradient; with rounding on (the GPU test's yardstick) its distance
    is a rounding-sized one - bf16 roundings of 2^-9 and the LeakyReLU slopes they flip - below 0.1; a dropped tensor is off by order
    one."""
    import _conv_bwd as B
    ops = N.chain_operands()
    want = N.chain_autograd64(ops)
    exact = N.chain_restated(ops, rounding=False)
    rounded = N.chain_restated(ops)
    for name in N.CHAIN_PARAMS:
        assert want[name].any() and B.rel_l2(exact[name], want[name]) <= 1e-9, name
        e = B.rel_l2(rounded[name], want[name])
        print(f"bn chain, float64 with the rounding points vs float64 autograd, relative L2 of d{name}: {e:.3e}")
        assert 0 < e <= 0.1, (name, e)
    for lay in rounded["layers"]:
        assert 0.15 < float((lay["y"] <= 0).double().mean()) < 0.85
