"""CPU tests of the downsample's backward (csrc/conv_down_bwd.hip, pytorch_yolo_amd.ops.down_block / down_bn_block):
the C ABI table, every refusal through every entry without a device, the ops' argument checks, the pick strings and the workspace
formula, the float64 restatement of tests/_conv_down.py against torch autograd, and the guards of the generators the GPU tests rely on."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd as B
import _conv_down as D
import pytorch_yolo_amd
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.ops import down_block, down_bn_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_conv2d_down_bwd_workspace_bytes", "yolo_conv2d_down_bwd_pick", "yolo_conv2d_down_bwd_weight",
               "yolo_conv2d_down_bwd_data", "yolo_pack_conv_weight_down_dev")
SMALL = [c for i, c in enumerate(D.CASES) if i != D.SPLIT_CASE]


def test_abi_is_additive():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2
    assert ctypes.sizeof(_lib.YoloConvDesc) == 23 * 4 == _lib.load().yolo_abi_sizeof(0)
    assert "models/yolo_base.py:19-44" in text[text.index("backward of the downsample"):text.index("yolo_conv2d_down_bwd_workspace_bytes(const")]
    for name in ("conv2d_down_bwd_workspace_bytes", "conv2d_down_bwd_pick", "conv2d_down_bwd_weight", "conv2d_down_bwd_data",
                 "pack_conv_weight_down_dev"):
        assert name in K.__all__ and callable(getattr(K, name))
    for name in ("down_block", "down_bn_block"):
        assert name in pytorch_yolo_amd.__all__ and getattr(pytorch_yolo_amd, name) is getattr(pytorch_yolo_amd.ops, name)


def test_library_refuses_what_the_downsample_backward_does_not_cover():
    """Every entry validates the forward's descriptor before anything else: YOLO_E_ARG with a message, no GPU needed."""
    lib = _lib.load()
    base = D.CASES[1]
    buf = ctypes.create_string_buffer(256)
    dummy = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(dummy) + 15) & ~15          # never dereferenced: every call below fails in its argument checks
    refusals = (("stride 1", dict(stride=1)), ("ksize 1", dict(ksize=1, kpad=64)), ("ksize 5", dict(ksize=5, pad=2, kpad=640)),
                ("one more row", dict(pad=0)), ("pad 0", dict(pad=0)), ("upsample", dict(upsample2x=1)), ("residual", dict(res=(40, 0))),
                ("pre-add", dict(aux=(40, 0))), ("f32 output", dict(out_dtype=_lib.DT_F32)), ("act", dict(act=_lib.ACT_RELU6)),
                ("act", dict(act=_lib.ACT_SWISH)), ("view", dict(in_c_total=28, in_c_offset=4)), ("cin", dict(cin=20, in_c_total=20)),
                ("cout", dict(cout=36, out_c_total=36)))
    for what, over in refusals:
        d = D.fwd_desc(base, **over)
        if what == "one more row":                    # Conv2dSamePadding on an even map: pad 0 + 1, ceil(h / 2) rows
            d.ho, d.wo = base[1] // 2, base[2] // 2
            assert d.ho == (base[1] - 3) // 2 + 2
        assert lib.yolo_conv2d_down_bwd_pick(ctypes.byref(d), buf, 256) == -1, what
        msg = lib.yolo_last_error().decode()
        assert msg.startswith("conv2d_down_bwd_pick"), msg
        assert lib.yolo_conv2d_down_bwd_workspace_bytes(ctypes.byref(d)) == 0, what
        assert lib.yolo_conv2d_down_bwd_weight(p, p, p, None, p, 1 << 30, ctypes.byref(d), None) == -1, what
        assert lib.yolo_last_error().decode().startswith("conv2d_down_bwd_weight")
        assert lib.yolo_conv2d_down_bwd_data(p, p, p, ctypes.byref(d), None) == -1, what
        assert lib.yolo_last_error().decode().startswith("conv2d_down_bwd_data")
    # a symmetric-pad descriptor with a wrong output size
    d = D.fwd_desc(base)
    d.ho += 1
    assert lib.yolo_conv2d_down_bwd_pick(ctypes.byref(d), buf, 256) == -1
    d = D.fwd_desc(base)
    assert lib.yolo_conv2d_down_bwd_weight(p, p, p, None, p, 16, ctypes.byref(d), None) == -3          # YOLO_E_WORKSPACE
    assert lib.yolo_conv2d_down_bwd_weight(None, p, p, None, p, 1 << 30, ctypes.byref(d), None) == -1
    assert lib.yolo_conv2d_down_bwd_data(p, None, p, ctypes.byref(d), None) == -1
    assert lib.yolo_conv2d_down_bwd_data(p + 2, p, p, ctypes.byref(d), None) == -1                      # misaligned
    assert lib.yolo_pack_conv_weight_down_dev(p, 12, 8, p, None) == -1 and lib.yolo_pack_conv_weight_down_dev(p, 8, 12, p, None) == -1
    assert lib.yolo_pack_conv_weight_down_dev(None, 8, 8, p, None) == -1
    # ... and the stride-1 entries still refuse the stride-2 descriptor (tests/test_conv_bwd_cpu.py pins that; here: both families disagree)
    assert lib.yolo_conv2d_bwd_pick(ctypes.byref(d), buf, 256) == -1


def test_down_block_argument_checks():
    x = torch.zeros((1, 8, 4, 4), dtype=torch.bfloat16)
    w = torch.zeros((8, 8, 3, 3))
    v = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        down_block(x, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        down_block(x, w, v, act="none")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        down_bn_block(x, w, v, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        down_bn_block(x, w, v, v, v, v + 1, training=False)
    for bad_x, bad_w, kw in ((x, torch.zeros((8, 8, 1, 1)), {}),                  # k
                             (x, torch.zeros((8, 8, 5, 5)), {}),
                             (x, torch.zeros((8, 8, 3, 1)), {}),
                             (x, torch.zeros((8, 16, 3, 3)), {}),                 # cin
                             (x[0], w, {}),
                             (x, w, dict(act="relu6")),                           # act
                             (x, torch.zeros((12, 8, 3, 3)), {}),                 # cout % 8
                             (x, w.double(), {})):
        with pytest.raises(ValueError):
            down_block(bad_x, bad_w, **kw)
        with pytest.raises(ValueError):
            down_bn_block(bad_x, bad_w, torch.zeros(bad_w.shape[0]), torch.zeros(bad_w.shape[0]), **kw)
    with pytest.raises(ValueError):
        down_block(x, w, torch.zeros(7))
    with pytest.raises(TypeError):
        down_block(x, w, stride=2)                                                # the op IS the stride: no such argument
    for kw in (dict(momentum=None), dict(momentum=1.5), dict(eps=-1.0), dict(training=False)):
        with pytest.raises(ValueError):
            down_bn_block(x, w, v, v, **kw)
    with pytest.raises(ValueError):
        down_bn_block(x, w, v, torch.zeros(7))
    with pytest.raises(ValueError, match="more than 1 value"):
        down_bn_block(x[:, :, :2, :2], w, v, v)                                  # one output pixel, one image


@pytest.mark.parametrize("index", range(len(D.CASES)), ids=lambda i: D.case_id(D.CASES[i]))
def test_pick_and_workspace(index):
    """The picks are pure functions of the descriptor, pinned by name; the workspace is splits x cout x (9 cin + 1) floats with the
    split rule of the stride-1 weight gradient applied to the n ho wo OUTPUT pixels; the dgrad tiles are the classes' pixel counts."""
    case = D.CASES[index]
    n, h, w, cin, cout, view = case
    d = D.fwd_desc(case)
    pick = K.conv2d_down_bwd_pick(d)
    assert pick == D.PICKS[index] == K.conv2d_down_bwd_pick(d)
    m = re.fullmatch(r"wgrad<(\d+)x128,BK64,tr_b16,s2> grid (\d+)x(\d+) splits (\d+); dgrad<128x(\d+),BK64,parity> grid (\d+)x(\d+) "
                     r"tiles (\d+)\+(\d+)\+(\d+)\+(\d+)", pick)
    assert m, pick
    tm, tn, tmm, splits, dn, gx, gy, *tiles = (int(v) for v in m.groups())
    assert tm == (64 if cout <= 64 else 128) and tn == -(-9 * cin // 128) and tmm == -(-cout // tm)
    assert K.conv2d_down_bwd_workspace_bytes(d) == 4 * splits * cout * (9 * cin + 1)
    ho, wo = D.out_hw(h, w)
    # the same split as the stride-1 rule on a map of the output's size
    same = B.fwd_desc((n, ho, wo, cin, cout, 3, "leaky", torch.bfloat16, None, None))
    assert int(K.conv2d_bwd_pick(same).rsplit(" ", 1)[1]) == splits and (splits >= 2) == (index == D.SPLIT_CASE)
    classes = [(1, 1), (1, 0), (0, 1), (0, 0)]
    assert tiles == [-(-n * ((h + 1 - ph) // 2) * ((w + 1 - pw) // 2) // 128) for ph, pw in classes]
    assert gx == sum(tiles) and dn == (64 if cin <= 64 else 128) and gy == -(-cin // dn)
    if h == 1:
        assert tiles[0] == tiles[1] == 0 and tiles[2] and tiles[3]


def test_split_case_under_other_cu_shares():
    """1024 output pixels are 16 stages: two splits of 8 whatever the compute-unit share (a split is worth a workgroup from 8 stages on);
    the share is restored."""
    d = D.fwd_desc(D.CASES[D.SPLIT_CASE])
    for cus in D.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            assert D.SPLIT_PICKS[cus] in K.conv2d_down_bwd_pick(d)
        finally:
            assert K.set_launch_cus(old) == cus
        assert old == 256


def test_split_count_follows_the_cu_share():
    """D.CU_CASE, the case the GPU test runs under other compute-unit shares: the split count differs between the shares (10, 10, 8),
    the workspace follows it, the dropped-split fault shows in its dW, and the share is restored."""
    n, h, w, cin, cout, view = D.CU_CASE
    d = D.fwd_desc(D.CU_CASE)
    splits = lambda: int(re.search(r"splits (\d+);", K.conv2d_down_bwd_pick(d)).group(1))
    assert splits() == D.CU_CASE_SPLITS[256]
    for cus in D.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            assert splits() == D.CU_CASE_SPLITS[cus]
            assert K.conv2d_down_bwd_workspace_bytes(d) == 4 * D.CU_CASE_SPLITS[cus] * cout * (9 * cin + 1)
        finally:
            assert K.set_launch_cus(old) == cus
        assert old == 256
    assert len(set(D.CU_CASE_SPLITS.values())) > 1 and splits() == D.CU_CASE_SPLITS[256]
    c = D.exact_conditions(D.CU_CASE)
    assert c["integers"] and c["largest_abs_sum"] < 2 ** 24 and c["y_nonpositive"] >= 0.15, c
    x, wt, b, dy = D.exact_operands(D.CU_CASE)
    y = D.forward(x, wt, b)
    good = D.grads(x, wt, dy, y)["dw"]
    bad = D.grads(x, wt, dy, y, inject=("pixels", 640, 1280))["dw"]          # the second of eight splits of 10 stages
    assert float((bad != good).double().mean()) >= 0.01


def test_picks_on_the_darknet_shapes():
    """SPP-640 x 32, the five stride-2 layers: the wgrad splits follow the output pixels, the dgrad grid the input pixels / 4 per class."""
    want = ["wgrad<64x128,BK64,tr_b16,s2> grid 3x1 splits 64; dgrad<128x64,BK64,parity> grid 102400x1 tiles 25600+25600+25600+25600",
            "wgrad<128x128,BK64,tr_b16,s2> grid 5x1 splits 64; dgrad<128x64,BK64,parity> grid 25600x1 tiles 6400+6400+6400+6400",
            "wgrad<128x128,BK64,tr_b16,s2> grid 9x2 splits 29; dgrad<128x128,BK64,parity> grid 6400x1 tiles 1600+1600+1600+1600",
            "wgrad<128x128,BK64,tr_b16,s2> grid 18x4 splits 8; dgrad<128x128,BK64,parity> grid 1600x2 tiles 400+400+400+400",
            "wgrad<128x128,BK64,tr_b16,s2> grid 36x8 splits 2; dgrad<128x128,BK64,parity> grid 400x4 tiles 100+100+100+100"]
    shapes = ((640, 32, 64), (320, 64, 128), (160, 128, 256), (80, 256, 512), (40, 512, 1024))
    assert [K.conv2d_down_bwd_pick(D.fwd_desc((32, h, h, ci, co, None))) for h, ci, co in shapes] == want


@pytest.mark.parametrize("case", SMALL, ids=D.case_id)
def test_restatement_equals_float64_autograd(case):
    """Rounding off: dx (computed one parity class at a time), dW and db of the restatement equal float64 torch autograd of
    leaky_relu(conv2d(x, w, b, stride=2, padding=1), 0.1) to 1e-11, for even and odd maps; T counts the in-bounds terms."""
    n, h, w_, cin, cout, view = case
    x, w, b, dy = D.random_operands(case)
    xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
    y = F.leaky_relu(F.conv2d(xa, wa, ba, stride=2, padding=1), 0.1)
    assert tuple(y.shape[2:]) == D.out_hw(h, w_) == tuple(dy.shape[2:])
    y.backward(dy)
    assert torch.equal(D.forward(x, w, b, rounding=False), y.detach())
    r = D.grads(x, w, dy, y.detach(), rounding=False)
    for name, got, want in (("dx", r["dx"], xa.grad), ("dW", r["dw"], wa.grad), ("db", r["db"], ba.grad)):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-11 * max(scale, 1.0), name
    ho, wo = D.out_hw(h, w_)
    assert float(r["dw_terms"].max()) <= n * ho * wo
    t = r["dx_terms"]
    two = lambda size: 2 if size >= 3 else 1            # an odd pixel has an output pixel on both sides from three pixels on
    assert float(t[:, :, 0::2, 0::2].max()) == cout and float(t.max()) == cout * two(h) * two(w_) and float(t.min()) >= cout
    if h % 2 == 0:                                      # the last (odd) row of an even map has no output row below it
        assert float(t[:, :, h - 1, 0::2].max()) == cout
    if h == 1:
        assert not r["dw"][:, :, 0].any() and not r["dw"][:, :, 2].any() and r["dw"][:, :, 1].any()


def test_chain_restatement_equals_float64_autograd():
    """The chain of tests/_conv_down.py (two downsamples, a residual unit between them, an fp32 head): with rounding off it equals float64
    autograd of the whole network to 1e-9 relative (the batch norms divide by small variances) in every parameter; with rounding on it
    is the GPU chain test's yardstick and stays within a rounding-sized distance (0.1 relative L2, the ceiling of
    tests/test_conv_bwd_cpu.py's chain)."""
    ops = D.chain_operands()
    want = D.chain_autograd64(ops)
    exact = D.chain_restated(ops, rounding=False)
    for name in D.CHAIN_PARAMS:
        assert want[name].any() and B.rel_l2(exact[name], want[name]) <= 1e-9, name
    rounded = D.chain_restated(ops)
    errs = {name: B.rel_l2(rounded[name], want[name]) for name in D.CHAIN_PARAMS}
    print("down chain, float64 with the rounding points vs float64 autograd, relative L2: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(0 < e <= 0.1 for e in errs.values()), errs


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_exact_case_guards(case):
    """The integer cases are exact in fp32 (float64 as the witness: integers everywhere, every sum of |terms| below 2^24), at least
    15 % of y is non-positive and at least 25 % of the dx elements with 128 or more terms need rounding.  Cases 1, 3, 4 and 7 have no such
    element (a pixel has at most 4 cout terms: 64, 16, 8 and 96), so the guard does not bind there."""
    c = D.exact_conditions(case)
    assert c["integers"] and c["largest_abs_sum"] < 2 ** 24, c
    assert c["y_nonpositive"] >= 0.15, c
    if c["dx_terms"] >= B.DX_ROUNDING_FROM_TERMS:
        assert c["dx_rounded"] is not None and c["dx_rounded"] >= 0.25, c
    else:
        assert c["dx_rounded"] is None and D.CASES.index(case) in (0, 2, 3, 6), c


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_injected_faults_show(case):
    """One wrong tap, one dropped stretch of output pixels (a 64-pixel stage; for the split case one whole split) or two swapped parity
    classes change at least 1 % of the elements of the exact dW / dx: the comparison the GPU tests make is not vacuous."""
    n, h, w_, cin, cout, view = case
    x, w, b, dy = D.exact_operands(case)
    y = D.forward(x, w, b)
    good = D.grads(x, w, dy, y)
    ho, wo = D.out_hw(h, w_)
    pixels = n * ho * wo
    lo, hi = 0, min(64, pixels)
    splits = int(re.search(r"splits (\d+)", K.conv2d_down_bwd_pick(D.fwd_desc(case))).group(1))
    if splits >= 2:
        per = -(-(-(-pixels // 64)) // splits) * 64
        lo, hi = per, min(2 * per, pixels)
    # taps whose pixel is inside the image for some output pixel: the corner tap 0 needs a second output row and column
    faults = [("pixels", lo, hi)] + [("tap", t) for t in ((0, 8) if min(ho, wo) > 1 else (4, 8) if h > 1 else (4,))]
    for inject in faults:
        bad = D.grads(x, w, dy, y, inject=inject)["dw"]
        assert float((bad != good["dw"]).double().mean()) >= 0.01, inject
    bad = D.grads(x, w, dy, y, inject=("parity",))["dx"]
    assert float((bad != good["dx"]).double().mean()) >= 0.01
