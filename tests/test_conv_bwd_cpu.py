"""CPU tests of the conv backward (csrc/conv_bwd.hip, pytorch_yolo_amd.ops.conv_block): the float64 restatement of tests/_conv_bwd.py
against torch autograd, the layout of the transposed weight pack, the C ABI table, the argument checks that need no GPU, the split
rule, and the guards of the case generators the GPU tests rely on."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd as B
import pytorch_yolo_amd
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.ops import conv_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_conv2d_bwd_workspace_bytes", "yolo_conv2d_bwd_pick", "yolo_conv2d_bwd_prepare", "yolo_conv2d_bwd_weight",
               "yolo_conv2d_bwd_data", "yolo_pack_conv_weight_dev")
SMALL = [c for i, c in enumerate(B.CASES) if i != B.SPLIT_CASE]     # the 12,800-pixel case is checked once, where it matters


fwd_desc = B.fwd_desc


@pytest.mark.parametrize("case", SMALL, ids=B.case_id)
def test_restatement_equals_float64_autograd(case):
    """Rounding off: dx, dW and db of the restatement - dx being a FORWARD conv with the flipped, transposed weights - equal float64
    torch autograd of leaky_relu(conv2d(x, w, b, padding=k//2), 0.1) (act none: of the conv) to 1e-11."""
    n, h, w_, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
    y = F.conv2d(xa, wa, ba, padding=k // 2)
    if act == "leaky":
        y = F.leaky_relu(y, 0.1)
    y.backward(dy)
    assert torch.equal(B.forward(x, w, b, k, act, rounding=False), y.detach())
    r = B.grads(x, w, dy, y.detach(), k, act, rounding=False)
    for name, got, want in (("dx", r["dx"], xa.grad), ("dW", r["dw"], wa.grad), ("db", r["db"], ba.grad)):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-11 * max(scale, 1.0), name
    # the bound quantities: T counts the in-bounds terms
    assert float(r["dw_terms"].max()) <= n * h * w_ and float(r["dx_terms"].max()) == cout * min(k, h) * min(k, w_)
    if h == 1:
        assert not r["dw"][:, :, 0].any() and not r["dw"][:, :, 2].any() and r["dw"][:, :, 1].any()    # only centre-row taps are in bounds


def test_chain_restatement_equals_float64_autograd():
    """The five-layer chain of tests/_conv_bwd.py (max-pool, upsample, concat and a two-consumer tensor between the layers): with
    rounding off, chain_restated - forward() / grads() per layer, the glue written out - equals float64 autograd of the whole network
    to 1e-11 in every parameter, x0 and r.  With rounding on it is the yardstick of the GPU chain test, so its own distance from float64
    autograd has to be a rounding-sized one.  Two parts: a gradient passes at most eight bf16 roundings of 2^-9 each (<= 2^-6 even if
    they added up linearly), and a LeakyReLU whose y the roundings moved across zero changes its g by 0.9 dy - with a share p of such
    elements in a layer that is 0.9 sqrt(p) / sqrt(0.505) = 1.27 sqrt(p) of the norm of g (half the slopes are 1, half 0.1).  The test
    counts p (below 0.4 %: |dy| 2^-9-sized against y of order one) and asserts 2^-6 + 1.27 sqrt(largest p) <= 0.1 as the ceiling; a
    dropped tensor or a wrong slice is off by order one."""
    ops = B.chain_operands()
    dw, db, gx0, gr = B.chain_autograd64(ops)
    exact = B.chain_restated(ops, rounding=False)
    for got, want in list(zip(exact["dw"], dw)) + list(zip(exact["db"], db)) + [(exact["x0_grad"], gx0), (exact["r_grad"], gr)]:
        assert want.any() and float((got - want).abs().max()) <= 1e-11 * max(float(want.abs().max()), 1.0)
    rounded = B.chain_restated(ops)
    errs = [B.rel_l2(g, w_) for g, w_ in list(zip(rounded["dw"], dw)) + list(zip(rounded["db"], db))]
    print("chain, float64 with the rounding points vs float64 autograd, relative L2 of dW1..5, db1..5: " + " ".join(f"{e:.2e}" for e in errs))
    flipped = [float(((cr["y"] > 0) != (ce["y"] > 0)).double().mean()) for cr, ce in zip(rounded["calls"][:3], exact["calls"][:3])]
    print("share of LeakyReLU outputs on the other side of zero, layers 1-3: " + " ".join(f"{100 * p:.3f} %" for p in flipped))
    assert max(flipped) < 0.004 and 2.0 ** -6 + 1.27 * max(flipped) ** 0.5 <= 0.1
    assert all(0 < e <= 0.1 for e in errs), errs
    assert all(c["r"]["dx"].any() for c in rounded["calls"]) and rounded["f_grads"][0].any() and rounded["f_grads"][1].any()


def test_rounding_points():
    """With rounding on, g is the fp32 product rounded to bf16 (slope 0.1f at y <= 0, torch's convention at y == 0) and dx a bf16 value."""
    case = B.CASES[0]
    n, h, w_, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    y = B.forward(x, w, b, k, act)
    y[0, 0, 0, 0] = 0.0
    r = B.grads(x, w, dy, y, k, act)
    want = torch.where(y > 0, dy.float(), dy.float() * torch.tensor(0.1, dtype=torch.float32)).to(torch.bfloat16).double()
    assert torch.equal(r["g"], want) and r["g"][0, 0, 0, 0] == want[0, 0, 0, 0] != dy[0, 0, 0, 0]
    assert B.needs_rounding(r["g"]) == 0 and B.needs_rounding(r["dx"]) == 0 and B.needs_rounding(r["dx_sum"]) > 0.9


@pytest.mark.parametrize("k,cout,cin_w", [(3, 5, 6), (1, 18, 16), (3, 40, 24)])
def test_transposed_pack_layout(k, cout, cin_w):
    """The matrix of the data gradient is the HOST packer applied to w.flip(2, 3).transpose(0, 1): row ci, column (kh k + kw) cg + co
    holds bf16(W[co][ci][k-1-kh][k-1-kw]); rows beyond cin_w, channels beyond cout and columns beyond k k cg are zero."""
    w = torch.randn((cout, cin_w, k, k), generator=torch.Generator().manual_seed(5))
    cg = K.roundup(cout, 8)
    packed, _, kpad, cout_pad = K.pack_conv_weight(w.flip(2, 3).transpose(0, 1), None, cg)
    assert tuple(packed.shape) == (K.roundup(cin_w, 128), K.roundup(k * k * cg, 64)) == (cout_pad, kpad)
    m = packed.float()
    wb = w.to(torch.bfloat16).float()
    for ci, co, kh, kw in ((0, 0, 0, 0), (cin_w - 1, cout - 1, k - 1, 0), (1, 2, k // 2, k - 1)):
        assert m[ci, (kh * k + kw) * cg + co] == wb[co, ci, k - 1 - kh, k - 1 - kw]
    assert not m[cin_w:].any() and not m[:, k * k * cg:].any()
    assert not m[:, :k * k * cg].reshape(cout_pad, k * k, cg)[:, :, cout:].any()
    # the library's own host packer (the twin the device packer is compared with) agrees with the torch one
    out = torch.empty((cout_pad, kpad), dtype=torch.bfloat16)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    rc = _lib.load().yolo_pack_conv_weight_f32(wt.data_ptr(), cin_w, cout, k, cg, cout_pad, kpad, out.data_ptr())
    assert rc == 0 and torch.equal(out.view(torch.int16), packed.view(torch.int16))


def test_abi_is_additive():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2
    assert ctypes.sizeof(_lib.YoloConvDesc) == 23 * 4 == _lib.load().yolo_abi_sizeof(0)
    assert "models/yolo_base.py:19-44" in text[text.index("backward of ConvBlock.forward"):text.index("yolo_conv2d_bwd_workspace_bytes(const")]
    for name in ("conv2d_bwd_workspace_bytes", "conv2d_bwd_pick", "conv2d_bwd_prepare", "conv2d_bwd_weight", "conv2d_bwd_data", "pack_conv_weight_dev"):
        assert name in K.__all__ and callable(getattr(K, name))


def test_conv_block_argument_checks():
    assert "conv_block" in pytorch_yolo_amd.__all__ and pytorch_yolo_amd.conv_block is conv_block
    x = torch.zeros((1, 8, 4, 4), dtype=torch.bfloat16)
    w = torch.zeros((8, 8, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv_block(x, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv_block(x, w, torch.zeros(8), act="none", out_dtype=torch.float32)
    for bad_x, bad_w, kw in ((x, torch.zeros((8, 8, 5, 5)), {}),                  # k
                             (x, torch.zeros((8, 8, 3, 1)), {}),
                             (x, torch.zeros((8, 16, 3, 3)), {}),                 # cin
                             (x[0], w, {}),
                             (x, w, dict(act="relu6")),                           # act
                             (x, w, dict(stride=2)),                              # stride
                             (x, w, dict(out_dtype=torch.float16)),
                             (x, torch.zeros((12, 8, 3, 3)), {}),                 # bf16 output needs cout % 8 == 0
                             (x, w.double(), {})):
        with pytest.raises(ValueError):
            conv_block(bad_x, bad_w, **kw)
    with pytest.raises(ValueError):
        conv_block(x, w, torch.zeros(7))


def test_library_refuses_what_the_backward_does_not_cover():
    """Every entry validates the forward's descriptor before anything else: YOLO_E_ARG with a message, no GPU needed."""
    lib = _lib.load()
    base = B.CASES[0]
    buf = ctypes.create_string_buffer(256)
    dummy = ctypes.create_string_buffer(128)
    p = (ctypes.addressof(dummy) + 15) & ~15          # never dereferenced: every call below fails in its argument checks
    for what, over in (("stride", dict(stride=2)), ("ksize", dict(ksize=5, pad=2, kpad=640)), ("upsample", dict(upsample2x=1)),
                       ("residual", dict(res=(40, 0))), ("pre-add", dict(aux=(40, 0))), ("act", dict(act=_lib.ACT_RELU6)),
                       ("act", dict(act=_lib.ACT_SWISH)), ("view", dict(in_c_total=28, in_c_offset=4)), ("pad", dict(pad=0))):
        d = fwd_desc(base, **over)
        if what == "pad":
            d.ho, d.wo = d.h, d.w
        assert lib.yolo_conv2d_bwd_pick(ctypes.byref(d), buf, 256) == -1, what
        msg = lib.yolo_last_error().decode()
        assert msg.startswith("conv2d_bwd_pick"), msg
        assert lib.yolo_conv2d_bwd_workspace_bytes(ctypes.byref(d)) == 0
        assert lib.yolo_conv2d_bwd_prepare(p, _lib.DT_BF16, p, p, ctypes.byref(d), None) == -1, what
        assert lib.yolo_conv2d_bwd_weight(p, p, p, None, p, 1 << 30, ctypes.byref(d), None) == -1, what
        assert lib.yolo_conv2d_bwd_data(p, p, p, ctypes.byref(d), None) == -1, what
    d = fwd_desc(base)
    assert lib.yolo_conv2d_bwd_prepare(p, 7, p, p, ctypes.byref(d), None) == -1                    # dy dtype
    assert lib.yolo_conv2d_bwd_weight(p, p, p, None, p, 16, ctypes.byref(d), None) == -3          # YOLO_E_WORKSPACE
    assert lib.yolo_pack_conv_weight_dev(p, 8, 8, 5, 8, 128, 256, 0, p, None) == -1
    assert lib.yolo_pack_conv_weight_dev(p, 40, 24, 3, 24, 128, 384, 1, p, None) == -1             # transposed: cin is g's channel count


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_pick_and_workspace(case):
    """The split rule is a pure function of the descriptor: the pick names tile, grid and splits, and the workspace is
    splits x cout x (k k cin + 1) floats.  Case 6 (12,800 pixels, 2 tiles) splits its reduction."""
    n, h, w, cin, cout, k, act, dt, view, oview = case
    d = fwd_desc(case)
    pick = K.conv2d_bwd_pick(d)
    m = re.fullmatch(r"wgrad<(\d+)x128,BK64,tr_b16> grid (\d+)x(\d+) splits (\d+)", pick)
    assert m, pick
    tm, tn, tmm, splits = (int(v) for v in m.groups())
    assert tm == (64 if cout <= 64 else 128) and tn == -(-k * k * cin // 128) and tmm == -(-cout // tm)
    assert K.conv2d_bwd_workspace_bytes(d) == 4 * splits * cout * (k * k * cin + 1)
    steps = -(-n * h * w // 64)
    assert 1 <= splits <= max(1, steps // 8) and K.conv2d_bwd_pick(d) == pick
    if case is B.CASES[B.SPLIT_CASE] or case is B.CASES[B.WIDE_SPLIT_CASE]:
        assert splits >= 2


def test_picks_of_the_wide_tile_cases():
    """Cases 9-15 by name (256 compute units): the 128x128 tile on a 2x2 grid, with three and with two full column tiles, with a
    split reduction, and the two heads' 64- and 128-row tiles."""
    wide = "wgrad<128x128,BK64,tr_b16> "
    want = [wide + "grid 2x2 splits 1", wide + "grid 3x1 splits 1", wide + "grid 2x1 splits 1", wide + "grid 3x2 splits 4",
            "wgrad<64x128,BK64,tr_b16> grid 1x1 splits 1", wide + "grid 2x1 splits 1", wide + "grid 2x1 splits 1"]
    assert [K.conv2d_bwd_pick(fwd_desc(c)) for c in B.CASES[8:]] == want
    assert B.CASES[B.WIDE_SPLIT_CASE][:6] == (5, 20, 20, 32, 136, 3)
    assert int(K.conv2d_bwd_pick(fwd_desc(B.CASES[B.WIDE_SPLIT_CASE])).rsplit(" ", 1)[1]) == min(-(-512 // 6), 32 // 8) >= 2


def _splits(case):
    return int(K.conv2d_bwd_pick(fwd_desc(case)).rsplit(" ", 1)[1])


@pytest.mark.parametrize("index", [B.SPLIT_CASE, B.WIDE_SPLIT_CASE], ids=lambda i: B.case_id(B.CASES[i]))
def test_split_count_follows_the_cu_share(index):
    """The split count is sized against the thread's compute-unit share: under B.CU_SHARES (the values the GPU test runs) at least one
    count differs from the 256-CU one, the workspace follows it, and the old share comes back."""
    case = B.CASES[index]
    n, h, w, cin, cout, k, act, dt, view, oview = case
    d = fwd_desc(case)
    base = _splits(case)
    counts = []
    for cus in B.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            counts.append(_splits(case))
            assert K.conv2d_bwd_workspace_bytes(d) == 4 * counts[-1] * cout * (k * k * cin + 1)
        finally:
            assert K.set_launch_cus(old) == cus
    assert old == 256 and _splits(case) == base
    assert any(c != base for c in counts) and all(c >= 1 for c in counts), (base, counts)
    if index == B.WIDE_SPLIT_CASE:       # 32 stages over 3 splits: 11, 11 and a short last split of 10 stages, the very last one partial
        assert (base, counts[0]) == (4, 3) and n * h * w % 64


def test_split_rule_on_the_measured_shapes():
    """SPP-640 x 32: the 80x80 128 -> 256 3x3 layer has 18 tiles and 204,800 pixels and splits; the 20x20 512 -> 1024 3x3 layer has
    288 tiles and does not need to."""
    big = (32, 80, 80, 128, 256, 3, "leaky", torch.bfloat16, None, None)
    assert K.conv2d_bwd_pick(fwd_desc(big)) == "wgrad<128x128,BK64,tr_b16> grid 9x2 splits 29"
    deep = (32, 20, 20, 512, 1024, 3, "leaky", torch.bfloat16, None, None)
    assert K.conv2d_bwd_pick(fwd_desc(deep)) == "wgrad<128x128,BK64,tr_b16> grid 36x8 splits 2"


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_exact_case_guards(case):
    """The integer cases are exact in fp32 (float64 as the witness: integers everywhere, every sum of |terms| below 2^24), at least
    15 % of y is non-positive and - where dx has the terms to leave the bf16 integers - at least 25 % of dx needs rounding."""
    c = B.exact_conditions(case)
    assert c["integers"] and c["largest_abs_sum"] < 2 ** 24, c
    assert c["y_nonpositive"] >= 0.15, c
    if c["dx_terms"] >= B.DX_ROUNDING_FROM_TERMS:
        assert c["dx_rounded"] >= 0.25, c
    else:
        assert 2.9 * c["dx_terms"] < 256, c            # cases 2, 5 and 7: dx stays (almost) inside the bf16 integers


@pytest.mark.parametrize("case", SMALL + [B.CASES[B.SPLIT_CASE]], ids=B.case_id)
def test_injected_faults_show(case):
    """One wrong tap, or one dropped stretch of pixels (a 64-pixel stage; for the split case one whole split), changes at least 1 % of
    the elements of the exact dW: the comparison the GPU tests make is not vacuous."""
    n, h, w_, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.exact_operands(case)
    y = B.forward(x, w, b, k, act)
    good = B.grads(x, w, dy, y, k, act)["dw"]
    pixels = n * h * w_
    lo, hi = (0, min(64, pixels))
    splits = int(K.conv2d_bwd_pick(fwd_desc(case)).rsplit(" ", 1)[1])
    assert (splits >= 2) == (case is B.CASES[B.SPLIT_CASE] or case is B.CASES[B.WIDE_SPLIT_CASE])
    if splits >= 2:
        per = -(-(-(-pixels // 64)) // splits) * 64
        lo, hi = per, min(2 * per, pixels)
    faults = [("pixels", lo, hi)] + [("tap", t) for t in ((0, k * k - 1) if k == 3 and h > 1 else (k * k // 2,))]
    for inject in faults:
        bad = B.grads(x, w, dy, y, k, act, inject=inject)["dw"]
        assert float((bad != good).double().mean()) >= 0.01, inject
    # one dropped 16-byte chunk column of one wave - 8 columns (tap, ci .. ci + 7) of 32 rows of D - would zero a block of the exact dW:
    # every such block holds a non-zero element (a one-row map has taps with no term at all)
    if h > 1:
        d2 = good.permute(0, 2, 3, 1).reshape(cout, k * k * cin)                 # the kernel's column order: tap, then channel
        rows = -(-cout // 32) * 32
        blocks = F.pad(d2, (0, 0, 0, rows - cout)).reshape(rows // 32, 32, k * k * cin // 8, 8)
        assert bool(blocks.ne(0).any(3).any(1).all())
