"""GPU tests of the ops and of the training-mode forward and backward of YOLOv3-tiny/SqueezeNet.

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs are NaN / 0xAA filled; the 0xFF and the 0x7F
run give equal bits, and so does a second run.
    the ceil-mode pool     y and idx bit-equal to F.max_pool2d(x, 3, 2, ceil_mode=True, return_indices=True) on the CPU, on small-integer
                           inputs with ties everywhere; dx bit-equal to torch autograd for a small-integer dy (the sums are exact) and to the
                           fixed-order restatement for a random dy
    fire_bwd_split / join  bit-equal to the restatement and to the compositions they replace (.contiguous() slices + prepare; a bf16 add +
                           prepare)
    ReLU conv backward     the stride-1 bf16 LeakyReLU cases of tests/_conv_bwd.py with the act swapped: bit-exact on integer operands, within
                           that file's bounds on random ones
    the stem's gradient    3 -> 64 on 17x19 and 18x20 (an unread last row and column), 8 -> 16 on 9x11, and a map whose pick splits: dW
                           and db bit-equal to float64 autograd on integer operands, within tests/_conv_bwd.py's bounds (the ones
                           tests/_conv_down.py uses) on random ones
Ops: conv_block(act="relu"), stem_block, max_pool_ceil; fire_block bit-equal - output and all seven gradients - to three
conv_block(act="relu") calls with torch.cat under autograd, within the bounds of the float64 restatement fed with the device's own
intermediates, gradients only where asked.
The model: every op call of one forward_train + compute_loss(...)[0].backward() against its restatement on that call's own inputs (the
method of tests/test_train_gpu.py: these random-weight batch-statistics networks are chaotic, so no end-to-end tolerance), the step's
contract, and the conv families of tests/_train_fire_families.py in the training role.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_bwd as B
import _guard as G
import _loss as L
import _train as T
import _train_families as TF
import _train_fire as FR
import _train_fire_families as FF
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT
from test_conv_bwd_gpu import check_untouched, device_chain, nchw64, nhwc, same_bits
from test_conv_exact_cpu import tuning
from test_train_fire_cpu import FIRE_CASES, STEM_CASES, fire_operands, stem_desc
from test_train_gpu import BF16, DEV, F32, F64, NAN, _cl, _nhwc, bits, both_poisons, check_head_call, f32np, t32
from test_train_pool_gpu import check_calls, recording_pool_ops

pytestmark = pytest.mark.gpu

U8 = torch.uint8


def small_ints(shape, seed, lo=-2, hi=3):
    """Small integers as float32 numpy: bf16 values with ties everywhere."""
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.float32)


# ---- the ceil-mode pool, bit for bit ---------------------------------------------------------------------------------------------------------
# (7, 9): every window whole; (8, 10): a partial last window both ways; (2, 3) and (3, 2): the minimum; c = 24: three chunks
POOL_CASES = [(2, h, w, c) for c in (8, 24) for (h, w) in ((7, 9), (8, 10), (2, 3), (3, 2))]


@functools.lru_cache(maxsize=None)
def pool_reference(case):
    """(x, integer dy, random dy, torch's y, torch's tap index, torch's dx for the integer dy): computed once on the CPU, left unchanged."""
    n, h, w, c = case
    x = small_ints(case, 101)
    out = (n, h // 2, w // 2, c)
    dy_int, dy_rand = small_ints(out, 102, 1, 4), T.N.bf16(np.random.default_rng(103).standard_normal(out).astype(np.float32))
    xt = t32(x).permute(0, 3, 1, 2).double().requires_grad_()
    y, where = F.max_pool2d(xt, 3, 2, ceil_mode=True, return_indices=True)
    y.backward(t32(dy_int).permute(0, 3, 1, 2).double())
    where = where.permute(0, 2, 3, 1).numpy()
    oy, ox = np.arange(out[1])[None, :, None, None], np.arange(out[2])[None, None, :, None]
    tap = (3 * (where // w - 2 * oy) + (where % w - 2 * ox)).astype(np.uint8)
    return x, dy_int, dy_rand, y.detach().permute(0, 2, 3, 1).numpy(), tap, xt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda s: "%dx%dx%d_c%d" % s)
def test_pool_kernels_equal_torch_and_the_restatement(case):
    n, h, w, c = case
    x, dy_int, dy_rand, want_y, want_idx, want_dx = pool_reference(case)
    out = want_y.shape

    def run(a):
        xd = a.like("x", t32(x).to(BF16))
        y, idx = a.alloc("y", out, BF16, NAN), a.alloc("idx", out, U8, 0xAA)
        K.maxpool3s2_train_fwd(xd, y, idx)
        res = dict(y=y, idx=idx)
        for name, dy in (("dx_int", dy_int), ("dx_rand", dy_rand)):
            res[name] = a.alloc(name, case, BF16, NAN)
            K.maxpool3s2_bwd(a.like("dy_" + name, t32(dy).to(BF16)), idx, res[name])
        return res

    got = both_poisons(run)
    assert np.array_equal(f32np(got["y"]), want_y) and np.array_equal(got["idx"].cpu().numpy(), want_idx)
    assert np.array_equal(f32np(got["dx_int"]), want_dx)
    assert np.array_equal(f32np(got["dx_rand"]), FR.pool3_backward(dy_rand, want_idx, case))
    assert want_dx.sum() == dy_int.sum() and (h < 7 or len(np.unique(want_idx)) == 9)
    if h >= 7:            # some pixel sums more than one window, and its random sum needs the one rounding
        assert (want_dx > dy_int.max()).any()
        assert not np.array_equal(FR.pool3_backward(dy_rand, want_idx, case), FR.pool3_backward(dy_rand, want_idx, case, rounding=False))


def test_max_pool_ceil_op():
    case = POOL_CASES[1]
    x, dy_int, _, want_y, _, want_dx = pool_reference(case)
    xd = t32(x).permute(0, 3, 1, 2).to(DEV).requires_grad_()                      # float32 NCHW: converted by torch
    y = Y.max_pool_ceil(xd)
    assert y.dtype == BF16 and tuple(y.shape) == (2, 8, 4, 5) and y.permute(0, 2, 3, 1).is_contiguous() and y.grad_fn is not None
    y.backward(_cl(t32(dy_int).permute(0, 3, 1, 2).to(BF16).to(DEV)))
    assert np.array_equal(_nhwc(y), want_y) and xd.grad.dtype == F32 and np.array_equal(_nhwc(xd.grad), want_dx)
    with torch.no_grad():
        assert Y.max_pool_ceil(xd).grad_fn is None
    for bad in (xd[:, :4], xd[:, :, :1], xd[0]):
        with pytest.raises(ValueError):
            Y.max_pool_ceil(bad)


# ---- fire_bwd_split / fire_bwd_join, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16_dy", "f32_dy"])
@pytest.mark.parametrize("case", [(71, 64, 64), (70, 8, 24), (300, 192, 192)], ids=lambda c: "%dpx_%d_%d" % c)
def test_fire_split_equals_the_restatement_and_the_composition(case, dt):
    pixels, e1, e3 = case
    gen = torch.Generator().manual_seed(111)
    y = torch.relu(torch.randn((1, pixels, 1, e1 + e3), generator=gen)).to(BF16)               # NHWC, about half zeros
    dy = torch.randn(y.shape, generator=gen).to(dt)
    want = FR.relu_upstream(dy.to(F64), y.to(F64))

    def run(a):
        yd, dyd = a.like("y_cat", y), a.like("dy", dy)
        g1, g3 = a.alloc("g1", (1, pixels, 1, e1), BF16, NAN), a.alloc("g3", (1, pixels, 1, e3), BF16, NAN)
        K.fire_bwd_split(dyd, yd, g1, g3)
        # what it replaces: a .contiguous() slice of dy and a prepare launch per half, reading y through its channel view
        c1, c3 = a.alloc("c1", g1.shape, BF16, NAN), a.alloc("c3", g3.shape, BF16, NAN)
        for c, e, off in ((c1, e1, 0), (c3, e3, e1)):
            d = K.conv_desc(n=1, h=pixels, w=1, cin=8, in_c_total=8, in_c_offset=0, cout=e, out_c_total=e1 + e3, out_c_offset=off, ksize=1,
                            stride=1, act=_lib.ACT_RELU, kpad=64, cout_pad=K.roundup(e, 128))
            K.conv2d_bwd_prepare(dyd[..., off:off + e].contiguous(), yd, c, d)
        return dict(g1=g1, g3=g3, c1=c1, c3=c3)

    got = both_poisons(run)
    assert torch.equal(got["g1"].cpu().to(F64), want[..., :e1]) and torch.equal(got["g3"].cpu().to(F64), want[..., e1:])
    assert torch.equal(bits(got["g1"]), bits(got["c1"])) and torch.equal(bits(got["g3"]), bits(got["c3"]))
    assert 0.3 < float((want == 0).double().mean()) < 0.7


@pytest.mark.parametrize("case", [(71, 16), (300, 48)], ids=lambda c: "%dpx_%d" % c)
def test_fire_join_equals_the_restatement_and_the_composition(case):
    pixels, sq = case
    gen = torch.Generator().manual_seed(112)
    shape = (1, pixels, 1, sq)
    s = torch.relu(torch.randn(shape, generator=gen)).to(BF16)
    d1, d3 = torch.randn(shape, generator=gen).to(BF16), (64 * torch.randn(shape, generator=gen)).to(BF16)      # (unequal scales: the sum rounds)
    want = FR.relu_upstream((d1.to(F64) + d3.to(F64)).to(F32), s.to(F64))

    def run(a):
        sd, a1, a3 = a.like("s", s), a.like("d1", d1), a.like("d3", d3)
        gs, c = a.alloc("g_s", shape, BF16, NAN), a.alloc("c", shape, BF16, NAN)
        K.fire_bwd_join(a1, a3, sd, gs)
        d = K.conv_desc(n=1, h=pixels, w=1, cin=8, in_c_total=8, in_c_offset=0, cout=sq, out_c_total=sq, out_c_offset=0, ksize=1, stride=1,
                        act=_lib.ACT_RELU, kpad=64, cout_pad=128)
        K.conv2d_bwd_prepare(a1 + a3, sd, c, d)                                   # torch's bf16 add, then a prepare launch
        return dict(gs=gs, c=c)

    got = both_poisons(run)
    assert torch.equal(got["gs"].cpu().to(F64), want) and torch.equal(bits(got["gs"]), bits(got["c"]))
    assert float(((d1.to(F64) + d3.to(F64)) != (d1 + d3).to(F64)).double().mean()) > 0.3


# ---- the ReLU slope of the conv backward and the stem's weight gradient: the kernel chain on guarded operands -----------------------------------
def chain(a, d, x, w, b, dy, fill=NAN):
    """The launches of one conv with its backward on allocations of ``a``: device pack, forward, prepare, weight / bias gradient and - at
    stride 1 - transposed pack and data gradient.  ``d``: the forward's descriptor, a stride-1 "same" conv or the unpadded stride-2 first
    layer (x and w with cin % 8 == 0).  float64 NCHW results on the host."""
    stem = d.stride == 2
    n, cin, cout, k = d.n, d.cin, d.cout, d.ksize
    xbuf, w_dev = a.like("x", nhwc(x, BF16)), a.like("w", w.to(F32))
    bias = a.alloc("bias", (d.cout_pad,), F32)
    bias[:cout] = b.to(F32).to(DEV)
    packed = a.alloc("w_packed", (d.cout_pad, d.kpad), BF16, fill)
    K.pack_conv_weight_dev(w_dev, cin, out=packed)
    ybuf = a.alloc("y", (n, d.ho, d.wo, cout), BF16, fill)
    K.conv2d(xbuf, packed, bias, ybuf, d)
    g = a.alloc("g", ybuf.shape, BF16, fill)
    od = d if not stem else K.conv_desc(n=n, h=d.ho, w=d.wo, cin=cout, in_c_total=cout, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0,
                                        ksize=1, stride=1, act=d.act, kpad=K.roundup(cout, 64), cout_pad=d.cout_pad)
    K.conv2d_bwd_prepare(a.like("dy", nhwc(dy, BF16)), ybuf, g, od)
    ws = a.alloc("workspace", ((K.conv2d_stem_bwd_workspace_bytes(d) if stem else K.conv2d_bwd_workspace_bytes(d)) // 4,), F32, fill)
    dw, db = a.alloc("dw", (cout, cin, k, k), F32, fill), a.alloc("db", (cout,), F32, fill)
    (K.conv2d_stem_bwd_weight if stem else K.conv2d_bwd_weight)(xbuf, g, dw, db, ws, d)
    out = dict(y=ybuf, g=g, dw=dw, db=db)
    if not stem:
        packed_t = a.alloc("w_packed_t", (K.roundup(cin, 128), K.roundup(k * k * cout, 64)), BF16, fill)
        K.pack_conv_weight_dev(w_dev, cout, transposed=True, out=packed_t)
        out["dx"] = a.alloc("dx", xbuf.shape, BF16, fill)
        K.conv2d_bwd_data(g, packed_t, out["dx"], d)
    torch.cuda.synchronize()
    assert torch.equal(xbuf.cpu(), nhwc(x, BF16))
    return out


def host(r):
    return {k_: (nchw64(v.cpu()) if v.dim() == 4 and k_ != "dw" else v.cpu().to(F64)) for k_, v in r.items()}


RELU_CASES = [c for c in B.CASES if c[6] == "leaky" and c[8] is None and c[9] is None and c[4] % 8 == 0]


@pytest.mark.parametrize("case", RELU_CASES, ids=B.case_id)
def test_relu_conv_backward_exact(case):
    """Integer operands: y, g, dW, db have one right value and dx is that integer rounded once to bf16 - torch.equal, under both poisons."""
    n, h, wd, cin, cout, k = case[:6]
    x, w, b, dy = B.exact_operands(case)
    d = B.fwd_desc(case, act=_lib.ACT_RELU)
    r = host(both_poisons(lambda a: chain(a, d, x, w, b, dy)))
    y64 = FR.relu_forward(x, w, b)
    want = FR.relu_grads(x, w, dy, y64)
    assert torch.equal(r["y"], B.bf16(y64))
    for name in ("g", "dw", "db", "dx"):
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ"
    assert 0.15 < float((y64 == 0).double().mean()) < 0.85 and want["dw"].any() and want["db"].any() and want["dx"].any()
    assert float(max(want["dw_abs"].max(), want["db_abs"].max(), want["dx_abs"].max())) < 2 ** 24               # the witness of exactness
    assert not torch.equal(want["g"], B.grads(x, w, dy, y64, k, "leaky")["g"])                                 # the slope matters


@pytest.mark.parametrize("case", RELU_CASES, ids=B.case_id)
def test_relu_conv_backward_random_within_bounds(case):
    x, w, b, dy = B.random_operands(case)
    d = B.fwd_desc(case, act=_lib.ACT_RELU)
    r = host(both_poisons(lambda a: chain(a, d, x, w, b, dy)))
    want = FR.relu_grads(x, w, dy, r["y"])
    assert torch.equal(r["g"], want["g"]) and 0.15 < float((r["y"] == 0).double().mean()) < 0.85
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  dx=B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    print(f"relu conv_bwd {B.case_id(case)}: largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_conv_block_relu_is_the_kernel_chain():
    """conv_block(act="relu"): the forward and .backward() give the chain's bits; the output has exact zeros; act="relu6" still raises."""
    case = RELU_CASES[0]
    x, w, b, dy = B.random_operands(case)
    ref = host(chain(G.Plain(DEV), B.fwd_desc(case, act=_lib.ACT_RELU), x, w, b, dy))
    xd = _cl(x.to(BF16).to(DEV)).requires_grad_()
    wp, bp = torch.nn.Parameter(w.to(F32).to(DEV)), torch.nn.Parameter(b.to(F32).to(DEV))
    out = Y.conv_block(xd, wp, bp, act="relu")
    out.backward(_cl(dy.to(BF16).to(DEV)))
    assert torch.equal(out.detach().cpu().to(F64), ref["y"]) and bool((out == 0).any()) and not bool((out < 0).any())
    assert torch.equal(xd.grad.cpu().to(F64), ref["dx"]) and torch.equal(wp.grad.cpu().to(F64), ref["dw"]) and torch.equal(bp.grad.cpu().to(F64), ref["db"])
    with pytest.raises(ValueError, match="relu"):
        Y.conv_block(xd, wp, bp, act="relu6")


# the issue's three maps, and one whose 2,112 output pixels (33 stages) split the reduction
STEM_GPU_CASES = STEM_CASES + [(4, 67, 69, 3, 64)]


def stem_operands(case, exact):
    n, h, w_, cin, cout = case
    gen = torch.Generator().manual_seed(6000 + h)
    if exact:
        r = lambda *s: torch.randint(-3, 4, s, generator=gen).to(F64)
        x, w, b, dy = r(n, cin, h, w_), r(cout, cin, 3, 3), r(cout), r(n, cout, (h - 3) // 2 + 1, (w_ - 3) // 2 + 1)
    else:
        rn = lambda *s: torch.randn(s, generator=gen)
        x, w = rn(n, cin, h, w_).to(BF16).to(F64), (rn(cout, cin, 3, 3) / (9 * cin) ** 0.5).to(F64)
        b, dy = rn(cout).to(F64), rn(n, cout, (h - 3) // 2 + 1, (w_ - 3) // 2 + 1).to(BF16).to(F64)
    return x, w, b, dy


def pad8(t):
    return F.pad(t, (0, 0, 0, 0, 0, -t.shape[1] % 8))


@pytest.mark.parametrize("case", STEM_GPU_CASES, ids=lambda c: "%dx%dx%d_%dto%d" % c)
def test_stem_weight_gradient_exact(case):
    """Integer operands: dW and db bit-equal to float64 autograd of relu(conv2d(x, w, b, stride=2)), from the kernel chain under both
    poisons and from stem_block."""
    n, h, w_, cin, cout = case
    x, w, b, dy = stem_operands(case, True)
    wa, ba = w.clone().requires_grad_(), b.clone().requires_grad_()
    y64 = F.relu(F.conv2d(x, wa, ba, stride=2))
    y64.backward(dy)
    d = stem_desc(n, h, w_, K.roundup(cin, 8), cout)
    splits = int(K.conv2d_stem_bwd_pick(d).rsplit(" ", 1)[1])
    assert (splits >= 2) == (case == STEM_GPU_CASES[-1])
    r = host(both_poisons(lambda a: chain(a, d, pad8(x), pad8(w), b, dy)))
    assert torch.equal(r["y"], B.bf16(y64.detach())) and torch.equal(r["g"], dy * (y64.detach() > 0))
    assert torch.equal(r["dw"][:, :cin], wa.grad) and not r["dw"][:, cin:].any() and torch.equal(r["db"], ba.grad)
    assert wa.grad.any() and ba.grad.any() and 0.15 < float((y64 == 0).double().mean()) < 0.85
    wp, bp = torch.nn.Parameter(w.to(F32).to(DEV)), torch.nn.Parameter(b.to(F32).to(DEV))
    out = Y.stem_block(x.to(F32).to(DEV), wp, bp)                                # float32 NCHW, 3 channels: the image
    out.backward(_cl(dy.to(BF16).to(DEV)))
    assert out.dtype == BF16 and tuple(out.shape) == tuple(y64.shape) and out.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(out.detach().cpu().to(F64), r["y"]) and torch.equal(wp.grad.cpu().to(F64), wa.grad) and torch.equal(bp.grad.cpu().to(F64), ba.grad)


@pytest.mark.parametrize("case", STEM_GPU_CASES, ids=lambda c: "%dx%dx%d_%dto%d" % c)
def test_stem_weight_gradient_random_within_bounds(case):
    n, h, w_, cin, cout = case
    x, w, b, dy = stem_operands(case, False)
    d = stem_desc(n, h, w_, K.roundup(cin, 8), cout)
    r = host(both_poisons(lambda a: chain(a, d, pad8(x), pad8(w), b, dy)))
    want = FR.stem_grads(pad8(x), pad8(w), dy, r["y"])
    assert torch.equal(r["g"], want["g"])
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])))
    print(f"stem wgrad {case}: largest error / bound  dW {ratios['dw']:.4f}  db {ratios['db']:.4f}")
    assert all(v <= 1.0 for v in ratios.values()) and want["dw"][:, :cin].any() and not r["dw"][:, cin:].any()


def test_stem_block_contract():
    x, w, b, dy = stem_operands(STEM_GPU_CASES[1], False)
    xd, wd_, bd = x.to(F32).to(DEV), w.to(F32).to(DEV), b.to(F32).to(DEV)
    assert Y.stem_block(xd, wd_, bd).grad_fn is None
    wp = torch.nn.Parameter(wd_.clone())
    out = Y.stem_block(xd, wp, bd)
    out.backward(_cl(dy.to(BF16).to(DEV)))
    assert wp.grad is not None and bd.grad is None and bool(torch.isfinite(wp.grad).all())
    leaky = Y.stem_block(xd, wd_, bd, act="leaky")
    assert bool((leaky < 0).any()) and torch.equal(torch.relu(leaky), out.detach())
    with pytest.raises(NotImplementedError, match="first layer"):
        Y.stem_block(xd.clone().requires_grad_(), wp, bd)
    with torch.no_grad():
        assert Y.stem_block(xd.clone().requires_grad_(), wp, bd).grad_fn is None
    with pytest.raises(ValueError):
        Y.stem_block(xd[:, :, :2], wp, bd)


# ---- fire_block -------------------------------------------------------------------------------------------------------------------------------------
GRADS = ("x", "squeeze_w", "squeeze_b", "e1_w", "e1_b", "e3_w", "e3_b")


def fire_leaves(x, p):
    return [_cl(x.to(BF16).to(DEV)).requires_grad_()] + [torch.nn.Parameter(t.to(F32).to(DEV)) for t in p]


def composition(leaves, dy):
    """Three conv_block(act="relu") calls and torch.cat under autograd: (y, s, the gradient of s, the seven gradients)."""
    xd, sw, sb, w1, b1, w3, b3 = leaves
    s = Y.conv_block(xd, sw, sb, act="relu")
    s.retain_grad()
    y = torch.cat([Y.conv_block(s, w1, b1, act="relu"), Y.conv_block(s, w3, b3, act="relu")], 1)
    y.backward(dy)
    return y.detach(), s.detach(), s.grad, [t.grad for t in leaves]


def check_fire(x, p, dy, y, grads, worst):
    """One fire_block call - x, the six parameters, dy and the op's output and seven gradients, all on the device - against (1) the
    composition it replaces, bit for bit, and (2) the float64 restatement of each conv fed with the device's own tensors: the bounds of
    tests/_conv_bwd.py.  The sum of the two expand data gradients is seen after its rounding: d1 and d3 are each within bound_dx of their
    sums S1 and S3, and bf16(d1 + d3) is one more rounding of a value within b1 + b3 of S1 + S3: |ds - (S1 + S3)| <= b1 + b3 +
    2^-8 (|S1 + S3| + b1 + b3)."""
    leaves = [x.detach().clone().requires_grad_()] + [torch.nn.Parameter(t.detach().clone()) for t in p]
    cy, s, ds, cg = composition(leaves, dy)
    assert torch.equal(bits(y), bits(cy)), "y"
    for name, got, want in zip(GRADS, grads, cg):
        assert got is not None and got.dtype == want.dtype and torch.equal(bits(got), bits(want)), name
    c64 = lambda t: t.detach().float().cpu().to(F64)
    e1 = p[2].shape[0]
    s64, y64, dy64 = c64(s), c64(y), c64(dy)
    r1, r3 = FR.relu_grads(s64, c64(p[2]), dy64[:, :e1], y64[:, :e1]), FR.relu_grads(s64, c64(p[4]), dy64[:, e1:], y64[:, e1:])
    rs = FR.relu_grads(c64(x), c64(p[0]), c64(ds), s64)
    sum_w = lambda r, g: B.ratio(c64(g), r["dw"], B.bound_sum(r["dw_terms"], r["dw_abs"]))
    sum_b = lambda r, g: B.ratio(c64(g), r["db"], B.bound_sum(r["db_terms"], r["db_abs"]))
    b1, b3 = (B.bound_dx(r["dx_sum"], r["dx_terms"], r["dx_abs"]) for r in (r1, r3))
    tot = r1["dx_sum"] + r3["dx_sum"]
    ratios = dict(fire_dW=max(sum_w(rs, grads[1]), sum_w(r1, grads[3]), sum_w(r3, grads[5])),
                  fire_db=max(sum_b(rs, grads[2]), sum_b(r1, grads[4]), sum_b(r3, grads[6])),
                  fire_ds=B.ratio(c64(ds), tot, b1 + b3 + 2.0 ** -8 * (tot.abs() + b1 + b3)),
                  fire_dx=B.ratio(c64(grads[0])[:, :rs["dx_sum"].shape[1]], rs["dx_sum"], B.bound_dx(rs["dx_sum"], rs["dx_terms"], rs["dx_abs"])))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
        worst[name] = max(worst.get(name, 0.0), v)
    return s


@pytest.mark.parametrize("case", FIRE_CASES + [(2, 13, 15, 256, 48, 192)], ids=lambda c: "%dx%dx%d_%d_%d_%d" % c)
def test_fire_block_equals_the_composition(case):
    x, p, dy = fire_operands(case)
    dyd = _cl(dy.to(BF16).to(DEV))
    runs = []
    for _ in range(2):
        leaves = fire_leaves(x, p)
        y = Y.fire_block(*leaves)
        y.backward(dyd)
        runs.append((y.detach(), [t.grad for t in leaves]))
    (y, grads), (y2, grads2) = runs
    n, h, w, cin, sq, e = case
    assert y.dtype == BF16 and tuple(y.shape) == (n, 2 * e, h, w) and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(bits(y), bits(y2)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, grads2))          # two runs: the same bits
    assert grads[0].dtype == BF16 and all(g.dtype == F32 and g.shape == t.shape for g, t in zip(grads[1:], p))
    worst = {}
    s = check_fire(fire_leaves(x, p)[0], [t.to(F32).to(DEV) for t in p], dyd, y, grads, worst)
    assert 0.2 < float((s == 0).float().mean()) < 0.8 and 0.2 < float((y == 0).float().mean()) < 0.8 and all(bool(g.any()) for g in grads)
    print(f"fire_block {case}: largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))


def test_fire_block_contract():
    """Gradients only where asked - a frozen squeeze conv and x launch neither a squeeze weight gradient nor an expand data gradient -,
    no grad_fn without a gradient to ask for, conversions of x by torch, errors before any launch."""
    x, p, dy = fire_operands(FIRE_CASES[0])
    dyd = _cl(dy.to(BF16).to(DEV))
    leaves = fire_leaves(x, p)
    full = Y.fire_block(*leaves)
    full.backward(dyd)
    want = [t.grad.clone() for t in leaves]
    launches = []
    names = ("conv2d_bwd_weight", "conv2d_bwd_data", "fire_bwd_split", "fire_bwd_join")
    real = {n: getattr(K, n) for n in names}
    try:
        for n in names:
            setattr(K, n, (lambda n: lambda *a, **kw: (launches.append((n, a[-1].cout if n.startswith("conv") else None)), real[n](*a, **kw))[1])(n))
        for asked in ((3, 4), (5,), (1,), (0,), (2, 6)):                          # indices into GRADS
            fresh = [t.detach().requires_grad_(i in asked) for i, t in enumerate(fire_leaves(x, p))]      # the others are frozen
            del launches[:]
            Y.fire_block(*fresh).backward(dyd)
            for i, t in enumerate(fresh):
                assert (t.grad is not None) == (i in asked), (asked, GRADS[i])
                assert t.grad is None or torch.equal(bits(t.grad), bits(want[i])), (asked, GRADS[i])
            kinds = [n for n, _ in launches]
            need_s = any(i < 3 for i in asked)
            assert kinds.count("fire_bwd_split") == 1 and kinds.count("fire_bwd_join") == int(need_s)
            assert kinds.count("conv2d_bwd_data") == (2 if need_s else 0) + int(0 in asked)
            wgrads = [c for n, c in launches if n == "conv2d_bwd_weight"]
            assert len(wgrads) == int(3 in asked or 4 in asked) + int(5 in asked or 6 in asked) + int(1 in asked or 2 in asked)
            if not need_s:
                assert 16 not in wgrads                                           # a frozen squeeze conv: no squeeze weight gradient
    finally:
        for n in names:
            setattr(K, n, real[n])
    det = [t.detach() for t in leaves]
    assert Y.fire_block(*det).grad_fn is None and torch.equal(bits(Y.fire_block(*det)), bits(full.detach()))
    with torch.no_grad():
        assert Y.fire_block(*leaves).grad_fn is None
    x32 = x.to(F32).to(DEV).contiguous().requires_grad_()                          # float32 NCHW: converted by torch, a float32 gradient
    Y.fire_block(x32, *det[1:]).backward(dyd)
    assert x32.grad.dtype == F32 and torch.equal(x32.grad, want[0].float())
    bad = list(det)
    bad[3] = det[3][:12]
    with pytest.raises(ValueError, match="fire_block"):
        Y.fire_block(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.fire_block(*[t.cpu() for t in det])


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------
def new_model():
    model = T.load_synthetic(Y.YOLOv3TinySqueeze(**FR.CTOR))
    model.hyper_params = dict(L.HYPER)
    return model.to(DEV).train()


def recording_fire_ops(calls):
    """tests/test_train_pool_gpu.recording_pool_ops with the four functions of DEVICE_OPS_FIRE recorded the same way."""
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))

    def alias(rec, key, t):
        if not t.requires_grad:
            rec[key] = t.detach()
            return t
        a = t.view_as(t)
        a.register_hook(keep(rec, "d" + key))
        rec[key] = a.detach()
        return a

    def watch(rec, key, t):
        rec[key] = t.detach()
        t.register_hook(keep(rec, "d" + key))
        return t

    def stem_block(x, w, b=None, *, act="relu"):
        rec = dict(kind="stem", x=x.detach(), params=(w, b))
        calls.append(rec)
        return watch(rec, "y", Y.stem_block(x, w, b, act=act))

    def fire_block(x, *p):
        rec = dict(kind="fire", params=p)
        calls.append(rec)
        return watch(rec, "y", Y.fire_block(alias(rec, "x", x), *p))

    def max_pool_ceil(x):
        rec = dict(kind="pool3")
        calls.append(rec)
        return watch(rec, "y", Y.max_pool_ceil(alias(rec, "x", x)))

    def concat(xs):
        rec = dict(kind="cat", n=len(xs))
        calls.append(rec)
        return watch(rec, "y", MT.DEVICE_OPS_FIRE.concat([alias(rec, f"x{i}", t) for i, t in enumerate(xs)]))

    base = recording_pool_ops(calls)
    table = dict(vars(base))
    table.update(stem_block=stem_block, fire_block=fire_block, max_pool_ceil=max_pool_ceil, concat=concat)
    return type(base)(**table)


def check_fire_calls(calls):
    worst = {}
    for rec in calls:
        if rec["kind"] == "stem":
            w, b = rec["params"]
            x64 = pad8(rec["x"].to(BF16).float().cpu().to(F64))
            want = FR.stem_grads(x64, pad8(w.detach().cpu().to(F64)), rec["dy"].float().cpu().to(F64), rec["y"].float().cpu().to(F64))
            v = max(B.ratio(w.grad.cpu().to(F64), want["dw"][:, :3], B.bound_sum(want["dw_terms"], want["dw_abs"])[:, :3]),
                    B.ratio(b.grad.cpu().to(F64), want["db"], B.bound_sum(want["db_terms"], want["db_abs"])))
            assert v <= 1.0, ("stem", v)
            worst["stem_dW_db"] = v
        elif rec["kind"] == "fire":
            check_fire(rec["x"], [t.detach() for t in rec["params"]], rec["dy"], rec["y"], [rec["dx"]] + [t.grad for t in rec["params"]], worst)
        elif rec["kind"] == "pool3":
            x = _nhwc(rec["x"])
            y, idx = FR.pool3_forward(x)
            assert np.array_equal(_nhwc(rec["y"]), y) and np.array_equal(_nhwc(rec["dx"]), FR.pool3_backward(_nhwc(rec["dy"]), idx, x.shape))
        elif rec["kind"] == "cat":
            xs = [rec[f"x{i}"] for i in range(rec["n"])]
            assert torch.equal(rec["y"], torch.cat(xs, 1))
            for dxi, part in zip([rec[f"dx{i}"] for i in range(rec["n"])], torch.split(rec["dy"], [t.shape[1] for t in xs], 1)):
                assert torch.equal(dxi, part)
    worst.update(check_calls([c for c in calls if c["kind"] not in ("stem", "fire", "pool3", "cat")]))
    return worst


def test_model_layer_by_layer():
    """Every op call of one device forward + backward, re-run on its restatement from the device's own inputs."""
    model = new_model()
    x, targets = FR.golden_inputs(model)
    calls = []
    p = MT.forward_train(model, x.to(DEV), ops=recording_fire_ops(calls))
    loss, _ = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    kinds = [c["kind"] for c in calls]
    assert kinds.count("stem") == 1 and kinds.count("fire") == 8 and kinds.count("pool3") == 3 and kinds.count("cat") == 1
    assert kinds.count("bn") == 3 and kinds.count("head") == 2 and len(calls) == 18
    assert [tuple(c["x"].shape[2:]) for c in calls if c["kind"] == "pool3"] == [(31, 47), (15, 23), (7, 11)]
    worst = check_fire_calls(calls)
    print(f"train layer by layer, squeeze: {len(calls)} op calls, largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))


@functools.lru_cache(maxsize=None)
def device_step():
    model = new_model()
    x, targets = FR.golden_inputs(model)
    p = Y.forward_train(model, x.to(DEV))
    loss, items = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    return model, [t.detach() for t in p], {n: t.grad for n, t in model.named_parameters()}, items


def test_model_training_step_contract():
    """p as the reference returns it; every parameter gets a finite gradient of its own shape; two steps from the same state give the same
    bits; the running statistics moved and every BN layer counted one batch; a following eval forward equals that of a fresh model loaded
    from state_dict() (model.invalidate(): no stale plan); model.train()(x) keeps raising."""
    model = new_model()
    x, targets = (t.to(DEV) for t in FR.golden_inputs(model))
    fresh_sd = {k_: v.clone() for k_, v in model.state_dict().items()}
    with torch.no_grad():
        io_before, _ = model.eval()(x)
    model.train()
    with pytest.raises(NotImplementedError, match="forward_train"):
        model(x)
    p = Y.forward_train(model, x)
    for t in p:
        assert t.dtype == F32 and t.is_contiguous() and t.grad_fn is not None and tuple(t.shape) == (2, 3, 3, 5, 7)
    loss, items = Y.compute_loss(p, targets, model)
    loss.backward()
    grads = {n: t.grad for n, t in model.named_parameters()}
    for n, t in model.named_parameters():
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and bool(t.grad.any()), n
    model2, p2, grads2, items2 = device_step()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(p, p2)) and torch.equal(items, items2) and bool(torch.isfinite(items).all())
    for n in grads:
        assert torch.equal(bits(grads[n]), bits(grads2[n])), n
    sd, sd2 = model.state_dict(), model2.state_dict()
    for k_ in sd:
        assert torch.equal(sd[k_], sd2[k_]), k_
        if k_.endswith("running_mean") or k_.endswith("running_var"):
            assert not torch.equal(sd[k_], fresh_sd[k_]), k_
        if k_.endswith("num_batches_tracked"):
            assert int(sd[k_]) == 1, k_
    clone = Y.YOLOv3TinySqueeze(**FR.CTOR)
    clone.load_state_dict({k_: v.cpu() for k_, v in sd.items()})
    with torch.no_grad():
        io_after, _ = model.eval()(x)
        io_clone, _ = clone.to(DEV).eval()(x)
    assert torch.equal(io_after, io_clone) and not torch.equal(io_after, io_before)


# ---- the conv families of a full-size step that tests/_train_families.py does not hold, in the training role ---------------------------------------
def assert_picks(c):
    want = {role: fam for (role, fam), case in FF.FIRE_FAMILY_CASES.items() if case is c}
    d = B.fwd_desc(c["case"])
    got = {"forward": TF.family(K.conv2d_pick(d)), "dgrad": TF.family(K.conv2d_pick(TF.dgrad_desc(d)))}
    assert want and all(got[role] == fam for role, fam in want.items()), (want, got)
    return got


def run_family(c, x, w, b, dy):
    runs = []
    with tuning(*c["knobs"]):
        picks = assert_picks(c)
        for poison in G.POISONS:
            a = G.Guard(poison, DEV)
            runs.append(device_chain(a, c["case"], x, w, b, dy))
            a.assert_intact()
            check_untouched(runs[-1])
    assert same_bits(*runs)
    return runs[0], picks


@pytest.mark.parametrize("c", FF.CASES, ids=TF.layer_id)
def test_family_exact(c):
    n, h, wd, cin, cout, k, act, dt, view, oview = c["case"]
    x, w, b, dy = B.exact_operands(c["case"])
    r, picks = run_family(c, x, w, b, dy)
    y64 = B.forward(x, w, b, k, act)
    assert torch.equal(r["y"], B.bf16(y64)), f"y: {int((r['y'] != B.bf16(y64)).sum())} of {y64.numel()} elements differ ({picks})"
    want = B.grads(x, w, dy, r["y"], k, act)
    for name in ("g", "dw", "db", "dx"):
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ ({picks})"
    assert want["dw"].any() and want["db"].any() and want["dx"].any()


@pytest.mark.parametrize("c", FF.CASES, ids=TF.layer_id)
def test_family_random_within_bounds(c):
    n, h, wd, cin, cout, k, act, dt, view, oview = c["case"]
    x, w, b, dy = B.random_operands(c["case"])
    r, picks = run_family(c, x, w, b, dy)
    want = B.grads(x, w, dy, r["y"], k, act)
    assert torch.equal(r["g"], want["g"])
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  dx=B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    print(f"fire families {TF.layer_id(c)} {picks}: largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in ratios.items()))
    assert want["dw"].any() and want["dx"].any() and all(v <= 1.0 for v in ratios.values()), ratios
