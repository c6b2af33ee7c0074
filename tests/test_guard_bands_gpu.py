"""Guarded runs of the C-ABI entry points that have no bit-exact case table: where does a kernel reach in memory along the PIXEL
direction?  (tests/test_conv_exact_gpu.py and tests/test_fused_exact_gpu.py run their own tables between the same margins.)

Every pointer argument of a call - inputs, outputs, weights, biases, workspaces, counters - is allocated by tests/_guard.py: in the
middle of a larger allocation whose margins (64 KiB, or one image plane of the operand where that is more) hold a poison byte.  One
test per entry point, at the smallest partial-tile shapes the value tests of that kernel already name:
  1. the call runs once on plain tensors;
  2. it runs once per poison (0xFF = NaN in every float type, -1 in int32; 0x7F = 3.39e38 in bf16 / f32, NaN in f16) on guarded ones;
  3. the guarded outputs are bit-equal to the plain ones (a stray READ that reaches a result shows here) and finite wherever those are;
  4. every margin still holds its poison (a stray WRITE shows here, with operand, side, count and first offset).
Where torch has a cheap exact reference (pools, SPP, shuffle, input packing, letterbox) the outputs are compared with it as well.
Input views keep the channel-direction guards of the value tests: x sits at a channel offset inside a wider buffer whose other
channels hold NaN, y among -77 values that must survive.

The limit of the method: a stray read whose value a later select discards stays invisible; nothing here can fault, every over-reach
of up to one image plane lands in memory the test owns."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases as CS
import _exact_cases as E
import _guard as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ANCHORS = [(10., 13.), (33., 23.), (59., 119.)]


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(-1).view(torch.uint8)


def _assert_same(name, got, want, poison):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    if not torch.equal(_bits(got), _bits(want)):
        g, w = got.detach().cpu(), want.detach().cpu()
        if g.is_floating_point():
            g, w = g.double(), w.double()
            bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
        else:
            bad = g != w
        idx = bad.nonzero()[:4].tolist()
        pytest.fail(f"{name} (poison 0x{poison:02X}): {int(bad.sum())} of {bad.numel()} values differ from the plain run - a read outside an "
                    f"operand; first at {idx}: got {[float(g[tuple(i)]) for i in idx]}, want {[float(w[tuple(i)]) for i in idx]}")
    if got.is_floating_point():
        fin = torch.isfinite(want.detach().cpu().double())
        assert bool(torch.isfinite(got.detach().cpu().double())[fin].all()), f"{name}: non-finite where the plain run is finite"


def guarded_runs(body, check=None):
    """body(a) launches on operands from the allocator ``a`` (G.Plain, then one G.Guard per poison) and returns {name: output};
    ``check(outputs)`` compares the plain outputs with a reference.  Returns the plain outputs."""
    want = body(G.Plain(DEV))
    torch.cuda.synchronize()
    want = {k: v.detach().clone() for k, v in want.items()}
    if check is not None:
        check(want)
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        got = body(g)
        torch.cuda.synchronize()
        assert set(got) == set(want)
        for k in want:
            _assert_same(k, got[k], want[k], poison)
        g.assert_intact()
    return want


def _view(a, name, x_nchw, dtype, c_total, c_offset, fill=NAN):
    """x NCHW (host) -> NHWC view at c_offset of an operand of c_total channels from allocator ``a``, ``fill`` elsewhere."""
    n, c, h, w = x_nchw.shape
    buf = a.alloc(name, (n, h, w, c_total), dtype, fill)
    buf[..., c_offset:c_offset + c] = x_nchw.permute(0, 2, 3, 1).to(dtype).to(DEV)
    return buf


def _act(name):
    from pytorch_yolo_amd import _lib
    return {"swish": _lib.ACT_SWISH, "relu6": _lib.ACT_RELU6, "relu": _lib.ACT_RELU, "none": _lib.ACT_NONE, "leaky": _lib.ACT_LEAKY01}[name]


def _lib_call(fn_name, *args):
    from pytorch_yolo_amd._lib import check, load
    check(getattr(load(), fn_name)(*args), fn_name)


def _stream():
    from pytorch_yolo_amd import kernels as K
    return K.stream_ptr()


# ------------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n,c,h,w", [(1, 8, 1, 1), (1, 48, 7, 33)])
def test_dwconv3x3_guarded(n, c, h, w, stride):
    """yolo_dwconv3x3_fwd (strip kernel, 8 output rows per thread): a one-pixel map and a height that is no multiple of the strip."""
    from pytorch_yolo_amd import kernels as K
    gen = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=gen)
    wt = (torch.randn(c, 1, 3, 3, generator=gen) * 0.3).reshape(c, 9).t().contiguous()
    b = torch.randn(c, generator=gen) * 0.1
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1

    def body(a):
        xin = _view(a, "x", x, BF16, c + 16, 8)
        y = a.alloc("y", (n, ho, wo, c + 8), BF16, -77.0)
        K.dwconv3x3(xin, a.like("w", wt), a.like("bias", b), y, n=n, h=h, w=w, c=c, in_view=(c + 16, 8), out_view=(c + 8, 8),
                    stride=stride, act=_act("relu6"))
        return {"y": y}

    def check(out):
        ref = F.relu6(F.conv2d(x.to(BF16).float(), wt.t().reshape(c, 1, 3, 3), b, stride=stride, padding=1, groups=c))
        torch.testing.assert_close(out["y"][..., 8:].float().permute(0, 3, 1, 2).cpu(), ref, rtol=1e-2, atol=1e-2)
        assert torch.all(out["y"][..., :8] == -77.0)
    guarded_runs(body, check)


DW_CASES = [(3, 1, 20, 26, 32, "swish", "same"), (3, 2, 26, 26, 96, "swish", "same"), (5, 2, 52, 52, 144, "swish", "same"),
            (5, 1, 13, 13, 672, "swish", "same"), (5, 2, 13, 13, 40, "relu6", "same"), (3, 2, 27, 27, 24, "none", "same")]
DW_F32_CASES = DW_CASES + [(3, 1, 9, 7, 12, "relu", "pad1"), (3, 2, 8, 8, 16, "leaky", "pad1")]


def _dw_geometry(k, stride, h, w, geometry):
    from pytorch_yolo_amd.engine import Recorder
    if geometry == "same":
        (ho, pad), (wo, _) = Recorder.tf_same(h, k, stride), Recorder.tf_same(w, k, stride)
        return ho, wo, pad
    return (h - 1) // stride + 1, (w - 1) // stride + 1, 1


@pytest.mark.parametrize("k,stride,h,w,c,act,geometry", DW_CASES)
def test_dwconv_guarded(k, stride, h, w, c, act, geometry):
    """yolo_dwconv_fwd: k 3 and 5, strides 1 and 2, even maps (the odd pad row / column below / right) and odd ones."""
    from pytorch_yolo_amd import kernels as K
    n = 2
    gen = torch.Generator().manual_seed(k * 100 + h + c)
    x = torch.randn(n, c, h, w, generator=gen)
    wt = (torch.randn(c, 1, k, k, generator=gen) * 0.3).reshape(c, k * k).t().contiguous()
    b = torch.randn(c, generator=gen) * 0.1
    ho, wo, pad = _dw_geometry(k, stride, h, w, geometry)

    def body(a):
        xin = _view(a, "x", x, BF16, c + 16, 8)
        y = a.alloc("y", (n, ho, wo, c + 8), BF16, -77.0)
        K.dwconv(xin, a.like("w", wt), a.like("bias", b), y, n=n, h=h, w=w, c=c, in_view=(c + 16, 8), out_view=(c + 8, 8), ho=ho, wo=wo,
                 ksize=k, stride=stride, pad=pad, act=_act(act))
        return {"y": y}
    out = guarded_runs(body)
    assert torch.all(out["y"][..., :8] == -77.0) and bool(torch.isfinite(out["y"].float()).all())


@pytest.mark.parametrize("k,stride,h,w,c,act,geometry", DW_F32_CASES)
def test_dwconv_f32_guarded(k, stride, h, w, c, act, geometry):
    """yolo_dwconv_f32_fwd: the shapes of the bf16 kernel plus torch's pad 1 on channel counts that are multiples of 4 only."""
    from pytorch_yolo_amd import kernels as K
    n = 2
    gen = torch.Generator().manual_seed(k * 100 + h + c)
    x = torch.randn(n, c, h, w, generator=gen)
    wt = (torch.randn(c, 1, k, k, generator=gen) * 0.3).reshape(c, k * k).t().contiguous()
    b = torch.randn(c, generator=gen) * 0.1
    ho, wo, pad = _dw_geometry(k, stride, h, w, geometry)

    def body(a):
        xin = _view(a, "x", x, F32, c + 12, 8)
        y = a.alloc("y", (n, ho, wo, c + 8), F32, -77.0)
        K.dwconv_f32(xin, a.like("w", wt), a.like("bias", b), y, n=n, h=h, w=w, c=c, in_view=(c + 12, 8), out_view=(c + 8, 4), ho=ho,
                     wo=wo, ksize=k, stride=stride, pad=pad, act=_act(act))
        return {"y": y}
    out = guarded_runs(body)
    assert torch.all(out["y"][..., :4] == -77.0) and torch.all(out["y"][..., 4 + c:] == -77.0) and bool(torch.isfinite(out["y"]).all())


# ------------------------------------------------------------------------------------------------ squeeze-excite, shuffle
@pytest.mark.parametrize("n,h,w,c,sq,dtype", [(2, 7, 9, 1152, 48, BF16), (3, 52, 52, 96, 4, BF16), (2, 7, 9, 1152, 48, F32), (3, 52, 52, 96, 4, F32),
                                              (1, 5, 3, 8, 4, F32)],          # a map smaller than one pixel range (test_se_f32_kernel)
                         ids=lambda v: str(v).replace("torch.", ""))
def test_squeeze_excite_guarded(n, h, w, c, sq, dtype):
    """yolo_se_fwd / yolo_se_f32_fwd with their workspace (pooled means, scales, partial sums of the pooling pass)."""
    from pytorch_yolo_amd import kernels as K
    gen = torch.Generator().manual_seed(c + sq)
    x = torch.randn(n, c, h, w, generator=gen)
    w1, b1 = torch.randn(sq, c, generator=gen) * (1.0 / c) ** 0.5, torch.randn(sq, generator=gen) * 0.1
    w2, b2 = (torch.randn(c, sq, generator=gen) * (1.0 / sq) ** 0.5).t().contiguous(), torch.randn(c, generator=gen) * 0.1
    fn = K.se if dtype == BF16 else K.se_f32

    def body(a):
        xin = _view(a, "x", x, dtype, c + 8, 8 if dtype == BF16 else 4)
        y = a.alloc("y", (n, h, w, c + 16), dtype, -77.0)
        ws = a.alloc("workspace", (K.se_workspace_bytes(n, c) // 4,), F32)
        fn(xin, y, a.like("w1", w1), a.like("b1", b1), a.like("w2", w2), a.like("b2", b2), ws, n=n, h=h, w=w, c=c,
           in_view=(c + 8, 8 if dtype == BF16 else 4), out_view=(c + 16, 8))
        return {"y": y, "pooled means": ws[:n * c]}

    def check(out):
        xr = x.to(dtype).float()
        torch.testing.assert_close(out["pooled means"].cpu().reshape(n, c), xr.mean((2, 3)), rtol=1e-4, atol=1e-5)
        assert torch.all(out["y"][..., :8] == -77.0) and torch.all(out["y"][..., 8 + c:] == -77.0)
    guarded_runs(body, check)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("half,slot", [(58, 64), (8, 8)])
def test_channel_shuffle_guarded(half, slot, dtype):
    """yolo_channel_shuffle2_fwd / yolo_channel_shuffle2_f32_fwd: a and b are two views of one wider buffer, y a view of a third."""
    from pytorch_yolo_amd import kernels as K
    n, h, w = 2, 9, 7
    gen = torch.Generator().manual_seed(half)
    ab = torch.randn(n, 2 * slot, h, w, generator=gen).to(dtype).float()
    ab[:, half:slot] = 0
    ab[:, slot + half:] = 0                                    # the pad channels of both slots are zero by contract
    ct_in, ct_out = 2 * slot + 8, 2 * slot + 16

    def body(a):
        buf = _view(a, "a, b", ab, dtype, ct_in, 8 if dtype == BF16 else 4)
        off = 8 if dtype == BF16 else 4
        y = a.alloc("y", (n, h, w, ct_out), dtype, -77.0)
        if dtype == BF16:
            _lib_call("yolo_channel_shuffle2_fwd", buf.data_ptr(), buf.data_ptr(), y.data_ptr(), n, h, w, half, slot, ct_in, off, ct_in,
                      off + slot, ct_out, 8, _stream())
        else:
            K.shuffle2_f32(buf, buf, y, n=n, h=h, w=w, half=half, c_slot=slot, a_view=(ct_in, off), b_view=(ct_in, off + slot), y_view=(ct_out, 8))
        return {"y": y}

    def check(out):
        got = out["y"][..., 8:8 + 2 * slot].float().permute(0, 3, 1, 2).cpu()
        logical = torch.cat([ab[:, :half], ab[:, slot:slot + half]], 1)
        want = logical.view(n, 2, half, h, w).transpose(1, 2).reshape(n, 2 * half, h, w)
        assert torch.equal(got[:, :half], want[:, :half]) and torch.equal(got[:, slot:slot + half], want[:, half:])
        assert torch.all(out["y"][..., :8] == -77.0) and torch.all(out["y"][..., 8 + 2 * slot:] == -77.0)
    guarded_runs(body, check)


# ------------------------------------------------------------------------------------------------ pools, SPP
def _ceil_out(n, k, s):
    o = -(-(n - k) // s) + 1
    return o - 1 if (o - 1) * s >= n else o


POOL_GEOMETRY = [(13, 20, k, s, False) for k, s in ((2, 2), (2, 1), (5, 1), (9, 1), (13, 1), (3, 2))] + \
                [(h, w, 3, 2, True) for h, w in ((10, 13), (64, 80), (7, 7), (103, 51))]


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("h,w,k,s,ceil", POOL_GEOMETRY)
def test_maxpool_guarded(h, w, k, s, ceil, dtype):
    """yolo_maxpool_fwd / _f16_fwd / _f32_fwd on every (k, s) of test_maxpool_exact and on the ceil-mode maps of the SqueezeNet
    encoder, whose last window hangs over the border.  A pool's taps outside the image are -inf; a kernel that read a pixel row
    outside the operand instead would take its maximum with the margin.  The 0x7F run is the one that matters here: 3.39e38 wins
    every maximum (in f16 the byte is NaN), while the NaN of 0xFF is dropped by a compare-and-select maximum."""
    from pytorch_yolo_amd import kernels as K
    n, c = 2, 16
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(100 * k + s + h)).to(dtype).float()
    if ceil:
        pad, dil, ho, wo = 0, 1, _ceil_out(h, k, s), _ceil_out(w, k, s)
        want = F.max_pool2d(x, k, s, ceil_mode=True)
    else:
        pad, dil = (1, 2) if (k, s) == (2, 1) else ((k - 1) // 2, 1)
        want = F.max_pool2d(x, k, s, padding=pad, dilation=dil)
        ho, wo = want.shape[2:]
    assert want.shape == (n, c, ho, wo)
    fn = {BF16: "yolo_maxpool_fwd", F16: "yolo_maxpool_f16_fwd", F32: "yolo_maxpool_f32_fwd"}[dtype]

    def body(a):
        xin = _view(a, "x", x, dtype, c + 8, 8)
        y = a.alloc("y", (n, ho, wo, c + 8), dtype, -77.0)
        _lib_call(fn, xin.data_ptr(), y.data_ptr(), n, h, w, c, c + 8, 8, ho, wo, c + 8, 8, k, s, pad, dil, _stream())
        return {"y": y}

    def check(out):
        assert torch.equal(out["y"][..., 8:].float().permute(0, 3, 1, 2).cpu(), want) and torch.all(out["y"][..., :8] == -77.0)
    guarded_runs(body, check)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("h,w,c", [(4, 3, 24), (13, 17, 24), (1, 9, 64), (13, 17, 64)])
def test_spp_guarded(h, w, c, dtype):
    """yolo_spp_fwd, both kernels (c % 64 == 0: whole 128-byte lines), on maps smaller than the 13-wide window; the one buffer is
    input and output.  As for the pools the 0x7F run is the one that matters (it orders 16-bit patterns: 0x7F7F is a large positive
    value in bf16 and in f16 alike)."""
    from pytorch_yolo_amd import kernels as K
    n = 3
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h * 100 + w)).to(dtype).float()
    want = torch.cat([F.max_pool2d(x, 5, 1, 2), F.max_pool2d(x, 9, 1, 4), F.max_pool2d(x, 13, 1, 6), x], 1)

    def body(a):
        buf = a.alloc("concat buffer", (n, h, w, 4 * c), dtype, 0.0)
        buf[..., 3 * c:] = x.permute(0, 2, 3, 1).to(dtype).to(DEV)
        K.spp(buf, n=n, h=h, w=w, c=c)
        return {"concat buffer": buf}

    def check(out):
        assert torch.equal(out["concat buffer"].float().permute(0, 3, 1, 2).cpu(), want)
    guarded_runs(body, check)


# ------------------------------------------------------------------------------------------------ decode and heads
@pytest.mark.parametrize("nc,ny,nx", [(3, 4, 6), (1, 5, 5), (80, 13, 13)])
def test_decode_guarded(nc, ny, nx):
    """yolo_decode_fwd: io rows at an offset inside a longer buffer, and p."""
    from pytorch_yolo_amd import kernels as K
    bs, na, no = 2, 3, nc + 5
    ct = K.roundup(na * no, 8)
    head = torch.randn(bs, ny, nx, ct, generator=torch.Generator().manual_seed(nc + ny)) * 2.0
    rows = na * ny * nx

    def body(a):
        io = a.alloc("io", (bs, rows + 7, no), F32, -7.0, plane=(rows + 7) * no)
        p = a.alloc("p", (bs, na, ny, nx, no), F32, -7.0)
        K.decode(a.like("head", head), ANCHORS, nc, 32.0, io, 5, p)
        return {"io": io, "p": p}
    out = guarded_runs(body)
    assert torch.all(out["io"][:, :5] == -7.0) and torch.all(out["io"][:, 5 + rows:] == -7.0) and bool(torch.isfinite(out["io"]).all())


_HEAD_ACT = {(2, 20, 20, 256, 1, 80): "leaky", (2, 14, 14, 96, 1, 80): "leaky", (2, 8, 8, 72, 1, 3): "none"}        # as test_fused_head_decode runs them
HEAD_CASES = [v["head"] + (_HEAD_ACT[v["head"]],) for v in E.BF16_INSTANCES.values() if "head" in v] + [(1, 10, 12, 64, 3, 80, "leaky")]   # + one 3x3 head
HEAD_F16_SHAPES = [(2, 20, 20, 256, 1, 80, "leaky"), (3, 13, 13, 96, 1, 80, "none"), (2, 10, 12, 40, 3, 3, "leaky")]    # HEAD_F16_CASES


def _head_operands(n, h, w, cin, k, nc, act, dtype):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F32
    na, no = 3, nc + 5
    cout = na * no
    gen = torch.Generator().manual_seed(h * 7 + cin + n)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=gen)
    wp, bp, kpad, cout_pad = (K.pack_conv_weight if dtype == BF16 else K.pack_conv_weight_f16)(wt, bias, cin)
    c_off = 8 if dtype == BF16 else 0          # the views of test_fused_head_decode / test_head_decode_f16
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 8, in_c_offset=c_off, cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                    ksize=k, stride=1, act=_act(act), kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F32)
    return x, wp, bp, d, na, no


def _head_decode_guarded(n, h, w, cin, k, nc, act, dtype):
    from pytorch_yolo_amd import kernels as K
    x, wp, bp, d, na, no = _head_operands(n, h, w, cin, k, nc, act, dtype)
    rows = na * h * w
    fn = K.head_decode if dtype == BF16 else K.head_decode_f16

    def body(a):
        xin = _view(a, "x", x, dtype, cin + 8, d.in_c_offset)
        io = a.alloc("io", (n, rows + 7, no), F32, -7.0, plane=(rows + 7) * no)
        p = a.alloc("p", (n, na, h, w, no), F32, -7.0)
        fn(xin, a.like("packed weights", wp), a.like("bias", bp), d, ANCHORS, nc, 16.0, io, 5, p)
        return {"io": io, "p": p}
    out = guarded_runs(body)
    assert torch.all(out["io"][:, :5] == -7.0) and torch.all(out["io"][:, 5 + rows:] == -7.0)
    assert bool(torch.isfinite(out["p"]).all()) and bool((out["p"] != -7.0).all())


@pytest.mark.parametrize("n,h,w,cin,k,nc,act", HEAD_CASES)
def test_head_decode_guarded(n, h, w, cin, k, nc, act):
    """yolo_head_decode_fwd: the three decode instances through the head= shapes of _exact_cases.BF16_INSTANCES, and a 3x3 head."""
    from pytorch_yolo_amd import kernels as K
    picks = {v["head"]: v["pick"] for v in E.BF16_INSTANCES.values() if "head" in v}
    if (n, h, w, cin, k, nc) in picks:
        d = _head_operands(n, h, w, cin, k, nc, act, BF16)[3]
        assert K.head_decode_pick(d, 3, nc).startswith("igemm" + picks[(n, h, w, cin, k, nc)]), K.head_decode_pick(d, 3, nc)
    _head_decode_guarded(n, h, w, cin, k, nc, act, BF16)


@pytest.mark.parametrize("n,h,w,cin,k,nc,act", HEAD_F16_SHAPES)
def test_head_decode_f16_guarded(n, h, w, cin, k, nc, act):
    """yolo_head_decode_f16_fwd on the shapes of HEAD_F16_CASES (tests/test_fp16_gpu.py): the three fp16 decode instances, one 3x3."""
    _head_decode_guarded(n, h, w, cin, k, nc, act, F16)


def _kept(dets, idx, cnt):
    """What the NMS contract defines: the counts and the first min(count, cap) rows of every image."""
    torch.cuda.synchronize()
    c = cnt.cpu().tolist()
    cap = dets.shape[1]
    rows = [dets[b, :min(m, cap)] for b, m in enumerate(c)]
    pivots = [idx[b, :min(m, cap)] for b, m in enumerate(c)]
    return {"count": cnt, "dets": torch.cat(rows), "idx": torch.cat(pivots)}


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,cin,k,nc,act,conf", [(2, 8, 8, 72, 1, 3, "none", 0.2), (5, 3, 3, 64, 1, 1, "none", 0.3),
                                                      (1, 10, 12, 64, 3, 80, "leaky", 0.02), (2, 14, 14, 96, 1, 80, "leaky", 0.001)])
def test_compact_nms_guarded(n, h, w, cin, k, nc, act, conf, dtype):
    """yolo_head_decode_filter_fwd / _f16_fwd followed by yolo_nms_merge_compact: the compact workspace (pre-filled with 0xCD), p,
    dets, idx and count between margins; shapes of test_head_decode_filter_is_the_plain_head_plus_nms."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import MAX_PER_CLASS, MIN_WH, nms_capacity
    x, wp, bp, d, na, no = _head_operands(n, h, w, cin, k, nc, act, dtype)
    rows = na * h * w                          # the one head covers every row: the workspace then needs no initialisation
    cap = nms_capacity(rows, nc)
    fn = K.head_decode_filter if dtype == BF16 else K.head_decode_filter_f16

    def body(a):
        xin = _view(a, "x", x, dtype, cin + 8, d.in_c_offset)
        ws = a.alloc("compact workspace", (K.nms_compact_workspace_bytes(n, rows, nc),), torch.uint8, 0xCD)
        p = a.alloc("p", (n, na, h, w, no), F32, -7.0)
        fn(xin, a.like("packed weights", wp), a.like("bias", bp), d, ANCHORS, nc, 16.0, rows, 0, conf, ws, min_wh=MIN_WH, p=p)
        dets = a.alloc("dets", (n, cap, 7), F32, -3.0, plane=cap * 7)
        idx = a.alloc("idx", (n, cap), torch.int32, -3, plane=cap)
        cnt = a.alloc("count", (n,), torch.int32, -3)
        K.nms_merge_compact(ws, n, rows, nc, 0.5, dets, idx, cnt, max_per_class=MAX_PER_CLASS)
        out = _kept(dets, idx, cnt)
        out["p"] = p
        return out
    out = guarded_runs(body)
    assert int(out["count"].sum()) > 0, "the case is vacuous: nothing survives"


@pytest.mark.parametrize("name", ["nms_small_nc2", "nms_none_pass", "rows_12000"])
def test_nms_merge_guarded(name):
    """yolo_nms_merge: pred, the workspace and the three outputs between margins; the 12000-row case sorts its keys in the global
    workspace instead of LDS (test_nms_many_survivors_global_sort_path)."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import MAX_PER_CLASS, MIN_WH, nms_capacity
    if name == "rows_12000":
        pred = CS.synth_predictions(77, 1, 12000, 4)
        pred[0, :, 4] = np.maximum(pred[0, :, 4], np.float32(0.5))
        conf, iou = 0.001, 0.5
    else:
        pred, conf, iou = CS.nms_case_inputs(name)
    bs, rows, no = pred.shape
    nc = no - 5
    cap = nms_capacity(rows, nc)
    pred_t = torch.from_numpy(pred.copy())

    def body(a):
        p = a.like("pred", pred_t, plane=rows * no)
        ws = a.alloc("workspace", (K.nms_workspace_bytes(bs, rows, nc),), torch.uint8, 0xCD)
        dets = a.alloc("dets", (bs, cap, 7), F32, -3.0, plane=cap * 7)
        idx = a.alloc("idx", (bs, cap), torch.int32, -3, plane=cap)
        cnt = a.alloc("count", (bs,), torch.int32, -3)
        K.nms_merge(p, conf, iou, dets, idx, cnt, ws, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS)
        out = _kept(dets, idx, cnt)
        out["pred"] = p
        return out

    def check(out):
        from oracle import nms as onms
        odets, okept = onms.non_max_suppression(pred.copy(), conf, iou)
        c = out["count"].cpu().tolist()
        assert c == [0 if o is None else len(o) for o in odets] and sum(c) > 0
        assert np.array_equal(out["dets"].cpu().numpy(), np.concatenate([o for o in odets if o is not None]))
        assert np.array_equal(out["idx"].cpu().numpy(), np.concatenate([o for o in okept if o is not None]))
        assert np.array_equal(out["pred"].cpu().numpy(), pred, equal_nan=True), "pred is read-only without mutate_conf"
    guarded_runs(body, check)


def test_scale_coords_and_pack_detections_guarded():
    """yolo_scale_coords (in place on dets, parameters on the device) and yolo_pack_detections (dets, idx, count -> packed rows and
    int64 pivots; a count beyond the capacity is clipped to it)."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import _scale_params
    gen = torch.Generator().manual_seed(3)
    bs, cap = 7, 20
    dets0 = torch.rand(bs, cap, 7, generator=gen) * 600.0
    idx0 = torch.randint(0, 1000, (bs, cap), generator=gen, dtype=torch.int32)
    counts = [3, 0, 20, 1, 0, 25, 7]
    kept = [min(m, cap) for m in counts]
    shapes = [(1080, 1920), (333, 500), (480, 640), (375, 500), (1080, 1920), (333, 500), (480, 640)]
    params0 = torch.tensor([_scale_params((640, 640), s0, m) for s0, m in zip(shapes, kept)], dtype=F32)

    def body(a):
        dets, params = a.like("dets", dets0, plane=cap * 7), a.like("params", params0)
        _lib_call("yolo_scale_coords", dets.data_ptr(), bs, cap, 7, params.data_ptr(), 1, _stream())
        packed = a.alloc("packed", (sum(kept), 7), F32, -1.0)
        pidx = a.alloc("packed idx", (sum(kept),), torch.int64, -1)
        K.pack_detections(dets, a.like("idx", idx0, plane=cap), a.like("count", torch.tensor(counts, dtype=torch.int32)), packed, pidx)
        torch.cuda.synchronize()               # (params lives until the launches are done)
        return {"dets": dets, "packed": packed, "packed idx": pidx}

    def check(out):
        d = out["dets"].cpu()
        assert all(torch.equal(d[b, m:], dets0[b, m:]) for b, m in enumerate(kept)), "rows beyond the count were touched"
        assert torch.equal(d[..., 4:], dets0[..., 4:])
        assert torch.equal(out["packed"].cpu(), torch.cat([d[b, :m] for b, m in enumerate(kept) if m]))
        assert torch.equal(out["packed idx"].cpu(), torch.cat([idx0[b, :m] for b, m in enumerate(kept) if m]).long())
    guarded_runs(body, check)


# ------------------------------------------------------------------------------------------------ preprocess and packing
@pytest.mark.parametrize("h,w,c,new_shape", [(97, 131, 3, 96), (33, 200, 4, 128), (48, 48, 1, 96), (100, 60, 3, 64)])
def test_letterbox_guarded(h, w, c, new_shape):
    """yolo_letterbox_u8_fwd, uint8 destination: odd source sizes, down- and up-scaling (BORDER_REPLICATE reads the edge pixels; an
    INTER_AREA window that ran past the last source row or column would read the margin: 0x7F and 0xFF are both bright pixels)."""
    from oracle import preprocess as O
    from pytorch_yolo_amd.utils import augs
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, c), dtype=np.uint8)
    want, p = O.letterbox(img, new_shape)
    assert augs.letterbox_params(h, w, new_shape) == p

    def body(a):
        src = a.like("src", torch.from_numpy(img), plane=h * w * c)
        dst = a.alloc("dst", (p["target_height"], p["target_width"], c), torch.uint8, 0x11, plane=p["target_height"] * p["target_width"] * c)
        augs._launch(src, p, dst_u8=dst)
        return {"dst": dst}

    def check(out):
        assert np.array_equal(out["dst"].cpu().numpy(), want)
    guarded_runs(body, check)


def test_preprocess_batch_guarded():
    """The batched preprocess (one letterbox launch per image into its slice of the float32 NCHW batch): every source and the batch
    between margins; images 0 .. n - 2 also border their neighbours' slices, which the oracle comparison covers."""
    from oracle import preprocess as O
    from pytorch_yolo_amd.utils.augs import preprocess_batch
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((60, 100, 3), (100, 60, 3), (64, 64, 3), (50, 111, 3))]
    want, wmeta = O.preprocess_batch(imgs, 64)

    def body(a):
        srcs = [a.like(f"src {i}", torch.from_numpy(im), plane=im.size) for i, im in enumerate(imgs)]
        out = a.alloc("batch", want.shape, F32, -77.0)
        got, meta = preprocess_batch(srcs, 64, out=out)
        assert meta == wmeta
        return {"batch": got}

    def check(out):
        assert np.array_equal(out["batch"].cpu().numpy(), want)
    guarded_runs(body, check)


@pytest.mark.parametrize("dtype,c_pad", [(BF16, 8), (F16, 8), (F32, 4)], ids=["bf16", "f16", "f32"])
def test_pack_input_guarded(dtype, c_pad):
    """yolo_pack_input_nchw_f32 / _f32_f16 / _f32_nhwc: float32 NCHW of odd sizes -> NHWC, channels zero-padded."""
    from pytorch_yolo_amd import kernels as K
    n, c, h, w = 3, 3, 17, 23
    x = torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(5))
    fn = {BF16: K.pack_input, F16: K.pack_input_f16, F32: K.pack_input_f32}[dtype]

    def body(a):
        out = a.alloc("out", (n, h, w, c_pad), dtype, 7.0)
        fn(a.like("x", x), out)
        return {"out": out}

    def check(out):
        got = out["out"].cpu()
        assert torch.equal(got[..., :c], x.permute(0, 2, 3, 1).to(dtype)) and torch.all(got[..., c:] == 0)
    guarded_runs(body, check)


@pytest.mark.parametrize("cin,cout,h,w,stride,pool", [(3, 32, 37, 50, 1, False), (1, 16, 20, 33, 1, False), (3, 32, 33, 17, 2, False),
                                                      (1, 16, 38, 50, 1, True), (3, 32, 32, 32, 1, True)])
def test_first_layer_from_nchw_guarded(cin, cout, h, w, stride, pool):
    """yolo_conv1_nchw_f32_fwd (stride 1 and the stride-2 form) and yolo_conv1_pool_nchw_f32_fwd: the float32 NCHW batch, the packed
    weights, the bias and the (pooled) output view between margins."""
    from pytorch_yolo_amd import kernels as K
    n = 2
    gen = torch.Generator().manual_seed(h * w + cin)
    x = torch.rand(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    wp, bp, kpad, cpad = K.pack_conv_weight(wt, b, 8)
    d = K.conv_desc(n=n, h=h, w=w, cin=8, in_c_total=8, in_c_offset=0, cout=cout, out_c_total=cout + 16, out_c_offset=8, ksize=3,
                    stride=stride, act=_act("leaky"), kpad=kpad, cout_pad=cpad)
    ho, wo = (h // 2, w // 2) if pool else (d.ho, d.wo)
    fn = "yolo_conv1_pool_nchw_f32_fwd" if pool else "yolo_conv1_nchw_f32_fwd"

    def body(a):
        y = a.alloc("y", (n, ho, wo, cout + 16), BF16, -77.0)
        xd, wd, bd = a.like("x (float32 NCHW)", x), a.like("packed weights", wp), a.like("bias", bp)
        _lib_call(fn, xd.data_ptr(), cin, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), C.byref(d), _stream())
        torch.cuda.synchronize()               # (the operands live until the launch is done)
        return {"y": y}

    def check(out):
        r = lambda t: t.to(BF16).float()
        ref = r(F.leaky_relu(F.conv2d(r(x), r(wt), b, stride=stride, padding=1), 0.1))
        if pool:
            ref = F.max_pool2d(ref, 2, 2)
        y = out["y"]
        torch.testing.assert_close(y[..., 8:8 + cout].float().permute(0, 3, 1, 2).cpu(), ref, rtol=2e-2, atol=2e-2)
        assert torch.all(y[..., :8] == -77.0) and torch.all(y[..., 8 + cout:] == -77.0)
    guarded_runs(body, check)


# ------------------------------------------------------------------------------------------------ the method itself, on the device
@pytest.mark.parametrize("poison", G.POISONS)
def test_guard_notices_a_pool_that_is_one_row_off(poison):
    """What a kernel with an off-by-one row bound would do, produced with a correct kernel and a wrong description: yolo_maxpool_fwd
    (3, 1, pad 1) is told of h + 1 rows while x and y hold h.  It reads one pixel row behind x and writes one behind y - 960 and
    1280 bytes into margins of 64 KiB, memory the test owns.  Each poison sees one half of it, which is why every test runs both:
      * 0xFF: the kernel's fmaxf drops the NaN of the stray input row, every value stays right - but the stray OUTPUT row (the
        maxima of the last real row) changes the margin behind y: reported as y / above / first byte 16 (the view's channel offset);
      * 0x7F: the stray input row's 3.39e38 wins every maximum of the last real output row, which no longer equals torch's - but the
        stray output row is 3.39e38 as well, the very bytes of the margin, and the write goes unseen."""
    n, c, h, w = 1, 16, 6, 20
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(9)).to(BF16).float()
    want = F.max_pool2d(x, 3, 1, 1)
    g = G.Guard(poison, DEV)
    xin = _view(g, "x", x, BF16, c + 8, 8)
    y = g.alloc("y", (n, h, w, c + 16), BF16, -77.0)
    _lib_call("yolo_maxpool_fwd", xin.data_ptr(), y.data_ptr(), n, h + 1, w, c, c + 8, 8, h + 1, w, c + 16, 8, 3, 1, 1, 1, _stream())
    torch.cuda.synchronize()
    rep = g.report()
    got = y[..., 8:8 + c].float().permute(0, 3, 1, 2).cpu()
    assert torch.equal(got[:, :, :h - 1], want[:, :, :h - 1]) and torch.all(y[..., :8] == -77.0) and torch.all(y[..., 8 + c:] == -77.0)
    if poison == 0xFF:
        # (w * c values of two bytes; a value whose low byte happens to be 0xFF leaves that byte of the margin as it was)
        assert len(rep) == 1 and rep[0][:2] == ("y", "above") and 0.95 * w * c * 2 <= rep[0][2] <= w * c * 2 and 16 <= rep[0][3] <= 18, rep
        with pytest.raises(AssertionError, match=r"y: 6\d\d byte\(s\) above the payload changed"):
            g.assert_intact()
        assert torch.equal(got[:, :, h - 1], want[:, :, h - 1])
    else:
        assert bool((got[:, :, h - 1] > 3e38).all()), "the stray row's poison did not reach the result"
        assert rep == [], rep
