"""Conv kernels on operands of 2 to 3.75 GiB, and beyond the limit the kernels that take over: bit-exact against the integer references of
tests/helpers.py.  Tables, geometry and the reasons in tests/_large_cases.py; tests/test_large_operands_cpu.py has checked the picks,
the operand sizes, the completeness of the tables and the host bounds without a GPU.

Every hot conv kernel addresses its operands with 32-bit byte offsets through buffer descriptors; a wrong offset there does not fault -
buffer loads return zero, buffer stores are dropped - it gives silently wrong values at large batch.  What a row pins:
  * the three images of data - the first image, the one that contains byte 2^31 (table D: 2^32) and the last one - are torch.equal to
    the reference; on the x side every other image and every channel outside the view holds NaN, so a read that wraps to another image
    or channel poisons the sum;
  * every channel outside the output views still holds -77 in ALL images (checked on the device, image by image; only the three slots
    are copied to the host);
  * Guard.assert_intact() under both poisons of tests/_guard.py.
The pick string is asserted right before each launch.

Memory: a poison run allocates its operands (up to three of 4 GB: y, a separate residual, the pre-add copy), checks, drops them and
empties the caching allocator before the next one; every case asserts its own peak (torch.cuda.max_memory_allocated) below 16 GiB and
prints it.  A case skips only where the device reports less than 24 GiB free."""
import gc

import pytest
import torch

import _guard as G
import _large_cases as L
from helpers import exact_chain, exact_conv
from test_conv_exact_cpu import knob, tuning
from test_conv_exact_gpu import DEV, _assert_equal, _nhwc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
GIB = 2 ** 30
ids = lambda rows: [r["id"] for r in rows]


def each_poison(body):
    """body(g) once per poison with a fresh Guard; the operands are dropped and the caching allocator emptied after each run."""
    for poison in G.POISONS:
        free = torch.cuda.mem_get_info(DEV)[0]
        if free < 24 * GIB:
            pytest.skip(f"{free / GIB:.1f} GiB of device memory free, the case wants 24")
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        g = G.Guard(poison, DEV)
        try:
            body(g)
            g.assert_intact()
            peak = torch.cuda.max_memory_allocated(DEV) - before
            print(f"\npoison 0x{poison:02X}: peak device memory of the case {peak / GIB:.2f} GiB")
            assert peak < 16 * GIB
        finally:
            g.items.clear()
            del g
            gc.collect()
            torch.cuda.empty_cache()


def place(buf, slots, off, c, data_nhwc):
    buf[list(slots), ..., off:off + c] = data_nhwc


def check_view(buf, slots, off, c, ref_nchw, what, fill=-77.0):
    """The slots' view equals the reference (three images go to the host); the channels outside the view hold `fill` in every image."""
    _assert_equal(buf[..., off:off + c][list(slots)], ref_nchw, what)
    ok = torch.ones((), dtype=torch.bool, device=buf.device)
    for b in range(buf.shape[0]):          # image by image: the comparison's temporary stays at one plane
        ok &= (buf[b, ..., :off] == fill).all() & (buf[b, ..., off + c:] == fill).all()
    assert bool(ok), f"{what}: channels outside the view were written"


# ---- tables A, B and D: one conv per launch -------------------------------------------------------------------------------------------------
def _launch_conv(r, xin, wp, bp, y, d, rin, aux):
    from pytorch_yolo_amd import kernels as K
    if r["api"] == "t20_f16":
        return K.conv3x3_t20_f16(xin, wp, bp, y, d, residual=rin, y_preadd=aux, force=True)
    with tuning(-1, r["knob1"], r["knob2"]):
        assert L.conv_pick(r, d) == r["pick"]
        (K.conv2d_f16 if r["api"] == "conv2d_f16" else K.conv2d)(xin, wp, bp, y, d, residual=rin, y_preadd=aux)


def _run_conv(r, g):
    from pytorch_yolo_amd import kernels as K
    dtype = DT[r["dtype"]]
    _, h, w, cin, cout, k, stride, act, use_res, use_aux, up, f32 = r["shape"]
    x, wt, bias, res, y_ref, aux_ref = exact_conv(r["shape"][:9], r["seed"], dtype, up=up, f32_out=f32)
    d, v, n, slots = L.conv_desc_of(r), L.conv_views(r), r["n"], r["slots"]
    xin = g.alloc("x", (n, h, w, v["x"][0]), dtype, NAN)
    place(xin, slots, v["x"][1], cin, _nhwc(x, dtype))
    y = g.alloc("y", (n, d.ho, d.wo, v["y"][0]), torch.float32 if f32 else dtype, -77.0)
    rin = None
    if use_res and r["in_place_res"]:
        place(y, slots, v["y"][1], cout, _nhwc(res, dtype))
        rin = y
    elif use_res:
        rin = g.alloc("residual", (n, d.ho, d.wo, v["res"][0]), dtype, NAN)
        place(rin, slots, v["res"][1], cout, _nhwc(res, dtype))
    aux = g.alloc("pre-add copy", (n, d.ho, d.wo, v["aux"][0]), dtype, -77.0) if use_aux else None
    wp, bp, kpad, cout_pad = (K.pack_conv_weight if dtype == BF16 else K.pack_conv_weight_f16)(wt, bias, cin)
    assert (kpad, cout_pad) == (d.kpad, d.cout_pad)
    _launch_conv(r, xin, g.like("packed weights", wp), g.like("bias", bp), y, d, rin, aux)
    torch.cuda.synchronize()
    check_view(y, slots, v["y"][1], cout, y_ref, "y")
    if use_aux:
        check_view(aux, slots, v["aux"][1], cout, aux_ref, "pre-add copy")


@pytest.mark.parametrize("r", L.TABLE_A, ids=ids(L.TABLE_A))
def test_x_in_the_band(r):
    """Table A: x is 26 x 190 x 198 x 2048 with the view at the far end of the pixel; the loads of every family run with offsets past 2^31."""
    each_poison(lambda g: _run_conv(r, g))


@pytest.mark.parametrize("r", L.TABLE_B, ids=ids(L.TABLE_B))
def test_y_residual_and_pre_add_copy_in_the_band(r):
    """Table B: what the epilogue writes and reads is 2048 wide; x is narrow."""
    each_poison(lambda g: _run_conv(r, g))


@pytest.mark.parametrize("r", L.TABLE_D, ids=ids(L.TABLE_D))
def test_beyond_the_limit_the_fallbacks(r):
    """Table D: a y of 4.3 GiB; the 32-bit forms have stepped aside, the halo and gather kernels write through 64-bit pointers past 2^32."""
    each_poison(lambda g: _run_conv(r, g))


# ---- the head instance -------------------------------------------------------------------------------------------------------------------
ANCHORS, HEAD_STRIDE = [(10., 13.), (33., 23.), (59., 119.)], 16.0


def head_reference():
    """(x, w, bias, p_ref [3, na, h, w, no]) of the head row: the exact conv with 255 float32 outputs, in the layout of p."""
    n, h, w, cin, k, nc = L.HEAD_ROW["head"]
    x, wt, bias, _, y_ref, _ = exact_conv((n, h, w, cin, 3 * (nc + 5), k, 1, "none", False), L.HEAD_ROW["seed"], BF16, f32_out=True)
    return x, wt, bias, y_ref.view(n, 3, nc + 5, h, w).permute(0, 1, 3, 4, 2).contiguous()


def _run_head(g):
    from pytorch_yolo_amd import kernels as K
    r = L.HEAD_ROW
    _, h, w, cin, k, nc = r["head"]
    na, no, n, slots = 3, nc + 5, r["n"], list(r["slots"])
    x, wt, bias, p_ref = head_reference()
    d = L.head_desc_of(r)
    xin = g.alloc("x", (n, h, w, d.in_c_total), BF16, NAN)
    place(xin, slots, d.in_c_offset, cin, _nhwc(x, BF16))
    wp, bp, kpad, cout_pad = K.pack_conv_weight(wt, bias, cin)
    wp, bp = g.like("packed weights", wp), g.like("bias", bp)
    rows_total, row_off = na * h * w + 7, 5
    io = g.alloc("io", (n, rows_total, no), torch.float32, -7.0, plane=rows_total * no)
    p = g.alloc("p", (n, na, h, w, no), torch.float32, -7.0)
    assert K.head_decode_pick(d, na, nc) == r["pick"]
    K.head_decode(xin, wp, bp, d, ANCHORS, nc, HEAD_STRIDE, io, row_off, p)
    torch.cuda.synchronize()
    got = p[slots].cpu()
    assert torch.equal(got, p_ref), f"raw p: {int((got != p_ref).sum())} of {p_ref.numel()} values differ ({int(torch.isnan(got).sum())} NaN)"
    # io against yolo_decode_fwd on the exact logits, within the bounds of test_gpu_parity.py::test_fused_head_decode
    head = torch.zeros((3, h, w, K.roundup(na * no, 8)), device=DEV)
    head[..., :na * no] = p_ref.permute(0, 2, 3, 1, 4).reshape(3, h, w, na * no).to(DEV)
    io2 = torch.full((3, rows_total, no), -7.0, device=DEV)
    K.decode(head, ANCHORS, nc, HEAD_STRIDE, io2, row_off)
    torch.cuda.synchronize()
    torch.testing.assert_close(io[slots], io2, rtol=2e-5, atol=1e-4)
    assert torch.all(io[:, :row_off] == -7.0) and torch.all(io[:, row_off + na * h * w:] == -7.0)


def test_head_decode_on_x_in_the_band():
    """k64x256_8w_decode (cin 256, nc 80) on the wide x: the raw logits p bit-equal to the exact conv, io as the decode kernel gives it."""
    each_poison(_run_head)


# ---- table C (and the stem row of D): the fused kernels ----------------------------------------------------------------------------------
IMG = [0, 0, 1]          # the reference image behind each slot: the middle slot repeats image 0


def _run_unit(r, g):
    from pytorch_yolo_amd import kernels as K
    _, h, w, c, act = r["shape"]
    n, slots = r["n"], r["slots"]
    x, stages, res, unit, y_ref, aux_ref, _ = exact_chain("unit", r["shape"], r["seed"])
    (w1, b1, _, _, _), (w2, b2, _, _, _) = stages
    w1p, b1p, kpad1, cpad1 = K.pack_conv_weight(w1, b1, c)
    w2p, b2p, kpad2, cpad2 = K.pack_conv_weight(w2, b2, c // 2)
    d = L.fused_desc_of(r, kpad2, cpad2)
    off = d.in_c_offset
    xin = g.alloc("x", (n, h, w, L.CT), BF16, NAN)
    place(xin, slots, off, c, _nhwc(x[IMG], BF16))
    dev = [g.like(name, t) for name, t in (("w1", w1p), ("b1", b1p), ("w2", w2p), ("b2", b2p))]
    y = g.alloc("y", (n, h, w, L.CT), BF16, -77.0)
    aux = g.alloc("pre-add copy", (n, h, w, L.CT), BF16, -77.0)
    with knob(3, r["knob3"]):
        assert K.resunit_pick(d, True) == r["pick"]
        K.resunit(xin, dev[0], dev[1], dev[2], dev[3], y, d, kpad1, cpad1, y_preadd=aux)
    torch.cuda.synchronize()
    check_view(y, slots, off, c, y_ref[IMG], "y")
    check_view(aux, slots, off, c, aux_ref[IMG], "pre-add copy")


def _run_stem(r, g):
    from pytorch_yolo_amd import kernels as K
    _, cin, h, w, act = r["shape"]
    n, slots = r["n"], r["slots"]
    x, stages, res, unit, y_ref, _, _ = exact_chain("stem", r["shape"], r["seed"])
    (w1, b1, _, _, _), (w2, b2, _, _, _) = stages
    w1p, b1p, kpad1, _ = K.pack_conv_weight(w1, b1, 8)
    w2p, b2p, kpad2, cpad2 = K.pack_conv_weight(w2, b2, 32)
    d = L.fused_desc_of(r, kpad2, cpad2)
    xd = g.alloc("x (float32 NCHW)", (n, cin, h, w), torch.float32, NAN)
    xd[list(slots)] = x[IMG].to(DEV)
    dev = [g.like(name, t) for name, t in (("w1", w1p), ("b1", b1p), ("w2", w2p), ("b2", b2p))]
    y = g.alloc("y", (n, d.ho, d.wo, L.CT), BF16, -77.0)
    assert K.stem_pick(cin, d).startswith(r["pick"]), K.stem_pick(cin, d)
    K.stem(xd, cin, dev[0], dev[1], kpad1, dev[2], dev[3], y, d)
    torch.cuda.synchronize()
    check_view(y, slots, d.out_c_offset, 64, y_ref[IMG], "y")


def _run_mbconv(r, g):
    from pytorch_yolo_amd import kernels as K
    _, h, w, cin, hidden, cout, stride = r["shape"]
    n, slots = r["n"], r["slots"]
    x, stages, res, unit, y_ref, _, _ = exact_chain("mbconv", r["shape"], r["seed"])
    (we, be, _, _, _), (wd, bd, _, _, _), (wp, bp, _, _, _) = stages
    a = L.mbconv_args(r)
    xin = g.alloc("x", (n, h, w, L.CT), BF16, NAN)
    place(xin, slots, a["in_view"][1], cin, _nhwc(x[IMG], BF16))
    y = g.alloc("y", (n, h, w, L.CT), BF16, -77.0)
    names = ("w expand", "b expand", "w depthwise", "b depthwise", "w project", "b project")
    packed = tuple(g.like(name, t) for name, t in zip(names, K.pack_mbconv(we, be, wd, bd, wp, bp, stride=stride)))
    assert K.mbconv_pick(**a).startswith(r["pick"]), K.mbconv_pick(**a)
    K.mbconv(xin, packed, y, has_res=res is not None, **a)
    torch.cuda.synchronize()
    check_view(y, slots, a["out_view"][1], cout, y_ref[IMG], "y")


@pytest.mark.parametrize("r", L.FUSED_ROWS, ids=ids(L.FUSED_ROWS))
def test_fused_kernels_on_wide_operands(r):
    """Table C: the six fused-unit kernels with x (their residual too), y and the pre-add copy in the band, the two-role stem writing a
    wide y, the MBConv tile form on wide views; and table D's stem: 30 images, the one-role kernel writing past 2^32."""
    run = {"unit": _run_unit, "stem": _run_stem, "mbconv": _run_mbconv}[r["kind"]]
    each_poison(lambda g: run(r, g))
