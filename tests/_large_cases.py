"""Case tables of the large-operand tests (tests/test_large_operands_cpu.py checks picks, sizes, completeness and the host bounds without
a GPU, tests/test_large_operands_gpu.py launches every row): conv kernels on operands of 2 to 3.75 GiB - the band in which the 32-bit
byte offsets of the buffer-descriptor kernels have their top bit set - and, beyond the limit, the kernels that take over.

The limit is kOobOffset = 0xF0000000 bytes (csrc/conv_common.h): an x view or a weight matrix of that size is refused, a y / residual /
pre-add copy of that size makes the 32-bit forms (t20v2, t20s2, stream1x1, stream1x1p, resunit64_t20, resunit_t20w, stem2) give way to
a kernel that writes through 64-bit pointers.  The wide MBConv form refuses an x view of 2^31 bytes and more.

How an operand gets large cheaply: its VIEW is wide, not the layer.  A wide operand has c_total = 2048 (the SPP concat width) and the
layer's channels at the far end of the pixel, offset 2048 - c - 8.  26 images of 190 x 198 pixels make 26 planes of 154 091 520 bytes =
0xEECC8000 = 4 006 379 520 bytes, less than one plane below the limit:
  * image 13 contains byte 2^31 (planes 13 * 154 091 520 = 2 003 189 760 .. 2 157 281 280);
  * images 14..25 lie wholly above it;
  * image 25 ends 20 MB below kOobOffset.
190 x 198 has partial 16x16 and 20x20 tiles in both directions, passes the 80x80 / cover conditions of the halo kernel and of the
fused units, and every row has at least two K steps.

Data: exact integer operands (tests/helpers.py::exact_conv / exact_chain) of three images go to SLOTS = 0, 13 and 25 (a fused row's two
images go to 0 and 25, slot 13 repeats image 0).  On the x side every other image and every channel outside the view holds NaN: a read
that wraps to another image or channel poisons the sum.  y, the pre-add copy and a separate residual are pre-filled with -77 / NaN.
Beyond the limit (table D) 30 images make 0x113898000 bytes, more than 2^32; image 27 contains byte 2^32: slots 0, 27, 29.

A row names the operands that are wide (`wide`: "x", "y", "res", "aux"); the others are narrow (x: cin + 16 channels, y: cout + 16,
residual: cout + 16, pre-add copy: cout + 8, all at offset 8).  The picks were returned by the host pick functions at 256 compute
units and are pinned here as full strings; both test files compare them, the GPU one right before each launch."""
import os
import re

from _exact_cases import CSRC, STREAM_FIRST_FORM, STREAM_ALWAYS, T20_ALWAYS, T20_NEVER, RU_T20_NEVER

STREAM_NEVER = 1024                        # kFamStreamNever (knob 2)
LIMIT = 0xF0000000                         # kOobOffset
H, W, CT = 190, 198, 2048
PLANE = H * W * CT * 2                     # bytes of one wide image
N_BAND, SLOTS_BAND = 26, (0, 13, 25)
N_BEYOND, SLOTS_BEYOND = 30, (0, 27, 29)
L, NO, R6 = "leaky", "none", "relu6"


def _c(rid, shape, pick, wide, knob1=0, knob2=0, dtype="bf16", api="conv2d", in_place_res=False, seed=11, n=N_BAND, slots=SLOTS_BAND):
    """shape as tests/_exact_cases.py: (images of data, h, w, cin, cout, k, stride, act, residual, pre-add copy, upsample, fp32 y)."""
    assert shape[0] == len(slots)
    return dict(id=rid, shape=shape, pick=pick, wide=frozenset((wide,) if isinstance(wide, str) else wide), knob1=knob1, knob2=knob2, dtype=dtype, api=api,
                in_place_res=in_place_res, seed=seed, n=n, slots=slots)


_S1 = (3, H, W, 32, 128, 3, 1, L, True, True, False, False)         # 3x3 32 -> 128 + residual + pre-add copy
_S2 = (3, H, W, 32, 128, 3, 2, L, False, False, False, False)
_S2B = (3, 2 * H, 2 * W, 32, 128, 3, 2, L, False, False, False, False)
_HALO = (3, H, W, 64, 128, 3, 1, L, False, False, False, False)
_P256 = (3, H, W, 256, 128, 1, 1, L, False, False, False, False)
_P128 = (3, H, W, 128, 64, 1, 1, L, False, False, False, False)
_GEN = (3, H, W, 24, 40, 3, 1, L, False, False, False, False)
_IG256 = "igemm<256x128,4x2 waves,BK32,2 stages,16x16x32> grid "

# ---- table A: the operand that is READ lies in the band (x 26 x 190 x 198 x 2048) -----------------------------------------------------
TABLE_A = [
    _c("a_t20v2", _S1, "t20v2<400px x 128 couts, 4 waves> grid 2600", "x"),
    _c("a_t20s2", _S2, "t20s2<400px x 128 couts, 4 waves, parity planes> grid 650", "x"),
    _c("a_halo", _HALO, "halo<16x16,128 couts,CK64,1 halo buffers,16x16x32> grid 4056", "x", knob2=T20_NEVER),
    _c("a_igemm_generic", _GEN, "igemm<256x64,4x1 waves,BK32,2 stages,generic,32x32x16> grid 3821", "x"),
    _c("a_stream1x1p", _P256, "stream1x1p<128 couts,K 256,80 px> grid 512", "x"),
    _c("a_stream1x1_first_form", _P256, "stream1x1<128 couts,K 256> grid 512", "x", knob1=STREAM_FIRST_FORM, knob2=STREAM_ALWAYS),
    _c("a_igemm_fast_lds", _P256, _IG256 + "3821", "x", knob2=STREAM_NEVER),
    _c("a_stream1x1_c64", _P128, "stream1x1<64 couts,K 128> grid 512", "x"),
    _c("a_igemm_k1024", (3, H, W, 1024, 512, 1, 1, L, False, False, False, False), "igemm<256x256,4x4 waves,BK64,2 stages,16x16x32> grid 7642", "x"),
    # the FAST gather with the direct epilogue: an fp32 y (out_c_total a multiple of 4, the view inside it)
    _c("a_igemm_fast_f32", (3, H, W, 256, 128, 1, 1, L, True, False, False, True), "igemm<256x128,4x2 waves,BK32,2 stages,32x32x16> grid 3821", "x", knob2=STREAM_NEVER),
    # fp16 twins.  yolo_conv3x3_t20_f16_fwd has no pick function: with force it launches t20v2_f16 (stride 1) / t20s2_f16 (stride 2)
    # or fails, so the entry point and the stride name the kernel (pick None).
    _c("a_t20v2_f16", _S1, None, "x", dtype="f16", api="t20_f16", in_place_res=True, seed=12),
    _c("a_t20s2_f16", _S2, None, "x", dtype="f16", api="t20_f16", seed=12),
    _c("a_igemm_f16_fast", _P256, "igemm_f16<256x128,4x2 waves,BK32,2 stages,16x16x32> grid 3821", "x", dtype="f16", api="conv2d_f16", seed=12),
    _c("a_igemm_f16_generic", _GEN, "igemm_f16<256x64,4x1 waves,BK32,2 stages,generic,32x32x16> grid 3821", "x", dtype="f16", api="conv2d_f16", seed=12),
]
# the head instance k64x256_8w_decode (cin 256, nc 80) on the wide x: (data images, h, w, cin, k, nc)
HEAD_ROW = dict(id="a_head_decode", head=(3, H, W, 256, 1, 80), pick="igemm<64x256,1x8 waves,BK64,2 stages,32x32x16,decode> grid 15284",
                wide=frozenset(("x",)), n=N_BAND, slots=SLOTS_BAND, seed=13)

# ---- table B: the operands that are WRITTEN, or read in the epilogue, lie in the band (y 26 x 190 x 198 x 2048, narrow x) -------------
TABLE_B = [
    # rr, ra and ry are three descriptors of the t20v2 epilogue: the residual once in place from the output view, once from a wide buffer
    _c("b_t20v2_res_in_place", _S1, "t20v2<400px x 128 couts, 4 waves> grid 2600", ("y", "aux"), knob2=T20_ALWAYS, in_place_res=True),
    _c("b_t20v2_res_separate", _S1, "t20v2<400px x 128 couts, 4 waves> grid 2600", ("y", "res", "aux"), knob2=T20_ALWAYS),
    _c("b_t20s2", _S2B, "t20s2<400px x 128 couts, 4 waves, parity planes> grid 2600", "y", knob2=T20_ALWAYS),
    _c("b_stream1x1p", _P256, "stream1x1p<128 couts,K 256,80 px> grid 512", "y"),
    _c("b_stream1x1", _P128, "stream1x1<64 couts,K 128> grid 512", "y"),
    _c("b_halo", _HALO, "halo<16x16,128 couts,CK64,1 halo buffers,16x16x32> grid 4056", "y", knob2=T20_NEVER),
]

# ---- table D: beyond the limit (y 30 x 190 x 198 x 2048 = 0x113898000 bytes), the kernels the 32-bit forms give way to ----------------
_D = dict(n=N_BEYOND, slots=SLOTS_BEYOND)
TABLE_D = [
    _c("d_halo_for_t20v2", (3, H, W, 32, 128, 3, 1, L, False, False, False, False), "halo<16x16,128 couts,CK32,1 halo buffers> grid 4680", "y", **_D),
    _c("d_igemm_for_stream1x1p", _P256, _IG256 + "4409", "y", **_D),
    _c("d_igemm_for_t20s2", _S2B, "igemm<128x128,2x2 waves,BK32,3 stages,32x32x16> grid 8818", "y", **_D),
]
CONV_ROWS = TABLE_A + TABLE_B + TABLE_D

# ---- table C: fused kernels; x, y and the pre-add copy all 2048 wide ---------------------------------------------------------------------
# data: exact_chain(kind, two images) in slots 0 and 25 (D: 0 and 29); the middle slot repeats image 0 and must equal its output


def _f(rid, kind, shape, pick, knob3=0, seed=21, n=N_BAND, slots=SLOTS_BAND, wide=("x", "y", "aux")):
    return dict(id=rid, kind=kind, shape=shape, pick=pick, knob3=knob3, seed=seed, n=n, slots=slots, wide=frozenset(wide))


FUSED_ROWS = [
    _f("c_resunit64_t20", "unit", (2, H, W, 64, L), "resunit64_t20<400px x 64 couts, 4 waves> grid 2600"),
    _f("c_resunit64_persistent", "unit", (2, H, W, 64, L), "resunit64<256px x 64 couts, 8 waves, persistent> grid 256", knob3=RU_T20_NEVER),
    _f("c_resunit_t20w_c128", "unit", (2, H, W, 128, L), "resunit_t20w<C 128, 400px x 128 couts, 4 waves> grid 2600"),
    _f("c_resunit_c128", "unit", (2, H, W, 128, L), "resunit<C 128, 256px x 128 couts, 8 waves> grid 4056", knob3=RU_T20_NEVER),
    _f("c_resunit_t20w_c256", "unit", (2, H, W, 256, L), "resunit_t20w<C 256, 160px x 256 couts, 4 waves> grid 6240"),
    _f("c_resunit_c256", "unit", (2, H, W, 256, L), "resunit<C 256, 256px x 256 couts, 8 waves> grid 4056", knob3=RU_T20_NEVER),
    # the stem's float32 NCHW input cannot reach the band while its output stays below the limit: an output-side row
    _f("c_stem2", "stem", (2, 3, 2 * H, 2 * W, L), "stem2<leaky,8x16 outputs> grid ", wide=("y",)),
    # the MBConv tile form uses 64-bit pointers; one row, because the planner hands it the same buffers.  (n, h, w, cin, hidden, cout, stride)
    _f("c_mbconv_tile", "mbconv", (2, H, W, 32, 192, 32, 1), "mbconv<S 1,4x8,expand,512 threads> grid ", wide=("x", "y"), seed=301),
    _f("d_stem_one_role", "stem", (2, 3, 2 * H, 2 * W, L), "stem<leaky,CIN 3,16x16 outputs> grid ", wide=("y",), **_D),
]
ALL_ROWS = CONV_ROWS + [HEAD_ROW] + FUSED_ROWS


def view(c, wide, narrow_total):
    """(c_total, c_offset) of an operand with c channels."""
    c8 = (c + 7) // 8 * 8
    return (CT, CT - c8 - 8) if wide else (narrow_total, 8)


def conv_views(r):
    """{operand: (c_total, c_offset)} of a conv row."""
    cin, cout, use_res, use_aux = r["shape"][3], r["shape"][4], r["shape"][8], r["shape"][9]
    c8 = (cout + 7) // 8 * 8
    v = dict(x=view(cin, "x" in r["wide"], cin + 16), y=view(cout, "y" in r["wide"], c8 + 16))
    if use_res:
        v["res"] = v["y"] if r["in_place_res"] else view(cout, "res" in r["wide"], c8 + 16)
    if use_aux:
        v["aux"] = view(cout, "aux" in r["wide"], c8 + 8)
    return v


def conv_desc_of(r, n=None):
    """The descriptor a conv row launches (n: another image count, for the boundary tests)."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU6, DT_BF16, DT_F16, DT_F32
    _, h, w, cin, cout, k, stride, act, use_res, use_aux, up, f32 = r["shape"]
    v = conv_views(r)
    return K.conv_desc(n=n or r["n"], h=h, w=w, cin=cin, in_c_total=v["x"][0], in_c_offset=v["x"][1], cout=cout, out_c_total=v["y"][0],
                       out_c_offset=v["y"][1], ksize=k, stride=stride, act={L: ACT_LEAKY01, NO: ACT_NONE, R6: ACT_RELU6}[act],
                       kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128), upsample2x=int(up),
                       out_dtype=DT_F32 if f32 else {"bf16": DT_BF16, "f16": DT_F16}[r["dtype"]], res=v.get("res", (0, 0)), aux=v.get("aux", (0, 0)))


def conv_pick(r, d=None):
    """What the library would launch for the row under its knobs (None for the fp16 tile entry, which has no pick function)."""
    from pytorch_yolo_amd import kernels as K
    from test_conv_exact_cpu import tuning
    d = d or conv_desc_of(r)
    use_res, use_aux = r["shape"][8], r["shape"][9]
    if r["api"] == "t20_f16":
        return None
    with tuning(-1, r["knob1"], r["knob2"]):
        return (K.conv2d_f16_pick if r["api"] == "conv2d_f16" else K.conv2d_pick)(d, use_res, use_aux)


def head_desc_of(r, n=None):
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_NONE, DT_F32
    _, h, w, cin, k, nc = r["head"]
    cout = 3 * (nc + 5)
    xv = view(cin, True, 0)
    return K.conv_desc(n=n or r["n"], h=h, w=w, cin=cin, in_c_total=xv[0], in_c_offset=xv[1], cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                       ksize=k, stride=1, act=ACT_NONE, kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_F32)


def fused_desc_of(r, kpad=None, cout_pad=None, n=None, ct=CT):
    """The YoloConvDesc of a fused unit / stem row (the 3x3's, as tests/_exact_cases.py::unit_desc / stem_desc build it); ct: the
    width of the wide operands."""
    from pytorch_yolo_amd import kernels as K
    from _exact_cases import ACTS
    n = n or r["n"]
    if r["kind"] == "unit":
        _, h, w, c, act = r["shape"]
        off = ct - c - 8
        return K.conv_desc(n=n, h=h, w=w, cin=c // 2, in_c_total=ct, in_c_offset=off, cout=c, out_c_total=ct, out_c_offset=off, ksize=3, stride=1,
                           act=ACTS[act], kpad=kpad or K.roundup(9 * (c // 2), 64), cout_pad=cout_pad or K.roundup(c, 128), aux=(ct, off))
    assert r["kind"] == "stem"
    _, cin, h, w, act = r["shape"]
    return K.conv_desc(n=n, h=h, w=w, cin=32, in_c_total=32, in_c_offset=0, cout=64, out_c_total=ct, out_c_offset=ct - 64 - 8, ksize=3, stride=2,
                       act=ACTS[act], kpad=kpad or 320, cout_pad=cout_pad or 128)


def mbconv_args(r, n=None):
    _, h, w, cin, hidden, cout, stride = r["shape"]
    return dict(n=n or r["n"], h=h, w=w, cin=cin, hidden=hidden, cout=cout, stride=stride, in_view=view(cin, True, 0), out_view=view(cout, True, 0))


def fused_pick(r):
    from pytorch_yolo_amd import kernels as K
    from test_conv_exact_cpu import knob
    if r["kind"] == "mbconv":
        return K.mbconv_pick(**mbconv_args(r))
    with knob(3, r["knob3"]):
        return K.resunit_pick(fused_desc_of(r), True) if r["kind"] == "unit" else K.stem_pick(r["shape"][1], fused_desc_of(r))


def operand_bytes(r):
    """{operand: bytes} of a row's wide operands."""
    if "head" in r:
        return dict(x=r["n"] * r["head"][1] * r["head"][2] * CT * 2)
    if "kind" in r:
        h, w = (r["shape"][1], r["shape"][2]) if r["kind"] != "stem" else (r["shape"][2] // 2, r["shape"][3] // 2)
        return {o: r["n"] * h * w * CT * 2 for o in r["wide"]}
    _, h, w, _, _, k, stride = r["shape"][:7]
    ho, wo = (h + 2 * ((k - 1) // 2) - k) // stride + 1, (w + 2 * ((k - 1) // 2) - k) // stride + 1
    # (a wide fp32 y would be twice as large: no row has one)
    return {o: r["n"] * (h * w if o == "x" else ho * wo) * CT * 2 for o in r["wide"]}


# ---- completeness: which source addresses which activation operand with a 32-bit offset, and the rows that run it there ------------------
# (source file, operand) -> rows.  tests/test_large_operands_cpu.py derives the keys from csrc/ by text search - every
# __builtin_amdgcn_make_buffer_rsrc on a.x / a.y / a.res / a.aux, every file that names kOobOffset - so a new family cannot join
# silently; a row must have the operand wide and pick one of the file's kernels (KERNELS_OF).
KERNELS_OF = {
    "conv_igemm.hip": ("igemm<", "igemm_f16<"), "conv3x3_halo.hip": ("halo<",), "conv3x3_t20.h": ("t20v2<", "t20s2<"),
    "conv3x3_t20_f16.hip": (None,), "conv1x1_stream.hip": ("stream1x1<", "stream1x1p<"), "conv_resunit.hip": ("resunit<", "resunit64<"),
    "conv_resunit_t20.hip": ("resunit64_t20<", "resunit_t20w<"), "conv_stem.hip": ("stem2<",),
}
COVERAGE = {
    ("conv_igemm.hip", "x"): ["a_igemm_generic", "a_igemm_fast_lds", "a_igemm_k1024", "a_igemm_fast_f32", "a_igemm_f16_fast", "a_igemm_f16_generic", "a_head_decode"],
    ("conv3x3_halo.hip", "x"): ["a_halo"],
    ("conv3x3_t20.h", "x"): ["a_t20v2", "a_t20s2"],
    ("conv3x3_t20.h", "y"): ["b_t20v2_res_in_place", "b_t20v2_res_separate", "b_t20s2"],
    ("conv3x3_t20.h", "res"): ["b_t20v2_res_separate"],
    ("conv3x3_t20.h", "aux"): ["b_t20v2_res_in_place", "b_t20v2_res_separate"],
    ("conv3x3_t20_f16.hip", "x"): ["a_t20v2_f16", "a_t20s2_f16"],
    ("conv1x1_stream.hip", "x"): ["a_stream1x1p", "a_stream1x1_first_form", "a_stream1x1_c64"],
    ("conv1x1_stream.hip", "y"): ["b_stream1x1p", "b_stream1x1"],
    ("conv_resunit.hip", "x"): ["c_resunit64_persistent", "c_resunit_c128", "c_resunit_c256"],
    # the fused units read their residual from the x view: rr is a descriptor over x
    ("conv_resunit_t20.hip", "x"): ["c_resunit64_t20", "c_resunit_t20w_c128", "c_resunit_t20w_c256"],
    ("conv_resunit_t20.hip", "y"): ["c_resunit64_t20", "c_resunit_t20w_c128", "c_resunit_t20w_c256"],
    ("conv_resunit_t20.hip", "res"): ["c_resunit64_t20", "c_resunit_t20w_c128", "c_resunit_t20w_c256"],
    ("conv_resunit_t20.hip", "aux"): ["c_resunit64_t20", "c_resunit_t20w_c128", "c_resunit_t20w_c256"],
    ("conv_stem.hip", "y"): ["c_stem2"],
}
# addressed with 32-bit offsets, and no band row, with the reason
NO_BAND_ROW = {
    ("conv_stem.hip", "x"): "the float32 NCHW batch: at 2 GiB of input the output is past the limit (test_the_stem_input_cannot_reach_the_band)",
    ("conv_mbwide.hip", "x"): "the wide MBConv form refuses tensors from 2^31 bytes on (test_wide_mbconv_flips_at_2_gib)",
    ("conv_common.h", None): "defines kOobOffset; no kernel of its own",
}


def addressed_by_text_search():
    """{(file, operand)} from the sources: a buffer descriptor over an activation operand, or (operand None) a file that names
    kOobOffset without building one."""
    out = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        ops = set(re.findall(r"make_buffer_rsrc\(\s*(?:\(void\*\))?\s*a\.(x|y|res|aux)\b", src))
        out |= {(name, o) for o in ops}
        if "kOobOffset" in src and not ops:
            out.add((name, None))
    return out
