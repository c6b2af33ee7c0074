"""Case tables of the bit-exact conv tests (tests/test_conv_exact_cpu.py checks the picks without a GPU, tests/test_conv_exact_gpu.py
launches them): one recipe per instance of the bf16 gather kernel, and the shapes of the other kernel families behind yolo_conv2d_fwd.

A recipe is a layer shape, the tuning words that make choose_igemm (csrc/conv_igemm.hip) hand that layer to the instance, and the
output view: "v8" puts every view at an 8-channel offset inside a wider buffer (the LDS-staged epilogue can address it), "v4" puts the
output at a 4-channel offset (only the direct epilogue can).  Rules every forced shape keeps, so that no kernel reads outside what the
host checks describe: cin % 64 == 0 and cout > 64 wherever knob 0 is >= 0, cout a multiple of 256 for the 256-cout-wide tiles and of
128 for the 128-wide ones under a forced variant; a ragged cout (255, 100, 40, 24, 16) appears only where the shipped rule itself
hands it to the instance.  Every shape has a partial last pixel tile and at least two K steps.

The second half holds the chained cases of the kernels that fuse several layers into one launch (tests/test_fused_exact_cpu.py runs
their references' guards and sensitivity checks, tests/test_fused_exact_gpu.py launches them).  Forced-shape rules there:
  * fused residual units: every map passes yolo_resunit_supported (>= 80x80 pixels, 16x16 tiles covering >= 85 %).  The form bits of
    knob 3 only choose AMONG kernels that compute any supported unit: kRuT20Always drops the tile-count and cover conditions of
    choose_resunit (csrc/conv_resunit.hip; a speed rule), kRuT20Never / kRuGeneric64 fall back to the generic 16x16-tile kernel.  No
    bit lifts a host check.
  * inverted residuals: knob 4 bit kMbStripForm ASKS for the row-strip form; choose_mbconv (csrc/conv_mbconv.hip) gives a block the
    strip form cannot hold to the tile form.  At stride 1 the strip form holds at most 128 padded hidden channels, at stride 2 its LDS
    rings end at 128 as well - so the 144-hidden blocks of test_fused_inverted_residual never reach it, and the strip row "hidden not
    a multiple of 32" is a block of its own (24-80-24).  The wide form's tiling follows from the shape (choose_mbwide): stride 2 ->
    7x7; stride 1 -> 13x13 when cin <= 96, cout <= 128 and there are >= 192 tiles of 13x13, else 7x7.
  * the stem takes stem2_kernel for 3 input channels and stem_kernel otherwise; conv + pool has one kernel per (cin, cout) pair.
No case rests on these sentences: yolo_resunit_pick / yolo_mbconv_pick / yolo_stem_pick name the kernel, tile and grid a case takes under
its knob, and both test files compare that with the row (*_pick_wanted below), the GPU one right before each launch."""
import os
import re

# kCd* bits of csrc/tuning.h (knob 1)
NO_LDS_EPI, NO_LOADERS, EIGHT_WAVES_256, MFMA32, FOUR_WAVES, LOADERS_2ST, TWO_STAGES_64 = 16, 256, 512, 2048, 8192, 16384, 4194304
STREAM_FIRST_FORM = 33554432
# kFam* bits (knob 2)
T20_ALWAYS, T20_NEVER, STREAM_ALWAYS = 16, 64, 2048

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch_yolo_amd", "csrc")


def parse_instances(macro):
    """{name: pick string} of an X-macro instance table in csrc/conv_igemm.hip (YOLO_IGEMM_INSTANCES, YOLO_IGEMM_F16_INSTANCES):
    X(id, BM, BN, WAVES_M, WAVES_N, BK, NS, FAST, LDS_EPI, MFMA16, DECODE, NP, SPLITK) -> what launch_cfg prints for it."""
    with open(os.path.join(CSRC, "conv_igemm.hip")) as f:
        src = f.read()
    body = src.split("#define %s(X)" % macro)[1].split("\n\n")[0]
    out = {}
    for m in re.finditer(r"\bX\((\w+),([^)]*)\)", body):
        bm, bn, wm, wn, bk, ns, fast, lds, m16, dec, np_, sk = [a.strip() for a in m.group(2).split(",")]
        assert m.group(1) not in out
        out[m.group(1)] = "<%sx%s,%sx%s waves%s,BK%s,%s stages%s%s%s%s>" % (
            bm, bn, wm, wn, "+4 loaders" if np_ != "0" else "", bk, ns, "" if fast == "true" else ",generic",
            ",16x16x32" if m16 == "true" else ",32x32x16", ",decode" if dec == "true" else "", ",splitK" if sk == "true" else "")
    return out


def _r(pick, shape, knob0=-1, knob1=0, view="v8"):
    return dict(pick=pick, shape=shape, knob0=knob0, knob1=knob1, view=view)


# instance -> pick string of yolo_conv2d_pick, and the recipe.  shape: n, h, w, cin, cout, k, stride, act, residual, aux, upsample, f32
BF16_INSTANCES = {
    # -- the three head instances: picked by the shapes of test_fused_head_decode (exp is not exact: their numerics stay there)
    "k64x256_8w_decode": dict(pick="<64x256,1x8 waves,BK64,2 stages,32x32x16,decode>", head=(2, 20, 20, 256, 1, 80)),
    "k64x256_bk32_decode": dict(pick="<64x256,1x4 waves,BK32,2 stages,32x32x16,decode>", head=(2, 14, 14, 96, 1, 80)),
    "k64x256_bk32_generic_decode": dict(pick="<64x256,1x4 waves,BK32,2 stages,generic,32x32x16,decode>", head=(2, 8, 8, 72, 1, 3)),
    # -- the shipped rules, no knob
    "k256x32_m32": _r("<256x32,4x1 waves,BK32,2 stages,32x32x16>", (2, 13, 13, 32, 32, 3, 1, "leaky", True, True, False, False)),
    "k256x32_m32_direct": _r("<256x32,4x1 waves,BK32,2 stages,32x32x16>", (2, 7, 9, 96, 24, 1, 1, "none", True, False, False, False)),
    "k256x32_m32_generic": _r("<256x32,4x1 waves,BK32,2 stages,generic,32x32x16>", (2, 15, 17, 8, 32, 3, 1, "leaky", False, False, False, False)),
    "k256x32_m32_generic_direct": _r("<256x32,4x1 waves,BK32,2 stages,generic,32x32x16>", (1, 21, 19, 16, 16, 3, 1, "relu6", False, False, False, False)),
    "k256x64_m32": _r("<256x64,4x1 waves,BK32,2 stages,32x32x16>", (1, 33, 29, 32, 64, 3, 2, "leaky", False, True, False, False)),
    "k256x64_m32_direct": _r("<256x64,4x1 waves,BK32,2 stages,32x32x16>", (2, 12, 10, 40, 40, 1, 1, "none", True, True, False, False)),
    "k256x64_m32_generic": _r("<256x64,4x1 waves,BK32,2 stages,generic,32x32x16>", (1, 20, 20, 16, 64, 3, 1, "leaky", True, False, False, False)),
    "k256x64_m32_generic_direct": _r("<256x64,4x1 waves,BK32,2 stages,generic,32x32x16>", (1, 20, 20, 24, 40, 3, 2, "leaky", False, False, True, False)),
    "k128x128_bk32_3st_m32": _r("<128x128,2x2 waves,BK32,3 stages,32x32x16>", (1, 20, 20, 96, 128, 3, 1, "leaky", True, True, False, False)),
    "k128x128_bk32_3st_m32_direct": _r("<128x128,2x2 waves,BK32,3 stages,32x32x16>", (2, 12, 10, 40, 255, 1, 1, "none", False, False, False, True)),
    "k128x128_bk32_3st_m32_generic": _r("<128x128,2x2 waves,BK32,3 stages,generic,32x32x16>", (1, 20, 20, 24, 128, 3, 1, "relu6", False, False, True, False)),
    "k128x128_bk32_3st_m32_generic_direct": _r("<128x128,2x2 waves,BK32,3 stages,generic,32x32x16>", (1, 20, 20, 40, 100, 3, 1, "leaky", True, True, False, False)),
    "k64x64_4st": _r("<64x64,2x2 waves,BK64,4 stages,16x16x32>", (2, 10, 10, 128, 64, 1, 1, "leaky", False, False, True, False)),
    "k128x128_8w": _r("<128x128,2x4 waves,BK64,2 stages,16x16x32>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False)),
    "k128x128_8w_3st": _r("<128x128,2x4 waves,BK64,3 stages,16x16x32>", (7, 21, 21, 256, 512, 1, 1, "leaky", True, False, False, False)),
    "k64x64": _r("<64x64,2x2 waves,BK64,2 stages,16x16x32>", (1, 9, 9, 1024, 512, 1, 1, "leaky", False, True, False, False)),
    "k128x256_16w_3st": _r("<128x256,2x8 waves,BK64,3 stages,16x16x32>", (8, 31, 33, 128, 512, 1, 1, "leaky", False, True, False, False)),
    "k128x256_loaders_3st": _r("<128x256,2x4 waves+4 loaders,BK64,3 stages,16x16x32>", (1, 26, 26, 384, 256, 3, 1, "leaky", False, False, False, False)),
    # -- knob 1 bits on the shipped rules
    "k128x128": _r("<128x128,2x2 waves,BK64,2 stages,16x16x32>", (3, 13, 11, 64, 128, 3, 2, "none", False, True, False, False), knob1=FOUR_WAVES),
    "k128x256_loaders": _r("<128x256,2x4 waves+4 loaders,BK64,2 stages,16x16x32>", (2, 13, 13, 64, 256, 3, 1, "leaky", True, False, False, False), knob1=LOADERS_2ST),
    "k128x256_8w": _r("<128x256,2x4 waves,BK64,2 stages,16x16x32>", (2, 27, 25, 64, 256, 3, 2, "leaky", False, True, False, False), knob1=NO_LOADERS),
    # -- knob 0: a tile configuration by number
    "k256x128_8w": _r("<256x128,4x2 waves,BK64,2 stages,16x16x32>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False), knob0=3),
    "k256x128_8w_bk32": _r("<256x128,4x2 waves,BK32,2 stages,16x16x32>", (3, 13, 13, 128, 128, 1, 1, "none", True, False, False, False), knob0=9),
    "k256x256_16w": _r("<256x256,4x4 waves,BK64,2 stages,16x16x32>", (2, 13, 13, 64, 256, 3, 1, "leaky", False, True, False, False), knob0=5),
    "k256x256_8w": _r("<256x256,4x2 waves,BK64,2 stages,16x16x32>", (2, 13, 13, 64, 512, 3, 1, "leaky", True, False, False, False), knob0=5, knob1=EIGHT_WAVES_256),
    # -- the 32x32x16 tiles: kCdMfma32x32 with the LDS-staged epilogue, ...
    "k128x128_m32": _r("<128x128,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False), knob0=0, knob1=MFMA32),
    "k256x128_8w_m32": _r("<256x128,4x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 128, 128, 1, 1, "leaky", False, False, True, False), knob0=3, knob1=MFMA32),
    "k128x128_bk32_m32": _r("<128x128,2x2 waves,BK32,2 stages,32x32x16>", (2, 13, 13, 64, 256, 3, 2, "leaky", False, True, False, False), knob0=7, knob1=MFMA32),
    "k128x64_m32": _r("<128x64,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "none", True, False, False, False), knob0=8, knob1=MFMA32),
    "k64x128_m32": _r("<64x128,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False), knob0=10, knob1=MFMA32),
    "k64x64_m32": _r("<64x64,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 128, 128, 1, 1, "leaky", True, False, False, False), knob0=11, knob1=MFMA32),
    "k256x128_8w_bk32_m32": _r("<256x128,4x2 waves,BK32,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", False, True, False, False), knob0=9, knob1=MFMA32),
    "k256x256_8w_m32": _r("<256x256,4x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 256, 3, 1, "leaky", True, True, False, False), knob0=5, knob1=MFMA32),
    # -- ... and their direct twins: an fp32 output view, or a bf16 one at a 4-channel offset
    "k128x128_m32_direct": _r("<128x128,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False), knob0=-1, view="v4"),
    "k256x128_8w_m32_direct": _r("<256x128,4x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, False, False, True), knob0=3),
    "k128x128_bk32_m32_direct": _r("<128x128,2x2 waves,BK32,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "none", False, True, False, False), knob0=7, view="v4"),
    "k128x64_m32_direct": _r("<128x64,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 2, "leaky", True, False, False, False), knob0=8, view="v4"),
    "k64x128_m32_direct": _r("<64x128,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 128, 128, 1, 1, "leaky", False, False, True, False), knob0=10, view="v4"),
    "k64x64_m32_direct": _r("<64x64,2x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", False, False, False, True), knob0=11),
    "k256x128_8w_bk32_m32_direct": _r("<256x128,4x2 waves,BK32,2 stages,32x32x16>", (2, 13, 13, 64, 128, 3, 1, "leaky", True, True, False, False), knob0=9, view="v4"),
    "k256x256_8w_m32_direct": _r("<256x256,4x2 waves,BK64,2 stages,32x32x16>", (2, 13, 13, 64, 256, 3, 1, "leaky", True, False, False, False), knob0=5, knob1=NO_LDS_EPI),
    # -- split-K (yolo_conv2d_splitk_fwd): the 13x13 1280 -> 64 shape of test_split_k_conv, and the smallest 3x3 layer of the one-round
    # 128x256 grid whose plan still splits (12 K steps = 2 x 6: cin 128 is the shortest K the planner splits)
    "k64x64_4st_splitk": _r("<64x64,2x2 waves,BK64,4 stages,16x16x32,splitK>", (3, 13, 13, 1280, 64, 3, 1, "leaky", False, True, False, False)),
    "k128x256_loaders_3st_splitk": _r("<128x256,2x4 waves+4 loaders,BK64,3 stages,16x16x32,splitK>", (1, 3, 3, 128, 256, 3, 1, "leaky", True, False, False, False)),
}
# what the two split-K shapes pick when they are launched without a split
SPLITK_PLAIN = {"k64x64_4st_splitk": "k64x64_4st", "k128x256_loaders_3st_splitk": "k128x256_loaders_3st"}
# a second recipe for an instance that two rules reach
BF16_EXTRA = {
    "k64x64/two_stages": ("k64x64", _r(None, (2, 9, 11, 64, 64, 3, 1, "leaky", True, False, False, False), knob1=TWO_STAGES_64)),
    "k128x128_m32_direct/f32": ("k128x128_m32_direct", _r(None, (2, 13, 13, 64, 128, 3, 1, "leaky", True, False, False, True))),
}

# ---- the other kernel families behind yolo_conv2d_fwd: (family prefix of the pick, knob 1, knob 2, shape) ---------------------------
FAMILY_CASES = [
    ("t20v2", 0, T20_ALWAYS, (1, 40, 40, 64, 128, 3, 1, "leaky", False, False, False, False)),
    ("t20v2", 0, T20_ALWAYS, (3, 37, 41, 96, 384, 3, 1, "leaky", True, True, False, False)),
    ("t20s2", 0, T20_ALWAYS, (2, 41, 40, 32, 128, 3, 2, "leaky", False, False, False, False)),
    ("t20s2", 0, T20_ALWAYS, (3, 75, 83, 96, 256, 3, 2, "leaky", False, True, False, False)),
    ("halo", 0, 0, (1, 80, 96, 64, 128, 3, 1, "leaky", True, True, False, False)),
    ("halo", 0, 0, (2, 94, 100, 96, 64, 3, 1, "none", True, False, False, False)),
    # the list of test_conv1x1_stream_kernel without its swish case (x * sigmoid(x) is not exact)
    ("stream1x1", 0, STREAM_ALWAYS, (2, 80, 80, 256, 128, 1, 1, "leaky", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (1, 160, 160, 128, 64, 1, 1, "leaky", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (3, 37, 41, 128, 128, 1, 1, "none", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (1, 20, 20, 256, 64, 1, 1, "relu6", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (9, 80, 80, 256, 128, 1, 1, "leaky", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (2, 83, 79, 384, 128, 1, 1, "leaky", False, False, False, False)),
    ("stream1x1", 0, STREAM_ALWAYS, (1, 9, 7, 128, 128, 1, 1, "relu6", False, False, False, False)),
    ("stream1x1", STREAM_FIRST_FORM, STREAM_ALWAYS, (3, 37, 41, 128, 128, 1, 1, "none", False, False, False, False)),
    ("stream1x1", STREAM_FIRST_FORM, STREAM_ALWAYS, (2, 80, 80, 256, 128, 1, 1, "leaky", False, False, False, False)),
]


def case_id(shape):
    return "n%d_%dx%d_c%d-%d_k%d_s%d_%s_r%d_a%d_u%d_f%d" % tuple(int(v) if not isinstance(v, str) else v for v in shape)


# ---- chained cases of the fused multi-conv kernels ------------------------------------------------------------------------------------
RU_GENERIC64, RU_T20_ALWAYS, RU_T20_NEVER = 32, 64, 128       # kRu* form bits (knob 3)
MB_STRIP = 128                                                 # kMbStripForm (knob 4)


def _u(kernel, c, knob3, n, h, w, act, tile, seed):
    return dict(kernel=kernel, c=c, knob3=knob3, shape=(n, h, w, c, act), tile=tile, seed=seed)


# 94x100 is the smallest map yolo_resunit_supported accepts with partial 16x16 tiles in both directions (6x7 tiles, last row of 14,
# last column of 4) and a partial last row of 20x20 / 8x20 tiles (14 / 6 rows); its width is five whole tiles of 20, so the
# 20-pixel-wide kernels get 94x101 as well (a last tile column of ONE pixel).  n = 7 gives the persistent kernel 294 tiles, more than
# the chip has CUs: its loop and prefetch run.  Every case runs with and without the pre-add copy.
# Achieved shares of the references (LeakyReLU, C = 64 / 128 / 256): 21-32 % negative before the first activation, 39-51 % before the
# second; 50-56 % of the intermediate beyond 256, 13-18 % of it needs rounding (13-16 % ties); 91-96 % of the outputs and of the
# pre-add copy need rounding, 3.1-5.8 % are ties.  ReLU6: intermediate 25-28 % at 0, 17-21 % at 6, 26-39 % need rounding; second
# activation 17-24 % at 0, 27-29 % at 6; 36-40 % of the outputs need rounding, 8.5-10 % are ties.
UNIT_CASES = [
    _u("resunit64_persistent", 64, 0, 7, 94, 100, "leaky", (16, 16), 101),
    _u("resunit_generic16_c64", 64, RU_GENERIC64, 2, 94, 100, "leaky", (16, 16), 102),
    _u("resunit64_t20", 64, RU_T20_ALWAYS, 2, 94, 100, "leaky", (20, 20), 102),
    _u("resunit_generic16_c128", 128, RU_T20_NEVER, 2, 94, 100, "leaky", (16, 16), 103),
    _u("resunit_t20w_c128", 128, RU_T20_ALWAYS, 2, 94, 100, "leaky", (20, 20), 103),
    _u("resunit_generic16_c256", 256, RU_T20_NEVER, 2, 94, 100, "leaky", (16, 16), 104),
    _u("resunit_t20w_c256", 256, RU_T20_ALWAYS, 2, 94, 100, "leaky", (8, 20), 104),
    _u("resunit64_t20_w101", 64, RU_T20_ALWAYS, 2, 94, 101, "leaky", (20, 20), 105),
    _u("resunit_t20w_c128_w101", 128, RU_T20_ALWAYS, 2, 94, 101, "leaky", (20, 20), 106),
    _u("resunit_t20w_c256_w101", 256, RU_T20_ALWAYS, 2, 94, 101, "leaky", (8, 20), 107),
    _u("resunit_generic16_c128_relu6", 128, RU_T20_NEVER, 2, 94, 100, "relu6", (16, 16), 108),
    _u("resunit64_t20_relu6", 64, RU_T20_ALWAYS, 2, 94, 100, "relu6", (20, 20), 109),
]

# (kernel, (n, cin, h, w, act), output tile, seed).  stem2_kernel walks tiles of 8x16 outputs, stem_kernel of 16x16.  Achieved shares
# (LeakyReLU): 23-28 % / 44-54 % negative before the two activations, 11-16 % of the intermediate need rounding (11-15 % ties),
# 91-92 % of the outputs do, 5-9 % are ties (the 2x2 image has 64 outputs: its seed is one whose reference clears the 2 % of ties).
# ReLU6: intermediate 25 % at 0, 17 % at 6, 38 % need rounding; output 22 % / 19 % at the clamps, 42 % need rounding, 14 % ties.
STEM_CASES = [
    ("stem2", (1, 3, 2, 2, "leaky"), (8, 16), 203),
    ("stem2", (1, 3, 33, 17, "leaky"), (8, 16), 202),
    ("stem2", (2, 3, 70, 106, "leaky"), (8, 16), 203),
    ("stem_one_role", (2, 1, 37, 50, "leaky"), (16, 16), 204),
    ("stem2", (1, 3, 33, 17, "relu6"), (8, 16), 205),
]

# (form, (n, h, w, cin, hidden, cout, stride), output tile).  Every block of test_fused_inverted_residual with at most about 100 000
# input pixels x channels per image - all but 4x104x104, 12x52x52, 3x104x104, 2x61x83 and 2x57x70, which are larger, and 70x26x26 and
# 20x28x28, whose 70 and 20 images only repeat a tiling the table has; 13x50x45 is larger too and stays, no smaller block selects the
# 13x13 tiling -, plus 24-80-24 (see the header) and 5x57x61 24-144-24: 320 tiles of 8x8 on 256 workgroups (the tile form's
# persistent loop).  Achieved shares: expand output 25-28 % at 0, 16-22 % at 6, 33-45 % need rounding (10-14 % ties);
# depthwise output 47-61 % at 0, 26-41 % at 6, 6-11 % need rounding (without expand conv: 25 % / 19-20 % at the clamps, 30-37 % need
# rounding); block output 88-96 % need rounding, 2.7-8.4 % ties.
MBCONV_CASES = [
    ("tile", (2, 26, 30, 32, 32, 16, 1), (8, 8)),        # no expand conv
    ("tile", (2, 40, 36, 16, 96, 24, 2), (4, 8)),        # stride 2, cout not a multiple of 16
    ("tile", (1, 23, 19, 24, 144, 24, 1), (8, 8)),       # residual, hidden not a multiple of 32
    ("tile", (3, 33, 41, 24, 144, 32, 2), (4, 8)),
    ("tile", (2, 16, 24, 32, 192, 32, 1), (4, 8)),       # residual, the half tile of the 192-hidden blocks
    ("tile", (1, 52, 52, 32, 192, 64, 2), (4, 8)),
    ("tile", (3, 30, 26, 32, 32, 32, 1), (8, 8)),        # residual without expand conv
    ("tile", (2, 24, 40, 16, 64, 16, 1), (8, 8)),
    ("tile", (5, 52, 52, 32, 192, 32, 1), (4, 8)),       # residual, 455 half tiles
    ("tile", (5, 57, 61, 24, 144, 24, 1), (8, 8)),       # more tiles than workgroups
    ("strip", (2, 26, 30, 32, 32, 16, 1), (8, 26)),      # no expand conv, two column segments
    ("strip", (2, 40, 36, 16, 96, 24, 2), (8, 26)),      # stride 2, cout not a multiple of 16
    ("strip", (3, 30, 26, 32, 32, 32, 1), (8, 26)),      # residual without expand conv
    ("strip", (2, 24, 40, 16, 64, 16, 1), (8, 26)),      # residual, two column segments
    ("strip", (2, 21, 31, 24, 80, 24, 1), (8, 26)),      # residual, hidden not a multiple of 32, cout not a multiple of 16
    ("strip", (1, 52, 52, 32, 128, 64, 2), (8, 26)),     # the widest stride-2 block the strip form holds
    ("wide13", (13, 50, 45, 96, 192, 96, 1), (13, 13)),  # partial tiles at both edges, residual
    ("wide7", (2, 26, 26, 64, 128, 96, 1), (7, 7)),
    ("wide7", (3, 13, 13, 160, 320, 160, 1), (7, 7)),    # five K steps, residual
    ("wide7", (2, 13, 13, 160, 192, 320, 1), (7, 7)),    # 20 cout tiles: the only block with cout > 160
    ("wide7", (2, 26, 26, 96, 192, 160, 2), (7, 7)),     # stride 2
    ("wide7", (1, 27, 23, 64, 192, 24, 2), (7, 7)),      # stride 2, odd sizes, cout not a multiple of 16
]
MBCONV_SEED = 301


# ---- what a chained case must launch: its descriptor, and the pick string (yolo_resunit_pick / _stem_pick / _mbconv_pick) up to the grid
ACTS = {"leaky": 1, "relu6": 2}                                # YOLO_ACT_LEAKY01, YOLO_ACT_RELU6


def unit_desc(u, use_aux=False, kpad=None, cout_pad=None):
    from pytorch_yolo_amd import kernels as K
    n, h, w, c, act = u["shape"]
    return K.conv_desc(n=n, h=h, w=w, cin=c // 2, in_c_total=c + 16, in_c_offset=8, cout=c, out_c_total=c + 16, out_c_offset=8, ksize=3, stride=1,
                       act=ACTS[act], kpad=kpad or (9 * (c // 2) + 63) // 64 * 64, cout_pad=cout_pad or (c + 127) // 128 * 128,
                       aux=(c + 16, 8) if use_aux else (0, 0))


def unit_pick_wanted(u):
    c, px = u["c"], u["tile"][0] * u["tile"][1]
    return {"resunit64_persistent": "resunit64<%dpx x 64 couts, 8 waves, persistent> grid " % px, "resunit_generic16": "resunit<C %d, %dpx x %d couts, 8 waves> grid " % (c, px, c),
            "resunit64_t20": "resunit64_t20<%dpx x 64 couts, 4 waves> grid " % px, "resunit_t20w": "resunit_t20w<C %d, %dpx x %d couts, 4 waves> grid " % (c, px, c)}[
        u["kernel"].split("_c")[0].split("_w101")[0].split("_relu6")[0]]


def stem_desc(shape, kpad=320, cout_pad=128):
    from pytorch_yolo_amd import kernels as K
    n, cin, h, w, act = shape
    return K.conv_desc(n=n, h=h, w=w, cin=32, in_c_total=32, in_c_offset=0, cout=64, out_c_total=80, out_c_offset=8, ksize=3, stride=2,
                       act=ACTS[act], kpad=kpad, cout_pad=cout_pad)


def stem_pick_wanted(kernel, shape, tile):
    return ("stem2<%s,%dx%d outputs> grid " if kernel == "stem2" else "stem<%s,CIN 0,%dx%d outputs> grid ") % (("leaky" if shape[4] == "leaky" else "any act",) + tile)


def mbconv_pick(shape):
    from pytorch_yolo_amd import kernels as K
    n, h, w, cin, hidden, cout, stride = shape
    return K.mbconv_pick(n=n, h=h, w=w, cin=cin, hidden=hidden, cout=cout, stride=stride, in_view=(cin + 16, 8), out_view=(cout + 8, 4))


def mbconv_pick_wanted(form, shape, tile):
    expand = "expand" if shape[4] != shape[3] else "no expand"
    return {"tile": "mbconv<S %d,%dx%d," + expand + ",", "strip": "mbstrip<S %d," + expand + ",%d rows x %d> grid "}.get(form, "mbwide<S %d,%dx%d,") % ((shape[6],) + tile)


# conv3x3 + MaxPool2d(2, 2) (csrc/conv_small.hip): every (cin, cout) pair with the pool, at odd sizes - the pool takes the floor, the
# last odd row / column is computed and dropped -, and every pair without (each (cin, cout, pool) is a template instantiation of its
# own); n, h, w, cin, cout, pool
POOL_CASES = [(2, 26, 38, 16, 32, True), (1, 21, 19, 16, 64, True), (1, 21, 19, 32, 32, True), (2, 26, 38, 32, 64, True),
              (1, 21, 19, 16, 32, False), (2, 26, 38, 16, 64, False), (1, 21, 19, 32, 32, False), (1, 21, 19, 32, 64, False)]
POOL_SEED = 6


# ---- first-layer, depthwise and squeeze-excite kernels (tests/test_pointwise_exact_cpu.py / _gpu.py) ----------------------------------
# A seed stands beside every row whose reference has guards: the smallest one (from the table's base) whose reference passes them
# for every activation the row runs with.  On the maps of a few pixels (2x2, 1x1: 16 to 128 outputs) the shares are coarse, and a seed
# is what decides them; on the others the first seed passes.

# yolo_conv1_nchw_f32_fwd / yolo_conv1_pool_nchw_f32_fwd at stride 1 (conv3x3_halo.hip: 16x16 tiles, 3 per workgroup, every halo
# requested up front): 19x50 is 2 tile rows (the last of 3 rows) and 4 tile columns (a group of 3 and a group of 1, the last of 2
# columns), on every instantiation - cout {16, 32} x pool x cin_real 3 (the CINR = 3 template) / 1 and 8 (the generic one); a 2x2
# image; 21x35 for the pooled form (the floor drops the odd row and column).  ((n, cin, h, w, cout, stride, act, pool), seed)
# Achieved shares of the references: x 59-88 % needs rounding, 12-33 % ties (66-69 % / 21-25 % from 19x50 on); LeakyReLU 46-53 %
# negative pre-activations, 72-85 % of the outputs need rounding, 8-11 % ties; ReLU6 24-30 % at 0, 17-24 % at 6, 30-37 % need rounding,
# 10-13 % ties; no activation 64-82 % need rounding, 12-20 % ties.  Truncated x changes 12-59 % of the outputs, un-narrowed x 8-42 %.
_S1 = [(cout, pool, cin) for cout in (16, 32) for pool in (False, True) for cin in (3, 1, 8)]
FIRST_S1_CASES = [((2, cin, 19, 50, cout, 1, ("leaky", "relu6", "none")[(i + i // 3) % 3], pool), 400 + i) for i, (cout, pool, cin) in enumerate(_S1)]
FIRST_S1_CASES += [((2, 3, 2, 2, 32, 1, "leaky", False), 420), ((2, 1, 2, 2, 16, 1, "relu6", False), 421), ((2, 8, 2, 2, 16, 1, "leaky", True), 422),
                   ((2, 3, 21, 35, 16, 1, "leaky", True), 423), ((2, 8, 21, 35, 32, 1, "relu6", True), 424)]
# the stride-2 form (conv_small.hip: 16x16 OUTPUT tiles, 5 per workgroup, two halo buffers used alternately): wo = 82 is a full group
# of five tiles plus a group of one tile of 2 columns; 35x163 / 36x164 are the odd / even right and bottom edges
FIRST_S2_CASES = [((2, cin, h, w, 32, 2, act, False), 440 + i) for i, (cin, (h, w), act) in enumerate(
    (cin, hw, act) for cin in (3, 1) for hw in ((35, 163), (36, 164)) for act in ("relu6", "leaky"))]
FIRST_CASES = FIRST_S1_CASES + FIRST_S2_CASES


def first_id(shape):
    return "n%d_c%d_%dx%d_co%d_s%d_%s_pool%d" % tuple(int(v) if not isinstance(v, str) else v for v in shape)


# every activation whose result is determined bit for bit (swish = x / (1 + expf(-x)) is not: it stays with the tolerance tests)
DW_ACTS = ("none", "leaky", "relu6", "relu")

# yolo_dwconv3x3_fwd (pointwise.hip: strips of 8 output rows per thread, the rows slide through three register slots), each at
# strides 1 and 2: a one-pixel map; h = 9, a last strip of ONE row, on a one-column map; 17 rows (odd, last strip of one row at
# stride 1, ho = 9 at stride 2) with three channel groups; 16 rows (even, whole strips); 18 rows (even, ho = 9).  n = 2: the rows
# outside an image must read zero, never the neighbouring image's rows (NaN cannot sit there, the values decide).  ((n, c, h, w), seed)
DW3_CASES = [((1, 8, 1, 1), 500), ((2, 8, 9, 1), 601), ((2, 24, 17, 5), 502), ((2, 16, 16, 7), 803), ((2, 24, 18, 6), 504)]
DW3_ROWS = [(shape, seed, stride) for shape, seed in DW3_CASES for stride in (1, 2)]


def dw3_shape(nchw, stride, act):
    """The exact_dw_case shape of a DW3_CASES row."""
    return tuple(nchw) + (3, stride, act)


# yolo_dwconv_fwd and yolo_dwconv_f32_fwd (efficient.hip, dwconv_kernel<bf16_t> and <float>): k {3, 5} x stride {1, 2} on 6x8, 7x9 and 1x1 maps of two
# images, in TensorFlow-"same" geometry and with torch's pad k // 2 where that is another one (an even map at stride 2: leading pad
# k // 2 - 1 against k // 2); c = 8 and 24 (bf16) / 12 (float32).  (k, stride, h, w, geometry)
def _dw_geometries():
    from helpers import dw_geometry
    out = []
    for k in (3, 5):
        for stride in (1, 2):
            for h, w in ((6, 8), (7, 9), (1, 1)):
                out.append((k, stride, h, w, "same"))
                if dw_geometry(h, w, k, stride, "torch") != dw_geometry(h, w, k, stride, "same"):
                    out.append((k, stride, h, w, "torch"))
    return out


DW_SEED, DW_F32_SEED = 520, 560
# (k, stride, h, w, geometry, c) -> seed, where DW_SEED itself does not pass the guards for every activation
DW_SEEDS = {r: 620 for r in ((3, 1, 7, 9, "same", 8), (3, 1, 1, 1, "same", 8), (3, 2, 7, 9, "same", 8), (3, 2, 1, 1, "same", 8),
                             (5, 1, 1, 1, "same", 8), (5, 1, 1, 1, "same", 24), (5, 2, 1, 1, "same", 8), (5, 2, 1, 1, "same", 24))}


def dw_rows():
    """[(k, stride, h, w, geometry, c, seed)] of the bf16 table."""
    return [g + (c, DW_SEEDS.get(g + (c,), DW_SEED)) for g in _dw_geometries() for c in (8, 24)]


def dw_f32_rows():
    return [g + (12, DW_F32_SEED) for g in _dw_geometries()]


# yolo_se_fwd / yolo_se_f32_fwd, (n, h, w, c, sq): c / 8 (bf16) and c / 4 (float32) chunks of 1, 2, 4, 8, 16, 33 and 144 reach every
# channel-group width of the pooling pass (1..32) and several groups with a partial last one; 42x50 is cut into 8 pixel ranges, 23x23
# into 2 (a range keeps >= 256 pixels), the others are one range; 5x3 and 3x3 are smaller than one stripe of 256 / cgb pixels.
SE_CASES = [(1, 42, 50, 8, 1), (1, 23, 23, 16, 4), (2, 5, 3, 32, 48), (2, 9, 7, 64, 64), (3, 4, 4, 128, 4), (2, 7, 9, 264, 48), (1, 3, 3, 1152, 64)]
SE_F32_CASES = [(n, h, w, c // 2, sq) for n, h, w, c, sq in SE_CASES]
SE_SEED = 600
