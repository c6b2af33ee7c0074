"""Case tables of the bit-exact conv tests (tests/test_conv_exact_cpu.py checks the picks without a GPU, tests/test_conv_exact_gpu.py
launches them): one recipe per instance of the bf16 gather kernel, and the shapes of the other kernel families behind yolo_conv2d_fwd.

A recipe is a layer shape, the tuning words that make choose_igemm (csrc/conv_igemm.hip) hand that layer to the instance, and the
output view: "v8" puts every view at an 8-channel offset inside a wider buffer (the LDS-staged epilogue can address it), "v4" puts the
output at a 4-channel offset (only the direct epilogue can).  Rules every forced shape keeps, so that no kernel reads outside what the
host checks describe: cin % 64 == 0 and cout > 64 wherever knob 0 is >= 0, cout a multiple of 256 for the 256-cout-wide tiles and of
128 for the 128-wide ones under a forced variant; a ragged cout (255, 100, 40, 24, 16) appears only where the shipped rule itself
hands it to the instance.  Every shape has a partial last pixel tile and at least two K steps."""
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
