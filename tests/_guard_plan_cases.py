"""Case table of the plan-level guard-band audit (tests/test_gpu_parity.py::test_small_launch_lists_stay_inside_their_buffers runs
the lists between poisoned margins on the GPU, tests/test_guard_bands_cpu.py::test_guarded_plan_cases_hold_every_launch_kind builds
them without one and pins the op kinds): the precision modes and model families the bench-shape audit does not reach.

Every case is batch 3 at an input of unequal sides, both multiples of 32: the one with the FEWEST PIXELS (ties: the less elongated)
at which the launch list holds every op kind the mode has for the family.  The op kinds of a list do not depend on the input size,
with three exceptions, all rules of the C library that want large maps:
  * OP_CONV_T20_F16 (fp16 mode, csrc/conv3x3_t20.h::t20_3x3_form): 3x3 convs with cin % 32 == 0 and cout % 128 == 0 - full-width
    models only - whose maps 20x20 tiles cover >= 90 % and whose tiles x cout / 128 fill half the chip (stride 1: >= 128 workgroups)
    or twice the chip (stride 2: >= 512).  With three images the stride-2 kernel first gets a layer - Darknet-53's 64 -> 128
    down-sampling conv - at 672 x 1472 (its output map 168 x 368: 3 x 9 x 19 = 513 tiles, covered 90.4 %); the stride-1 kernel has
    two layers there.  YOLOv3-tiny has no stride-2 conv: its one stride-1 layer (64 -> 128 on the 1/8 map) needs 576 x 1760
    (3 x 4 x 11 = 132 tiles; 288 x 3520 has as many pixels and is more elongated).  A search over every pair of multiples of 32 with
    the rule's arithmetic found these sizes; the CPU test pins what they yield.
  * OP_RESUNIT / OP_STEM (bf16 YOLOv3): full width (the stem is 3 -> 32 -> 64, the fused units have 64 / 128 / 256 channels) and a
    map of >= 80 x 80 pixels in front of the first unit: 160 x 192.
  * OP_CONV1_POOL (bf16 Lite): full width (16 | 32 output channels).
Every other case runs at 64 x 96; the encoder families have no width parameter.  `kinds` are names of pytorch_yolo_amd._lib; for
OP_CONV_T20_F16 the case also names the strides it must hold."""
import _cases as C

_SPP = dict(n_class=80, kernels_divider=1, anchors=C.SPP_ANCHORS)
_TINY = dict(n_class=80, kernels_divider=1, anchors=C.TINY_ANCHORS)
_F16 = ("OP_CONV_F16", "OP_HEAD_DECODE_F16")
_F32 = ("OP_CONV_F32",)

# name -> (family, constructor arguments, precision, environment, (bs, h, w), op kinds of the list, strides of its OP_CONV_T20_F16 ops)
PLAN_CASES = {
    "fp16_spp":          ("spp", _SPP, "fp16", {}, (3, 672, 1472), _F16 + ("OP_SPP", "OP_CONV_T20_F16"), (1, 2)),
    "fp16_spp_t20off":   ("spp", _SPP, "fp16", {"YOLO_FP16_T20": "0"}, (3, 672, 1472), _F16 + ("OP_SPP",), ()),
    "fp16_yolov3":       ("yolov3", _SPP, "fp16", {}, (3, 672, 1472), _F16 + ("OP_CONV_T20_F16",), (1, 2)),
    "fp16_yolov3_t20off": ("yolov3", _SPP, "fp16", {"YOLO_FP16_T20": "0"}, (3, 672, 1472), _F16, ()),
    "fp16_tiny":         ("tiny", _TINY, "fp16", {}, (3, 576, 1760), _F16 + ("OP_MAXPOOL_F16", "OP_CONV_T20_F16"), (1,)),
    "fp16_tiny_t20off":  ("tiny", _TINY, "fp16", {"YOLO_FP16_T20": "0"}, (3, 576, 1760), _F16 + ("OP_MAXPOOL_F16",), ()),
    "fp32_mobile":       ("mobile", dict(n_class=80), "fp32", {}, (3, 64, 96), _F32 + ("OP_DWCONV_F32",), ()),
    "fp32_shuffle":      ("shuffle", dict(n_class=80), "fp32", {}, (3, 64, 96), _F32 + ("OP_DWCONV_F32", "OP_SHUFFLE_F32", "OP_MAXPOOL_F32"), ()),
    "fp32_efficient":    ("efficient", dict(n_class=80), "fp32", {}, (3, 64, 96), _F32 + ("OP_DWCONV_F32", "OP_SE_F32"), ()),
    "fp32_squeeze":      ("squeeze", dict(n_class=80), "fp32", {}, (3, 64, 96), _F32 + ("OP_MAXPOOL_F32",), ()),
    "bf16_efficient":    ("efficient", dict(n_class=80), "bf16", {}, (3, 64, 96), ("OP_CONV", "OP_DWCONV", "OP_SE", "OP_HEAD_DECODE"), ()),
    "bf16_shuffle":      ("shuffle", dict(n_class=80), "bf16", {}, (3, 64, 96),
                          ("OP_CONV", "OP_CONV1_NCHW", "OP_DWCONV", "OP_SHUFFLE", "OP_MAXPOOL", "OP_HEAD_DECODE"), ()),
    "bf16_squeeze":      ("squeeze", dict(n_class=80), "bf16", {}, (3, 64, 96), ("OP_CONV", "OP_MAXPOOL", "OP_HEAD_DECODE"), ()),
    "bf16_yolov3":       ("yolov3", _SPP, "bf16", {}, (3, 160, 192), ("OP_CONV", "OP_STEM", "OP_RESUNIT", "OP_HEAD_DECODE"), ()),
    "bf16_lite":         ("lite", _SPP, "bf16", {}, (3, 64, 96), ("OP_CONV", "OP_CONV1_POOL", "OP_CONV_POOL", "OP_MAXPOOL", "OP_HEAD_DECODE"), ()),
}


def build_model(family, kw):
    import pytorch_yolo_amd as P
    cls = {"spp": P.YOLOv3SPP, "tiny": P.YOLOv3Tiny, "yolov3": P.YOLOv3, "lite": P.LiteYOLOv3, "mobile": P.YOLOv3TinyMobile,
           "shuffle": P.YOLOv3TinyShuffle, "efficient": P.YOLOv3TinyEfficient, "squeeze": P.YOLOv3TinySqueeze}[family]
    return cls(**kw).eval()


def plan_kinds(plan):
    """({names of the op kinds of the list}, {strides of its OP_CONV_T20_F16 ops})."""
    from pytorch_yolo_amd import _lib
    names = {getattr(_lib, k): k for k in dir(_lib) if k.startswith("OP_")}
    ops = [plan.op_array[i] for i in range(plan.n_ops)]
    return {names[o.kind] for o in ops}, {o.conv.stride for o in ops if o.kind == _lib.OP_CONV_T20_F16}
