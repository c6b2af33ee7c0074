"""Host-side tests of the fp16 forms of the 20x20-tile 3x3 kernels (csrc/conv3x3_t20.h, conv3x3_t20_f16.hip): the
rule entry point, the plans that hold YOLO_OP_CONV_T20_F16, and the device assembly of the new translation unit.  No GPU needed."""
import bisect
import ctypes
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import _cases as C
from pytorch_yolo_amd import LiteYOLOv3, YOLOv3, YOLOv3SPP, YOLOv3Tiny, _lib, engine
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import (ACT_LEAKY01, ACT_SWISH, DT_BF16, DT_F16, DT_F32, OP_CONV_F16, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16, OP_SPP,
                                   YoloConvDesc)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"spp": lambda: YOLOv3SPP(anchors=C.SPP_ANCHORS), "tiny": YOLOv3Tiny, "yolov3": lambda: YOLOv3(anchors=C.SPP_ANCHORS),
            "lite": lambda: LiteYOLOv3(anchors=C.SPP_ANCHORS)}


def _t20_kind():
    return _lib.OP_CONV_T20_F16


def _dry_plan(model, hw, bs=1, precision="fp16"):
    rec = engine.Recorder(bs, 3, hw, hw)
    model._trace(rec, rec.input)
    return engine.Plan(rec, torch.device("cpu"), model.n_class, hw, precision)


def _ops(plan):
    return [plan.op_array[i] for i in range(plan.n_ops)]


def _desc(n, h, w, cin, cout, k=3, stride=1, act=ACT_LEAKY01, dt=DT_F16, up=0):
    return K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                       ksize=k, stride=stride, act=act, kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128), out_dtype=dt,
                       upsample2x=up)


def _twin(d, dt=DT_BF16):
    e = YoloConvDesc.from_buffer_copy(d)
    e.out_dtype = dt
    return e


# name -> (fp16 descriptor, the answer at 256 compute units)
RULE_TABLE = {
    "80x80 128->256 x32": (_desc(32, 80, 80, 128, 256), 1),
    "40x40 256->512 x32": (_desc(32, 40, 40, 256, 512), 1),
    "20x20 512->1024 x16": (_desc(16, 20, 20, 512, 1024), 1),                 # 16 tiles x 8 cout tiles = 128 = 256 / 2
    "160->80 stride 2 128->256 x32": (_desc(32, 160, 160, 128, 256, stride=2), 1),
    "1x1": (_desc(32, 80, 80, 256, 128, k=1), 0),
    "cout 255": (_desc(32, 80, 80, 128, 255), 0),
    "cin 24": (_desc(32, 80, 80, 24, 256), 0),
    "swish": (_desc(32, 80, 80, 128, 256, act=ACT_SWISH), 0),
    "upsample2x": (_desc(32, 80, 80, 128, 256, up=1), 0),
    "26x26 map": (_desc(32, 26, 26, 256, 512), 0),                              # 676 of the 1600 pixels of its four tiles
    "80x80 64->128 x1": (_desc(1, 80, 80, 64, 128), 0),                        # 16 workgroups
    "40->20 stride 2 512->1024 x32": (_desc(32, 40, 40, 512, 1024, stride=2), 0),   # 256 workgroups < 2 x 256
}


def test_supported_truth_table():
    """yolo_conv3x3_t20_f16_supported: the shipped rule of the bf16 20x20-tile kernels with out_dtype == YOLO_DT_F16.  Every fp16
    descriptor of the table gets the answer yolo_conv2d_pick gives its bf16 twin (the same descriptor with out_dtype = YOLO_DT_BF16:
    "t20v2<" / "t20s2<" or another family); a descriptor whose out_dtype is bf16 or fp32 is never taken, whatever its twin gets.  No
    yolo_set_tuning word changes an answer (the bf16 picker does follow knob 2); the compute units of the launch do."""
    assert K.set_launch_cus(256) == 256                                        # (the default the table is written for)
    answers = {}
    for name, (d, want) in RULE_TABLE.items():
        got = K.conv3x3_t20_f16_supported(d)
        answers[name] = got
        assert got == bool(want), name
        pick = K.conv2d_pick(_twin(d))
        assert got == pick.startswith(("t20v2<", "t20s2<")), f"{name}: fp16 rule {got}, the bf16 twin runs {pick}"
        if got:
            assert pick.startswith("t20s2<" if d.stride == 2 else "t20v2<")
    yes = RULE_TABLE["80x80 128->256 x32"][0]
    for dt in (DT_BF16, DT_F32):
        assert not K.conv3x3_t20_f16_supported(_twin(yes, dt))
    views = YoloConvDesc.from_buffer_copy(yes)                                  # residual and pre-add copy: views of 8-channel multiples
    views.res_c_total, views.res_c_offset, views.aux_c_total, views.aux_c_offset = 256, 0, 264, 8
    assert K.conv3x3_t20_f16_supported(views, True, True) and K.conv2d_pick(_twin(views), True, True).startswith("t20v2<")
    odd = YoloConvDesc.from_buffer_copy(yes)
    odd.res_c_total, odd.res_c_offset = 260, 4
    assert not K.conv2d_pick(_twin(odd), True, False).startswith("t20")
    assert K.conv3x3_t20_f16_supported(odd, False, False) and not K.conv3x3_t20_f16_supported(odd, True, False)
    lib = _lib.load()
    for knob, word in ((1, 1 << 3), (1, 0x7fff), (2, 16), (2, 64)):             # conv_debug bits; families: t20 always / never
        old = lib.yolo_set_tuning(knob, word)
        try:
            assert {n: K.conv3x3_t20_f16_supported(d) for n, (d, _) in RULE_TABLE.items()} == answers, (knob, word)
        finally:
            lib.yolo_set_tuning(knob, old)
    # ... and it is sized against launch_cus(): half the chip takes half the workgroups
    small = _desc(8, 20, 20, 512, 1024)
    assert not K.conv3x3_t20_f16_supported(small)
    old = K.set_launch_cus(128)
    try:
        assert K.conv3x3_t20_f16_supported(small) and K.conv2d_pick(_twin(small)).startswith("t20v2<")
    finally:
        K.set_launch_cus(old)
    assert not K.conv3x3_t20_f16_supported(small)


def test_fwd_reports_argument_errors_without_a_gpu():
    """yolo_conv3x3_t20_f16_fwd checks its arguments before it launches: null pointers and a non-fp16 output are YOLO_E_ARG, a layer
    the rule does not take is YOLO_E_UNSUPPORTED under force = 0, a layer the kernels cannot compute under force = 1 too."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    yes, no = RULE_TABLE["80x80 128->256 x32"][0], RULE_TABLE["80x80 64->128 x1"][0]
    call = lambda d, force, x=p: lib.yolo_conv3x3_t20_f16_fwd(x, p, p, None, p, None, ctypes.byref(d), force, None)
    assert call(yes, 0, None) == -1 and b"null pointer" in lib.yolo_last_error()
    assert call(_twin(yes), 0) == -1 and b"out_dtype" in lib.yolo_last_error()
    assert call(no, 0) == -2 and b"shipped rule" in lib.yolo_last_error()
    assert call(RULE_TABLE["1x1"][0], 1) == -2 and call(RULE_TABLE["cin 24"][0], 1) == -2 and call(RULE_TABLE["swish"][0], 1) == -2
    bad = YoloConvDesc.from_buffer_copy(yes)
    bad.in_c_total = 64                                                         # the view is narrower than cin
    assert call(bad, 1) == -1 and b"input view" in lib.yolo_last_error()
    same = YoloConvDesc.from_buffer_copy(yes)
    same.ho += 1                                                                # "same" padding: no such form
    assert call(same, 1) == -2 and not K.conv3x3_t20_f16_supported(same)


def _expected_spp640_bs8():
    """The 3x3 layers of YOLOv3-SPP at 640 px x 8 images the rule takes at 256 compute units, as {(input map, stride, cin, cout): launches}.
    Stride 1 needs images x tiles x cout / 128 >= 128 workgroups: the 160x160 maps (8 x 64 x 1), the 80x80 maps (8 x 16 x 2) and the
    40x40 maps (8 x 4 x 4 = 128) pass, the 20x20 maps (8 x 1 x 8 = 64) and the 64-cout layers of the 320x320 maps do not.  Stride 2
    needs 512: only 320 -> 160 (8 x 64 x 1) has them.  Darknet-53 has 2 / 8 / 8 residual units on the 160 / 80 / 40 maps (one 3x3
    each); the detection branches of the 40 and 80 maps hold three more 3x3 layers each (the last one feeds the head)."""
    return {(320, 2, 64, 128): 1, (160, 1, 64, 128): 2, (80, 1, 128, 256): 8 + 3, (40, 1, 256, 512): 8 + 3}


def _audit(plan):
    """The static memory audit of test_fp16_launches_stay_inside_the_plans_allocations, with OP_CONV_T20_F16 read as OP_CONV_F16
    (same fields; the kernels address x / w / y / residual / pre-add copy through buffer descriptors of exactly these sizes)."""
    T20 = _t20_kind()
    allocs = {}
    for b in plan._bufs:
        t = b.tensor
        size = t.numel() * t.element_size()
        assert allocs.setdefault(t.data_ptr(), size) == size, "two buffers share storage but not their size"
    for t in plan._keep:
        allocs[t.data_ptr()] = t.numel() * t.element_size()
    starts = sorted(allocs)

    def inside(ptr, nbytes, what):
        assert ptr and nbytes > 0, what
        i = bisect.bisect_right(starts, ptr) - 1
        assert i >= 0 and ptr + nbytes <= starts[i] + allocs[starts[i]], f"{what}: [{ptr:#x}, +{nbytes}) is not inside one allocation of the plan"

    checked = 0
    for i, op in enumerate(_ops(plan)):
        d, tag = op.conv, f"op {i} kind {op.kind}"
        m_in, m_out = d.n * d.h * d.w, d.n * d.ho * d.wo
        if op.kind in (OP_CONV_F16, OP_HEAD_DECODE_F16, T20):
            inside(op.x, m_in * d.in_c_total * 2, tag + " x")
            assert d.in_c_offset + d.cin <= d.in_c_total and d.cin % 8 == 0 and d.in_c_offset % 8 == 0
            inside(op.w, d.cout_pad * d.kpad * 2, tag + " w")
            inside(op.bias, d.cout_pad * 4, tag + " bias")
            assert d.kpad >= d.ksize * d.ksize * d.cin and d.kpad % 64 == 0 and d.cout_pad >= d.cout and d.cout_pad % 128 == 0, tag
            if op.kind == OP_HEAD_DECODE_F16:
                assert not op.y and not op.y_aux
            else:
                inside(op.y, m_out * (4 if d.upsample2x else 1) * d.out_c_total * (4 if d.out_dtype == DT_F32 else 2), tag + " y")
                assert d.out_c_offset + d.cout <= d.out_c_total
                if op.residual:
                    inside(op.residual, m_out * d.res_c_total * 2, tag + " residual")
                    assert d.res_c_offset + d.cout <= d.res_c_total and not d.upsample2x
                if op.y_aux:
                    inside(op.y_aux, m_out * d.aux_c_total * 2, tag + " pre-add copy")
                    assert d.aux_c_offset + d.cout <= d.aux_c_total
            if op.kind == T20:      # what the tile kernels add: 16-byte rows on every view, fp16 out, no upsampling store
                assert d.out_dtype == DT_F16 and not d.upsample2x and d.ksize == 3 and d.pad == 1 and d.cin % 32 == 0 and d.cout % 128 == 0
                assert d.out_c_offset % 8 == 0 and d.out_c_total % 8 == 0 and d.in_c_total % 8 == 0
                assert not op.residual or (d.res_c_offset % 8 == 0 and d.res_c_total % 8 == 0)
                assert not op.y_aux or (d.aux_c_offset % 8 == 0 and d.aux_c_total % 8 == 0)
        elif op.kind == OP_MAXPOOL_F16:
            inside(op.x, m_in * d.in_c_total * 2, tag + " x")
            inside(op.y, m_out * d.out_c_total * 2, tag + " y")
            assert d.in_c_offset + d.cin <= d.in_c_total and d.out_c_offset + d.cin <= d.out_c_total
        else:
            assert op.kind == OP_SPP, tag
            inside(op.y, m_in * 4 * d.cin * 2, tag + " concat buffer")
        checked += 1
    assert checked == plan.n_ops > 10


def _same_desc(a, b):
    return bytes(a) == bytes(b)


def test_spp640_bs8_plan_holds_the_new_op_where_the_rule_says(monkeypatch):
    """A dry fp16 plan of YOLOv3-SPP at 640 px x 8 images (zero-filled host buffers: the pages are never touched): OP_CONV_T20_F16
    exactly on the convs yolo_conv3x3_t20_f16_supported accepts - the layers of _expected_spp640_bs8 -, OP_CONV_F16 on the rest;
    same list, work and bytes as with YOLO_FP16_T20=0, which holds no such op; every launch inside the plan's allocations."""
    T20 = _t20_kind()
    model = FAMILIES["spp"]().eval()
    monkeypatch.delenv("YOLO_FP16_T20", raising=False)
    plan = _dry_plan(model, 640, bs=8)
    ops = _ops(plan)
    assert {o.kind for o in ops} == {OP_CONV_F16, T20, OP_HEAD_DECODE_F16, OP_SPP}
    got = {}
    for o in ops:
        if o.kind in (OP_CONV_F16, T20):
            assert (o.kind == T20) == K.conv3x3_t20_f16_supported(o.conv, bool(o.residual), bool(o.y_aux)), (o.conv.h, o.conv.cin, o.conv.cout)
        if o.kind == T20:
            key = (o.conv.h, o.conv.stride, o.conv.cin, o.conv.cout)
            got[key] = got.get(key, 0) + 1
    assert got == _expected_spp640_bs8()
    # in-place residual and pre-add copy stay fused on the new op
    assert any(o.kind == T20 and o.residual and o.residual == o.y for o in ops) and any(o.kind == T20 and o.y_aux for o in ops)
    _audit(plan)
    monkeypatch.setenv("YOLO_FP16_T20", "0")
    off = _dry_plan(model, 640, bs=8)
    ops0 = _ops(off)
    assert T20 not in {o.kind for o in ops0} and off.n_ops == plan.n_ops
    assert all((a.kind == b.kind or (a.kind, b.kind) == (T20, OP_CONV_F16)) and _same_desc(a.conv, b.conv) and bool(a.residual) == bool(b.residual)
               and bool(a.y_aux) == bool(b.y_aux) for a, b in zip(ops, ops0))
    assert plan.conv_flops() == off.conv_flops() > 0
    assert plan.algorithmic_bytes() == off.algorithmic_bytes() and plan.algorithmic_bytes(detect=True) == off.algorithmic_bytes(detect=True)
    assert plan.activation_bytes() == off.activation_bytes() and plan.shared_buffers == off.shared_buffers
    assert [L.kind for L in plan.launches] == [L.kind for L in off.launches]


def test_small_pinned_plans_and_the_other_modes_do_not_change(monkeypatch):
    """The fp16 plans the existing tests pin (128 px x 2 of the four families, tiny-416 x 4, SPP-320 x 1) hold no OP_CONV_T20_F16 - no
    layer of theirs fills the chip - and the bf16 / fp32 launch lists are the same with the switch on, off, and after fp16 plans
    have been built."""
    T20 = _t20_kind()
    monkeypatch.delenv("YOLO_FP16_T20", raising=False)
    kinds = lambda p: [(o.kind, o.conv.out_dtype, o.conv.cin, o.conv.cout, o.conv.h, o.conv.stride) for o in _ops(p)]
    model = FAMILIES["spp"]().eval()
    before = [kinds(_dry_plan(model, 320, bs=4, precision=p)) for p in ("bf16", "fp32")]
    for family, bs, hw in [(f, 2, 128) for f in FAMILIES] + [("tiny", 4, 416), ("spp", 1, 320)]:
        plan = _dry_plan(FAMILIES[family]().eval(), hw, bs=bs)
        assert {o.kind for o in _ops(plan)} <= {OP_CONV_F16, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16, OP_SPP}, (family, bs, hw)
    assert before == [kinds(_dry_plan(model, 320, bs=4, precision=p)) for p in ("bf16", "fp32")]
    monkeypatch.setenv("YOLO_FP16_T20", "0")
    assert before == [kinds(_dry_plan(model, 320, bs=4, precision=p)) for p in ("bf16", "fp32")]
    assert all(k[0] != T20 for lst in before for k in lst)


def _kernel_metadata(path):
    """{kernel name: {field: int}} from the amdhsa.kernels notes of a device assembly file."""
    meta, cur = {}, {}
    for line in open(path):
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name" and val.startswith("_Z"):
            cur["name"] = val
        elif key in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "agpr_count", "max_flat_workgroup_size") and val.isdigit():
            cur[key] = int(val)
        if key == "wavefront_size":                     # the last field of a kernel's record
            meta[cur.pop("name")] = cur
            cur = {}
    return meta


def test_fp16_t20_device_assembly(tmp_path):
    """test_asm_mfma_kernels_keep_their_accumulator_distance for the fp16 translation unit (tools/isa_hazards.py over the ISA hipcc
    emits for csrc/conv3x3_t20_f16.hip): six kernels as in the bf16 file, each with >= 400 MFMAs, all of them v_mfma_f32_16x16x32_f16,
    no non-MFMA instruction on an accumulator within D_WINDOW wait states, no accumulator reused within 4.  From the kernels'
    metadata: no scratch, <= 256 registers and the LDS size of the bf16 twin - what two workgroups per CU need.  The analyser is
    first shown a planted hazard written with the _f16 opcode."""
    spec = importlib.util.spec_from_file_location("isa_hazards", os.path.join(ROOT, "tools", "isa_hazards.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    planted = tmp_path / "planted.s"
    planted.write_text("_Z4testv:\n\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]\n\ts_nop 2\n\tv_add_f32_e32 v20, v1, v21\n"
                       "\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]\n\ts_nop 15\n\ts_nop 15\n\tv_mov_b32_e32 v9, 0\n\ts_endpgm\n.Lfunc_end0:\n")
    n, best = H.analyse(H.parse(str(planted))["_Z4testv"])
    assert n == 2 and best["d_touch"][0] == 3 and best["d_reuse"][0] == 4 and best["war_valu"][0] == 32
    csrc = os.path.join(ROOT, "pytorch_yolo_amd", "csrc")
    files = ["conv3x3_t20_f16.hip", "conv3x3_t20.hip"]
    with ThreadPoolExecutor(2) as pool:
        f16_s, bf16_s = pool.map(lambda f: H.device_asm(os.path.join(csrc, f), str(tmp_path / (f + ".s"))), files)
    seen = {}
    for name, insts in H.parse(f16_s).items():
        n, best = H.analyse(insts)
        if not n:
            continue
        seen[name] = n
        assert n >= 400, f"{name}: {n} MFMAs - not the fully unrolled tile loop?"
        assert {mn for mn, _, _ in insts if mn.startswith("v_mfma")} == {"v_mfma_f32_16x16x32_f16"}, name
        assert best["d_touch"] is None or best["d_touch"][0] >= H.D_WINDOW, \
            f"{name}: a non-MFMA instruction touches an accumulator {best['d_touch'][0]} wait states behind its MFMA (asm line {best['d_touch'][1]} -> {best['d_touch'][2]}: {best['d_touch'][3]})"
        assert best["d_reuse"] is None or best["d_reuse"][0] >= 4, f"{name}: accumulator reused {best['d_reuse'][0]} wait states behind its MFMA"
    bf16_kernels = {name: H.analyse(insts)[0] for name, insts in H.parse(bf16_s).items()}
    bf16_kernels = {k: v for k, v in bf16_kernels.items() if v}
    assert len(seen) == len(bf16_kernels) == 6                                   # t20v2 x 2, t20s2 x 4 (x LeakyReLU fast path / generic)
    assert all("bf16" in mn for insts in H.parse(bf16_s).values() for mn, _, _ in insts if mn.startswith("v_mfma"))
    m16, mb = _kernel_metadata(f16_s), _kernel_metadata(bf16_s)
    assert set(seen) <= set(m16) and set(bf16_kernels) <= set(mb)
    for name in seen:
        twin = name.replace("IDF16_", "IDF16b")                                  # the Itanium manglings of _Float16 and __bf16
        assert twin != name and twin in bf16_kernels and seen[name] == bf16_kernels[twin], name
        k = m16[name]
        assert k["private_segment_fixed_size"] == 0, f"{name}: scratch"
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, f"{name}: {k} - one workgroup per CU"
        assert k["group_segment_fixed_size"] == mb[twin]["group_segment_fixed_size"] <= 72 * 1024, name
        assert k["max_flat_workgroup_size"] == 256
