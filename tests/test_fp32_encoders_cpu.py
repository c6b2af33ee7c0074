"""What the fp32 mode of the depthwise encoder families shows without a device: the launch lists of the four encoder models in
fp32 (op kinds, real kernel size / pad on every depthwise op, 4-channel-aligned float32 views), the accounting over the new op
kinds, that fp16 keeps refusing these families and says fp32 exists, and the argument checks of the new entry points (they
return before any launch)."""
import ctypes

import pytest
import torch

import pytorch_yolo_amd as P
from pytorch_yolo_amd import _lib, emit, engine
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import (OP_CONV_F32, OP_DWCONV, OP_DWCONV_F32, OP_MAXPOOL_F32, OP_SE, OP_SE_F32, OP_SHUFFLE, OP_SHUFFLE_F32,
                                   YoloConvDesc)

FAMILIES = {"mobile": P.YOLOv3TinyMobile, "shuffle": P.YOLOv3TinyShuffle, "efficient": P.YOLOv3TinyEfficient,
            "squeeze": P.YOLOv3TinySqueeze}


def _dry_plan(model, hw, bs=1, precision="fp32"):
    rec = engine.Recorder(bs, 3, hw, hw)
    model._trace(rec, rec.input)
    return engine.Plan(rec, torch.device("cpu"), model.n_class, hw, precision)


def _ops(plan):
    return [plan.op_array[i] for i in range(plan.n_ops)]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fp32_plan_of_the_encoder_families(family):
    """One fp32 launch per layer: the bf16 list with every fusion off (YOLO_FUSE_MBCONV=0 for MobileNetV2) has the same depthwise /
    squeeze-excite / shuffle launches, here as their _F32 kinds; nothing 16-bit is in the list; every depthwise op carries its real
    kernel size and leading pad; every view is 4-channel aligned inside a float32 buffer."""
    torch.manual_seed(0)
    model = FAMILIES[family](n_class=3).eval()
    plan = _dry_plan(model, 416, bs=2)
    ops = _ops(plan)
    kinds = [o.kind for o in ops]
    assert set(kinds) <= {OP_CONV_F32, OP_MAXPOOL_F32, OP_DWCONV_F32, OP_SE_F32, OP_SHUFFLE_F32}
    want = {"mobile": (17, 0, 0), "shuffle": (19, 0, 16), "efficient": (16, 16, 0), "squeeze": (0, 0, 0)}[family]
    assert (kinds.count(OP_DWCONV_F32), kinds.count(OP_SE_F32), kinds.count(OP_SHUFFLE_F32)) == want
    assert all(b.tensor.dtype == torch.float32 for b in plan._bufs)
    for o in ops:
        d = o.conv
        if o.kind == OP_DWCONV_F32:
            assert d.ksize in (3, 5) and 0 <= d.pad < d.ksize and (d.ho - 1) * d.stride - d.pad < d.h and (d.wo - 1) * d.stride - d.pad < d.w
            if family != "efficient":
                assert (d.ksize, d.pad, d.ho) == (3, 1, (d.h - 1) // d.stride + 1)           # torch's pad 1, never the ksize 0 selector
        if o.kind in (OP_DWCONV_F32, OP_SE_F32):
            assert d.cin % 4 == 0 and d.in_c_offset % 4 == 0 and d.in_c_total % 4 == 0 and d.out_c_offset % 4 == 0 and d.out_c_total % 4 == 0
            assert d.in_c_offset + d.cin <= d.in_c_total and d.out_c_offset + d.cin <= d.out_c_total
        if o.kind == OP_SE_F32:
            assert o.workspace and o.ws_bytes >= K.se_workspace_bytes(d.n, d.cin) // 4 * 4 and 1 <= o.kpad_pre <= 64
        if o.kind == OP_SHUFFLE_F32:                                                         # cin = slot, cout = logical half
            assert d.cout <= d.cin and d.cin % 4 == 0 and d.out_c_offset % 4 == 0 and d.out_c_offset + 2 * d.cin <= d.out_c_total
            assert d.in_c_offset + d.cin <= d.in_c_total and d.res_c_offset + d.cin <= d.res_c_total
    if family == "efficient":            # the stride-2 "same" convs and depthwise layers on even maps: one more row than the symmetric size
        assert any(o.kind == OP_CONV_F32 and o.conv.ho == (o.conv.h + 2 * o.conv.pad - o.conv.ksize) // o.conv.stride + 2 for o in ops)
        assert {o.conv.ksize for o in ops if o.kind == OP_DWCONV_F32} == {3, 5}


@pytest.mark.parametrize("family", ["mobile", "shuffle", "efficient"])
def test_fp32_accounting_counts_the_new_kinds(family, monkeypatch):
    """conv_flops counts a depthwise fp32 op with its real kernel size; algorithmic_bytes counts the three new kinds at 4 bytes per
    element: twice what the 16-bit twin of the same launch moves."""
    monkeypatch.setenv("YOLO_FUSE_MBCONV", "0")
    torch.manual_seed(0)
    model = FAMILIES[family](n_class=3).eval()
    p32, p16 = _dry_plan(model, 416), _dry_plan(model, 416, precision="bf16")
    twins = {OP_DWCONV_F32: OP_DWCONV, OP_SE_F32: OP_SE, OP_SHUFFLE_F32: OP_SHUFFLE}
    new32 = [o for o in _ops(p32) if o.kind in twins]
    old16 = [o for o in _ops(p16) if o.kind in twins.values()]
    assert new32 and [twins[o.kind] for o in new32] == [o.kind for o in old16]
    one = lambda fn, o: fn((_lib.YoloOp * 1)(o), 1, 3)
    for a, b in zip(new32, old16):
        assert (a.conv.n, a.conv.h, a.conv.w, a.conv.cin, a.conv.ho, a.conv.wo) == (b.conv.n, b.conv.h, b.conv.w, b.conv.cin, b.conv.ho, b.conv.wo)
        assert one(emit.algorithmic_bytes, a) == 2 * one(emit.algorithmic_bytes, b) > 0
        if a.kind == OP_DWCONV_F32:
            assert one(emit.conv_flops, a) == 2.0 * a.conv.n * a.conv.ho * a.conv.wo * a.conv.cin * a.conv.ksize ** 2
        else:
            assert one(emit.conv_flops, a) == 0


@pytest.mark.parametrize("family", ["mobile", "shuffle", "efficient"])
def test_fp16_still_refuses_and_names_fp32(family):
    model = FAMILIES[family](n_class=3).eval()
    with pytest.raises(NotImplementedError) as e:
        _dry_plan(model, 96, precision="fp16")
    msg = str(e.value)
    assert "fp16" in msg and "precision='fp32'" in msg and any(f"'{k}'" in msg for k in ("dwconv", "se", "shuffle"))


def test_new_entry_points_check_their_arguments():
    """Every YOLO_REQUIRE of the three entry points, the checks their 16-bit siblings and the three max pools share with them, and
    the relaxed output-size rule of yolo_conv2d_f32_fwd return YOLO_E_ARG before anything is launched (the pointers are host memory:
    nothing may dereference them)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.yolo_last_error()
    # depthwise: (n, h, w, c, in_ct, in_co, ho, wo, out_ct, out_co, k, stride, pad, act)
    dw = lambda *a, x=p: lib.yolo_dwconv_f32_fwd(x, p, p, p, *a, None)
    assert dw(1, 8, 8, 16, 16, 0, 8, 8, 16, 0, 3, 1, 1, 0, x=None) == -1 and b"bad arguments" in err()
    assert dw(1, 8, 8, 6, 8, 0, 8, 8, 8, 0, 3, 1, 1, 0) == -1 and b"bad arguments" in err()             # c % 4
    assert dw(1, 8, 8, 16, 16, 0, 8, 8, 16, 0, 7, 1, 3, 0) == -1 and b"k 7" in err()
    assert dw(1, 8, 8, 16, 16, 0, 8, 8, 16, 0, 3, 3, 1, 0) == -1 and b"stride 3" in err()
    assert dw(1, 8, 8, 16, 16, 0, 8, 8, 16, 0, 3, 1, 1, 9) == -1 and b"activation" in err()
    assert dw(1, 8, 8, 16, 16, 0, 6, 8, 16, 0, 3, 2, 1, 0) == -1 and b"inconsistent" in err()          # row 5 starts at 9 >= 8
    assert dw(1, 8, 8, 16, 16, 4, 8, 8, 16, 0, 3, 1, 1, 0) == -1 and b"aligned" in err()               # view past the buffer
    assert dw(1, 8, 8, 16, 18, 2, 8, 8, 16, 0, 3, 1, 1, 0) == -1 and b"aligned" in err()
    # squeeze-excite: (n, h, w, c, in_ct, in_co, out_ct, out_co), weights, squeeze, workspace, bytes
    se = lambda n, h, w, c, ict, ico, oct_, oco, sq, ws: lib.yolo_se_f32_fwd(p, p, n, h, w, c, ict, ico, oct_, oco, p, p, p, p, sq, p, ws, None)
    need = lib.yolo_se_workspace_bytes(2, 16)
    assert se(2, 4, 4, 16, 16, 0, 16, 0, 4, need - 4) == -1 and b"workspace" in err()
    assert se(2, 4, 4, 16, 16, 0, 16, 0, 65, need) == -1 and b"squeezed" in err()
    assert se(2, 4, 4, 10, 16, 0, 16, 0, 4, need) == -1 and b"bad arguments" in err()
    assert se(2, 4, 4, 16, 16, 0, 16, 4, 4, need) == -1 and b"aligned" in err()
    # shuffle: (n, h, w, half, c_slot, a_ct, a_co, b_ct, b_co, y_ct, y_co)
    sh = lambda *a: lib.yolo_channel_shuffle2_f32_fwd(p, p, p, *a, None)
    assert sh(1, 4, 4, 9, 8, 8, 0, 8, 0, 16, 0) == -1 and b"logical channels" in err()                 # half > slot
    assert sh(1, 4, 4, 6, 6, 6, 0, 6, 0, 12, 0) == -1 and b"logical channels" in err()                 # slot % 4
    assert sh(1, 4, 4, 6, 8, 8, 0, 8, 0, 12, 0) == -1 and b"bad views" in err()                        # y too narrow
    assert sh(1, 4, 4, 6, 8, 8, 4, 8, 0, 16, 0) == -1 and b"bad views" in err()                        # a past its buffer
    # every precision of an op goes through one validator: what only the fp32 (or only the 16-bit) entry point used to check
    # max pool: (n, h, w, c, in_ct, in_co, ho, wo, out_ct, out_co, k, stride, pad, dilation)
    for pool, lanes in ((lib.yolo_maxpool_fwd, 8), (lib.yolo_maxpool_f16_fwd, 8), (lib.yolo_maxpool_f32_fwd, 4)):
        mp = lambda *a: pool(p, p, *a, None)
        text = b"multiple of 8" if lanes == 8 else b"multiples of 4"
        assert mp(1, 8, 8, 16, 16, lanes, 4, 4, 16, 0, 2, 2, 0, 1) == -1 and text in err()             # input view past its buffer
        assert mp(1, 8, 8, 16, 16, 0, 4, 4, 16, lanes, 2, 2, 0, 1) == -1 and text in err()             # output view past its buffer
        assert mp(1, 8, 8, 16, 16, -lanes, 4, 4, 32, 0, 2, 2, 0, 1) == -1 and text in err()            # negative offset
        assert mp(1, 7, 7, 16, 16, 0, 5, 4, 16, 0, 2, 2, 0, 1) == -1 and b"inconsistent" in err()      # ceil mode allows 4 rows, not 5
        assert mp(1, 8, 8, 16, 16, 0, 5, 4, 16, 0, 2, 2, 0, 1) == -1 and b"inconsistent" in err()      # row 4 would start at 8 >= h
    dw16 = lambda *a: lib.yolo_dwconv_fwd(p, p, p, p, *a, None)
    assert dw16(1, 8, 8, 16, 16, 0, 8, 8, 16, 0, 3, 1, 1, 9) == -1 and b"activation" in err()
    assert dw16(1, 8, 8, 16, 16, -8, 8, 8, 16, 0, 3, 1, 1, 0) == -1 and b"aligned" in err()            # negative offset
    # conv_f32: one row / column beyond the symmetric-pad size is accepted only while its window starts inside the image
    def desc(h, k, stride, pad, extra):
        d = K.conv_desc(n=1, h=h, w=h, cin=8, in_c_total=8, in_c_offset=0, cout=8, out_c_total=8, out_c_offset=0, ksize=k, stride=stride,
                        act=0, kpad=K.roundup(k * k * 8, 32), cout_pad=128, pad=pad)
        d.ho += extra
        return d
    cv = lambda d: lib.yolo_conv2d_f32_fwd(p, p, p, None, p, None, ctypes.byref(d), None)
    assert cv(desc(8, 3, 2, 0, 2)) == -1 and b"inconsistent" in err()                                  # two rows more: never
    assert cv(desc(5, 3, 2, 1, 1)) == -1 and b"inconsistent" in err()                                  # row 3 would start at 5 >= h
    bad = YoloConvDesc.from_buffer_copy(desc(8, 3, 2, 0, 0))
    bad.wo -= 1
    assert cv(bad) == -1 and b"inconsistent" in err()
