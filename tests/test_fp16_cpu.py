"""Host-side tests of the fp16-operand mode (model.precision = "fp16"): no GPU needed - plans are built on the CPU, the weight
packer runs on the host, the instance picker launches nothing."""
import bisect

import pytest
import torch

import _cases as C
from pytorch_yolo_amd import LiteYOLOv3, YOLOv3, YOLOv3SPP, YOLOv3Tiny, engine
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import OP_SPP

FAMILIES = {"spp": lambda: YOLOv3SPP(anchors=C.SPP_ANCHORS), "tiny": YOLOv3Tiny, "yolov3": lambda: YOLOv3(anchors=C.SPP_ANCHORS),
            "lite": lambda: LiteYOLOv3(anchors=C.SPP_ANCHORS)}


def _dry_plan(model, hw, bs=1, precision="fp16"):
    rec = engine.Recorder(bs, 3, hw, hw)
    model._trace(rec, rec.input)
    return engine.Plan(rec, torch.device("cpu"), model.n_class, hw, precision)


def _ops(plan):
    return [plan.op_array[i] for i in range(plan.n_ops)]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fp16_plan_construction(family):
    """An fp16 plan is one gather-kernel launch per layer (+ max pools, + ONE SPP launch), heads decoded in their conv: nothing that
    exists in bf16 only (stem, fused units / blocks / pools, the NCHW-reading first layers) may appear in it."""
    from pytorch_yolo_amd._lib import DT_F16, DT_F32, OP_CONV_F16, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16
    model = FAMILIES[family]().eval()
    plan = _dry_plan(model, 128, bs=2)
    ops = _ops(plan)
    assert plan.precision == "fp16" and plan.f16 and not plan.f32
    assert {o.kind for o in ops} <= {OP_CONV_F16, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16, OP_SPP}
    assert all(L.kind in ("conv", "head", "pool", "spp") and not (L.reads_nchw or L.pooled) for L in plan.launches)
    assert not plan.fused_input and plan.compact_ok
    assert [o.kind for o in ops].count(OP_HEAD_DECODE_F16) == len(plan.heads) and all(hd["op"] is not None for hd in plan.heads)
    assert [o.kind for o in ops].count(OP_SPP) == (1 if family == "spp" else 0)
    assert all(b.tensor.dtype == torch.float16 for b in plan._bufs)
    assert plan.input_buffer.dtype == torch.float16 and plan.input_buffer.shape[-1] == 8
    assert all(o.conv.out_dtype in (DT_F16, DT_F32) for o in ops if o.kind == OP_CONV_F16)
    # the first layer is a plain conv on the packed input (cin padded to 8)
    assert ops[0].kind == OP_CONV_F16 and ops[0].conv.cin == 8 and ops[0].x == plan.input_buffer.data_ptr()
    # same number of conv launches as the fp32 mode (both run one conv per layer) and the same work
    p32 = _dry_plan(model, 128, bs=2, precision="fp32")
    assert plan.conv_flops() == p32.conv_flops() > 0
    assert plan.algorithmic_bytes() > 0 and plan.algorithmic_bytes(detect=True) < plan.algorithmic_bytes()


def test_fp16_leaves_the_other_modes_alone():
    """The bf16 and fp32 launch lists of a model do not depend on fp16 plans having been built."""
    model = YOLOv3SPP(anchors=C.SPP_ANCHORS).eval()
    kinds = lambda p: [(o.kind, o.conv.out_dtype, o.conv.cin, o.conv.cout) for o in _ops(p)]
    before = [kinds(_dry_plan(model, 128, bs=2, precision=p)) for p in ("bf16", "fp32")]
    _dry_plan(model, 128, bs=2)
    assert before == [kinds(_dry_plan(model, 128, bs=2, precision=p)) for p in ("bf16", "fp32")]
    from pytorch_yolo_amd._lib import OP_CONV_F32, OP_STEM
    assert before[0][0][0] == OP_STEM and before[1][0][0] == OP_CONV_F32


@pytest.mark.parametrize("ctor,kind", [("YOLOv3TinyMobile", "dwconv"), ("YOLOv3TinyEfficient", "dwconv"), ("YOLOv3TinyShuffle", "dwconv")])
def test_fp16_encoder_families_raise(ctor, kind):
    import pytorch_yolo_amd
    model = getattr(pytorch_yolo_amd, ctor)().eval()
    with pytest.raises(NotImplementedError) as e:
        _dry_plan(model, 128)
    msg = str(e.value)
    assert "fp16" in msg and any(f"'{k}'" in msg for k in ("dwconv", "se", "shuffle"))
    with pytest.raises(ValueError):
        _dry_plan(YOLOv3Tiny().eval(), 128, precision="fp8")


@pytest.mark.parametrize("cout,cin_w,cin,k", [(5, 3, 8, 3), (255, 40, 40, 1), (16, 24, 32, 3)])
def test_fp16_weight_packer(cout, cin_w, cin, k):
    """OIHW f32 -> [cout_pad][kpad] fp16 with k = (kh * ks + kw) * cin + c: bit-equal to torch's round-to-nearest-even conversion in
    the packed positions (normals, half subnormals, values that round to zero), zero elsewhere; finite values beyond +-65504 clamp."""
    g = torch.Generator().manual_seed(cout * 131 + cin)
    w = torch.randn(cout, cin_w, k, k, generator=g) * torch.tensor(10.0) ** torch.randint(-9, 4, (cout, cin_w, k, k), generator=g).float()
    w.view(-1)[:6] = torch.tensor([65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -14), 0.0])
    b = torch.randn(cout, generator=g)
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f16(w, b, cin)
    assert wp.dtype == torch.float16 and tuple(wp.shape) == (cout_pad, kpad) == (K.roundup(cout, 128), K.roundup(k * k * cin, 64))
    want = torch.zeros(cout_pad, kpad, dtype=torch.float16)
    want[:cout, :k * k * cin] = torch.nn.functional.pad(w.permute(0, 2, 3, 1), (0, cin - cin_w)).reshape(cout, -1).to(torch.float16)
    assert torch.equal(wp.view(torch.int16), want.view(torch.int16))
    assert torch.equal(bp[:cout], b) and torch.count_nonzero(bp[cout:]) == 0
    # same sizes and k order as the bf16 packing
    _, _, kpad_b, cout_pad_b = K.pack_conv_weight(w.clamp(-1e3, 1e3), b, cin)
    assert (kpad_b, cout_pad_b) == (kpad, cout_pad)


def test_fp16_weight_packer_clamps_and_keeps_nonfinite():
    w = torch.tensor([1e6, -1e6, 65519.9, 65520.0, float("inf"), float("-inf"), float("nan"), 3.0e38]).reshape(8, 1, 1, 1)
    wp, _, _, _ = K.pack_conv_weight_f16(w, None, 8)
    got = wp[:8, 0].float()
    assert got[:4].tolist() == [65504.0, -65504.0, 65504.0, 65504.0] and got[7] == 65504.0
    assert got[4] == float("inf") and got[5] == float("-inf") and torch.isnan(got[6])


@pytest.mark.parametrize("family,bs,hw", [("tiny", 4, 416), ("spp", 1, 320)])
def test_fp16_launches_stay_inside_the_plans_allocations(family, bs, hw):
    """The static memory audit of test_every_launch_stays_inside_the_plans_allocations on fp16 plans: every pointer of every launch,
    over the byte range the C ABI lets the kernel dereference, lies inside ONE allocation the plan owns."""
    from pytorch_yolo_amd._lib import DT_F32, OP_CONV_F16, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16
    plan = _dry_plan(FAMILIES[family]().eval(), hw, bs=bs)
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
        if op.kind in (OP_CONV_F16, OP_HEAD_DECODE_F16):
            inside(op.x, m_in * d.in_c_total * 2, tag + " x")
            assert d.in_c_offset + d.cin <= d.in_c_total and d.cin % 8 == 0 and d.in_c_offset % 8 == 0
            inside(op.w, d.cout_pad * d.kpad * 2, tag + " w")
            inside(op.bias, d.cout_pad * 4, tag + " bias")
            assert d.kpad >= d.ksize * d.ksize * d.cin and d.kpad % 64 == 0 and d.cout_pad >= d.cout and d.cout_pad % 128 == 0, tag
            if op.kind == OP_HEAD_DECODE_F16:
                assert not op.y and not op.y_aux            # io / p of the call: bound per call
            else:
                inside(op.y, m_out * (4 if d.upsample2x else 1) * d.out_c_total * (4 if d.out_dtype == DT_F32 else 2), tag + " y")
                assert d.out_c_offset + d.cout <= d.out_c_total
                if op.residual:
                    inside(op.residual, m_out * d.res_c_total * 2, tag + " residual")
                    assert d.res_c_offset + d.cout <= d.res_c_total and not d.upsample2x
                if op.y_aux:
                    inside(op.y_aux, m_out * d.aux_c_total * 2, tag + " pre-add copy")
                    assert d.aux_c_offset + d.cout <= d.aux_c_total
        elif op.kind == OP_MAXPOOL_F16:
            inside(op.x, m_in * d.in_c_total * 2, tag + " x")
            inside(op.y, m_out * d.out_c_total * 2, tag + " y")
            assert d.in_c_offset + d.cin <= d.in_c_total and d.out_c_offset + d.cin <= d.out_c_total
        else:
            assert op.kind == OP_SPP, tag
            inside(op.y, m_in * 4 * d.cin * 2, tag + " concat buffer")
        checked += 1
    assert checked == plan.n_ops > 10


def _desc(n, h, w, cin, cout, k, stride=1, f32=False, out_ct=None, out_co=0, res=(0, 0)):
    from pytorch_yolo_amd._lib import ACT_LEAKY01, DT_F16, DT_F32
    return K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=out_ct or K.roundup(cout, 8),
                       out_c_offset=out_co, ksize=k, stride=stride, act=ACT_LEAKY01, kpad=K.roundup(k * k * cin, 64),
                       cout_pad=K.roundup(cout, 128), out_dtype=DT_F32 if f32 else DT_F16, res=res)


def test_fp16_picker_is_a_pure_function_of_the_shape():
    """yolo_conv2d_f16_pick: the fp16 table's own names, never another kernel family, whatever the bf16 tuning word says."""
    from pytorch_yolo_amd import _lib
    shapes = [_desc(32, 80, 80, 128, 256, 3, 2), _desc(32, 40, 40, 256, 512, 3), _desc(32, 20, 20, 512, 1024, 3),
              _desc(32, 80, 80, 256, 128, 1), _desc(32, 20, 20, 1024, 512, 1), _desc(32, 640, 640, 8, 32, 3),
              _desc(32, 320, 320, 64, 32, 1), _desc(2, 160, 160, 64, 128, 3)]
    first = [K.conv2d_f16_pick(d) for d in shapes]
    assert all(s.startswith("igemm_f16<") and "loaders" not in s and "splitK" not in s for s in first), first
    # the shapes the bf16 mode hands to its t20 / stream / halo kernels stay in the gather kernel here
    assert not K.conv2d_pick(_bf16(shapes[1])).startswith("igemm") and not K.conv2d_pick(_bf16(shapes[3])).startswith("igemm")
    old = _lib.load().yolo_set_tuning(1, 1 << 3)
    try:
        assert [K.conv2d_f16_pick(d) for d in shapes] == first
    finally:
        _lib.load().yolo_set_tuning(1, old)
    # the 16x16x32 LDS-epilogue tiles and their _direct partners (a view the 16-byte epilogue cannot address: out_c_total 260)
    assert "256x256,4x4 waves,BK64,2 stages,16x16x32" in K.conv2d_f16_pick(_desc(32, 40, 40, 256, 512, 3))
    assert "256x256,4x2 waves,BK64,2 stages,32x32x16" in K.conv2d_f16_pick(_desc(32, 40, 40, 256, 512, 3, out_ct=516, out_co=4))
    head = _desc(32, 20, 20, 1024, 255, 1, f32=True)
    assert "decode" in K.head_decode_f16_pick(head, 3, 80) and K.head_decode_f16_pick(head, 3, 80, True).startswith("igemm_f16<64x256,1x8")
    with pytest.raises(RuntimeError):
        K.conv2d_f16_pick(_bf16(shapes[0]))              # out_dtype must be DT_F16 or DT_F32


def _bf16(d):
    from pytorch_yolo_amd._lib import DT_BF16, YoloConvDesc
    e = YoloConvDesc.from_buffer_copy(d)
    e.out_dtype = DT_BF16
    return e
