"""fp32 reference-precision mode of the depthwise encoder families (the float instances of csrc/efficient.hip and
csrc/pointwise.hip; MobileNetV2, ShuffleNetV2,
EfficientNet-B0 and - no new kernel, never driven before - SqueezeNet): kernels against torch fp32 on the CPU on the SAME fp32
operands, models against the fp32 oracle forwards, kept-index sets against the oracle NMS.

Bounds:
  * dwconv / squeeze-excite / conv: rtol = atol = 2e-5, the bound of test_conv_f32_kernel - only the summation order differs;
    the pooled means of squeeze-excite rtol 1e-4 / atol 1e-5 as the bf16 test holds them; the channel shuffle is a copy: exact.
  * models: the defaults of test_gpu_parity._assert_fp32_close (boxes 2e-3 px + 2e-5 relative, scores 2e-5).
The encoder oracles restate the published architectures (torchvision / efficientnet_pytorch are absent): their parity with those
packages is unpinned, in this mode as in bf16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77.0


def _nchw(t):      # NHWC on device -> NCHW f32 on host
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def _view_in(x, c_total, c_offset):
    """x NCHW f32 (host) -> device NHWC buffer of c_total channels holding x at c_offset and NaN everywhere else: a kernel that
    reads outside its view poisons its output."""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, c_total), float("nan"), dtype=torch.float32, device=DEV)
    buf[..., c_offset:c_offset + c] = x.permute(0, 2, 3, 1).to(DEV)
    return buf


def _assert_sentinel_outside(y, c_offset, c):
    assert torch.all(y[..., :c_offset] == SENTINEL) and torch.all(y[..., c_offset + c:] == SENTINEL), "stored outside the output view"


def _acts():
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH
    from oracle.efficientnet import swish
    return {"swish": (ACT_SWISH, swish), "relu6": (ACT_RELU6, F.relu6), "relu": (ACT_RELU, F.relu), "none": (ACT_NONE, lambda t: t),
            "leaky": (ACT_LEAKY01, lambda t: F.leaky_relu(t, 0.1))}


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("k,stride,h,w,c,act,geometry", [
    (3, 1, 20, 26, 32, "swish", "same"), (3, 2, 26, 26, 96, "swish", "same"), (5, 2, 52, 52, 144, "swish", "same"),
    (5, 1, 13, 13, 672, "swish", "same"), (5, 2, 13, 13, 40, "relu6", "same"), (3, 2, 27, 27, 24, "none", "same"),
    (3, 1, 9, 7, 12, "relu", "pad1"),            # c a multiple of 4 only
    (3, 2, 8, 8, 16, "leaky", "pad1")])
def test_dwconv_f32_kernel(k, stride, h, w, c, act, geometry):
    """yolo_dwconv_f32_fwd against torch's fp32 depthwise conv: both kernel sizes and strides, TensorFlow "same" geometry on even
    maps (the odd pad row / column below / right) and odd ones, torch's pad 1, every activation, channel-offset views on both sides."""
    from oracle.efficientnet import conv_same
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.engine import Recorder
    n = 2
    g = torch.Generator().manual_seed(k * 100 + h + c)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(c, 1, k, k, generator=g) * 0.3
    b = torch.randn(c, generator=g) * 0.1
    code, fn = _acts()[act]
    if geometry == "same":
        (ho, pad), (wo, _) = Recorder.tf_same(h, k, stride), Recorder.tf_same(w, k, stride)
        ref = fn(conv_same(x, wt, b, stride=stride, groups=c))
    else:
        ho, wo, pad = (h - 1) // stride + 1, (w - 1) // stride + 1, 1
        ref = fn(F.conv2d(x, wt, b, stride=stride, padding=1, groups=c))
    assert ref.shape[-2:] == (ho, wo)
    xin = _view_in(x, c + 12, 8)
    y = torch.full((n, ho, wo, c + 8), SENTINEL, dtype=torch.float32, device=DEV)
    K.dwconv_f32(xin, wt.reshape(c, k * k).t().contiguous().to(DEV), b.to(DEV), y, n=n, h=h, w=w, c=c, in_view=(c + 12, 8),
                 out_view=(c + 8, 4), ho=ho, wo=wo, ksize=k, stride=stride, pad=pad, act=code)
    torch.cuda.synchronize()
    got = _nchw(y[..., 4:4 + c])
    print(f"[dwconv_f32 k{k} s{stride} {h}x{w} c{c} {act}] max abs err {(got - ref).abs().max().item():.2e}")
    torch.testing.assert_close(got, ref, rtol=2e-5, atol=2e-5)
    _assert_sentinel_outside(y, 4, c)


@pytest.mark.parametrize("n,h,w,c,sq", [(2, 13, 13, 672, 28), (3, 52, 52, 96, 4), (2, 7, 9, 1152, 48),
                                        (1, 5, 3, 8, 4)])           # a map smaller than one pixel range
def test_se_f32_kernel(n, h, w, c, sq):
    """yolo_se_f32_fwd against torch: y = x * sigmoid(W2 swish(W1 mean(x) + b1) + b2); the pooled means themselves; a second run
    into a fresh buffer is bit-identical."""
    from oracle.efficientnet import swish
    from pytorch_yolo_amd import kernels as K
    g = torch.Generator().manual_seed(c + sq)
    x = torch.randn(n, c, h, w, generator=g)
    w1, b1 = torch.randn(sq, c, generator=g) * (1.0 / c) ** 0.5, torch.randn(sq, generator=g) * 0.1
    w2, b2 = torch.randn(c, sq, generator=g) * (1.0 / sq) ** 0.5, torch.randn(c, generator=g) * 0.1
    xin = _view_in(x, c + 8, 4)
    dw = [t.to(DEV) for t in (w1, b1, w2.t().contiguous(), b2)]

    def run():
        y = torch.full((n, h, w, c + 12), SENTINEL, dtype=torch.float32, device=DEV)
        ws = torch.zeros(K.se_workspace_bytes(n, c) // 4, dtype=torch.float32, device=DEV)
        K.se_f32(xin, y, *dw, ws, n=n, h=h, w=w, c=c, in_view=(c + 8, 4), out_view=(c + 12, 8))
        torch.cuda.synchronize()
        return y, ws
    y, ws = run()
    s_ = F.conv2d(swish(F.conv2d(F.adaptive_avg_pool2d(x, 1), w1[:, :, None, None], b1)), w2[:, :, None, None], b2)
    ref = torch.sigmoid(s_) * x
    got = _nchw(y[..., 8:8 + c])
    print(f"[se_f32 n{n} {h}x{w} c{c} sq{sq}] max abs err {(got - ref).abs().max().item():.2e}")
    torch.testing.assert_close(got, ref, rtol=2e-5, atol=2e-5)
    _assert_sentinel_outside(y, 8, c)
    torch.testing.assert_close(ws[:n * c].cpu().reshape(n, c), x.mean((2, 3)), rtol=1e-4, atol=1e-5)
    y2, _ = run()
    assert torch.equal(y, y2), "squeeze-excite differs from run to run"


@pytest.mark.parametrize("half,slot", [(58, 64), (116, 120), (232, 232), (8, 8)])
def test_channel_shuffle_f32_kernel_exact(half, slot):
    """yolo_channel_shuffle2_f32_fwd against torch's view / transpose / reshape channel shuffle of cat(a, b): halves that do not fill
    their slots, views into wider buffers; the pad channels of both output slots come out as exact zeros over the sentinel."""
    from pytorch_yolo_amd import kernels as K
    n, h, w = 2, 9, 7
    g = torch.Generator().manual_seed(half)
    a = torch.randn(n, slot, h, w, generator=g)
    b = torch.randn(n, slot, h, w, generator=g)
    a[:, half:] = 0
    b[:, half:] = 0                                           # the pad channels of both slots are zero by contract
    ab = _view_in(torch.cat([a, b], 1), 2 * slot + 8, 4)      # a and b: two views of one wider buffer
    y = torch.full((n, h, w, 2 * slot + 12), SENTINEL, dtype=torch.float32, device=DEV)
    K.shuffle2_f32(ab, ab, y, n=n, h=h, w=w, half=half, c_slot=slot, a_view=(2 * slot + 8, 4), b_view=(2 * slot + 8, 4 + slot),
                   y_view=(2 * slot + 12, 8))
    torch.cuda.synchronize()
    got = _nchw(y[..., 8:8 + 2 * slot])
    logical = torch.cat([a[:, :half], b[:, :half]], 1)
    want = logical.view(n, 2, half, h, w).transpose(1, 2).reshape(n, 2 * half, h, w)
    assert torch.equal(got[:, :half], want[:, :half]) and torch.equal(got[:, slot:slot + half], want[:, half:])
    assert torch.all(got[:, half:slot] == 0) and torch.all(got[:, slot + half:] == 0), "pad channels are not exact zeros"
    _assert_sentinel_outside(y, 8, 2 * slot)


@pytest.mark.parametrize("act", ["swish", "relu"])
@pytest.mark.parametrize("h,w,cin,cout,k,stride", [(32, 48, 8, 32, 3, 2), (40, 40, 64, 96, 3, 2), (26, 26, 96, 24, 1, 1)])
def test_conv_f32_tf_same_swish_relu(h, w, cin, cout, k, stride, act):
    """yolo_conv2d_f32_fwd with the output one row / column beyond the symmetric-pad size (TensorFlow "same" at stride 2 on an even
    map: the first two shapes) and the swish / ReLU epilogues, against oracle.efficientnet.conv_same."""
    from oracle.efficientnet import conv_same
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import DT_F32
    from pytorch_yolo_amd.engine import Recorder
    n = 2
    g = torch.Generator().manual_seed(h + cin)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    (ho, pad), (wo, _) = Recorder.tf_same(h, k, stride), Recorder.tf_same(w, k, stride)
    code, fn = _acts()[act]
    wp, bp, kpad, cout_pad = K.pack_conv_weight_f32(wt, bias, cin)
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 8, in_c_offset=4, cout=cout, out_c_total=cout + 8, out_c_offset=4,
                    ksize=k, stride=stride, act=code, kpad=kpad, cout_pad=cout_pad, pad=pad, out_dtype=DT_F32)
    if stride == 2:
        assert (ho, wo) == (d.ho + 1, d.wo + 1)           # the geometry under test
    d.ho, d.wo = ho, wo
    y = torch.full((n, ho, wo, cout + 8), SENTINEL, dtype=torch.float32, device=DEV)
    K.conv2d_f32(_view_in(x, cin + 8, 4), wp.to(DEV), bp.to(DEV), y, d)
    torch.cuda.synchronize()
    ref = fn(conv_same(x, wt, bias, stride=stride))
    assert ref.shape[-2:] == (ho, wo)
    got = _nchw(y[..., 4:4 + cout])
    print(f"[conv_f32 same {h}x{w} {cin}->{cout} k{k} s{stride} {act}] max abs err {(got - ref).abs().max().item():.2e}")
    torch.testing.assert_close(got, ref, rtol=2e-5, atol=2e-5)
    _assert_sentinel_outside(y, 4, cout)


# ------------------------------------------------------------------------------------------------ models
def _assert_fp32_close(io, io_ref, tag, box_atol=2e-3, box_rtol=2e-5, score_atol=2e-5):
    """fp32 mode vs the fp32 oracle (copy of test_gpu_parity._assert_fp32_close, the project's fp32 bar): only BN folding and
    summation order differ."""
    io, io_ref = io.double(), io_ref.double()
    box = (io[..., :4] - io_ref[..., :4]).abs()
    score = (io[..., 4:] - io_ref[..., 4:]).abs()
    print(f"[{tag}] fp32 mode vs fp32 oracle: max box abs {box.max().item():.6f} px, max score abs {score.max().item():.2e}")
    assert bool((box <= box_atol + box_rtol * io_ref[..., :4].abs()).all()), f"{tag}: boxes differ by {box.max().item()} px"
    assert score.max().item() <= score_atol, f"{tag}: scores differ by {score.max().item()}"


def _family(name):
    import pytorch_yolo_amd as P
    from oracle import models as om
    return {"mobile": (P.YOLOv3TinyMobile, om.tiny_mobile_forward, (2, 96, 128)),
            "shuffle": (P.YOLOv3TinyShuffle, om.tiny_shuffle_forward, (2, 96, 128)),
            "efficient": (P.YOLOv3TinyEfficient, om.tiny_efficient_forward, (2, 96, 128)),
            "squeeze": (P.YOLOv3TinySqueeze, om.tiny_squeeze_forward, (2, 127, 159))}[name]


_CASES = {}


def _case(name, wseed=5):
    """(model in eval mode with synthetic weights, x, oracle io, oracle p), computed once per (family, weight seed).  Do not modify."""
    if (name, wseed) not in _CASES:
        from oracle import models as om
        from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict
        ctor, fwd, (n, h, w) = _family(name)
        model = ctor(n_class=3).eval()
        sd = synth_state_dict(model.state_dict(), wseed, n_class=3)
        model.load_state_dict(sd)
        x = synth_images(n, h, w, 3)
        with torch.no_grad():
            io_ref, p_ref = fwd(sd, x, om.TINY_ANCHORS, 3)
        _CASES[(name, wseed)] = (model, x, io_ref, p_ref)
    return _CASES[(name, wseed)]


@pytest.mark.parametrize("name", ["mobile", "shuffle", "efficient", "squeeze"])
def test_fp32_mode_encoder_families_vs_oracle(name):
    """model.precision = 'fp32' on the four encoder families against the fp32 oracle forward at the project's fp32 bar (boxes
    2e-3 px + 2e-5 relative, scores 2e-5: the defaults of _assert_fp32_close, for every family).  The plan cache is keyed by precision: bf16 afterwards
    gives another io, and fp16 raises for the families with depthwise / squeeze-excite / shuffle layers."""
    model, x, io_ref, p_ref = _case(name)
    model = model.to(DEV)
    model.precision = "fp32"
    try:
        with torch.no_grad():
            io, p = model(x.to(DEV))
        assert io.shape == io_ref.shape and [tuple(q.shape) for q in p] == [tuple(q.shape) for q in p_ref]
        print(f"[{name}] max |raw logit| of the oracle: {max(float(q.abs().max()) for q in p_ref):.2f}")
        _assert_fp32_close(io.cpu(), io_ref, name + "/fp32")
        model.precision = "bf16"
        with torch.no_grad():
            io_b, _ = model(x.to(DEV))
        assert io_b.shape == io.shape and not torch.equal(io_b, io)
        if name != "squeeze":
            model.precision = "fp16"
            with pytest.raises(NotImplementedError, match="fp32"):
                with torch.no_grad():
                    model(x.to(DEV))
    finally:
        model.precision = "bf16"


# conf_thres / nms_thres / weight seed chosen on the CPU with the oracle alone (inputs: the 2 x 3 x 96 x 128 images of the model
# tests): >= 10 kept boxes per image (mobile 14 / 15, efficient 13 / 22), no row's conf within 1e-3 of conf_thres (nearest: mobile
# 1.8e-3, efficient 9.6e-3); also no same-class IoU within 0.08 of nms_thres and no two same-class candidates' conf within 1e-4
KEPT_CASES = {"mobile": dict(wseed=20, conf_thres=0.0313, nms_thres=0.6), "efficient": dict(wseed=10, conf_thres=0.1701, nms_thres=0.5)}


@pytest.mark.parametrize("name", list(KEPT_CASES))
def test_fp32_mode_kept_sets_equal_the_oracles(name):
    """non_max_suppression on the fp32-mode io keeps the row set oracle.nms keeps on the oracle's io, per image: classes equal,
    conf / class_conf to 1e-4; boxes under the MERGE caveat, conditions taken from test_full_size_detection_sets_vs_reference
    (>= 97 % within 1e-2 px, all within 8 px: a borderline merge member may flip).  The input is checked first, on the oracle's
    data alone: a vacuous or knife-edge one fails as such."""
    from oracle import nms as onms
    from pytorch_yolo_amd.utils.utils import non_max_suppression
    kc = KEPT_CASES[name]
    model, x, io_ref, _ = _case(name, kc["wseed"])
    ref = io_ref.numpy()
    odets, okept = onms.non_max_suppression(ref.copy(), kc["conf_thres"], kc["nms_thres"])
    assert all(d is not None and len(d) >= 10 for d in odets), f"vacuous input: the oracle keeps {[0 if d is None else len(d) for d in odets]}"
    conf = ref[..., 4] * ref[..., 5:].max(-1)
    margin = float(np.abs(conf - np.float32(kc["conf_thres"])).min())
    assert margin >= 1e-3, f"knife-edge input: a row's conf is {margin:.2e} from conf_thres"
    model = model.to(DEV)
    model.precision = "fp32"
    try:
        with torch.no_grad():
            io, _ = model(x.to(DEV))
    finally:
        model.precision = "bf16"
    dets, idx = non_max_suppression(io, kc["conf_thres"], kc["nms_thres"], with_indices=True)
    for b in range(io.shape[0]):
        d, k = dets[b].cpu().numpy(), idx[b].cpu().numpy()
        assert set(k.tolist()) == set(okept[b].tolist()), f"image {b}: kept-index set differs from the oracle's"
        assert np.array_equal(k, okept[b]) and np.array_equal(d[:, 6], odets[b][:, 6])
        np.testing.assert_allclose(d[:, 4:6], odets[b][:, 4:6], rtol=0, atol=1e-4)
        dbox = np.abs(d[:, :4] - odets[b][:, :4]).max(1)
        print(f"[{name}] image {b}: {len(d)} kept, merged boxes vs the oracle's: max {dbox.max():.5f} px")
        assert (dbox <= 1e-2).mean() >= 0.97 and dbox.max() <= 8.0
