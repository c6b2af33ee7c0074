"""Python-side wrappers of the C-ABI entry points (shape / dtype validation
happens here, before the FFI crossing — include/yolo_hip.h "Errors").

All tensors are torch CUDA (ROCm) tensors; launches go to the current stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import (ACT_LEAKY01, ACT_NONE, ACT_RELU6, DT_BF16, DT_F16, DT_F32, YoloConvDesc, YoloMbconvDesc,
                   check, load)

__all__ = ["stream_ptr", "pack_input", "conv2d", "conv2d_pick", "head_decode_pick", "stem", "stem_pick", "resunit", "resunit_supported", "resunit_form", "resunit_pick", "maxpool", "spp", "dwconv3x3", "dwconv", "se", "se_workspace_bytes", "mbconv", "mbconv_supported", "mbconv_form", "mbconv_pick", "pack_mbconv", "conv3x3_pool", "conv3x3_pool_supported", "conv2d_splitk", "conv2d_splitk_plan", "decode", "head_decode", "head_decode_supported",
           "nms_merge", "nms_styled", "nms_styled_compact", "loss_workspace_bytes", "build_targets_fwd", "loss_fwd", "loss_bwd", "LOSS_REC_WORDS", "coco_workspace_bytes", "coco_match_fwd", "coco_accumulate_fwd", "coco_sweep_chunk", "coco_max_gt",
           "COCO_T", "COCO_R", "COCO_A", "COCO_M", "pack_conv_weight", "roundup", "run_ops",
           "conv2d_bwd_workspace_bytes", "conv2d_bwd_pick", "conv2d_bwd_prepare", "conv2d_bwd_weight", "conv2d_bwd_data", "pack_conv_weight_dev",
           "conv2d_down_bwd_workspace_bytes", "conv2d_down_bwd_pick", "conv2d_down_bwd_weight", "conv2d_down_bwd_data", "pack_conv_weight_down_dev",
           "bn_workspace_bytes", "bn_pick", "bn_train_stats", "bn_eval_stats", "bn_act_fwd", "bn_act_bwd",
           "bn_act_add_fwd", "spp_train_fwd", "spp_bwd", "upsample2_concat_fwd", "upsample2_concat_bwd",
           "maxpool_train_fwd", "maxpool_bwd", "bn_act_pool_fwd", "concat_upsample2_fwd", "concat_upsample2_bwd",
           "maxpool3s2_train_fwd", "maxpool3s2_bwd", "fire_bwd_split", "fire_bwd_join",
           "conv2d_stem_bwd_workspace_bytes", "conv2d_stem_bwd_pick", "conv2d_stem_bwd_weight",
           "bn_clamp_fwd", "bn_clamp_bwd", "bn_add_rounded_fwd", "dwconv3x3_bwd_data", "dwconv3x3_bwd_weight_workspace_bytes", "dwconv3x3_bwd_weight_pick",
           "dwconv3x3_bwd_weight", "dwconv3x3_bnin_fwd", "dwconv3x3_bnin_bwd_weight",
           "maxpool3s2p1_train_fwd", "maxpool3s2p1_bwd", "channel_shuffle2_fwd", "channel_shuffle2_bwd"]


def roundup(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pytorch_yolo_amd kernels need tensors on a ROCm device (no CPU fallback)")


def pack_conv_weight(w_oihw: torch.Tensor, bias: torch.Tensor | None, cin: int):
    """OIHW f32 weights (+bias) -> (bf16 [cout_pad, kpad], f32 [cout_pad]) on the host.
    k = (kh*ks + kw)*cin + c ; cin >= w.shape[1] pads extra input channels with zeros."""
    w = w_oihw.detach().float().cpu()
    cout, cin_w, k, _ = w.shape
    kpad, cout_pad = roundup(k * k * cin, 64), roundup(cout, 128)
    packed = torch.zeros((cout_pad, k * k, cin), dtype=torch.float32)
    packed[:cout, :, :cin_w] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin_w)
    packed = torch.nn.functional.pad(packed.reshape(cout_pad, k * k * cin), (0, kpad - k * k * cin))
    b = torch.zeros(cout_pad, dtype=torch.float32)
    if bias is not None:
        b[:cout] = bias.detach().float().cpu()
    return packed.to(torch.bfloat16).contiguous(), b, kpad, cout_pad


def pack_conv_weight_f32(w_oihw: torch.Tensor, bias: torch.Tensor | None, cin: int):
    """fp32 mode: OIHW f32 weights (+bias) -> (f32 [cout_pad, kpad], f32 [cout_pad]) on the host, same k order as the bf16 form
    (kpad = roundup(k*k*cin, 32), cout_pad = roundup(cout, 128))."""
    w = w_oihw.detach().float().cpu()
    cout, cin_w, k, _ = w.shape
    kpad, cout_pad = roundup(k * k * cin, 32), roundup(cout, 128)
    packed = torch.zeros((cout_pad, k * k, cin), dtype=torch.float32)
    packed[:cout, :, :cin_w] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin_w)
    packed = torch.nn.functional.pad(packed.reshape(cout_pad, k * k * cin), (0, kpad - k * k * cin))
    b = torch.zeros(cout_pad, dtype=torch.float32)
    if bias is not None:
        b[:cout] = bias.detach().float().cpu()
    return packed.contiguous(), b, kpad, cout_pad


def pack_conv_weight_f16(w_oihw: torch.Tensor, bias: torch.Tensor | None, cin: int):
    """fp16 mode: OIHW f32 weights (+bias) -> (fp16 [cout_pad, kpad], f32 [cout_pad]) on the host through the library's packer
    (yolo_pack_conv_weight_f32_f16): sizes and k order of the bf16 form, round to nearest even, finite values beyond +-65504
    clamped to +-65504."""
    w = w_oihw.detach().float().cpu().contiguous()
    cout, cin_w, k, _ = w.shape
    kpad, cout_pad = roundup(k * k * cin, 64), roundup(cout, 128)
    packed = torch.empty((cout_pad, kpad), dtype=torch.float16)
    check(load().yolo_pack_conv_weight_f32_f16(_ptr(w), cout, cin_w, k, cin, cout_pad, kpad, _ptr(packed)), "pack_conv_weight_f16")
    b = torch.zeros(cout_pad, dtype=torch.float32)
    if bias is not None:
        b[:cout] = bias.detach().float().cpu()
    return packed, b, kpad, cout_pad


def pack_input_f16(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """fp16 mode: f32 NCHW -> fp16 NHWC (channels zero-padded to out.shape[-1])."""
    _need_cuda(x, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("pack_input_f16: x must be contiguous float32 NCHW")
    n, c, h, w = x.shape
    if out.dtype != torch.float16 or tuple(out.shape[:3]) != (n, h, w) or not out.is_contiguous():
        raise RuntimeError("pack_input_f16: out must be contiguous fp16 [n,h,w,c_pad]")
    check(load().yolo_pack_input_nchw_f32_f16(_ptr(x), _ptr(out), n, c, h, w, out.shape[3], stream_ptr()), "pack_input_f16")
    return out


def conv2d_f16(x, w_packed, bias, y, desc: YoloConvDesc, residual=None, y_preadd=None):
    """fp16 mode conv (yolo_conv2d_f16_fwd): x / residual / y_preadd / w_packed fp16, y fp16 or (desc.out_dtype = DT_F32) float32."""
    _need_cuda(x, w_packed, bias, y, residual, y_preadd)
    for t in (x, w_packed, residual, y_preadd):
        if t is not None and t.dtype != torch.float16:
            raise RuntimeError("conv2d_f16: x, w_packed, residual and y_preadd must be float16")
    if y.dtype != (torch.float32 if desc.out_dtype == DT_F32 else torch.float16):
        raise RuntimeError("conv2d_f16: y must match desc.out_dtype (DT_F16 or DT_F32)")
    check(load().yolo_conv2d_f16_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(y), _ptr(y_preadd),
                                     C.byref(desc), stream_ptr()), "conv2d_f16")
    return y


def conv3x3_t20_f16_supported(desc: YoloConvDesc, has_residual=False, has_preadd=False) -> bool:
    """The shipped rule hands this fp16 layer to the 20x20-tile 3x3 kernels (yolo_conv3x3_t20_f16_supported: no launch, works
    without a GPU; sized against the thread's launch CUs)."""
    return bool(load().yolo_conv3x3_t20_f16_supported(C.byref(desc), int(has_residual), int(has_preadd)))


def conv3x3_t20_f16(x, w_packed, bias, y, desc: YoloConvDesc, residual=None, y_preadd=None, force=False):
    """fp16 3x3 conv on the 20x20-tile kernels (yolo_conv3x3_t20_f16_fwd): tensors as conv2d_f16, y fp16.  ``force``: every layer
    the kernels can compute instead of the shipped rule's."""
    _need_cuda(x, w_packed, bias, y, residual, y_preadd)
    for t in (x, w_packed, y, residual, y_preadd):
        if t is not None and t.dtype != torch.float16:
            raise RuntimeError("conv3x3_t20_f16: x, w_packed, y, residual and y_preadd must be float16")
    check(load().yolo_conv3x3_t20_f16_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(y), _ptr(y_preadd),
                                          C.byref(desc), int(force), stream_ptr()), "conv3x3_t20_f16")
    return y


def conv2d_f16_pick(desc: YoloConvDesc, has_residual=False, has_preadd=False) -> str:
    """Name + grid of the fp16 instance yolo_conv2d_f16_fwd would launch for ``desc`` (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_conv2d_f16_pick(C.byref(desc), int(has_residual), int(has_preadd), buf, 256), "conv2d_f16_pick")
    return buf.value.decode()


def head_decode_f16_pick(desc: YoloConvDesc, na: int, nc: int, filter: bool = False) -> str:
    buf = C.create_string_buffer(256)
    check(load().yolo_head_decode_f16_pick(C.byref(desc), na, nc, int(filter), buf, 256), "head_decode_f16_pick")
    return buf.value.decode()


def maxpool_f16(x, y, *, n, h, w, c, in_view, out_view, ksize, stride, pad, dilation=1):
    _need_cuda(x, y)
    ho = (h + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    check(load().yolo_maxpool_f16_fwd(_ptr(x), _ptr(y), n, h, w, c, in_view[0], in_view[1], ho, wo, out_view[0],
                                      out_view[1], ksize, stride, pad, dilation, stream_ptr()), "maxpool_f16")
    return y


def head_decode_f16(x, w_packed, bias, desc: YoloConvDesc, anchors_px, nc, stride_px, io, io_row_offset, p=None):
    """fp16 head conv + YOLOLayer decode in one launch (yolo_head_decode_f16_fwd)."""
    _need_cuda(x, w_packed, bias, io, p)
    na = len(anchors_px)
    flat = (C.c_float * (2 * na))(*[float(v) for a in anchors_px for v in a])
    check(load().yolo_head_decode_f16_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), C.byref(desc), flat, na, nc, float(stride_px),
                                          _ptr(io), io.shape[1], io_row_offset, _ptr(p), stream_ptr()), "head_decode_f16")
    return io


def head_decode_filter_f16(x, w_packed, bias, desc: YoloConvDesc, anchors_px, nc, stride_px, rows_total, io_row_offset, conf_thres,
                           workspace, *, min_wh=2.0, p=None):
    """fp16 head conv + decode + NMS row filter in one launch (yolo_head_decode_filter_f16_fwd)."""
    _need_cuda(x, w_packed, bias, workspace, p)
    na = len(anchors_px)
    flat = (C.c_float * (2 * na))(*[float(v) for a in anchors_px for v in a])
    check(load().yolo_head_decode_filter_f16_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), C.byref(desc), flat, na, nc, float(stride_px),
                                                 rows_total, io_row_offset, float(conf_thres), float(min_wh), _ptr(workspace),
                                                 workspace.numel() * workspace.element_size(), _ptr(p), stream_ptr()),
          "head_decode_filter_f16")


def pack_input_f32(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """fp32 mode: f32 NCHW -> f32 NHWC (channels zero-padded to out.shape[-1])."""
    _need_cuda(x, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("pack_input_f32: x must be contiguous float32 NCHW")
    n, c, h, w = x.shape
    if out.dtype != torch.float32 or tuple(out.shape[:3]) != (n, h, w) or not out.is_contiguous():
        raise RuntimeError("pack_input_f32: out must be contiguous f32 [n,h,w,c_pad]")
    check(load().yolo_pack_input_nchw_f32_nhwc(_ptr(x), _ptr(out), n, c, h, w, out.shape[3], stream_ptr()), "pack_input_f32")
    return out


def conv2d_f32(x, w_packed, bias, y, desc: YoloConvDesc, residual=None, y_preadd=None):
    """fp32 mode conv (yolo_conv2d_f32_fwd): all tensors float32, ``desc`` as for conv2d with the fp32 packing sizes."""
    _need_cuda(x, w_packed, bias, y, residual, y_preadd)
    for t in (x, w_packed, bias, y, residual, y_preadd):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("conv2d_f32: every tensor must be float32")
    check(load().yolo_conv2d_f32_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(y), _ptr(y_preadd),
                                     C.byref(desc), stream_ptr()), "conv2d_f32")
    return y


def maxpool_f32(x, y, *, n, h, w, c, in_view, out_view, ksize, stride, pad, dilation=1):
    _need_cuda(x, y)
    ho = (h + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    check(load().yolo_maxpool_f32_fwd(_ptr(x), _ptr(y), n, h, w, c, in_view[0], in_view[1], ho, wo, out_view[0],
                                      out_view[1], ksize, stride, pad, dilation, stream_ptr()), "maxpool_f32")
    return y


def _need_f32(what, *tensors):
    _need_cuda(*tensors)
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"{what}: every tensor must be contiguous float32")


def dwconv_f32(x, wkc, bias, y, *, n, h, w, c, in_view, out_view, ho, wo, ksize, stride, pad, act):
    """fp32 mode depthwise k x k (3 or 5) conv with an explicit leading pad (yolo_dwconv_f32_fwd); wkc: f32 [k*k][c]; torch's
    3x3 / pad 1 is ksize=3, pad=1."""
    _need_f32("dwconv_f32", x, wkc, bias, y)
    check(load().yolo_dwconv_f32_fwd(_ptr(x), _ptr(wkc), _ptr(bias), _ptr(y), n, h, w, c, in_view[0], in_view[1], ho, wo, out_view[0],
                                     out_view[1], ksize, stride, pad, act, stream_ptr()), "dwconv_f32")
    return y


def se_f32(x, y, w1, b1, w2, b2, workspace, *, n, h, w, c, in_view, out_view):
    """fp32 mode squeeze-and-excitation (yolo_se_f32_fwd): tensors and workspace (se_workspace_bytes) as ``se``, all float32."""
    _need_f32("se_f32", x, y, w1, b1, w2, b2, workspace)
    check(load().yolo_se_f32_fwd(_ptr(x), _ptr(y), n, h, w, c, in_view[0], in_view[1], out_view[0], out_view[1], _ptr(w1), _ptr(b1),
                                 _ptr(w2), _ptr(b2), w1.shape[0], _ptr(workspace), workspace.numel() * workspace.element_size(),
                                 stream_ptr()), "se_f32")
    return y


def shuffle2_f32(a, b, y, *, n, h, w, half, c_slot, a_view, b_view, y_view):
    """fp32 mode channel_shuffle(cat(a, b), 2) in the two-slot layout (yolo_channel_shuffle2_f32_fwd); views = (c_total, c_offset)."""
    _need_f32("shuffle2_f32", a, b, y)
    check(load().yolo_channel_shuffle2_f32_fwd(_ptr(a), _ptr(b), _ptr(y), n, h, w, half, c_slot, a_view[0], a_view[1], b_view[0],
                                               b_view[1], y_view[0], y_view[1], stream_ptr()), "shuffle2_f32")
    return y


def pack_input(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """f32 NCHW -> bf16 NHWC (channels zero-padded to out.shape[-1])."""
    _need_cuda(x, out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("pack_input: x must be contiguous float32 NCHW")
    n, c, h, w = x.shape
    if out.dtype != torch.bfloat16 or tuple(out.shape[:3]) != (n, h, w) or not out.is_contiguous():
        raise RuntimeError("pack_input: out must be contiguous bf16 [n,h,w,c_pad]")
    check(load().yolo_pack_input_nchw_f32(_ptr(x), _ptr(out), n, c, h, w, out.shape[3], stream_ptr()), "pack_input")
    return out


def conv_desc(*, n, h, w, cin, in_c_total, in_c_offset, cout, out_c_total, out_c_offset, ksize, stride,
              act, kpad, cout_pad, upsample2x=0, out_dtype=DT_BF16, res=(0, 0), aux=(0, 0), pad=None) -> YoloConvDesc:
    pad = (ksize - 1) // 2 if pad is None else pad
    d = YoloConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_total, d.in_c_offset = n, h, w, cin, in_c_total, in_c_offset
    d.ho, d.wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    d.cout, d.out_c_total, d.out_c_offset = cout, out_c_total, out_c_offset
    d.ksize, d.stride, d.pad, d.act, d.upsample2x, d.out_dtype = ksize, stride, pad, act, upsample2x, out_dtype
    d.kpad, d.cout_pad = kpad, cout_pad
    d.res_c_total, d.res_c_offset = res
    d.aux_c_total, d.aux_c_offset = aux
    return d


def conv2d_pick(desc: YoloConvDesc, has_residual=False, has_preadd=False) -> str:
    """Name + grid of the kernel instance yolo_conv2d_fwd would launch for ``desc`` (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_conv2d_pick(C.byref(desc), int(has_residual), int(has_preadd), buf, 256), "conv2d_pick")
    return buf.value.decode()


def head_decode_pick(desc: YoloConvDesc, na: int, nc: int, filter: bool = False) -> str:
    """Name + grid of the kernel instance a head op would launch (yolo_head_decode_fwd, or with ``filter`` yolo_head_decode_filter_fwd)
    for ``desc`` (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_head_decode_pick(C.byref(desc), na, nc, int(filter), buf, 256), "head_decode_pick")
    return buf.value.decode()


def conv2d(x, w_packed, bias, y, desc: YoloConvDesc, residual=None, y_preadd=None):
    _need_cuda(x, w_packed, bias, y, residual, y_preadd)
    check(load().yolo_conv2d_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(y), _ptr(y_preadd),
                                 C.byref(desc), stream_ptr()), "conv2d")
    return y


def conv2d_bwd_workspace_bytes(desc: YoloConvDesc) -> int:
    """Bytes of caller-owned workspace yolo_conv2d_bwd_weight needs for the forward's ``desc`` (no launch, works without a GPU)."""
    n = load().yolo_conv2d_bwd_workspace_bytes(C.byref(desc))
    if n == 0:
        check(-1, "conv2d_bwd_workspace_bytes")
    return int(n)


def conv2d_bwd_pick(desc: YoloConvDesc) -> str:
    """Tile, grid and split count of the weight-gradient launch for the forward's ``desc`` (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_conv2d_bwd_pick(C.byref(desc), buf, 256), "conv2d_bwd_pick")
    return buf.value.decode()


def _dt_of(t, what):
    if t.dtype == torch.bfloat16:
        return DT_BF16
    if t.dtype == torch.float32:
        return DT_F32
    raise RuntimeError(f"{what} must be bfloat16 or float32, not {t.dtype}")


def conv2d_bwd_prepare(dy, y, g, desc: YoloConvDesc):
    """g = bf16(dy * act'(y)): ``dy`` dense [n,h,w,cout] (bf16 or f32), ``y`` the forward's output in ``desc``'s output view (None is
    allowed for act none), ``g`` bf16 [n,h,w,roundup(cout,8)] - every element written."""
    _need_cuda(dy, y, g)
    pixels, cg = desc.n * desc.h * desc.w, roundup(desc.cout, 8)
    if not dy.is_contiguous() or dy.numel() != pixels * desc.cout:
        raise RuntimeError("conv2d_bwd_prepare: dy must be dense [n,h,w,cout]")
    if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.numel() != pixels * cg:
        raise RuntimeError("conv2d_bwd_prepare: g must be contiguous bf16 [n,h,w,roundup(cout,8)]")
    if y is not None and _dt_of(y, "y") != desc.out_dtype:
        raise RuntimeError("conv2d_bwd_prepare: y must be the forward's output (desc.out_dtype, read through desc's output view)")
    check(load().yolo_conv2d_bwd_prepare(_ptr(dy), _dt_of(dy, "dy"), _ptr(y), _ptr(g), C.byref(desc), stream_ptr()), "conv2d_bwd_prepare")
    return g


def conv2d_bwd_weight(x, g, dw, dbias, workspace, desc: YoloConvDesc):
    """dW (f32 OIHW [cout,cin,k,k]) and, unless ``dbias`` is None, db (f32 [cout]) of the forward ``desc``; ``workspace``: a tensor of at
    least conv2d_bwd_workspace_bytes(desc) bytes whose content does not matter."""
    _need_cuda(x, g, dw, dbias, workspace)
    if dw.dtype != torch.float32 or not dw.is_contiguous() or tuple(dw.shape) != (desc.cout, desc.cin, desc.ksize, desc.ksize):
        raise RuntimeError("conv2d_bwd_weight: dw must be contiguous float32 [cout,cin,k,k]")
    if dbias is not None and (dbias.dtype != torch.float32 or not dbias.is_contiguous() or dbias.numel() != desc.cout):
        raise RuntimeError("conv2d_bwd_weight: dbias must be contiguous float32 [cout]")
    check(load().yolo_conv2d_bwd_weight(_ptr(x), _ptr(g), _ptr(dw), _ptr(dbias), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                        C.byref(desc), stream_ptr()), "conv2d_bwd_weight")
    return dw, dbias


def conv2d_bwd_data(g, w_packed_t, dx, desc: YoloConvDesc):
    """dx (bf16, ``desc``'s INPUT view of the buffer ``dx``) = conv(g, transposed flipped W) through the forward dispatcher;
    ``w_packed_t`` from pack_conv_weight_dev(..., transposed=True)."""
    _need_cuda(g, w_packed_t, dx)
    check(load().yolo_conv2d_bwd_data(_ptr(g), _ptr(w_packed_t), _ptr(dx), C.byref(desc), stream_ptr()), "conv2d_bwd_data")
    return dx


def pack_conv_weight_dev(w_oihw: torch.Tensor, cin: int, transposed: bool = False, out: torch.Tensor | None = None):
    """Device twin of pack_conv_weight: f32 OIHW [cout,cin_w,k,k] on the device -> bf16 [cout_pad, kpad], no host copy.
    ``transposed``: the data gradient's matrix [roundup(cin_w,128), roundup(k*k*cin,64)] with ``cin`` = the channel count of g
    (roundup(cout, 8)).  Returns (packed, kpad, cout_pad)."""
    _need_cuda(w_oihw, out)
    if w_oihw.dtype != torch.float32 or not w_oihw.is_contiguous() or w_oihw.dim() != 4 or w_oihw.shape[2] != w_oihw.shape[3]:
        raise RuntimeError("pack_conv_weight_dev: w must be contiguous float32 [cout,cin,k,k]")
    cout, cin_w, k, _ = w_oihw.shape
    kpad, cout_pad = roundup(k * k * cin, 64), roundup(cin_w if transposed else cout, 128)
    if out is None:
        out = torch.empty((cout_pad, kpad), dtype=torch.bfloat16, device=w_oihw.device)
    elif out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() != cout_pad * kpad:
        raise RuntimeError("pack_conv_weight_dev: out must be contiguous bf16 [cout_pad, kpad]")
    check(load().yolo_pack_conv_weight_dev(_ptr(w_oihw), cout, cin_w, k, cin, cout_pad, kpad, int(transposed), _ptr(out), stream_ptr()),
          "pack_conv_weight_dev")
    return out, kpad, cout_pad


# ---- backward of the 3x3 stride-2 downsample (csrc/conv_down_bwd.hip) ---------------------------------------------------
def conv2d_down_bwd_workspace_bytes(desc: YoloConvDesc) -> int:
    """Bytes of caller-owned workspace yolo_conv2d_down_bwd_weight needs for the forward's stride-2 ``desc`` (no launch, works without a GPU)."""
    n = load().yolo_conv2d_down_bwd_workspace_bytes(C.byref(desc))
    if n == 0:
        check(-1, "conv2d_down_bwd_workspace_bytes")
    return int(n)


def conv2d_down_bwd_pick(desc: YoloConvDesc) -> str:
    """Tile, grid and split count of the weight-gradient launch and tile, grid and per-class pixel tiles of the parity data-gradient launch
    for the forward's stride-2 ``desc`` (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_conv2d_down_bwd_pick(C.byref(desc), buf, 256), "conv2d_down_bwd_pick")
    return buf.value.decode()


def conv2d_down_bwd_weight(x, g, dw, dbias, workspace, desc: YoloConvDesc):
    """dW (f32 OIHW [cout,cin,3,3]) and, unless ``dbias`` is None, db (f32 [cout]) of the stride-2 forward ``desc``; ``g`` dense bf16
    [n,ho,wo,cout]; ``workspace``: a tensor of at least conv2d_down_bwd_workspace_bytes(desc) bytes whose content does not matter."""
    _need_cuda(x, g, dw, dbias, workspace)
    if dw.dtype != torch.float32 or not dw.is_contiguous() or tuple(dw.shape) != (desc.cout, desc.cin, desc.ksize, desc.ksize):
        raise RuntimeError("conv2d_down_bwd_weight: dw must be contiguous float32 [cout,cin,3,3]")
    if dbias is not None and (dbias.dtype != torch.float32 or not dbias.is_contiguous() or dbias.numel() != desc.cout):
        raise RuntimeError("conv2d_down_bwd_weight: dbias must be contiguous float32 [cout]")
    if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.numel() != desc.n * desc.ho * desc.wo * desc.cout:
        raise RuntimeError("conv2d_down_bwd_weight: g must be contiguous bf16 [n,ho,wo,cout]")
    check(load().yolo_conv2d_down_bwd_weight(_ptr(x), _ptr(g), _ptr(dw), _ptr(dbias), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                             C.byref(desc), stream_ptr()), "conv2d_down_bwd_weight")
    return dw, dbias


def conv2d_down_bwd_data(g, w_packed_d, dx, desc: YoloConvDesc):
    """dx (bf16, ``desc``'s INPUT view of the buffer ``dx``) of the stride-2 forward ``desc``: the parity kernel, one launch;
    ``w_packed_d`` from pack_conv_weight_down_dev."""
    _need_cuda(g, w_packed_d, dx)
    if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.numel() != desc.n * desc.ho * desc.wo * desc.cout:
        raise RuntimeError("conv2d_down_bwd_data: g must be contiguous bf16 [n,ho,wo,cout]")
    if w_packed_d.dtype != torch.bfloat16 or not w_packed_d.is_contiguous() or w_packed_d.numel() != 9 * desc.cin * desc.cout:
        raise RuntimeError("conv2d_down_bwd_data: w_packed_d must be contiguous bf16 [3,3,cin,cout]")
    if dx.dtype != torch.bfloat16 or not dx.is_contiguous() or dx.numel() != desc.n * desc.h * desc.w * desc.in_c_total:
        raise RuntimeError("conv2d_down_bwd_data: dx must be contiguous bf16 [n,h,w,in_c_total]")
    check(load().yolo_conv2d_down_bwd_data(_ptr(g), _ptr(w_packed_d), _ptr(dx), C.byref(desc), stream_ptr()), "conv2d_down_bwd_data")
    return dx


def pack_conv_weight_down_dev(w_oihw: torch.Tensor, out: torch.Tensor | None = None):
    """The data gradient's operand of the downsample: f32 OIHW [cout,cin,3,3] on the device -> bf16 [3,3,cin,cout], no host copy."""
    _need_cuda(w_oihw, out)
    if w_oihw.dtype != torch.float32 or not w_oihw.is_contiguous() or w_oihw.dim() != 4 or tuple(w_oihw.shape[2:]) != (3, 3):
        raise RuntimeError("pack_conv_weight_down_dev: w must be contiguous float32 [cout,cin,3,3]")
    cout, cin = w_oihw.shape[:2]
    if out is None:
        out = torch.empty((3, 3, cin, cout), dtype=torch.bfloat16, device=w_oihw.device)
    elif out.dtype != torch.bfloat16 or not out.is_contiguous() or out.numel() != 9 * cin * cout:
        raise RuntimeError("pack_conv_weight_down_dev: out must be contiguous bf16 [3,3,cin,cout]")
    check(load().yolo_pack_conv_weight_down_dev(_ptr(w_oihw), cout, cin, _ptr(out), stream_ptr()), "pack_conv_weight_down_dev")
    return out


# ---- batch norm between the conv and its backward (csrc/batchnorm.hip) ----------------------------------------------
def bn_workspace_bytes(pixels: int, c: int) -> int:
    """Bytes of caller-owned workspace bn_train_stats / bn_act_bwd need for a dense [pixels, c] map (no launch, works without a GPU):
    the c1 | c2 vector (2 c floats), then the splits' float64 partials."""
    n = load().yolo_bn_workspace_bytes(int(pixels), int(c))
    if n == 0:
        check(-1, "bn_workspace_bytes")
    return int(n)


def bn_pick(pixels: int, c: int) -> str:
    """Pass shape, grid and passes per split of the two batch-norm reductions (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_bn_pick(int(pixels), int(c), buf, 256), "bn_pick")
    return buf.value.decode()


def _bn_map(t, pixels, c, what, dtypes=(torch.bfloat16,)):
    if t.dtype not in dtypes or not t.is_contiguous() or t.numel() != pixels * c:
        raise RuntimeError(f"{what} must be dense [pixels, c] ({' or '.join(str(d) for d in dtypes)})")


def _bn_vec(t, c, what, rows=1):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != rows * c):
        raise RuntimeError(f"{what} must be contiguous float32 [{'%d, ' % rows if rows > 1 else ''}c]")


def bn_train_stats(z, gamma, beta, eps, momentum, running_mean, running_var, saved, workspace):
    """Batch statistics of ``z`` (bf16, dense [..., c]) -> ``saved`` f32 [4, c] = mean, invstd, scale, shift; ``running_mean`` /
    ``running_var`` (each may be None) are updated in place.  ``workspace``: at least bn_workspace_bytes bytes, content irrelevant."""
    _need_cuda(z, gamma, beta, running_mean, running_var, saved, workspace)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_train_stats: z")
    for t, what in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _bn_vec(t, c, f"bn_train_stats: {what}")
    _bn_vec(saved, c, "bn_train_stats: saved", 4)
    check(load().yolo_bn_train_stats(_ptr(z), pixels, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
                                     _ptr(running_var), _ptr(saved), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                     stream_ptr()), "bn_train_stats")
    return saved


def bn_eval_stats(gamma, beta, running_mean, running_var, eps, saved):
    """``saved`` f32 [4, c] from the running statistics; nothing is reduced or updated."""
    _need_cuda(gamma, beta, running_mean, running_var, saved)
    c = gamma.numel()
    for t, what in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _bn_vec(t, c, f"bn_eval_stats: {what}")
    _bn_vec(saved, c, "bn_eval_stats: saved", 4)
    check(load().yolo_bn_eval_stats(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), c, float(eps), _ptr(saved), stream_ptr()),
          "bn_eval_stats")
    return saved


def bn_act_fwd(z, saved, y, act):
    """y = bf16(act(f32(z) scale + shift)) on dense [..., c] bf16 maps; ``act``: ACT_NONE or ACT_LEAKY01."""
    _need_cuda(z, saved, y)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_act_fwd: z")
    _bn_map(y, pixels, c, "bn_act_fwd: y")
    _bn_vec(saved, c, "bn_act_fwd: saved", 4)
    check(load().yolo_bn_act_fwd(_ptr(z), _ptr(saved), _ptr(y), pixels, c, int(act), stream_ptr()), "bn_act_fwd")
    return y


def bn_act_bwd(dy, z, saved, act, batch_stats, g, dgamma, dbeta, workspace):
    """The batch-norm + activation backward: ``g`` (bf16, the conv backward's operand), ``dgamma``, ``dbeta`` (f32 [c]); each of the
    three may be None.  ``dy`` dense [..., c] bf16 or f32; ``batch_stats``: saved came from bn_train_stats.  After the call the first
    2 c floats of ``workspace`` hold c1 | c2."""
    _need_cuda(dy, z, saved, g, dgamma, dbeta, workspace)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_act_bwd: z")
    _bn_map(dy, pixels, c, "bn_act_bwd: dy", (torch.bfloat16, torch.float32))
    if g is not None:
        _bn_map(g, pixels, c, "bn_act_bwd: g")
    _bn_vec(saved, c, "bn_act_bwd: saved", 4)
    _bn_vec(dgamma, c, "bn_act_bwd: dgamma")
    _bn_vec(dbeta, c, "bn_act_bwd: dbeta")
    check(load().yolo_bn_act_bwd(_ptr(dy), _dt_of(dy, "dy"), _ptr(z), _ptr(saved), pixels, c, int(act), int(bool(batch_stats)), _ptr(g),
                                 _ptr(dgamma), _ptr(dbeta), _ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr()),
          "bn_act_bwd")
    return g, dgamma, dbeta


# ---- the layers between the convs of a training step (csrc/route.hip, one entry of csrc/batchnorm.hip) ---------------
def bn_act_add_fwd(z, saved, residual, y, y_preadd, act):
    """bn_act_fwd with the residual add: y = bf16(t + f32(residual)), y_preadd (may be None) = bf16(t), t = act(f32(z) scale + shift)."""
    _need_cuda(z, saved, residual, y, y_preadd)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_act_add_fwd: z")
    _bn_map(residual, pixels, c, "bn_act_add_fwd: residual")
    _bn_map(y, pixels, c, "bn_act_add_fwd: y")
    if y_preadd is not None:
        _bn_map(y_preadd, pixels, c, "bn_act_add_fwd: y_preadd")
    _bn_vec(saved, c, "bn_act_add_fwd: saved", 4)
    check(load().yolo_bn_act_add_fwd(_ptr(z), _ptr(saved), _ptr(residual), _ptr(y), _ptr(y_preadd), pixels, c, int(act), stream_ptr()),
          "bn_act_add_fwd")
    return y, y_preadd


def _nhwc(t, shape, what, dtype=torch.bfloat16):
    """``what``: the tensor's name in the message, or its parts (binding, name), joined only when the message is raised."""
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what if isinstance(what, str) else ': '.join(what)} must be contiguous {dtype} {list(shape)}")


def spp_train_fwd(x, y, idx):
    """y [n,h,w,4c] = cat([maxpool5(x), maxpool9(x), maxpool13(x), x]) of the dense bf16 x [n,h,w,c]; idx uint8 [n,h,w,3c]: the windows'
    argmax offsets (first maximum in row-major order)."""
    _need_cuda(x, y, idx)
    if x.dim() != 4:
        raise RuntimeError("spp_train_fwd: x must be [n, h, w, c]")
    n, h, w, c = x.shape
    _nhwc(x, (n, h, w, c), "spp_train_fwd: x")
    _nhwc(y, (n, h, w, 4 * c), "spp_train_fwd: y")
    _nhwc(idx, (n, h, w, 3 * c), "spp_train_fwd: idx", torch.uint8)
    check(load().yolo_spp_train_fwd(_ptr(x), _ptr(y), _ptr(idx), n, h, w, c, stream_ptr()), "spp_train_fwd")
    return y, idx


def spp_bwd(dy, idx, dx):
    """dx [n,h,w,c] from dy [n,h,w,4c] and spp_train_fwd's idx: a gather with a fixed fp32 summation order, rounded once."""
    _need_cuda(dy, idx, dx)
    if dx.dim() != 4:
        raise RuntimeError("spp_bwd: dx must be [n, h, w, c]")
    n, h, w, c = dx.shape
    _nhwc(dx, (n, h, w, c), "spp_bwd: dx")
    _nhwc(dy, (n, h, w, 4 * c), "spp_bwd: dy")
    _nhwc(idx, (n, h, w, 3 * c), "spp_bwd: idx", torch.uint8)
    check(load().yolo_spp_bwd(_ptr(dy), _ptr(idx), _ptr(dx), n, h, w, c, stream_ptr()), "spp_bwd")
    return dx


def upsample2_concat_fwd(a, b, y):
    """y [n,2h,2w,ca+cb] = cat([nearest_x2(a), b]) of the dense bf16 a [n,h,w,ca] and b [n,2h,2w,cb]."""
    _need_cuda(a, b, y)
    if a.dim() != 4 or b.dim() != 4:
        raise RuntimeError("upsample2_concat_fwd: a must be [n, h, w, ca] and b [n, 2h, 2w, cb]")
    n, h, w, ca = a.shape
    cb = b.shape[3]
    _nhwc(a, (n, h, w, ca), "upsample2_concat_fwd: a")
    _nhwc(b, (n, 2 * h, 2 * w, cb), "upsample2_concat_fwd: b")
    _nhwc(y, (n, 2 * h, 2 * w, ca + cb), "upsample2_concat_fwd: y")
    check(load().yolo_upsample2_concat_fwd(_ptr(a), _ptr(b), _ptr(y), n, h, w, ca, cb, stream_ptr()), "upsample2_concat_fwd")
    return y


def upsample2_concat_bwd(dy, da, db, *, n, h, w, ca, cb):
    """da [n,h,w,ca] = the fp32 2x2 block sums of dy[..., :ca] rounded once, db [n,2h,2w,cb] = dy[..., ca:]; either may be None."""
    _need_cuda(dy, da, db)
    _nhwc(dy, (n, 2 * h, 2 * w, ca + cb), "upsample2_concat_bwd: dy")
    if da is not None:
        _nhwc(da, (n, h, w, ca), "upsample2_concat_bwd: da")
    if db is not None:
        _nhwc(db, (n, 2 * h, 2 * w, cb), "upsample2_concat_bwd: db")
    check(load().yolo_upsample2_concat_bwd(_ptr(dy), _ptr(da), _ptr(db), n, h, w, ca, cb, stream_ptr()), "upsample2_concat_bwd")
    return da, db


# ---- the max-pools of a training step: YOLOv3-tiny / LiteYOLOv3's here, SqueezeNet's and ShuffleNetV2's below (csrc/pool_train.hip, one
# entry of csrc/batchnorm.hip, two of csrc/route.hip) ---------------------------------------------------------------------
# the window pools of a training step (csrc/pool_train.hip): form -> the output map of an h x w input
POOL_OUT = {"2/2": lambda h, w: (h // 2, w // 2),                           # MaxPool2d(2, 2): floor
            "2/1": lambda h, w: (h, w),                                     # MaxPool2d(2, 1, padding=1, dilation=2)
            "3/2 ceil": lambda h, w: (h // 2, w // 2),                      # MaxPool2d(3, 2, ceil_mode=True), h and w >= 2
            "3/2/1": lambda h, w: ((h - 1) // 2 + 1, (w - 1) // 2 + 1)}     # MaxPool2d(3, 2, 1)


def _pool(entry, fn, form, backward, x, y, idx, stride=None):
    """The checks and the call of the six window-pool bindings ``fn``, library entry ``entry``.  ``x``: the unpooled map (dx where ``backward``),
    ``y`` the pooled one (dy) and ``idx`` of its shape, all dense NHWC.  The maxpool pair gives its ``stride`` (the entry's last argument)
    in place of a form."""
    big, small = ("dx", "dy") if backward else ("x", "y")
    _need_cuda(x, y, idx)
    if x.dim() != 4:
        raise RuntimeError(f"{fn}: {big} must be [n, h, w, c]")
    n, h, w, c = x.shape
    rest = ()
    if stride is not None:
        if stride not in (1, 2):
            raise RuntimeError(f"max-pool stride {stride} unsupported (1 or 2)")
        form, rest = "2/2" if stride == 2 else "2/1", (int(stride),)
    ho, wo = POOL_OUT[form](h, w)
    out = (n, ho, wo, c)
    _nhwc(x, (n, h, w, c), (fn, big))
    _nhwc(y, out, (fn, small))
    _nhwc(idx, out, (fn, "idx"), torch.uint8)
    ptrs = (_ptr(y), _ptr(idx), _ptr(x)) if backward else (_ptr(x), _ptr(y), _ptr(idx))
    check(entry(*ptrs, n, h, w, c, *rest, stream_ptr()), fn)


def maxpool_train_fwd(x, y, idx, stride):
    """The reference's MaxPool of the dense bf16 x [n,h,w,c].  stride 2: y [n,h/2,w/2,c] = MaxPool2d(2, 2)(x); stride 1: y [n,h,w,c] =
    MaxPool2d(2, 1, padding=1, dilation=2)(x).  idx uint8 of y's shape: the tap 0..3 of each window's first maximum."""
    _pool(load().yolo_maxpool_train_fwd, "maxpool_train_fwd", None, False, x, y, idx, stride)
    return y, idx


def maxpool_bwd(dy, idx, dx, stride):
    """dx [n,h,w,c] (every element written) from dy and maxpool_train_fwd's idx: a copy at stride 2, a gather of up to four terms with a
    fixed fp32 summation order, rounded once, at stride 1."""
    _pool(load().yolo_maxpool_bwd, "maxpool_bwd", None, True, dx, dy, idx, stride)
    return dx


def bn_act_pool_fwd(z, saved, y, idx, act):
    """bn_act_fwd with MaxPool2d(2, 2) inside: y [n,h/2,w/2,c] and idx of the dense bf16 z [n,h,w,c]; bit-equal to bn_act_fwd followed by
    maxpool_train_fwd(stride 2), the full-resolution activation is never written."""
    _need_cuda(z, saved, y, idx)
    if z.dim() != 4:
        raise RuntimeError("bn_act_pool_fwd: z must be [n, h, w, c]")
    n, h, w, c = z.shape
    _nhwc(z, (n, h, w, c), "bn_act_pool_fwd: z")
    _nhwc(y, (n, h // 2, w // 2, c), "bn_act_pool_fwd: y")
    _nhwc(idx, (n, h // 2, w // 2, c), "bn_act_pool_fwd: idx", torch.uint8)
    _bn_vec(saved, c, "bn_act_pool_fwd: saved", 4)
    check(load().yolo_bn_act_pool_fwd(_ptr(z), _ptr(saved), _ptr(y), _ptr(idx), n, h, w, c, int(act), stream_ptr()), "bn_act_pool_fwd")
    return y, idx


def concat_upsample2_fwd(b, a, y):
    """y [n,2h,2w,cb+ca] = cat([b, nearest_x2(a)]) of the dense bf16 b [n,2h,2w,cb] and a [n,h,w,ca]: YOLOv3-tiny's order."""
    _need_cuda(a, b, y)
    if a.dim() != 4 or b.dim() != 4:
        raise RuntimeError("concat_upsample2_fwd: b must be [n, 2h, 2w, cb] and a [n, h, w, ca]")
    n, h, w, ca = a.shape
    cb = b.shape[3]
    _nhwc(a, (n, h, w, ca), "concat_upsample2_fwd: a")
    _nhwc(b, (n, 2 * h, 2 * w, cb), "concat_upsample2_fwd: b")
    _nhwc(y, (n, 2 * h, 2 * w, ca + cb), "concat_upsample2_fwd: y")
    check(load().yolo_concat_upsample2_fwd(_ptr(b), _ptr(a), _ptr(y), n, h, w, cb, ca, stream_ptr()), "concat_upsample2_fwd")
    return y


def concat_upsample2_bwd(dy, db, da, *, n, h, w, cb, ca):
    """db [n,2h,2w,cb] = dy[..., :cb], da [n,h,w,ca] = the fp32 2x2 block sums of dy[..., cb:] rounded once; either may be None."""
    _need_cuda(dy, da, db)
    _nhwc(dy, (n, 2 * h, 2 * w, ca + cb), "concat_upsample2_bwd: dy")
    if da is not None:
        _nhwc(da, (n, h, w, ca), "concat_upsample2_bwd: da")
    if db is not None:
        _nhwc(db, (n, 2 * h, 2 * w, cb), "concat_upsample2_bwd: db")
    check(load().yolo_concat_upsample2_bwd(_ptr(dy), _ptr(db), _ptr(da), n, h, w, cb, ca, stream_ptr()), "concat_upsample2_bwd")
    return db, da


# ---- the layers of a training step of YOLOv3-tiny/SqueezeNet (an instance of csrc/pool_train.hip, csrc/fire_train.hip, three entries of
# csrc/conv_down_bwd.hip) -------------------------------------------------------------------------------------------------
def maxpool3s2_train_fwd(x, y, idx):
    """y [n,h//2,w//2,c] = MaxPool2d(3, 2, ceil_mode=True)(x) of the dense bf16 x [n,h,w,c] (h, w >= 2; ceil((h - 3) / 2) + 1 = h // 2);
    idx uint8 of y's shape: the tap 3i + j (0..8) of each window's first maximum among its in-bounds taps."""
    _pool(load().yolo_maxpool3s2_train_fwd, "maxpool3s2_train_fwd", "3/2 ceil", False, x, y, idx)
    return y, idx


def maxpool3s2_bwd(dy, idx, dx):
    """dx [n,h,w,c] (every element written) from dy and maxpool3s2_train_fwd's idx: a gather of up to four terms with a fixed fp32
    summation order, rounded once."""
    _pool(load().yolo_maxpool3s2_bwd, "maxpool3s2_bwd", "3/2 ceil", True, dx, dy, idx)
    return dx


def fire_bwd_split(dy, y_cat, g1, g3):
    """g1 [..., e1] | g3 [..., e3] = bf16(dy * (y_cat > 0)) split at channel e1: ``dy`` (bf16 or f32) and ``y_cat`` (bf16) dense
    [..., e1 + e3], the outputs dense bf16 - every element written."""
    _need_cuda(dy, y_cat, g1, g3)
    e1, e3 = g1.shape[-1], g3.shape[-1]
    pixels = y_cat.numel() // (e1 + e3)
    _bn_map(y_cat, pixels, e1 + e3, "fire_bwd_split: y_cat")
    _bn_map(dy, pixels, e1 + e3, "fire_bwd_split: dy", (torch.bfloat16, torch.float32))
    _bn_map(g1, pixels, e1, "fire_bwd_split: g1")
    _bn_map(g3, pixels, e3, "fire_bwd_split: g3")
    check(load().yolo_fire_bwd_split(_ptr(dy), _dt_of(dy, "dy"), _ptr(y_cat), _ptr(g1), _ptr(g3), pixels, e1, e3, stream_ptr()), "fire_bwd_split")
    return g1, g3


def fire_bwd_join(d1, d3, s_act, g_s):
    """g_s = bf16((f32(d1) + f32(d3)) * (s_act > 0)) on dense bf16 [..., sq] maps - every element written."""
    _need_cuda(d1, d3, s_act, g_s)
    sq = s_act.shape[-1]
    pixels = s_act.numel() // sq
    for t, what in ((d1, "d1"), (d3, "d3"), (s_act, "s_act"), (g_s, "g_s")):
        _bn_map(t, pixels, sq, f"fire_bwd_join: {what}")
    check(load().yolo_fire_bwd_join(_ptr(d1), _ptr(d3), _ptr(s_act), _ptr(g_s), pixels, sq, stream_ptr()), "fire_bwd_join")
    return g_s


def conv2d_stem_bwd_workspace_bytes(desc: YoloConvDesc) -> int:
    """Bytes of caller-owned workspace yolo_conv2d_stem_bwd_weight needs for the forward's stride-2 pad-0 ``desc`` (no launch, works
    without a GPU)."""
    n = load().yolo_conv2d_stem_bwd_workspace_bytes(C.byref(desc))
    if n == 0:
        check(-1, "conv2d_stem_bwd_workspace_bytes")
    return int(n)


def conv2d_stem_bwd_pick(desc: YoloConvDesc) -> str:
    """Tile, grid and split count of the weight-gradient launch for the forward's stride-2 pad-0 ``desc`` (no launch, works without a
    GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_conv2d_stem_bwd_pick(C.byref(desc), buf, 256), "conv2d_stem_bwd_pick")
    return buf.value.decode()


def conv2d_stem_bwd_weight(x, g, dw, dbias, workspace, desc: YoloConvDesc):
    """dW (f32 OIHW [cout,cin,3,3]) and, unless ``dbias`` is None, db (f32 [cout]) of the unpadded stride-2 forward ``desc``; ``g`` dense
    bf16 [n,ho,wo,cout]; ``workspace``: a tensor of at least conv2d_stem_bwd_workspace_bytes(desc) bytes whose content does not matter."""
    _need_cuda(x, g, dw, dbias, workspace)
    if dw.dtype != torch.float32 or not dw.is_contiguous() or tuple(dw.shape) != (desc.cout, desc.cin, desc.ksize, desc.ksize):
        raise RuntimeError("conv2d_stem_bwd_weight: dw must be contiguous float32 [cout,cin,3,3]")
    if dbias is not None and (dbias.dtype != torch.float32 or not dbias.is_contiguous() or dbias.numel() != desc.cout):
        raise RuntimeError("conv2d_stem_bwd_weight: dbias must be contiguous float32 [cout]")
    if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.numel() != desc.n * desc.ho * desc.wo * desc.cout:
        raise RuntimeError("conv2d_stem_bwd_weight: g must be contiguous bf16 [n,ho,wo,cout]")
    if x.dtype != torch.bfloat16 or x.numel() != desc.n * desc.h * desc.w * desc.in_c_total:
        raise RuntimeError("conv2d_stem_bwd_weight: x must be the dense bf16 [n,h,w,in_c_total] map")
    check(load().yolo_conv2d_stem_bwd_weight(_ptr(x), _ptr(g), _ptr(dw), _ptr(dbias), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                             C.byref(desc), stream_ptr()), "conv2d_stem_bwd_weight")
    return dw, dbias


# ---- MobileNetV2's inverted residual as it trains (csrc/batchnorm.hip's clamp entries, csrc/dw_train.hip) ---------------
def bn_clamp_fwd(z, saved, y, lo, hi):
    """bn_act_fwd with a clamp: y = bf16(min(max(f32(z) scale + shift, lo), hi)) on dense [..., c] bf16 maps (ReLU6: 0, 6)."""
    _need_cuda(z, saved, y)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_clamp_fwd: z")
    _bn_map(y, pixels, c, "bn_clamp_fwd: y")
    _bn_vec(saved, c, "bn_clamp_fwd: saved", 4)
    check(load().yolo_bn_clamp_fwd(_ptr(z), _ptr(saved), _ptr(y), pixels, c, float(lo), float(hi), stream_ptr()), "bn_clamp_fwd")
    return y


def bn_clamp_bwd(dy, z, saved, lo, hi, batch_stats, g, dgamma, dbeta, workspace):
    """bn_act_bwd with the clamp's slope ((a > lo and a < hi) ? 1 : 0, torch's hardtanh rule); arguments, workspace (bn_workspace_bytes)
    and results as bn_act_bwd."""
    _need_cuda(dy, z, saved, g, dgamma, dbeta, workspace)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_clamp_bwd: z")
    _bn_map(dy, pixels, c, "bn_clamp_bwd: dy", (torch.bfloat16, torch.float32))
    if g is not None:
        _bn_map(g, pixels, c, "bn_clamp_bwd: g")
    _bn_vec(saved, c, "bn_clamp_bwd: saved", 4)
    _bn_vec(dgamma, c, "bn_clamp_bwd: dgamma")
    _bn_vec(dbeta, c, "bn_clamp_bwd: dbeta")
    check(load().yolo_bn_clamp_bwd(_ptr(dy), _dt_of(dy, "dy"), _ptr(z), _ptr(saved), pixels, c, float(lo), float(hi), int(bool(batch_stats)),
                                   _ptr(g), _ptr(dgamma), _ptr(dbeta), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                   stream_ptr()), "bn_clamp_bwd")
    return g, dgamma, dbeta


def bn_add_rounded_fwd(z, saved, residual, y):
    """The linear bottleneck's normalise pass with its add (act none): y = bf16(f32(bf16(f32(z) scale + shift)) + f32(residual)) on dense
    [..., c] bf16 maps - bit-equal to bn_act_fwd(ACT_NONE) followed by a bf16 add."""
    _need_cuda(z, saved, residual, y)
    c = z.shape[-1]
    pixels = z.numel() // c
    _bn_map(z, pixels, c, "bn_add_rounded_fwd: z")
    _bn_map(residual, pixels, c, "bn_add_rounded_fwd: residual")
    _bn_map(y, pixels, c, "bn_add_rounded_fwd: y")
    _bn_vec(saved, c, "bn_add_rounded_fwd: saved", 4)
    check(load().yolo_bn_add_rounded_fwd(_ptr(z), _ptr(saved), _ptr(residual), _ptr(y), pixels, c, stream_ptr()), "bn_add_rounded_fwd")
    return y


def _dw_out(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def dwconv3x3_bwd_weight_workspace_bytes(n, h, w, c, stride) -> int:
    """Bytes of caller-owned workspace dwconv3x3_bwd_weight needs for the depthwise conv on x [n, h, w, c] (no launch, works without a
    GPU): the splits' float64 partials [9][c]."""
    nbytes = load().yolo_dwconv3x3_bwd_weight_workspace_bytes(int(n), int(h), int(w), int(c), int(stride))
    if nbytes == 0:
        check(-1, "dwconv3x3_bwd_weight_workspace_bytes")
    return int(nbytes)


def dwconv3x3_bwd_weight_pick(n, h, w, c, stride) -> str:
    """Pass shape, grid and passes per split of the depthwise weight gradient (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_dwconv3x3_bwd_weight_pick(int(n), int(h), int(w), int(c), int(stride), buf, 256), "dwconv3x3_bwd_weight_pick")
    return buf.value.decode()


def dwconv3x3_bwd_data(g, w9c, dx, stride):
    """dx (bf16 [n, h, w, c], every element written) of the depthwise 3x3 conv (pad 1) from ``g`` (bf16 [n, ho, wo, c]) and ``w9c`` (f32
    [9, c], tap-major): an fmaf chain in tap order, rounded once."""
    _need_cuda(g, w9c, dx)
    n, h, w, c = dx.shape
    _nhwc(dx, (n, h, w, c), "dwconv3x3_bwd_data: dx")
    _nhwc(g, (n,) + _dw_out(h, w, stride) + (c,), "dwconv3x3_bwd_data: g")
    _nhwc(w9c, (9, c), "dwconv3x3_bwd_data: w9c", torch.float32)
    check(load().yolo_dwconv3x3_bwd_data(_ptr(g), _ptr(w9c), _ptr(dx), n, h, w, c, int(stride), stream_ptr()), "dwconv3x3_bwd_data")
    return dx


def dwconv3x3_bwd_weight(x, g, dw, workspace, stride):
    """dw (f32, 9 c elements laid out [c, 3, 3]: the [c, 1, 3, 3] parameter) of the depthwise 3x3 conv (pad 1) from ``x`` (bf16 [n, h, w,
    c]) and ``g`` (bf16 [n, ho, wo, c]): float64 sums of exact fp32 products; ``workspace``: at least
    dwconv3x3_bwd_weight_workspace_bytes bytes, content irrelevant."""
    _need_cuda(x, g, dw, workspace)
    n, h, w, c = x.shape
    _nhwc(x, (n, h, w, c), "dwconv3x3_bwd_weight: x")
    _nhwc(g, (n,) + _dw_out(h, w, stride) + (c,), "dwconv3x3_bwd_weight: g")
    if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.numel() != 9 * c:
        raise RuntimeError("dwconv3x3_bwd_weight: dw must be contiguous float32 [c, 1, 3, 3]")
    check(load().yolo_dwconv3x3_bwd_weight(_ptr(x), _ptr(g), _ptr(dw), _ptr(workspace), workspace.numel() * workspace.element_size(), n, h, w,
                                           c, int(stride), stream_ptr()), "dwconv3x3_bwd_weight")
    return dw


def dwconv3x3_bnin_fwd(zin, saved, lo, hi, w9c, z, stride):
    """z (bf16 [n, ho, wo, c]) of the depthwise 3x3 conv (pad 1, no bias, no activation) on y = bf16(min(max(f32(zin) scale + shift, lo),
    hi)) - bn_clamp_fwd's value of ``zin`` (bf16 [n, h, w, c]) and ``saved`` (f32 [4, c]), zero outside the map - without writing y:
    bit-equal to dwconv3x3 on the materialised y."""
    _need_cuda(zin, saved, w9c, z)
    n, h, w, c = zin.shape
    _nhwc(zin, (n, h, w, c), "dwconv3x3_bnin_fwd: zin")
    _nhwc(z, (n,) + _dw_out(h, w, stride) + (c,), "dwconv3x3_bnin_fwd: z")
    _nhwc(w9c, (9, c), "dwconv3x3_bnin_fwd: w9c", torch.float32)
    _bn_vec(saved, c, "dwconv3x3_bnin_fwd: saved", 4)
    check(load().yolo_dwconv3x3_bnin_fwd(_ptr(zin), _ptr(saved), float(lo), float(hi), _ptr(w9c), _ptr(z), n, h, w, c, int(stride),
                                         stream_ptr()), "dwconv3x3_bnin_fwd")
    return z


def dwconv3x3_bnin_bwd_weight(zin, saved, lo, hi, g, dw, workspace, stride):
    """dwconv3x3_bwd_weight on the same y of ``zin`` and ``saved`` as dwconv3x3_bnin_fwd, without writing it: bit-equal to
    dwconv3x3_bwd_weight on the materialised y; workspace and pick are dwconv3x3_bwd_weight's."""
    _need_cuda(zin, saved, g, dw, workspace)
    n, h, w, c = zin.shape
    _nhwc(zin, (n, h, w, c), "dwconv3x3_bnin_bwd_weight: zin")
    _nhwc(g, (n,) + _dw_out(h, w, stride) + (c,), "dwconv3x3_bnin_bwd_weight: g")
    _bn_vec(saved, c, "dwconv3x3_bnin_bwd_weight: saved", 4)
    if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.numel() != 9 * c:
        raise RuntimeError("dwconv3x3_bnin_bwd_weight: dw must be contiguous float32 [c, 1, 3, 3]")
    check(load().yolo_dwconv3x3_bnin_bwd_weight(_ptr(zin), _ptr(saved), float(lo), float(hi), _ptr(g), _ptr(dw), _ptr(workspace),
                                                workspace.numel() * workspace.element_size(), n, h, w, c, int(stride), stream_ptr()),
          "dwconv3x3_bnin_bwd_weight")
    return dw


# ---- the layers of a training step of YOLOv3-tiny/ShuffleNetV2 that are no conv (an instance of csrc/pool_train.hip, csrc/shuffle_train.hip,
# and the forward shuffle of csrc/pointwise.hip) ----------------------------------------------------------------------------
def maxpool3s2p1_train_fwd(x, y, idx):
    """y [n,ho,wo,c] = MaxPool2d(3, 2, padding=1)(x) of the dense bf16 x [n,h,w,c], ho = (h - 1) // 2 + 1; the taps outside the map are no
    candidates (-inf).  idx uint8 of y's shape: the tap 3i + j (0..8) of each window's first maximum among its in-bounds taps."""
    _pool(load().yolo_maxpool3s2p1_train_fwd, "maxpool3s2p1_train_fwd", "3/2/1", False, x, y, idx)
    return y, idx


def maxpool3s2p1_bwd(dy, idx, dx):
    """dx [n,h,w,c] (every element written) from dy and maxpool3s2p1_train_fwd's idx: a gather of up to four terms with a fixed fp32
    summation order, rounded once."""
    _pool(load().yolo_maxpool3s2p1_bwd, "maxpool3s2p1_bwd", "3/2/1", True, dx, dy, idx)
    return dx


def _shuffle_views(fn, nhw, bufs):
    """The (c_total, c_offset) of each (name, buffer [n,h,w,c_total] or None, channel offset, view width, alignment): dense bf16 buffers of
    one pixel grid, each view inside its buffer."""
    views = []
    for what, t, off, width, v in bufs:
        if t is None:
            views.append((width, 0))
            continue
        if t.dim() != 4 or tuple(t.shape[:3]) != nhw:
            raise RuntimeError(f"{fn}: {what} must be [n, h, w, c_total] on the grid {nhw}")
        _nhwc(t, tuple(t.shape), f"{fn}: {what}")
        ct = t.shape[3]
        if off < 0 or off + width > ct or off % v or ct % v:
            raise RuntimeError(f"{fn}: the view of {what} ({width} channels at {off} of {ct}) leaves its buffer or is not {v}-channel aligned")
        views.append((ct, off))
    return views


def channel_shuffle2_fwd(a, b, y, half, c_slot, a_offset=0, b_offset=0, y_offset=0):
    """channel_shuffle(cat(a, b), 2) in the two-slot layout (yolo_channel_shuffle2_fwd): ``a`` and ``b`` are the views [offset, offset +
    c_slot) of dense bf16 [n,h,w,c_total] buffers holding ``half`` logical channels each, ``y`` the view [y_offset, y_offset + 2 c_slot):
    every channel of it is written, the pad channels as zero."""
    _need_cuda(a, b, y)
    if y.dim() != 4:
        raise RuntimeError("channel_shuffle2_fwd: y must be [n, h, w, c_total]")
    n, h, w = y.shape[:3]
    (a_v, b_v, y_v) = _shuffle_views("channel_shuffle2_fwd", (n, h, w), (("a", a, a_offset, c_slot, 1), ("b", b, b_offset, c_slot, 1),
                                                                         ("y", y, y_offset, 2 * c_slot, 8)))
    check(load().yolo_channel_shuffle2_fwd(_ptr(a), _ptr(b), _ptr(y), n, h, w, int(half), int(c_slot), a_v[0], a_v[1], b_v[0], b_v[1], y_v[0],
                                           y_v[1], stream_ptr()), "channel_shuffle2_fwd")
    return y


def channel_shuffle2_bwd(dy, da, db, half, c_slot, dy_offset=0, da_offset=0, db_offset=0):
    """The inverse of channel_shuffle2_fwd (yolo_channel_shuffle2_bwd): da[q] = dy_logical[2q], db[q] = dy_logical[2q + 1] for q < half,
    zero for the pad channels [half, c_slot).  ``dy`` is the view [dy_offset, dy_offset + 2 c_slot) of a dense bf16 [n,h,w,c_total] buffer
    (its pad channels are never read), ``da`` and ``db`` the 8-channel aligned views [offset, offset + c_slot) of theirs - every channel of
    a view is written, nothing outside it.  ``da`` or ``db`` may be None (not both)."""
    _need_cuda(dy, da, db)
    if dy.dim() != 4:
        raise RuntimeError("channel_shuffle2_bwd: dy must be [n, h, w, c_total]")
    if da is None and db is None:
        raise RuntimeError("channel_shuffle2_bwd: one of da and db is needed")
    n, h, w = dy.shape[:3]
    (y_v, a_v, b_v) = _shuffle_views("channel_shuffle2_bwd", (n, h, w), (("dy", dy, dy_offset, 2 * c_slot, 1), ("da", da, da_offset, c_slot, 8),
                                                                         ("db", db, db_offset, c_slot, 8)))
    check(load().yolo_channel_shuffle2_bwd(_ptr(dy), _ptr(da), _ptr(db), n, h, w, int(half), int(c_slot), y_v[0], y_v[1], a_v[0], a_v[1],
                                           b_v[0], b_v[1], stream_ptr()), "channel_shuffle2_bwd")
    return da, db


def conv2d_splitk_plan(desc: YoloConvDesc, has_residual=False, has_preadd=False):
    """(splits, workspace bytes, int32 counters) a layer wants for yolo_conv2d_splitk_fwd; splits == 1: it does not take it."""
    sp, wb, nc = C.c_int(1), C.c_size_t(0), C.c_int(0)
    check(load().yolo_conv2d_splitk_plan(C.byref(desc), int(has_residual), int(has_preadd), C.byref(sp), C.byref(wb), C.byref(nc)),
          "conv2d_splitk_plan")
    return sp.value, wb.value, nc.value


def conv2d_splitk(x, w_packed, bias, y, desc: YoloConvDesc, splits, workspace, counters, residual=None, y_preadd=None):
    """yolo_conv2d_splitk_fwd: ``workspace`` a byte / float tensor of at least the planned size, ``counters`` int32 zeros."""
    _need_cuda(x, w_packed, bias, y, residual, y_preadd, workspace, counters)
    check(load().yolo_conv2d_splitk_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(residual), _ptr(y), _ptr(y_preadd), C.byref(desc),
                                        splits, _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(counters),
                                        stream_ptr()), "conv2d_splitk")
    return y


def stem_pick(cin_real: int, desc: YoloConvDesc) -> str:
    """Name + grid of the kernel yolo_stem_fwd would launch under the current tuning (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_stem_pick(cin_real, C.byref(desc), buf, 256), "stem_pick")
    return buf.value.decode()


def stem(x_nchw, cin_real, w1_packed, b1, kpad1, w2_packed, b2, y, desc: YoloConvDesc):
    """conv3x3/s1 (cin_real -> 32) + conv3x3/s2 (32 -> 64) straight from the float32 NCHW batch (yolo_stem_fwd)."""
    _need_cuda(x_nchw, w1_packed, b1, w2_packed, b2, y)
    check(load().yolo_stem_fwd(_ptr(x_nchw), cin_real, _ptr(w1_packed), _ptr(b1), kpad1, _ptr(w2_packed), _ptr(b2), _ptr(y),
                               C.byref(desc), stream_ptr()), "stem")
    return y


def resunit_supported(c: int, h: int, w: int) -> bool:
    return bool(load().yolo_resunit_supported(c, h, w))


def resunit_form(c: int, n: int, h: int, w: int) -> int:
    """0 not supported, 1 generic 16x16-tile kernel, 2 persistent 64-channel kernel, 3 the 20-pixel-wide tile kernels (yolo_resunit_form)."""
    return int(load().yolo_resunit_form(c, n, h, w))


def resunit_pick(desc: YoloConvDesc, has_preadd=False) -> str:
    """Name + grid of the kernel yolo_resunit_fwd would launch under the current tuning (no launch, works without a GPU)."""
    buf = C.create_string_buffer(256)
    check(load().yolo_resunit_pick(C.byref(desc), int(has_preadd), buf, 256), "resunit_pick")
    return buf.value.decode()


def resunit(x, w1_packed, b1, w2_packed, b2, y, desc: YoloConvDesc, kpad1: int, cout_pad1: int, y_preadd=None):
    """One Darknet residual unit: y = x + act(conv3x3(act(conv1x1(x)))) (yolo_resunit_fwd); ``desc`` is the 3x3's."""
    _need_cuda(x, w1_packed, b1, w2_packed, b2, y, y_preadd)
    check(load().yolo_resunit_fwd(_ptr(x), _ptr(w1_packed), _ptr(b1), _ptr(w2_packed), _ptr(b2), _ptr(y), _ptr(y_preadd),
                                  C.byref(desc), kpad1, cout_pad1, stream_ptr()), "resunit")
    return y


def maxpool(x, y, *, n, h, w, c, in_view, out_view, ksize, stride, pad, dilation=1):
    _need_cuda(x, y)
    ho = (h + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1
    check(load().yolo_maxpool_fwd(_ptr(x), _ptr(y), n, h, w, c, in_view[0], in_view[1], ho, wo, out_view[0],
                                  out_view[1], ksize, stride, pad, dilation, stream_ptr()), "maxpool")
    return y


def spp(buf, *, n, h, w, c):
    _need_cuda(buf)
    check(load().yolo_spp_fwd(_ptr(buf), n, h, w, c, stream_ptr()), "spp")
    return buf


def se_workspace_bytes(n, c) -> int:
    return int(load().yolo_se_workspace_bytes(n, c))


def dwconv(x, wkc, bias, y, *, n, h, w, c, in_view, out_view, ho, wo, ksize, stride, pad, act):
    """Depthwise k x k (3 or 5) conv with an explicit leading pad (yolo_dwconv_fwd); wkc: f32 [k*k][c]."""
    _need_cuda(x, wkc, bias, y)
    check(load().yolo_dwconv_fwd(_ptr(x), _ptr(wkc), _ptr(bias), _ptr(y), n, h, w, c, in_view[0], in_view[1], ho, wo, out_view[0],
                                 out_view[1], ksize, stride, pad, act, stream_ptr()), "dwconv")
    return y


def se(x, y, w1, b1, w2, b2, workspace, *, n, h, w, c, in_view, out_view):
    """Squeeze-and-excitation (yolo_se_fwd): w1 f32 [sq][c], w2 f32 [sq][c] (the expand weight transposed)."""
    _need_cuda(x, y, w1, b1, w2, b2, workspace)
    check(load().yolo_se_fwd(_ptr(x), _ptr(y), n, h, w, c, in_view[0], in_view[1], out_view[0], out_view[1], _ptr(w1), _ptr(b1),
                             _ptr(w2), _ptr(b2), w1.shape[0], _ptr(workspace), workspace.numel() * workspace.element_size(),
                             stream_ptr()), "se")
    return y


def dwconv3x3(x, w9c, bias, y, *, n, h, w, c, in_view, out_view, stride, act):
    _need_cuda(x, w9c, bias, y)
    ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    check(load().yolo_dwconv3x3_fwd(_ptr(x), _ptr(w9c), _ptr(bias), _ptr(y), n, h, w, c, in_view[0], in_view[1],
                                    ho, wo, out_view[0], out_view[1], stride, act, stream_ptr()), "dwconv3x3")
    return y


def conv3x3_pool_supported(cin: int, cout: int) -> bool:
    return bool(load().yolo_conv3x3_pool_supported(cin, cout))


def conv3x3_pool(x, w_packed, bias, y, desc: YoloConvDesc, pool: bool = True):
    """3x3 / s1 ConvBlock with 16 | 32 input and 32 | 64 output channels (+ MaxPool2d(2, 2) when ``pool``): y is the
    pooled map then (yolo_conv3x3_pool_fwd)."""
    _need_cuda(x, w_packed, bias, y)
    check(load().yolo_conv3x3_pool_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), _ptr(y), C.byref(desc), 1 if pool else 0,
                                       stream_ptr()), "conv3x3_pool")
    return y


def mbconv_supported(cin: int, hidden: int, cout: int, stride: int) -> bool:
    return bool(load().yolo_mbconv_supported(cin, hidden, cout, stride))


def mbconv_form(cin: int, hidden: int, cout: int, stride: int) -> int:
    """0: not covered; 1: whole hidden tile in LDS (csrc/conv_mbconv.hip); 2: hidden dimension streamed in chunks of 64
    (csrc/conv_mbwide.hip, the blocks with 64..160 input channels).  The two forms read different weight images."""
    return int(load().yolo_mbconv_supported(cin, hidden, cout, stride))


def pack_mbconv(w_exp, b_exp, w_dw, b_dw, w_proj, b_proj, stride: int = 1):
    """Folded weights of one inverted-residual block -> the images yolo_mbconv_fwd reads (host tensors).
    w_exp [hidden,cin,1,1] or None, w_dw [hidden,1,3,3], w_proj [cout,hidden,1,1]; biases f32.
    Returns (we bf16 [ce,48] | None, be f32 [ce] | None, wd f32 [9,ce], bd f32 [ce], wp bf16 [cout_pad,dstride/2],
    bp f32 [cout_pad]); for the wide form (mbconv_form() == 2, hidden a multiple of 64) the plain matrices:
    (we bf16 [hidden,cin], be f32 [hidden], wd f32 [9,hidden], bd f32 [hidden], wp bf16 [cout_pad,hidden], bp f32 [cout_pad])."""
    hidden, cout = w_dw.shape[0], w_proj.shape[0]
    if w_exp is not None and mbconv_form(w_exp.shape[1], hidden, cout, stride) == 2:
        cop = roundup(cout, 16)
        wp = torch.zeros((cop, hidden), dtype=torch.float32)
        wp[:cout] = w_proj.detach().float().cpu().reshape(cout, hidden)
        bp = torch.zeros(cop, dtype=torch.float32)
        bp[:cout] = b_proj.detach().float().cpu()
        return (w_exp.detach().float().cpu().reshape(hidden, -1).to(torch.bfloat16).contiguous(), b_exp.detach().float().cpu().contiguous(),
                w_dw.detach().float().cpu().reshape(hidden, 9).t().contiguous(), b_dw.detach().float().cpu().contiguous(),
                wp.to(torch.bfloat16).contiguous(), bp)
    ce, cop = roundup(hidden, 32), roundup(cout, 16)
    dstride = load().yolo_mbconv_dstride(ce)
    we = be = None
    if w_exp is not None:
        cin = w_exp.shape[1]
        we = torch.zeros((ce, 48), dtype=torch.float32)
        we[:hidden, :cin] = w_exp.detach().float().cpu().reshape(hidden, cin)
        we = we.to(torch.bfloat16).contiguous()
        be = torch.zeros(ce, dtype=torch.float32)
        be[:hidden] = b_exp.detach().float().cpu()
    wd = torch.zeros((9, ce), dtype=torch.float32)
    wd[:, :hidden] = w_dw.detach().float().cpu().reshape(hidden, 9).t()
    bd = torch.zeros(ce, dtype=torch.float32)
    bd[:hidden] = b_dw.detach().float().cpu()
    wp = torch.zeros((cop, dstride // 2), dtype=torch.float32)
    wp[:cout, :hidden] = w_proj.detach().float().cpu().reshape(cout, hidden)
    bp = torch.zeros(cop, dtype=torch.float32)
    bp[:cout] = b_proj.detach().float().cpu()
    return we, be, wd.contiguous(), bd, wp.to(torch.bfloat16).contiguous(), bp


def mbconv_pick(*, n, h, w, cin, hidden, cout, stride, in_view=None, out_view=None, has_res=None) -> str:
    """Name + grid of the kernel yolo_mbconv_fwd would launch under the current tuning (no launch, works without a GPU); dense views
    and the residual of a stride-1 block with cin == cout unless said otherwise."""
    in_view, out_view = in_view or (cin, 0), out_view or (cout, 0)
    has_res = (stride == 1 and cin == cout) if has_res is None else has_res
    d = YoloMbconvDesc(n=n, h=h, w=w, cin=cin, in_c_total=in_view[0], in_c_offset=in_view[1], hidden=hidden, cout=cout,
                       out_c_total=out_view[0], out_c_offset=out_view[1], stride=stride,
                       has_expand=int(hidden != cin), has_res=int(has_res))
    buf = C.create_string_buffer(256)
    check(load().yolo_mbconv_pick(C.byref(d), buf, 256), "mbconv_pick")
    return buf.value.decode()


def mbconv(x, packed, y, *, n, h, w, cin, hidden, cout, in_view, out_view, stride, has_res):
    """One MobileNetV2 inverted-residual block (yolo_mbconv_fwd); ``packed`` = pack_mbconv(...) moved to the device."""
    we, be, wd, bd, wp, bp = packed
    _need_cuda(x, we, be, wd, bd, wp, bp, y)
    d = YoloMbconvDesc(n=n, h=h, w=w, cin=cin, in_c_total=in_view[0], in_c_offset=in_view[1], hidden=hidden, cout=cout,
                       out_c_total=out_view[0], out_c_offset=out_view[1], stride=stride,
                       has_expand=0 if we is None else 1, has_res=1 if has_res else 0)
    check(load().yolo_mbconv_fwd(_ptr(x), _ptr(we), _ptr(be), _ptr(wd), _ptr(bd), _ptr(wp), _ptr(bp), _ptr(y),
                                 C.byref(d), stream_ptr()), "mbconv")
    return y


def decode(head, anchors_px, nc, stride_px, io, io_row_offset, p=None):
    """head f32 [bs,ny,nx,ct] -> rows of io f32 [bs,rows_total,5+nc] (+ p f32 [bs,na,ny,nx,5+nc])."""
    _need_cuda(head, io, p)
    bs, ny, nx, ct = head.shape
    na = len(anchors_px)
    if head.dtype != torch.float32 or io.dtype != torch.float32 or not head.is_contiguous() or not io.is_contiguous():
        raise RuntimeError("decode: head and io must be contiguous float32")
    if io.shape[0] != bs or io.shape[2] != nc + 5:
        raise RuntimeError("decode: io shape mismatch")
    if p is not None and (tuple(p.shape) != (bs, na, ny, nx, nc + 5) or p.dtype != torch.float32 or not p.is_contiguous()):
        raise RuntimeError("decode: p shape mismatch")
    flat = (C.c_float * (2 * na))(*[float(v) for a in anchors_px for v in a])
    check(load().yolo_decode_fwd(_ptr(head), ct, flat, na, nc, bs, ny, nx, float(stride_px), _ptr(io), io.shape[1],
                                 io_row_offset, _ptr(p), stream_ptr()), "decode")
    return io


def head_decode_supported(cout: int, na: int, nc: int) -> bool:
    return bool(load().yolo_head_decode_supported(cout, na, nc))


def head_decode(x, w_packed, bias, desc: YoloConvDesc, anchors_px, nc, stride_px, io, io_row_offset, p=None):
    """Head conv + YOLOLayer decode in one launch (yolo_head_decode_fwd): x bf16 NHWC view described by ``desc``."""
    _need_cuda(x, w_packed, bias, io, p)
    na = len(anchors_px)
    bs, ny, nx = desc.n, desc.ho, desc.wo
    if io.dtype != torch.float32 or not io.is_contiguous() or io.shape[0] != bs or io.shape[2] != nc + 5:
        raise RuntimeError("head_decode: io must be contiguous float32 [bs, rows, 5+nc]")
    if p is not None and (tuple(p.shape) != (bs, na, ny, nx, nc + 5) or p.dtype != torch.float32 or not p.is_contiguous()):
        raise RuntimeError("head_decode: p shape mismatch")
    flat = (C.c_float * (2 * na))(*[float(v) for a in anchors_px for v in a])
    check(load().yolo_head_decode_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), C.byref(desc), flat, na, nc, float(stride_px),
                                      _ptr(io), io.shape[1], io_row_offset, _ptr(p), stream_ptr()), "head_decode")
    return io


def nms_workspace_bytes(bs, rows, nc) -> int:
    return int(load().yolo_nms_workspace_bytes(bs, rows, nc))


def nms_merge(pred, conf_thres, nms_thres, out_dets, out_idx, out_count, workspace, *, min_wh=2.0,
              max_per_class=100, mutate_conf=False):
    _need_cuda(pred, out_dets, out_idx, out_count, workspace)
    if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_contiguous():
        raise RuntimeError("nms: prediction must be contiguous float32 [bs, rows, 5+nc]")
    bs, rows, no = pred.shape
    cap = out_dets.shape[1]
    if tuple(out_dets.shape) != (bs, cap, 7) or tuple(out_idx.shape) != (bs, cap) or out_count.numel() != bs:
        raise RuntimeError("nms: output shape mismatch")
    if out_dets.dtype != torch.float32 or out_idx.dtype != torch.int32 or out_count.dtype != torch.int32:
        raise RuntimeError("nms: output dtype mismatch")
    check(load().yolo_nms_merge(_ptr(pred), bs, rows, no - 5, float(conf_thres), float(nms_thres), float(min_wh),
                                int(max_per_class), int(bool(mutate_conf)), _ptr(out_dets), _ptr(out_idx),
                                _ptr(out_count), cap, _ptr(workspace), workspace.numel() * workspace.element_size(),
                                stream_ptr()), "nms_merge")


def nms_styled(pred, conf_thres, nms_thres, out_dets, out_idx, out_count, workspace, *, style=_lib.NMS_MERGE, min_wh=2.0,
               max_per_class=100, mutate_conf=False):
    """``nms_merge`` with the suppression style as an argument (yolo_nms_styled; ``style`` = a _lib.NMS_* value)."""
    _need_cuda(pred, out_dets, out_idx, out_count, workspace)
    if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_contiguous():
        raise RuntimeError("nms: prediction must be contiguous float32 [bs, rows, 5+nc]")
    bs, rows, no = pred.shape
    cap = out_dets.shape[1]
    if tuple(out_dets.shape) != (bs, cap, 7) or tuple(out_idx.shape) != (bs, cap) or out_count.numel() != bs:
        raise RuntimeError("nms: output shape mismatch")
    if out_dets.dtype != torch.float32 or out_idx.dtype != torch.int32 or out_count.dtype != torch.int32:
        raise RuntimeError("nms: output dtype mismatch")
    check(load().yolo_nms_styled(_ptr(pred), bs, rows, no - 5, float(conf_thres), float(nms_thres), float(min_wh),
                                 int(max_per_class), int(bool(mutate_conf)), _ptr(out_dets), _ptr(out_idx),
                                 _ptr(out_count), cap, _ptr(workspace), workspace.numel() * workspace.element_size(),
                                 int(style), stream_ptr()), "nms_styled")


LOSS_REC_WORDS = 12     # int32 words of one record of yolo_build_targets_fwd: valid, b, a, gj, gi, class, txy[2], twh[2], flagged, 0


def _loss_geometry(geom, anchor_vec):
    """ctypes arrays of (na, ny, nx) per layer and of the layers' anchor_vec (w, h) pairs back to back."""
    nl = len(geom)
    arr = lambda k: (C.c_int32 * max(nl, 1))(*[int(g[k]) for g in geom])
    flat = [float(v) for layer in anchor_vec for pair in layer for v in pair]
    return nl, arr(0), arr(1), arr(2), (C.c_float * max(len(flat), 1))(*flat)


def loss_workspace_bytes(geom, bs, nt) -> int:
    """Bytes of the workspace of build_targets_fwd / loss_fwd; ``geom`` = [(na, ny, nx)] per YOLO layer."""
    nl, na, ny, nx, _ = _loss_geometry(geom, [])
    n = int(load().yolo_loss_workspace_bytes(nl, na, ny, nx, int(bs), int(nt)))
    if n == 0:
        check(-1, "loss_workspace_bytes")
    return n


def _loss_targets(targets):
    if targets.dim() != 2 or targets.shape[1] != 6 or targets.dtype != torch.float32 or not targets.is_contiguous():
        raise RuntimeError("loss: targets must be a contiguous float32 [nt, 6] tensor (image, class, x, y, w, h)")
    return targets.shape[0]


def build_targets_fwd(targets, geom, anchor_vec, bs, nc, iou_thresh, workspace):
    """Target assignment of reference build_targets (yolo_build_targets_fwd): fills the tconf map and the records at the start of
    ``workspace`` (int32 [nl, max(nt, 1), LOSS_REC_WORDS])."""
    _need_cuda(targets, workspace)
    nt = _loss_targets(targets)
    nl, na, ny, nx, av = _loss_geometry(geom, anchor_vec)
    check(load().yolo_build_targets_fwd(_ptr(targets) if nt else None, nt, nl, na, ny, nx, av, int(bs), int(nc), float(iou_thresh),
                                        _ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr()), "build_targets")


def _loss_heads(p, geom, nc, class_weight, what="head"):
    """Checks of the head tensors (or tensors of their shape) against ``geom``; returns the batch size."""
    if len(geom) != len(p) or not p:
        raise RuntimeError(f"loss: one geometry entry per {what} tensor")
    bs = p[0].shape[0]
    for t, (na_l, ny_l, nx_l) in zip(p, geom):
        if tuple(t.shape) != (bs, na_l, ny_l, nx_l, nc + 5) or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"loss: {what} tensor {tuple(t.shape)} is not contiguous float32 [{bs}, {na_l}, {ny_l}, {nx_l}, {nc + 5}]")
    if class_weight is not None and (class_weight.dtype != torch.float32 or class_weight.numel() != nc or not class_weight.is_contiguous()):
        raise RuntimeError(f"loss: class_weight must be contiguous float32 [{nc}]")
    return bs


def loss_fwd(p, targets, geom, anchor_vec, nc, iou_thresh, gains, class_weight, workspace, out, status):
    """compute_loss forward (yolo_loss_fwd): ``p`` = the raw head tensors [bs, na, ny, nx, 5 + nc] (contiguous float32), ``gains`` =
    (k xy_loss, k wh_loss, k cls_loss, k conf_loss); writes out f32 [5] and status int32 [1 + nl]."""
    _need_cuda(targets, class_weight, workspace, out, status, *p)
    nt = _loss_targets(targets)
    bs = _loss_heads(p, geom, nc, class_weight)
    if out.dtype != torch.float32 or out.numel() != 5 or status.dtype != torch.int32 or status.numel() != 1 + len(p) \
            or not out.is_contiguous() or not status.is_contiguous():
        raise RuntimeError("loss: out must be float32 [5] and status int32 [1 + layers]")
    nl, na, ny, nx, av = _loss_geometry(geom, anchor_vec)
    ptrs = (C.c_void_p * nl)(*[t.data_ptr() for t in p])
    check(load().yolo_loss_fwd(ptrs, _ptr(targets) if nt else None, nt, nl, na, ny, nx, av, bs, int(nc), float(iou_thresh),
                               (C.c_float * 4)(*[float(v) for v in gains]), _ptr(class_weight), _ptr(workspace),
                               workspace.numel() * workspace.element_size(), _ptr(out), _ptr(status), stream_ptr()), "loss")


def loss_bwd(p, targets, geom, anchor_vec, nc, iou_thresh, gains, class_weight, workspace, grad_loss, grad_p):
    """Gradient of compute_loss with respect to ``p`` (yolo_loss_bwd): the arguments of loss_fwd, ``grad_loss`` = the upstream gradient
    of the loss (device float32 [1], read on the device) and ``grad_p`` = one contiguous float32 tensor of the shape of p[l] per layer,
    EVERY element of which is written.  ``workspace`` as for loss_fwd; nothing a forward call left in it is used."""
    _need_cuda(targets, class_weight, workspace, grad_loss, *p, *grad_p)
    nt = _loss_targets(targets)
    bs = _loss_heads(p, geom, nc, class_weight)
    if _loss_heads(grad_p, geom, nc, None, "gradient") != bs:
        raise RuntimeError("loss: the gradient tensors must have the shapes of the head tensors")
    if grad_loss.dtype != torch.float32 or grad_loss.numel() != 1:
        raise RuntimeError("loss: grad_loss must be a float32 tensor of one element")
    nl, na, ny, nx, av = _loss_geometry(geom, anchor_vec)
    ptrs = (C.c_void_p * nl)(*[t.data_ptr() for t in p])
    gptrs = (C.c_void_p * nl)(*[t.data_ptr() for t in grad_p])
    check(load().yolo_loss_bwd(ptrs, _ptr(targets) if nt else None, nt, nl, na, ny, nx, av, bs, int(nc), float(iou_thresh),
                               (C.c_float * 4)(*[float(v) for v in gains]), _ptr(class_weight), _ptr(workspace),
                               workspace.numel() * workspace.element_size(), _ptr(grad_loss), gptrs, stream_ptr()), "loss_bwd")


COCO_T, COCO_R, COCO_A, COCO_M = 10, 101, 4, 3      # fixed counts of csrc/coco_eval.hip: IoU thresholds, recall thresholds, area ranges, maxDets


def coco_sweep_chunk() -> int:
    """Detections one step of the precision / recall sweep covers (kChunk of csrc/coco_eval.hip)."""
    return int(load().yolo_coco_sweep_chunk())


def coco_max_gt() -> int:
    """Cap on the GTs of one (image, category) group."""
    return int(load().yolo_coco_max_gt())


def coco_workspace_bytes(n_dt) -> int:
    n = int(load().yolo_coco_workspace_bytes(int(n_dt)))
    if n == 0:
        check(-1, "coco_workspace_bytes")
    return n


def _coco_typed(what, t, dtype, numel):
    if t.dtype != dtype or t.numel() != numel or not t.is_contiguous():
        raise RuntimeError(f"coco: {what} must be contiguous {dtype} with {numel} elements, not {t.dtype} {tuple(t.shape)}")


def coco_match_fwd(dt_box, dt_off, gt_box, gt_area, gt_crowd, gt_off, n_img, n_cat, max_gt, iou_thrs, area_rng, dt_match, dt_ignore,
                   npig, iou_sum, iou_cnt, status, workspace):
    """IoU and greedy matching (yolo_coco_match_fwd).  dt_box f64 [nD, 4] in evaluation order inside each (image, category) group,
    gt_box f64 [nG, 4], gt_area f64 [nG], gt_crowd u8 [nG], dt_off / gt_off int32 [n_img * n_cat + 1]; writes dt_match / dt_ignore
    int64 [nD] (bit a * 10 + t), npig int32 [n_cat, 4], iou_sum f64 / iou_cnt int32 [n_img * n_cat], status int32 [1]."""
    _need_cuda(dt_box, dt_off, gt_box, gt_area, gt_crowd, gt_off, iou_thrs, area_rng, dt_match, dt_ignore, npig, iou_sum, iou_cnt, status,
               workspace)
    n_dt, n_gt, ng = dt_box.shape[0], gt_box.shape[0], int(n_img) * int(n_cat)
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    for what, t, dtype, numel in (("dt_box", dt_box, f64, n_dt * 4), ("dt_off", dt_off, i32, ng + 1), ("gt_box", gt_box, f64, n_gt * 4),
                                  ("gt_area", gt_area, f64, n_gt), ("gt_crowd", gt_crowd, torch.uint8, n_gt), ("gt_off", gt_off, i32, ng + 1),
                                  ("iou_thrs", iou_thrs, f64, COCO_T), ("area_rng", area_rng, f64, COCO_A * 2),
                                  ("dt_match", dt_match, i64, n_dt), ("dt_ignore", dt_ignore, i64, n_dt), ("npig", npig, i32, n_cat * COCO_A),
                                  ("iou_sum", iou_sum, f64, ng), ("iou_cnt", iou_cnt, i32, ng), ("status", status, i32, 1)):
        _coco_typed(what, t, dtype, numel)
    check(load().yolo_coco_match_fwd(_ptr(dt_box), _ptr(dt_off), n_dt, _ptr(gt_box), _ptr(gt_area), _ptr(gt_crowd), _ptr(gt_off), n_gt,
                                     int(n_img), int(n_cat), int(max_gt), _ptr(iou_thrs), _ptr(area_rng), _ptr(dt_match), _ptr(dt_ignore),
                                     _ptr(npig), _ptr(iou_sum), _ptr(iou_cnt), _ptr(status), _ptr(workspace),
                                     workspace.numel() * workspace.element_size(), stream_ptr()), "coco_match")


def coco_accumulate_fwd(order, cat_off, n_cat, dt_match, dt_ignore, npig, rec_thrs, max_dets, eps, workspace, precision, recall):
    """Precision / recall sweep (yolo_coco_accumulate_fwd) over the flags coco_match_fwd wrote (same workspace).  order int32 [nD]:
    detection indices category by category (cat_off int32 [n_cat + 1]), descending score inside; writes precision f64
    [10, 101, n_cat, 4, 3] and recall f64 [10, n_cat, 4, 3]."""
    _need_cuda(order, cat_off, dt_match, dt_ignore, npig, rec_thrs, workspace, precision, recall)
    n_dt = order.numel()
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    for what, t, dtype, numel in (("order", order, i32, n_dt), ("cat_off", cat_off, i32, n_cat + 1), ("dt_match", dt_match, i64, n_dt),
                                  ("dt_ignore", dt_ignore, i64, n_dt), ("npig", npig, i32, n_cat * COCO_A), ("rec_thrs", rec_thrs, f64, COCO_R),
                                  ("precision", precision, f64, COCO_T * COCO_R * n_cat * COCO_A * COCO_M),
                                  ("recall", recall, f64, COCO_T * n_cat * COCO_A * COCO_M)):
        _coco_typed(what, t, dtype, numel)
    md = (C.c_int32 * COCO_M)(*[int(v) for v in max_dets])
    check(load().yolo_coco_accumulate_fwd(_ptr(order), _ptr(cat_off), n_dt, int(n_cat), _ptr(dt_match), _ptr(dt_ignore), _ptr(npig),
                                          _ptr(rec_thrs), md, float(eps), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                          _ptr(precision), _ptr(recall), stream_ptr()), "coco_accumulate")


def nms_compact_workspace_bytes(bs, rows, nc) -> int:
    return int(load().yolo_nms_compact_workspace_bytes(bs, rows, nc))


def head_decode_filter(x, w_packed, bias, desc: YoloConvDesc, anchors_px, nc, stride_px, rows_total, io_row_offset, conf_thres,
                       workspace, *, min_wh=2.0, p=None):
    """Head conv + decode + NMS row filter in one launch (yolo_head_decode_filter_fwd): survivors go to ``workspace``."""
    _need_cuda(x, w_packed, bias, workspace, p)
    na = len(anchors_px)
    flat = (C.c_float * (2 * na))(*[float(v) for a in anchors_px for v in a])
    check(load().yolo_head_decode_filter_fwd(_ptr(x), _ptr(w_packed), _ptr(bias), C.byref(desc), flat, na, nc, float(stride_px),
                                             rows_total, io_row_offset, float(conf_thres), float(min_wh), _ptr(workspace),
                                             workspace.numel() * workspace.element_size(), _ptr(p), stream_ptr()), "head_decode_filter")


def nms_merge_compact(workspace, bs, rows, nc, nms_thres, out_dets, out_idx, out_count, *, max_per_class=100):
    """Sort / MERGE / final order over the survivors the head epilogues left in ``workspace`` (yolo_nms_merge_compact)."""
    _need_cuda(workspace, out_dets, out_idx, out_count)
    cap = out_dets.shape[1]
    if tuple(out_dets.shape) != (bs, cap, 7) or tuple(out_idx.shape) != (bs, cap) or out_count.numel() != bs:
        raise RuntimeError("nms: output shape mismatch")
    if out_dets.dtype != torch.float32 or out_idx.dtype != torch.int32 or out_count.dtype != torch.int32:
        raise RuntimeError("nms: output dtype mismatch")
    check(load().yolo_nms_merge_compact(_ptr(workspace), workspace.numel() * workspace.element_size(), bs, rows, nc, float(nms_thres),
                                        int(max_per_class), _ptr(out_dets), _ptr(out_idx), _ptr(out_count), cap, stream_ptr()),
          "nms_merge_compact")


def nms_styled_compact(workspace, bs, rows, nc, nms_thres, out_dets, out_idx, out_count, *, style=_lib.NMS_MERGE, max_per_class=100):
    """``nms_merge_compact`` with the suppression style as an argument (yolo_nms_styled_compact; ``style`` = a _lib.NMS_* value)."""
    _need_cuda(workspace, out_dets, out_idx, out_count)
    cap = out_dets.shape[1]
    if tuple(out_dets.shape) != (bs, cap, 7) or tuple(out_idx.shape) != (bs, cap) or out_count.numel() != bs:
        raise RuntimeError("nms: output shape mismatch")
    if out_dets.dtype != torch.float32 or out_idx.dtype != torch.int32 or out_count.dtype != torch.int32:
        raise RuntimeError("nms: output dtype mismatch")
    check(load().yolo_nms_styled_compact(_ptr(workspace), workspace.numel() * workspace.element_size(), bs, rows, nc, float(nms_thres),
                                         int(max_per_class), _ptr(out_dets), _ptr(out_idx), _ptr(out_count), cap, int(style),
                                         stream_ptr()), "nms_styled_compact")


def cu_masked_stream(cu_bits, device):
    """A torch stream (ExternalStream over hipExtStreamCreateWithCUMask) whose kernels run only on the listed CU
    indices (CU i sits on XCD i % 8).  The HIP stream lives as long as the process: it is never destroyed behind torch."""
    cu_bits = list(cu_bits)
    if not cu_bits or min(cu_bits) < 0:
        raise RuntimeError("cu_masked_stream: empty or negative CU list")
    n_words = (max(cu_bits) + 32) // 32
    words = (C.c_uint32 * n_words)()
    for b in cu_bits:
        words[b // 32] |= 1 << (b % 32)
    out = C.c_void_p()
    with torch.cuda.device(device):
        check(load().yolo_stream_create_cu_mask(words, n_words, C.byref(out)), "stream_create_cu_mask")
    return torch.cuda.ExternalStream(out.value, device=device)


def set_launch_cus(n_cu: int) -> int:
    """CUs the coming launches of this thread may use (tile rules size grids against it); returns the previous value."""
    old = load().yolo_set_launch_cus(int(n_cu))
    if old < 0:
        check(old, "set_launch_cus")
    return old


class Event:
    """A HIP event owned by this library's C side (yolo_event_*): no timing, recorded / waited for by yolo_pipeline_step."""

    def __init__(self):
        h = C.c_void_p()
        check(load().yolo_event_create(C.byref(h)), "event_create")
        self.handle = h.value

    def record(self, stream: int = None):
        check(load().yolo_event_record(self.handle, stream_ptr() if stream is None else stream), "event_record")

    def synchronize(self):
        check(load().yolo_event_synchronize(self.handle), "event_synchronize")      # (ctypes releases the GIL while it waits)

    def __del__(self):
        try:
            load().yolo_event_destroy(self.handle)
        except Exception:                                   # noqa: BLE001 (interpreter teardown)
            pass


def pipeline_step(step):
    check(load().yolo_pipeline_step(C.byref(step)), "pipeline_step")


def pack_detections(dets, idx, count, packed, packed_idx=None):
    """Kept rows of all images back to back (yolo_pack_detections): dets [bs, cap, 7], count int32 [bs] on the device -> packed
    [total, 7] (+ packed_idx int64 [total] from idx int32 [bs, cap])."""
    _need_cuda(dets, count, packed, idx, packed_idx)
    bs, cap = dets.shape[0], dets.shape[1]
    check(load().yolo_pack_detections(_ptr(dets), _ptr(idx), _ptr(count), bs, cap, _ptr(packed), _ptr(packed_idx), stream_ptr()),
          "pack_detections")
    return packed


def run_ops(op_array, n_ops: int):
    check(load().yolo_run_ops(op_array, n_ops, stream_ptr()), "run_ops")
