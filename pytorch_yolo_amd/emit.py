"""Emission: the planner's ``Launch`` records become the ``YoloOp`` array ``yolo_run_ops`` walks; and the FLOP / byte
accounting over such an array.

One emitter per launch kind (``EMITTERS``), each returning the op(s) of one launch; ``build_ops`` is the loop over the records
for every precision (fp32: the same emitters with the fp32 packing and op kinds, max pools instead of the SPP kernel; fp16: the
fp16 packing and op kinds, the SPP kernel itself - it orders 16-bit patterns -, no kernel for the depthwise / SE / shuffle layers;
its large 3x3 layers go to the 20x20-tile kernels)."""
from __future__ import annotations

import os

import torch

from . import diag
from . import kernels as K
from ._lib import (ACT_LEAKY01, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH, DT_BF16, DT_F16, DT_F32, OP_SE, OP_CONV, OP_CONV1_NCHW, OP_CONV_F16, OP_CONV_T20_F16,
                   OP_CONV_F32, OP_DWCONV, OP_DWCONV_F32, OP_SE_F32, OP_SHUFFLE_F32, OP_CONV1_POOL, OP_CONV_POOL, OP_HEAD_DECODE_F16, OP_MAXPOOL_F16, OP_MAXPOOL_F32, OP_MBCONV,
                   OP_SHUFFLE, OP_HEAD_DECODE, OP_MAXPOOL, OP_RESUNIT, OP_SPP, OP_STEM, YoloOp)

_ACT = {"leaky": ACT_LEAKY01, "relu6": ACT_RELU6, "relu": ACT_RELU, "none": ACT_NONE, "swish": ACT_SWISH}


def _ptr(s):
    return s.buf.tensor.data_ptr()


def _in_view(d, x):
    d.n, d.h, d.w, d.cin, d.in_c_total, d.in_c_offset = x.n, x.h, x.w, x.c, x.buf.c_total, x.c_offset


def _out_view(d, y):
    d.ho, d.wo, d.out_c_total, d.out_c_offset = y.h, y.w, y.buf.c_total, y.c_offset


def _slice_of(s):
    """(c_total, c_offset) of an optional residual / pre-add tensor."""
    return (s.buf.c_total, s.c_offset) if s is not None else (0, 0)


def _keep(plan, *tensors):
    """Packed weights / biases go to the device and stay alive with the plan; returns their device pointers."""
    return tuple(None if t is None else plan._dev(t).data_ptr() for t in tensors)


def _op(kind, **fields):
    op = YoloOp()
    op.kind = kind
    for name, value in fields.items():
        setattr(op, name, value)
    return op


def _emit_stem(plan, L):
    nd1, nd, y = L.pre[0], L.node, L.dst
    mid = nd.srcs[0]
    w1p, b1p, kpad1, _ = K.pack_conv_weight(*nd1.attrs["weight"], 8)
    w2p, b2p, kpad2, cout_pad2 = K.pack_conv_weight(*nd.attrs["weight"], 32)
    op = _op(OP_STEM, x=None, y=_ptr(y), kpad_pre=kpad1)
    op.w_pre, op.bias_pre, op.w, op.bias = _keep(plan, w1p, b1p, w2p, b2p)
    op.conv = K.conv_desc(n=mid.n, h=mid.h, w=mid.w, cin=32, in_c_total=32, in_c_offset=0, cout=64,
                          out_c_total=y.buf.c_total, out_c_offset=y.c_offset, ksize=3, stride=2,
                          act=_ACT[nd.attrs["act"]], kpad=kpad2, cout_pad=cout_pad2)
    op.conv.res_c_total = plan.rec.c_in            # real input channels
    return [op]


def _emit_head(plan, L):
    nd, x = L.node, L.src
    hd = next(h for h in plan.heads if h["sym"] is nd.outs[0])
    w, b = nd.attrs["weight"]
    wp, bp, kpad, cout_pad = (K.pack_conv_weight_f16 if plan.f16 else K.pack_conv_weight)(w, b, x.c)
    op = _op(OP_HEAD_DECODE_F16 if plan.f16 else OP_HEAD_DECODE, x=_ptr(x), y=None, y_aux=None)                     # io / p of the call: bound in _bind_outputs
    op.w, op.bias = _keep(plan, wp, bp)
    op.conv = K.conv_desc(n=x.n, h=x.h, w=x.w, cin=x.c, in_c_total=x.buf.c_total, in_c_offset=x.c_offset,
                          cout=w.shape[0], out_c_total=K.roundup(w.shape[0], 8), out_c_offset=0,
                          ksize=w.shape[2], stride=1, act=_ACT[nd.attrs["act"]], kpad=kpad,
                          cout_pad=cout_pad, out_dtype=DT_F32)
    for i, (aw, ah) in enumerate(hd["anchors"]):
        op.head_anchors_px[2 * i], op.head_anchors_px[2 * i + 1] = float(aw), float(ah)
    op.head_stride_px, op.head_na, op.head_nc = float(hd["stride"]), hd["na"], plan.n_class
    op.io_rows_total, op.io_row_offset = plan.rows_total, hd["row"]
    hd["op"] = op                               # (build_ops turns it into the op's index once the list is final)
    return [op]


def _emit_mbconv(plan, L):
    nd, dwn, x, y = L.node, L.pre[-1], L.src, L.dst
    we_b = L.pre[0].attrs["weight"] if len(L.pre) == 2 else (None, None)              # (expand, depthwise) or (depthwise,)
    packed = K.pack_mbconv(we_b[0], we_b[1], *dwn.attrs["weight"], *nd.attrs["weight"], stride=dwn.attrs["stride"])
    op = _op(OP_MBCONV, x=_ptr(x), y=_ptr(y), kpad_pre=dwn.srcs[0].c)                 # kpad_pre: hidden channels
    op.w_pre, op.bias_pre, op.w_dw, op.bias_dw, op.w, op.bias = _keep(plan, *packed)
    d = op.conv
    _in_view(d, x)
    _out_view(d, y)
    d.cout, d.ksize, d.stride, d.res_c_total = y.c, 3, dwn.attrs["stride"], 1 if nd.attrs["has_res"] else 0
    return [op]


def _emit_resunit(plan, L):
    nd, pa, x, y = L.node, L.pre[0], L.src, L.dst
    mid = nd.srcs[0]
    aux = nd.outs[1] if len(nd.outs) > 1 else None
    w1p, b1p, kpad1, cout_pad1 = K.pack_conv_weight(*pa.attrs["weight"], x.c)
    w2p, b2p, kpad2, cout_pad2 = K.pack_conv_weight(*nd.attrs["weight"], mid.c)
    op = _op(OP_RESUNIT, x=_ptr(x), y=_ptr(y), y_aux=_ptr(aux) if aux is not None else None, kpad_pre=kpad1, cout_pad_pre=cout_pad1)
    op.w_pre, op.bias_pre, op.w, op.bias = _keep(plan, w1p, b1p, w2p, b2p)
    op.conv = K.conv_desc(n=x.n, h=x.h, w=x.w, cin=mid.c, in_c_total=x.buf.c_total, in_c_offset=x.c_offset,
                          cout=x.c, out_c_total=y.buf.c_total, out_c_offset=y.c_offset, ksize=3, stride=1,
                          act=_ACT[nd.attrs["act"]], kpad=kpad2, cout_pad=cout_pad2, aux=_slice_of(aux))
    return [op]


def _emit_conv(plan, L):
    """The plain conv of either precision with its epilogue options (upsampling store, residual, pre-add copy) and, bf16 only,
    the NCHW-reading / pooling / split-K forms.  fp16: the layers the shipped rule of the 20x20-tile 3x3 kernels takes
    (yolo_conv3x3_t20_f16_supported, asked here, once, with the CUs of the whole chip) become OP_CONV_T20_F16 - same fields, same
    buffers; YOLO_FP16_T20=0 (read when the plan is built) keeps every layer in the gather kernel for A/B runs."""
    nd, x, dst = L.node, L.src, L.dst
    y = nd.outs[0]
    w, b = nd.attrs["weight"]
    pack, plain = (K.pack_conv_weight_f32, OP_CONV_F32) if plan.f32 else (K.pack_conv_weight, OP_CONV)
    if plan.f16:
        pack, plain = K.pack_conv_weight_f16, OP_CONV_F16
    wp, bp, kpad, cout_pad = pack(w, b, x.c)
    res = nd.srcs[1] if nd.attrs["has_res"] else None
    aux = nd.outs[1] if len(nd.outs) > 1 else None
    d = K.conv_desc(n=x.n, h=x.h, w=x.w, cin=x.c, in_c_total=x.buf.c_total if x.buf is not None else x.c, in_c_offset=x.c_offset,
                    cout=w.shape[0], out_c_total=dst.buf.c_total, out_c_offset=dst.c_offset,
                    ksize=w.shape[2], stride=nd.attrs["stride"], act=_ACT[nd.attrs["act"]],
                    kpad=kpad, cout_pad=cout_pad, upsample2x=1 if L.up else 0,
                    out_dtype=DT_F32 if (plan.f32 or y.f32) else (DT_F16 if plan.f16 else DT_BF16), pad=nd.attrs.get("pad"),
                    res=_slice_of(res), aux=_slice_of(aux))
    if not L.up and not L.pooled:
        d.ho, d.wo = y.h, y.w                  # (tf_same convs: one more row / column than the symmetric-pad formula)
    if L.reads_nchw:
        kind = OP_CONV1_POOL if L.pooled else OP_CONV1_NCHW
        d.res_c_total = plan.rec.c_in          # real input channels (x pointer is patched per call)
    else:
        kind = OP_CONV_POOL if L.pooled else plain
        if kind == OP_CONV_F16 and os.environ.get("YOLO_FP16_T20", "1") != "0" and K.conv3x3_t20_f16_supported(d, res is not None, aux is not None):
            kind = OP_CONV_T20_F16
    op = _op(kind, x=None if L.reads_nchw else _ptr(x), y=_ptr(dst), residual=_ptr(res) if res is not None else None,
             y_aux=_ptr(aux) if aux is not None else None, conv=d)
    op.w, op.bias = _keep(plan, wp, bp)
    # split-K launches are OFF by default: correct and deterministic (tests), but on MI355X the cross-XCD exchange
    # of the fp32 partials (agent-scope accesses that bypass the per-XCD L2) costs more than the idle CUs it
    # fills: 0.041 -> 0.13 ms on YOLOv3-tiny's 3x3 256 -> 512 layer at 13x13 x 32
    if kind == OP_CONV and os.environ.get("YOLO_SPLITK", "0") == "1":
        sp, wb, _ = K.conv2d_splitk_plan(d, res is not None, aux is not None)
        if sp >= 2:                            # few pixels, long K: split-K launch (yolo_conv2d_splitk_fwd); workspace: build_ops
            op.splits, op.ws_bytes = sp, wb
    return [op]


def _emit_dwconv(plan, L):
    nd, x, y = L.node, L.src, L.dst
    w, b = nd.attrs["weight"]
    kk = w.shape[2] * w.shape[3]
    op = _op(OP_DWCONV_F32 if plan.f32 else OP_DWCONV, x=_ptr(x), y=_ptr(y))
    op.w, op.bias = _keep(plan, w.detach().float().reshape(x.c, kk).t().contiguous(), b.detach().float().contiguous())
    d = op.conv
    _in_view(d, x)
    _out_view(d, y)
    d.stride, d.act = nd.attrs["stride"], _ACT[nd.attrs["act"]]
    d.ksize, d.pad = nd.attrs.get("ksize", 0), nd.attrs.get("pad", 0)      # ksize 0: the 3x3 / pad 1 strip kernel
    if plan.f32:                                                           # one fp32 kernel: the torch-style layers are k 3 / pad 1
        d.ksize, d.pad = nd.attrs.get("ksize", 3), nd.attrs.get("pad", 1)
    return [op]


def _emit_se(plan, L):
    nd, x, y = L.node, L.src, L.dst
    sq = nd.attrs["w1"].shape[0]
    f = lambda t: t.detach().float()
    ws_bytes = K.se_workspace_bytes(x.n, x.c) // 4 * 4
    op = _op(OP_SE_F32 if plan.f32 else OP_SE, x=_ptr(x), y=_ptr(y), kpad_pre=sq, ws_bytes=ws_bytes)
    op.w, op.w_pre, op.bias, op.bias_pre, op.workspace = _keep(plan, f(nd.attrs["w1"]).reshape(sq, x.c).contiguous(),
                               f(nd.attrs["w2"]).reshape(x.c, sq).t().contiguous(),    # [sq][c]
                               f(nd.attrs["b1"]).contiguous(), f(nd.attrs["b2"]).contiguous(),
                               torch.zeros(ws_bytes // 4, dtype=torch.float32))
    _in_view(op.conv, x)
    _out_view(op.conv, y)
    return [op]


def _emit_shuffle(plan, L):
    nd, y = L.node, L.dst
    a_, b_ = nd.srcs
    op = _op(OP_SHUFFLE_F32 if plan.f32 else OP_SHUFFLE, x=_ptr(a_), residual=_ptr(b_), y=_ptr(y))
    d = op.conv
    _in_view(d, a_)                                                         # cin = physical channels per slot
    d.res_c_total, d.res_c_offset = b_.buf.c_total, b_.c_offset
    d.out_c_total, d.out_c_offset, d.cout = y.buf.c_total, y.c_offset, nd.attrs["half"]   # cout = logical half
    return [op]


def _maxpool(kind, x, y, size, stride, pad, dil, out_c_offset):
    op = _op(kind, x=_ptr(x), y=_ptr(y))
    d = op.conv
    _in_view(d, x)
    _out_view(d, y)
    d.out_c_offset = out_c_offset
    d.ksize, d.stride, d.pad, d.upsample2x = size, stride, pad, dil        # (upsample2x carries the dilation)
    return op


def _emit_pool(plan, L):
    a = L.node.attrs
    return [_maxpool(OP_MAXPOOL_F32 if plan.f32 else (OP_MAXPOOL_F16 if plan.f16 else OP_MAXPOOL), L.src, L.dst, a["size"], a["stride"], a["pad"], a["dil"], L.dst.c_offset)]


def _emit_spp(plan, L):
    x, y = L.src, L.dst
    if plan.f32:      # cat([p5, p9, p13, x]) (yolov3_spp.py:129) as three pool launches: x already sits in slice [3c, 4c)
        return [_maxpool(OP_MAXPOOL_F32, x, y, k, 1, k // 2, 1, y.c_offset + lvl * x.c) for lvl, k in enumerate((5, 9, 13))]
    op = _op(OP_SPP, y=_ptr(y))
    op.conv.n, op.conv.h, op.conv.w, op.conv.cin = x.n, x.h, x.w, x.c
    return [op]


EMITTERS = {"conv": _emit_conv, "stem": _emit_stem, "resunit": _emit_resunit, "mbconv": _emit_mbconv, "head": _emit_head,
            "dwconv": _emit_dwconv, "se": _emit_se, "shuffle": _emit_shuffle, "pool": _emit_pool, "spp": _emit_spp}


def build_ops(plan):
    """``plan.launches`` -> ``plan.op_array`` (+ ``n_ops``, and per op its ``op_launches`` record and ``op_nodes`` node), the
    head table ``plan.heads`` / ``rows_total`` and the split-K workspace."""
    # heads: io row ranges in the order the model declares them (yolov3_spp.py:156-164)
    plan.heads = []
    row = 0
    for x, layer in plan.rec.heads:
        na = len(layer.anchors_px)
        stride = plan.img_size / max(x.w, x.h)          # yolo_layer.py:102 (python float)
        plan.heads.append(dict(sym=x, anchors=layer.anchors_px, stride=stride, row=row, na=na, layer=layer, op=None))
        row += na * x.h * x.w
    plan.rows_total = row
    ops, op_launches = [], []
    for L in plan.launches:
        if plan.f16 and L.kind in ("dwconv", "shuffle", "se"):
            raise NotImplementedError(f"precision='fp16' covers the Darknet families (YOLOv3-SPP / -tiny / YOLOv3 / Lite); "
                                      f"no fp16 kernel for '{L.kind}' layers (precision='fp32' and 'bf16' run them)")
        assert not (L.reads_nchw and ops)               # feed() patches op 0's x with the caller's batch
        for op in EMITTERS[L.kind](plan, L):
            ops.append(op); op_launches.append(L)
    ops, op_launches = diag.rewrite_list(plan, ops, op_launches)
    index = {id(op): i for i, op in enumerate(ops)}     # (the rewrites move the head and split-K ops, they never copy them)
    for hd in plan.heads:
        if hd["op"] is not None:
            hd["op"] = index[id(hd["op"])]
    splitk = [K.conv2d_splitk_plan(op.conv, bool(op.residual), bool(op.y_aux)) for op in ops if op.splits >= 2]
    if splitk:      # one fp32 workspace and one zeroed counter array per plan: the launches run in stream order
        plan._splitk_ws = torch.empty((max(wb for _, wb, _ in splitk) + 3) // 4, dtype=torch.float32, device=plan.device)
        plan._splitk_cnt = torch.zeros(max(nc for _, _, nc in splitk), dtype=torch.int32, device=plan.device)
        for op in ops:
            if op.splits >= 2:
                op.workspace, op.counters = plan._splitk_ws.data_ptr(), plan._splitk_cnt.data_ptr()
    plan.n_ops = len(ops)
    plan.op_launches = op_launches                      # the Launch each op comes from: .node the graph node, .dst the tensor it writes
    plan.op_nodes = [L.node for L in op_launches]
    plan.op_array = (YoloOp * len(ops))(*ops)


# -- accounting --------------------------------------------------------------------------------------
_CONVS = (OP_CONV, OP_CONV1_NCHW, OP_CONV1_POOL, OP_CONV_POOL, OP_HEAD_DECODE, OP_CONV_F32, OP_CONV_F16, OP_HEAD_DECODE_F16, OP_CONV_T20_F16)


def conv_flops(op_array, n_ops: int, c_in: int) -> float:
    """Exact algorithmic FLOPs of the conv launches of a list (2*M*Cout*K with logical sizes); ``c_in``: the model's real
    input channels."""
    total = 0.0
    first = True
    for i in range(n_ops):
        op = op_array[i]
        d = op.conv
        if op.kind in _CONVS:
            cin = c_in if first else d.cin               # the first layer's 3 -> 8 channel pad is not work
            first = False
            total += 2.0 * d.n * d.ho * d.wo * d.cout * d.ksize * d.ksize * cin
        elif op.kind == OP_STEM:                         # conv1 (real input channels) + the stride-2 conv
            first = False
            total += 2.0 * d.n * d.h * d.w * 32 * 9 * c_in + 2.0 * d.n * d.ho * d.wo * 64 * 9 * 32
        elif op.kind == OP_RESUNIT:                      # 1x1 C->C/2 plus 3x3 C/2->C (the halo recompute is not work)
            total += 2.0 * d.n * d.h * d.w * (d.cout * d.cin) * 10
        elif op.kind == OP_DWCONV:
            total += 2.0 * d.n * d.ho * d.wo * d.cin * 9
        elif op.kind == OP_DWCONV_F32:                   # (always carries the real kernel size)
            total += 2.0 * d.n * d.ho * d.wo * d.cin * d.ksize * d.ksize
        elif op.kind == OP_MBCONV:                       # expand at the input size, depthwise + projection at the output size
            hid = op.kpad_pre
            total += (2.0 * d.n * d.h * d.w * d.cin * hid if op.w_pre else 0.0) + 2.0 * d.n * d.ho * d.wo * hid * (9 + d.cout)
    return total


def algorithmic_bytes(op_array, n_ops: int, c_in: int, detect: bool = False) -> float:
    """HBM bytes one pass must move if every tensor that exists in HBM is read once and written once:
    per launch its input view, its output (x4 for a 2x2-replicated store, fp32 head rows + decoded rows for a fused head),
    the residual and the pre-add copy, and its weights.  Fused launches count only what crosses the chip boundary.
    ``detect=True``: the pass of ``detect()`` in the compact NMS form - a head writes one 8-byte key per row instead of p and io."""
    total = 0.0
    first = True
    for i in range(n_ops):
        op = op_array[i]
        d = op.conv
        m_in, m_out = d.n * d.h * d.w, d.n * d.ho * d.wo
        if op.kind in _CONVS:
            x_b = m_in * (c_in * 4 if (first and op.kind in (OP_CONV1_NCHW, OP_CONV1_POOL)) else d.cin * (4 if op.kind == OP_CONV_F32 else 2))
            first = False
            pooled = 4 if op.kind in (OP_CONV1_POOL, OP_CONV_POOL) else 1       # only the 2x2-pooled map is written
            y_b = m_out * d.cout * (4 if d.out_dtype == DT_F32 else 2) * (4 if d.upsample2x else 1) / pooled
            if op.kind in (OP_HEAD_DECODE, OP_HEAD_DECODE_F16):
                y_b = 2.0 * m_out * d.cout * 4                                   # p (raw) + io (decoded), fp32
                if detect:
                    y_b = m_out * op.head_na * 8.0                               # one sort key per (pixel, anchor) row
            total += x_b + y_b + d.cout * d.ksize * d.ksize * d.cin * 2
            total += (m_out * d.cout * 2 if op.residual else 0) + (m_out * d.cout * 2 if op.y_aux else 0)
        elif op.kind == OP_STEM:
            first = False
            total += m_in * c_in * 4 + m_out * 64 * 2
        elif op.kind == OP_RESUNIT:
            total += m_in * d.cout * 2 * (3 if op.y_aux else 2)
        elif op.kind == OP_MBCONV:
            total += m_in * d.cin * 2 + m_out * d.cout * 2
        elif op.kind in (OP_MAXPOOL, OP_DWCONV, OP_MAXPOOL_F32, OP_MAXPOOL_F16, OP_DWCONV_F32):
            total += (m_in + m_out) * d.cin * (4 if op.kind in (OP_MAXPOOL_F32, OP_DWCONV_F32) else 2)
        elif op.kind in (OP_SE, OP_SE_F32):
            total += 3.0 * m_in * d.cin * (4 if op.kind == OP_SE_F32 else 2)     # pooled once, read again for the rescale, written
        elif op.kind == OP_SPP:
            total += m_in * d.cin * 2 * 4                                        # reads c, writes the three pooled copies
        elif op.kind in (OP_SHUFFLE, OP_SHUFFLE_F32):
            total += 2.0 * m_in * d.cin * (4 if op.kind == OP_SHUFFLE_F32 else 2)
    return total
