"""Planner passes over a recorded graph: fuse (which nodes become which launch), place (which tensor lives where), allocate.

``fuse`` runs the fusion rules of ``RULES`` - one matcher per rule, the table's order is the priority - and returns one
``Launch`` per launch, in node order.  ``place`` gives every tensor that exists in HBM a buffer (concat / SPP slices, upsample
targets, in-place residual adds, views), ``alloc`` the storage, shared between buffers whose live ranges do not overlap.
None of them writes to ``Node.attrs``.  To add a fusion: write a matcher, give it a line in ``RULES`` and, if it launches a new
kernel, an emitter in emit.py."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import kernels as K
from .graph import Buf, Node, Recorder, Sym

# which residual-unit widths run as ONE launch (bit mask of C: 64 | 128 | 256); see DESIGN.md §3.3 for the
# measurements behind the default (round 3, three interleaved rounds on one box, images/s: 64 -> 6,180; 64 | 128 -> 6,222;
# 64 | 128 | 256 -> 6,022: profiles/r03_fuse_resunit_ab.txt).  YOLO_FUSE_RESUNIT overrides it (tuning only).
FUSE_RESUNIT_DEFAULT = 64 | 128

NO_LAUNCH = ("input", "up", "cat", "slice", "head")          # node kinds that never launch: glue the placement resolves


@dataclass(eq=False)
class Launch:
    """One launch of the list: the node whose place in the list it takes, the nodes it swallowed, what it reads and writes."""
    kind: str                          # conv | stem | resunit | mbconv | head | dwconv | se | shuffle | pool | spp
    node: Node
    pre: tuple = ()                    # swallowed nodes: conv1 of the stem, the 1x1 of a unit, (expand,) depthwise of a block, the pool, the upsample
    src: Optional[Sym] = None          # what it reads (the fused forms: the first swallowed node's input)
    dst: Optional[Sym] = None          # what it really writes: the plain, upsampled or pooled output (None: a head's rows of io)
    up: bool = False                   # conv: stores every pixel 2x2 (the Upsample behind it)
    pooled: bool = False               # conv: stores the MaxPool2d(2, 2) of its output only
    reads_nchw: bool = False           # reads the caller's float32 NCHW batch itself (its x is patched per call)
    layer: object = None               # head: the YOLOLayer it decodes for


# -- fusion rules ------------------------------------------------------------------------------------
class _Fusion:
    """What the rules may look at besides the graph; the planner's env knobs are read here and nowhere else.  ``f32`` (the
    reference-precision mode) keeps the epilogue options - upsample here; concat and residual placement - and fuses nothing else.
    ``f16`` (the fp16-operand mode) does the same, except that the head fusion stays on: it lives in the gather kernel, the one
    kernel family with an fp16 form - the fused stem / units / blocks / pools and the NCHW-reading first layers are bf16-only."""

    def __init__(self, rec: Recorder, f32: bool, n_class: int, f16: bool = False):
        env = os.environ.get
        self.rec, self.n_class = rec, n_class
        plain = f32 or f16
        self.resunit_mask = 0 if plain else int(env("YOLO_FUSE_RESUNIT", str(FUSE_RESUNIT_DEFAULT)))
        # "1" all covered blocks, "narrow" only those of csrc/conv_mbconv.hip (hidden <= 192), "0" none
        self.mbconv = "0" if plain else env("YOLO_FUSE_MBCONV", "1")
        self.pool, self.stem, self.conv1_s2 = (not plain and env(k, "1") == "1" for k in (
            "YOLO_FUSE_POOL", "YOLO_FUSE_STEM", "YOLO_FUSE_CONV1_S2"))
        self.head = not f32 and env("YOLO_FUSE_HEAD", "1") == "1"
        self.nchw = not plain


def _ksize(nd):
    return nd.attrs["weight"][0].shape[2]


def _only_consumer(s: Sym, kind: str):
    """The node of ``kind`` that is the one consumer of ``s`` (so ``s`` is no concat / SPP input and nobody else needs it in
    HBM), or None."""
    return s.consumers[0] if len(s.consumers) == 1 and s.consumers[0].kind == kind else None


def _pool_2x2(s: Sym):
    """The MaxPool2d(2, 2) node that alone consumes the even-sized ``s``, or None."""
    ndp = _only_consumer(s, "pool")
    if ndp is None or (ndp.attrs["size"], ndp.attrs["stride"], ndp.attrs["pad"], ndp.attrs["dil"]) != (2, 2, 0, 1) or s.h % 2 or s.w % 2:
        return None
    return ndp


def fuse_upsample(fz, nd):
    """conv -> Upsample(2): the conv stores the replicated pixels itself, into the upsample's output."""
    if nd.kind != "up":
        return None
    x = nd.srcs[0]
    if x.producer.kind != "conv" or len(x.consumers) != 1:
        raise RuntimeError("upsample must directly follow a conv with no other consumer")
    return Launch("conv", x.producer, pre=(nd,), src=x.producer.srcs[0], dst=nd.outs[0], up=True)


def fuse_resunit(fz, nd):
    """Darknet residual units (1x1 C->C/2, 3x3 C/2->C, add) on the large maps: one launch (yolo_resunit_fwd); the intermediate
    never leaves the chip and the output gets its own buffer (no in-place add there)."""
    if nd.kind != "conv" or not nd.attrs["has_res"]:
        return None
    mid, res = nd.srcs
    pa = mid.producer
    if pa is None or pa.kind != "conv" or pa.attrs["has_res"] or len(pa.outs) != 1 or len(mid.consumers) != 1:
        return None
    (w1, _), (w2, _) = pa.attrs["weight"], nd.attrs["weight"]
    c = res.c
    if (pa.srcs[0] is not res or w1.shape[2] != 1 or w2.shape[2] != 3 or nd.attrs["stride"] != 1 or pa.attrs["stride"] != 1
            or w2.shape[0] != c or w1.shape[0] * 2 != c or w1.shape[1] != c or pa.attrs["act"] != nd.attrs["act"] or nd.outs[0].f32):
        return None
    # (above 64 channels only where the 20-pixel-wide tile kernel takes the unit: the generic fused kernel is slower than two launches)
    if (fz.resunit_mask & c) and K.resunit_supported(c, res.h, res.w) and (c == 64 or K.resunit_form(c, res.n, res.h, res.w) == 3):
        return Launch("resunit", nd, pre=(pa,), src=res, dst=nd.outs[0])
    return None


def fuse_mbconv(fz, nd):
    """MobileNetV2 inverted-residual blocks ([1x1 expand + ReLU6,] depthwise 3x3 + ReLU6, linear 1x1 [+ x]) with few channels,
    i.e. the large maps: one launch (yolo_mbconv_fwd), the 6x-expanded tensor and the depthwise output never exist in HBM; the
    output gets its own buffer (neighbouring tiles read x)."""
    if (fz.mbconv == "0" or nd.kind != "conv" or len(nd.outs) != 1 or nd.outs[0].f32 or nd.attrs["act"] != "none"
            or nd.attrs["stride"] != 1 or _ksize(nd) != 1):
        return None
    dsym = nd.srcs[0]
    dwn = dsym.producer
    if dwn is None or dwn.kind != "dwconv" or dwn.attrs["act"] != "relu6" or len(dsym.consumers) != 1:
        return None
    esym = dwn.srcs[0]
    ex = esym.producer
    has_exp = (ex is not None and ex.kind == "conv" and _ksize(ex) == 1 and ex.attrs["act"] == "relu6" and ex.attrs["stride"] == 1
               and not ex.attrs["has_res"] and len(ex.outs) == 1 and len(esym.consumers) == 1 and not esym.f32)
    x = ex.srcs[0] if has_exp else esym
    if x is fz.rec.input or x.f32 or (nd.attrs["has_res"] and nd.srcs[1] is not x):
        return None
    form = K.mbconv_form(x.c, esym.c, nd.attrs["weight"][0].shape[0], dwn.attrs["stride"])
    if form == 1 or (form == 2 and has_exp and fz.mbconv != "narrow"):
        return Launch("mbconv", nd, pre=(ex, dwn) if has_exp else (dwn,), src=x, dst=nd.outs[0])
    return None


def fuse_conv_pool(fz, nd):
    """ConvPoolBlocks with few input channels (YOLOv3-tiny's second and third: 16 -> 32, 32 -> 64): conv + MaxPool2d(2, 2) in one
    launch (yolo_conv3x3_pool_fwd), the full-resolution conv output is never written."""
    if (not fz.pool or nd.kind != "conv" or nd.attrs["has_res"] or len(nd.outs) != 1 or nd.attrs["stride"] != 1
            or nd.srcs[0] is fz.rec.input):
        return None
    w, _ = nd.attrs["weight"]
    mid = nd.outs[0]
    ndp = _pool_2x2(mid)
    if w.shape[2] != 3 or mid.f32 or ndp is None or not K.conv3x3_pool_supported(w.shape[1], w.shape[0]):
        return None
    return Launch("conv", nd, pre=(ndp,), src=nd.srcs[0], dst=ndp.outs[0], pooled=True)


def _first_conv_stride(fz, nd):
    """The stride (1 or 2) of ``nd`` if it is the model's first layer in a shape whose kernel reads the caller's float32 NCHW batch
    itself (yolo_conv1_nchw_f32_fwd) - the NHWC bf16 copy of the input is then never made -, else 0.  (Its output may be a
    concat slice: every bf16 tensor is a multiple of 8 channels wide, so every slice starts where the kernel can store.)"""
    x = fz.rec.input
    if not fz.nchw or nd.kind != "conv" or nd.srcs[0] is not x or len(x.consumers) != 1 or fz.rec.c_in > 8:
        return 0
    cout, stride = nd.attrs["weight"][0].shape[0], nd.attrs["stride"]
    s1 = cout in (16, 32) and stride == 1
    s2 = cout == 32 and stride == 2 and fz.conv1_s2                                   # MobileNetV2
    ok = (s1 or s2) and _ksize(nd) == 3 and "pad" not in nd.attrs and not nd.attrs["has_res"] and len(nd.outs) == 1 and not nd.outs[0].f32
    return stride if ok else 0


def fuse_stem(fz, nd1):
    """Darknet stem: conv1 (3x3/s1 -> 32) followed only by a 3x3/s2 32 -> 64 conv becomes ONE launch (yolo_stem_fwd); the
    32-channel full-resolution intermediate is never materialised."""
    nd2 = _only_consumer(nd1.outs[0], "conv") if fz.stem and _first_conv_stride(fz, nd1) == 1 else None
    if (nd2 is None or tuple(nd2.attrs["weight"][0].shape) != (64, 32, 3, 3) or nd2.attrs["stride"] != 2 or nd2.attrs["has_res"]
            or len(nd2.outs) != 1 or nd2.outs[0].f32 or nd2.attrs["act"] != nd1.attrs["act"] or nd2.srcs[0] is not nd1.outs[0]):
        return None
    return Launch("stem", nd2, pre=(nd1,), src=nd1.srcs[0], dst=nd2.outs[0], reads_nchw=True)


def fuse_conv1_pool(fz, nd):
    """First ConvPoolBlock of YOLOv3-tiny: conv1 followed only by MaxPool2d(2, 2) becomes ONE launch
    (yolo_conv1_pool_nchw_f32_fwd); the full-resolution conv output is never written."""
    ndp = _pool_2x2(nd.outs[0]) if fz.pool and _first_conv_stride(fz, nd) == 1 else None
    return None if ndp is None else Launch("conv", nd, pre=(ndp,), src=nd.srcs[0], dst=ndp.outs[0], pooled=True, reads_nchw=True)


def fuse_conv1_nchw(fz, nd):
    """The first conv on its own reads the NCHW batch (stride 1, or MobileNetV2's stride 2)."""
    return Launch("conv", nd, src=nd.srcs[0], dst=nd.outs[0], reads_nchw=True) if _first_conv_stride(fz, nd) else None


def _head_layer(rec, nd):
    """The YOLOLayer fed by conv node ``nd`` (its f32 output goes to a head and nowhere else), or None."""
    if nd.kind != "conv" or not nd.outs[0].f32 or _only_consumer(nd.outs[0], "head") is None:
        return None
    return next((layer for x, layer in rec.heads if x is nd.outs[0]), None)


def fuse_head(fz, nd):
    """Detection heads: the head conv decodes in its epilogue (yolo_head_decode_fwd); no head tensor."""
    layer = _head_layer(fz.rec, nd) if fz.head else None
    if layer is None or nd.attrs["has_res"] or len(nd.outs) != 1 or nd.attrs["stride"] != 1:
        return None
    if not K.head_decode_supported(nd.attrs["weight"][0].shape[0], len(layer.anchors_px), fz.n_class):
        return None
    return Launch("head", nd, src=nd.srcs[0], layer=layer)


# The rules, most specific first.  Each is tried on every node; one that matches claims the launch's node and the nodes it
# swallows, and a rule whose match touches a node another rule has claimed does not fire - the order below is the priority.
RULES = (fuse_upsample,        # OP_CONV with the 2x2-replicating store
         fuse_resunit,         # OP_RESUNIT
         fuse_mbconv,          # OP_MBCONV
         fuse_conv_pool,       # OP_CONV_POOL
         fuse_stem,            # OP_STEM
         fuse_conv1_pool,      # OP_CONV1_POOL
         fuse_conv1_nchw,      # OP_CONV1_NCHW
         fuse_head)            # OP_HEAD_DECODE


def fuse(rec: Recorder, f32: bool, n_class: int, f16: bool = False) -> List[Launch]:
    """The launches of the graph in node order: what the rules claimed, and one plain launch for every other layer."""
    fz = _Fusion(rec, f32, n_class, f16)
    claimed = {}                                               # id(node) -> the Launch that took it
    for rule in RULES:
        for nd in rec.nodes:
            launch = rule(fz, nd)
            if launch is not None and not any(id(m) in claimed for m in (launch.node,) + launch.pre):
                claimed.update((id(m), launch) for m in (launch.node,) + launch.pre)
    launches = []
    for nd in rec.nodes:
        launch = claimed.get(id(nd))
        if launch is None and nd.kind not in NO_LAUNCH:
            launch = Launch(nd.kind, nd, src=nd.srcs[0], dst=nd.outs[0])
        if launch is not None and launch.node is nd:
            launches.append(launch)
    return launches


# -- placement ---------------------------------------------------------------------------------------
def place(rec: Recorder, launches: List[Launch]) -> List[Buf]:
    """Fill ``Sym.buf`` / ``Sym.c_offset`` of every tensor that exists in HBM; returns the buffers in creation order (which
    ``alloc`` keeps for buffers first touched by the same node).  Tensors inside a fused launch and the input a first layer
    reads as NCHW get none."""
    nodes = rec.nodes
    order = {id(nd): i for i, nd in enumerate(nodes)}
    by_node = {id(L.node): L for L in launches}
    swallowed = {id(m) for L in launches for m in L.pre}
    bufs = []

    def own_buf(s: Sym):
        s.buf, s.c_offset = Buf(s.n, s.h, s.w, s.c, f32=s.f32), 0
        bufs.append(s.buf)

    # 1. concat / spp outputs own a buffer; their inputs are placed into slices of it
    for nd in nodes:
        if nd.kind == "cat":
            y = nd.outs[0]
            if y.buf is None:
                own_buf(y)
            off = y.c_offset
            for x in nd.srcs:
                if x.buf is not None:
                    raise RuntimeError("a tensor feeds two concats: needs a copy (not required by any model here)")
                x.buf, x.c_offset = y.buf, off
                off += x.c
        elif nd.kind == "spp":
            y, x = nd.outs[0], nd.srcs[0]
            if y.buf is None:
                own_buf(y)
            if y.c_offset != 0 or y.buf.c_total != y.c:
                raise RuntimeError("spp output must own its buffer")
            if x.buf is not None:
                raise RuntimeError("spp input already placed")
            x.buf, x.c_offset = y.buf, 3 * x.c
    # 2. upsample outputs (the producing conv stores into them)
    for nd in nodes:
        if nd.kind == "up" and nd.outs[0].buf is None:
            own_buf(nd.outs[0])
    # 3. residual adds are written in place of the residual input when it is dead afterwards
    in_place = []                                              # ... which may get its own buffer only in step 4: resolved last
    for L in launches:
        nd = L.node
        if L.kind == "conv" and nd.attrs["has_res"]:
            res, y = nd.srcs[1], nd.outs[0]
            dead = all(order[id(cn)] <= order[id(nd)] for cn in res.consumers)
            if dead and y.buf is None and res.buf is not None and not y.f32:
                y.buf, y.c_offset = res.buf, res.c_offset
            elif dead and y.buf is None and res.buf is None:
                in_place.append(nd)
    # 4. everything else gets its own buffer
    fused_input = any(L.reads_nchw for L in launches)
    for nd in nodes:
        L = by_node.get(id(nd))
        if id(nd) in swallowed or nd.kind == "slice" or (L is not None and L.kind == "head") or (nd.kind == "input" and fused_input):
            continue                                           # (a slice is a view: resolved below)
        if L is not None and L.pooled:                         # the full-resolution map is never materialised, the pooled one is
            if L.dst.buf is None:
                own_buf(L.dst)
            continue
        for o in nd.outs:
            if o.buf is None and not (o.slot == 0 and L is not None and (L.up or nd in in_place)):
                own_buf(o)
    for nd in nodes:      # channel views (in node order: a view of a view resolves too)
        if nd.kind == "slice":
            src, y = nd.srcs[0], nd.outs[0]
            y.buf, y.c_offset = src.buf, src.c_offset + nd.attrs["offset"]
    for nd in in_place:   # in-place adds, now that the residual inputs have buffers
        res, y = nd.srcs[1], nd.outs[0]
        y.buf, y.c_offset = res.buf, res.c_offset
    return bufs


def _live_ranges(rec: Recorder, launches: List[Launch]):
    """[first, last] node-order index at which each buffer is touched.  A buffer is touched by the producer and by every
    consumer of each tensor placed in it (views, concat slices, in-place residual outputs and upsample targets share their
    buffer, so they widen ITS range), and by the launch that reads or writes it in another node's stead; pinned: a buffer some
    tensor of which has no producer / is a model output."""
    order = {id(nd): i for i, nd in enumerate(rec.nodes)}
    rng = {}
    pinned = set()

    def touch(s: Optional[Sym], i):
        if s is not None and s.buf is not None:
            lo, hi = rng.get(id(s.buf), (i, i))
            rng[id(s.buf)] = (min(lo, i), max(hi, i))

    for nd in rec.nodes:
        for s_ in nd.srcs + nd.outs:
            touch(s_, order[id(nd)])
            if nd.kind in ("input", "head") and s_.buf is not None:
                pinned.add(id(s_.buf))
    for L in launches:    # a fused launch reads its first swallowed node's input and may store into another node's output
        touch(L.src, order[id(L.node)])
        touch(L.dst, order[id(L.node)])
    return rng, pinned


def alloc(rec: Recorder, launches: List[Launch], bufs: List[Buf], f32: bool, zeros, f16: bool = False) -> int:
    """One torch tensor (``zeros(shape, dtype)``) per buffer; buffers of identical shape whose live ranges do not overlap share
    storage (YOLO_REUSE_BUFFERS=0 turns that off); returns how many share.  Sharing keeps a residual stage's working set - the
    stream x (in place) and ONE intermediate t instead of one per unit - inside the 256 MB Infinity Cache, and a dead
    intermediate is overwritten there instead of being written back to HBM.  Only buffers that their producers fill completely
    take part (a padded buffer relies on its zero fill)."""
    reuse = os.environ.get("YOLO_REUSE_BUFFERS", "1") == "1" and not f32
    rng, pinned = _live_ranges(rec, launches) if reuse else ({}, set())
    filled = {}
    for nd in rec.nodes:
        for s_ in nd.outs:
            if s_.buf is not None:
                filled[id(s_.buf)] = filled.get(id(s_.buf), 0) + s_.c
    pool = {}                                                   # shape key -> [(last use, tensor)]
    shared = 0
    for b in sorted(bufs, key=lambda b_: rng.get(id(b_), (0, 0))[0]):
        dt = torch.float32 if (b.f32 or f32) else (torch.float16 if f16 else torch.bfloat16)
        ct = K.roundup(b.c_total, 8)
        exact = ct == b.c_total and filled.get(id(b), 0) == b.c_total
        b.c_total = ct
        lo, hi = rng.get(id(b), (None, None))
        if reuse and exact and lo is not None and id(b) not in pinned:
            free = pool.setdefault((b.n, b.h, b.w, ct, dt), [])
            hit = next((e for e in free if e[0] < lo), None)
            if hit is not None:
                free.remove(hit)
                b.tensor = hit[1]
                shared += 1
            else:
                b.tensor = zeros((b.n, b.h, b.w, ct), dt)
            free.append((hi, b.tensor))
        else:      # zero-filled once: padded channels (e.g. 255 -> 256 head rows) are never written
            b.tensor = zeros((b.n, b.h, b.w, ct), dt)
    return shared
