"""Host mirror of the post-process part of reference utils/utils.py.

``non_max_suppression`` keeps the reference signature and return value
(utils.py:200-206,293) and runs the batched NMS kernels (csrc/nms.hip) in one of the
reference's four styles (``nms_style=``: 'MERGE', which the reference hard-codes, 'OR', 'AND', 'SOFT').

``compute_loss`` and ``build_targets`` (utils.py:124-197) run the kernels of csrc/loss.hip on the raw head tensors of an eval-mode
forward: the reference's loss, and - where some ``p[i]`` requires grad - its gradient with respect to ``p`` through autograd
(``loss_grad_raw``); the chain ends at ``p``, nothing propagates through the convolutions.  ``wh_iou``, ``bbox_iou`` and
``xyxy2xywh`` are the reference's tensor helpers on whatever device their inputs live on.

``bench_results`` and ``test_model`` (utils.py:330-393) score a results list with the COCO bbox metrics on the device
(utils/coco_eval.py, csrc/coco_eval.hip) instead of pycocotools.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K
from .._lib import nms_style_id
from . import coco_helper
from .coco_eval import STAT_NAMES, coco_eval

MIN_WH = 2.0               # reference utils.py:207
MAX_PER_CLASS = 100        # reference utils.py:247-250

_ws_cache = {}
MAX_CACHED_WORKSPACES = 16


def _workspace(device, bs, rows, nc, slot=None):
    """NMS scratch (keys / counters / staging), cached per (device, shape, STREAM): launches on one stream are ordered, so
    they can share it; two same-shape calls on different streams get different buffers and cannot race.  Bounded: the
    least recently used entry is dropped (its memory returns to torch's allocator once queued work has finished)."""
    key = (device, bs, rows, nc, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.pop(key, None)
    if ws is None:
        ws = torch.empty(K.nms_workspace_bytes(bs, rows, nc), dtype=torch.uint8, device=device)
    _ws_cache[key] = ws                                  # most recently used last
    while len(_ws_cache) > MAX_CACHED_WORKSPACES:
        old = _ws_cache.pop(next(iter(_ws_cache)))
        old.record_stream(torch.cuda.current_stream(device))
    return ws


def nms_capacity(rows: int, nc: int) -> int:
    """Upper bound on kept rows per image: every class keeps at most MAX_PER_CLASS."""
    return max(1, min(rows, nc * MAX_PER_CLASS))


def nms_raw(prediction: torch.Tensor, conf_thres: float, nms_thres: float, inplace_conf: bool = False,
            out=None, nms_style: str = "MERGE"):
    """Launch only (no host sync).  Returns (dets [bs,cap,7], idx [bs,cap], count [bs]) device tensors;
    rows beyond count[b] are unspecified.  ``out`` lets a caller pass static buffers (graph capture)."""
    style = nms_style_id(nms_style)
    if prediction.dim() != 3:
        raise RuntimeError("prediction must be [bs, rows, 5+nc]")
    if not prediction.is_cuda:
        raise RuntimeError("pytorch_yolo_amd.non_max_suppression runs on a ROCm device only (no CPU fallback)")
    if prediction.dtype != torch.float32 or not prediction.is_contiguous():
        if inplace_conf:
            raise RuntimeError("inplace_conf needs a contiguous float32 prediction tensor")
        prediction = prediction.float().contiguous()
    bs, rows, no = prediction.shape
    nc = no - 5
    if out is None:
        cap = nms_capacity(rows, nc)
        dev = prediction.device
        out = (torch.empty((bs, cap, 7), dtype=torch.float32, device=dev),
               torch.empty((bs, cap), dtype=torch.int32, device=dev),
               torch.empty((bs,), dtype=torch.int32, device=dev))
    with torch.cuda.device(prediction.device):          # the library launches on the current device's stream
        K.nms_styled(prediction, conf_thres, nms_thres, out[0], out[1], out[2], _workspace(prediction.device, bs, rows, nc),
                     style=style, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS, mutate_conf=inplace_conf)
    return out


def nms_launch(prediction, conf_thres, nms_thres, out, slot=0, inplace_conf=False, nms_style="MERGE"):
    """Launch the NMS kernels on the current stream into ``out`` = (dets, idx, count); the workspace is private to the
    current stream (``slot`` is kept for callers of the old signature and ignored)."""
    style = nms_style_id(nms_style)
    bs, rows, no = prediction.shape
    with torch.cuda.device(prediction.device):
        K.nms_styled(prediction, conf_thres, nms_thres, out[0], out[1], out[2],
                     _workspace(prediction.device, bs, rows, no - 5), style=style, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS,
                     mutate_conf=inplace_conf)
    return out


def split_detections(dets, idx, count, with_indices=False):
    """Device buffers -> the reference's ``list[Tensor[n,7] | None]`` (one D2H copy of the counts).  The kept rows of all
    images are gathered into ONE packed tensor (an index built on the host, one index_select) and handed out as its per-image
    slices: two launches per call instead of one clone per image, and the big output buffers are not kept alive."""
    counts = count.cpu().tolist()
    cap = dets.shape[1]
    for b, n in enumerate(counts):
        if n > cap:
            raise RuntimeError(f"image {b}: {n} detections exceed the output capacity {cap}")
    total = sum(counts)
    if total == 0:
        out = [None] * len(counts)
        return (out, list(out)) if with_indices else out
    rows = np.concatenate([np.arange(b * cap, b * cap + n, dtype=np.int64) for b, n in enumerate(counts) if n])
    rows = torch.from_numpy(rows).to(dets.device, non_blocking=True)
    packed = dets.reshape(-1, dets.shape[2]).index_select(0, rows)
    parts = iter(torch.split(packed, [n for n in counts if n]))
    out = [next(parts) if n else None for n in counts]
    if not with_indices:
        return out
    packed_idx = idx.reshape(-1).index_select(0, rows).long()
    parts = iter(torch.split(packed_idx, [n for n in counts if n]))
    return out, [next(parts) if n else None for n in counts]


def non_max_suppression(prediction, conf_thres=0.5, nms_thres=0.5, inplace_conf=False, with_indices=False, nms_style="MERGE"):
    """Drop-in for reference ``non_max_suppression`` (utils.py:200-293).

    ``nms_style`` is the reference's one-word switch (utils.py:240; names as there, case-sensitive): 'MERGE' (what the reference
    ships with: conf-weighted mean boxes, :266-275), 'OR' (greedy hard NMS, :253-259; a row with iou == nms_thres is removed),
    'AND' (:260-265: a head is kept only if it overlaps a remaining row by more than 0.5; lone rows of a class with several rows
    are erased) and 'SOFT' (:277-287: nothing is removed, conf decays by exp(-iou^2 / 0.5) per earlier row).  In 'OR', 'AND' and
    'SOFT' the boxes are the input rows' corners, unchanged.  'SOFT' conf values carry the rounding of expf (<= 4e-5 relative
    over a class's chain of up to 99 factors); everything else is bit-defined.  Anything else raises ``ValueError``.

    Returns a list (len bs) of ``Tensor[n,7]`` = (x1, y1, x2, y2, conf, class_conf, class) sorted by
    conf descending, or ``None`` for an image with no detections.

    Differences, both opt-in to the reference behaviour:
      * the reference overwrites ``prediction[..., 4]`` with obj*class_conf (:213); here the input
        is left untouched unless ``inplace_conf=True``;
      * ``with_indices=True`` additionally returns, per image, the input row of each kept box.
    The reference's unstable argsort (:237,:291) is replaced by a total order
    (conf desc, then class, then input row) — identical whenever conf values are distinct.
    """
    return split_detections(*nms_raw(prediction, conf_thres, nms_thres, inplace_conf, nms_style=nms_style), with_indices=with_indices)


def xywh2xyxy(x):
    """Reference utils.py:46-60 (kept for API compatibility; the NMS kernel does this itself)."""
    y = torch.zeros_like(x)
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def xyxy2xywh(x):
    """Reference utils.py:29-43: rows (x1, y1, x2, y2) -> rows (x centre, y centre, w, h); a torch tensor or a numpy array [n, 4]."""
    out = torch.zeros_like(x) if isinstance(x, torch.Tensor) else np.zeros_like(x)
    for axis in (0, 1):
        lo, hi = x[:, axis], x[:, axis + 2]
        out[:, axis] = (lo + hi) / 2
        out[:, axis + 2] = hi - lo
    return out


def _corner_columns(box, corners):
    """(x1, y1, x2, y2) of ``box`` ([4] or [4, n]) given as corners or as (x, y, w, h): x -+ w / 2 like xywh2xyxy."""
    if corners:
        return box[0], box[1], box[2], box[3]
    half_w, half_h = box[2] / 2, box[3] / 2
    return box[0] - half_w, box[1] - half_h, box[0] + half_w, box[1] + half_h


def bbox_iou(box1, box2, x1y1x2y2=True):
    """Reference utils.py:63-96: IoU of one box ``box1`` [4] with every row of ``box2`` [n, 4]; both as corners (default) or as
    (x, y, w, h).  Operation order as the reference's: area1 carries the + 1e-16, the union is (area1 + area2) - intersection."""
    ax1, ay1, ax2, ay2 = _corner_columns(box1, x1y1x2y2)
    bx1, by1, bx2, by2 = _corner_columns(box2.t(), x1y1x2y2)
    overlap_w = (torch.min(ax2, bx2) - torch.max(ax1, bx1)).clamp(0)
    overlap_h = (torch.min(ay2, by2) - torch.max(ay1, by1)).clamp(0)
    inter = overlap_w * overlap_h
    area1 = (ax2 - ax1) * (ay2 - ay1) + 1e-16
    return inter / (area1 + (bx2 - bx1) * (by2 - by1) - inter)


def wh_iou(box1, box2):
    """Reference utils.py:99-121: IoU of the (w, h) pair ``box1`` [2] with every row of ``box2`` [n, 2], as boxes sharing a centre -
    the anchor-to-target measure of build_targets (the assignment kernel of csrc/loss.hip forms it the same way)."""
    w, h = box1[0], box1[1]
    others = box2.t()
    inter = torch.min(w, others[0]) * torch.min(h, others[1])
    return inter / ((w * h + 1e-16) + others[0] * others[1] - inter)


def _scale_params(img1_shape, img0_shape, n_rows):
    """(pad_x, pad_y, gain, n_rows) exactly as the reference computes them in python floats (utils.py:298-300)."""
    gain = max(img1_shape) / max(img0_shape)
    return [(img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2, gain, float(n_rows)]


def scale_coords(img1_shape, coords, img0_shape, round_result=False):
    """Drop-in for reference ``scale_coords`` (utils.py:296-303): rescale xyxy boxes (columns 0..3 of ``coords``
    [n, >=4], modified IN PLACE like the reference) from the network-input frame ``img1_shape`` (h, w) to the
    original image frame ``img0_shape``.  Runs ``yolo_scale_coords`` on the device."""
    if not coords.is_cuda:
        raise RuntimeError("pytorch_yolo_amd.scale_coords runs on a ROCm device only (no CPU fallback)")
    if coords.dim() != 2 or coords.shape[1] < 4 or coords.dtype != torch.float32 or not coords.is_contiguous():
        raise RuntimeError("scale_coords: coords must be a contiguous float32 [n, >=4] tensor")
    n = coords.shape[0]
    if n == 0:
        return coords
    params = torch.tensor([_scale_params(img1_shape, img0_shape, n)], dtype=torch.float32, device=coords.device)
    from .._lib import check, load
    with torch.cuda.device(coords.device):
        check(load().yolo_scale_coords(coords.data_ptr(), 1, n, coords.shape[1], params.data_ptr(), int(round_result),
                                       K.stream_ptr()), "scale_coords")
    return coords


def scale_detections(dets, count, img1_shape, img0_shapes, round_result=True):
    """Batched form used after ``nms_raw``: dets [bs,cap,7] in place, one original (h, w) per image; counts are
    read on the host (they are needed there anyway to split the list)."""
    counts = count.cpu().tolist()
    params = torch.tensor([_scale_params(img1_shape, s0, n) for s0, n in zip(img0_shapes, counts)],
                          dtype=torch.float32, device=dets.device)
    from .._lib import check, load
    with torch.cuda.device(dets.device):
        check(load().yolo_scale_coords(dets.data_ptr(), dets.shape[0], dets.shape[1], dets.shape[2], params.data_ptr(),
                                       int(round_result), K.stream_ptr()), "scale_coords")
    return dets


# ---- compute_loss / build_targets (reference utils.py:124-197) on the device: csrc/loss.hip ---------------------------------------
HYPER_KEYS = ("iou_thresh", "xy_loss", "wh_loss", "cls_loss", "conf_loss")
_loss_ws_cache = {}
LOSS_TARGET_STEP = 256       # the cached loss workspace is sized for the target count rounded up to this


def _hyper_params(model):
    h = getattr(model, "hyper_params", None)
    if h is None or any(k not in h for k in HYPER_KEYS):
        raise ValueError("compute_loss / build_targets need model.hyper_params with the keys " + ", ".join(HYPER_KEYS)
                         + f" (reference utils.py:134,162), got {None if h is None else sorted(h)}")
    return h


def _layer_geometry(layer):
    """(n_anchors, (nx, ny) of n_grids, anchor_vec as nested lists) of a YOLO layer, read from the attributes the reference's
    build_targets reads (utils.py:169,171,190).  The two tensors are copied to the host once per (tensor, version): a forward at a new
    input size replaces them (YOLOLayer._sync_grid_attrs), and only then does the next call copy - and synchronise - again."""
    av, ng = layer.anchor_vec, layer.n_grids
    if not isinstance(av, torch.Tensor) or not isinstance(ng, torch.Tensor):
        return None                                       # no forward yet: the reference's attributes are still the int 0
    cached = layer.__dict__.get("_loss_geometry")
    if cached is None or cached[0] is not av or cached[1] is not ng or cached[2] != (av._version, ng._version):
        vec = [[float(w), float(h)] for w, h in av.detach().cpu().tolist()]
        grids = tuple(ng.detach().cpu().tolist())
        cached = (av, ng, (av._version, ng._version), (len(vec), grids, vec))
        layer.__dict__["_loss_geometry"] = cached
    return cached[3]


def _loss_geometry(model, shapes=None):
    """([(na, ny, nx)], [anchor_vec]) of model.yolo_layers; with ``shapes`` (those of the head tensors) every layer is checked against
    its tensor."""
    geom, vecs = [], []
    layers = list(model.yolo_layers)
    if shapes is not None and len(shapes) != len(layers):
        raise RuntimeError(f"compute_loss: {len(shapes)} head tensors for {len(layers)} YOLO layers")
    for i, layer in enumerate(layers):
        lg = _layer_geometry(layer)
        if lg is None:
            raise RuntimeError(f"YOLO layer {i} has no grid yet (anchor_vec / n_grids are set by a forward): run the model at this input size first")
        na, (nxf, nyf), vec = lg
        nx, ny = int(nxf), int(nyf)
        if shapes is not None:
            sh = tuple(shapes[i])
            if len(sh) != 5 or (sh[1], sh[2], sh[3]) != (na, ny, nx) or sh[4] != int(layer.n_classes) + 5:
                raise RuntimeError(f"YOLO layer {i}: its grid attributes (anchors {na}, n_grids ({nx}, {ny}), classes {int(layer.n_classes)}) do not match "
                                   f"the head tensor {sh}: run the model forward at this input size before compute_loss")
        geom.append((na, ny, nx))
        vecs.append(vec)
    return geom, vecs


def _loss_workspace(device, geom, bs, nt):
    """Scratch of the loss kernels (records / tconf map / partial sums), cached like the NMS scratch: per (device, shapes, stream), least
    recently used entry dropped; sized for the target count rounded up to LOSS_TARGET_STEP so that batches with different counts share it."""
    nt_cap = max(1, -(-nt // LOSS_TARGET_STEP)) * LOSS_TARGET_STEP
    key = (device, tuple(geom), bs, nt_cap, torch.cuda.current_stream(device).cuda_stream)
    ws = _loss_ws_cache.pop(key, None)
    if ws is None:
        ws = torch.empty(K.loss_workspace_bytes(geom, bs, nt_cap), dtype=torch.uint8, device=device)
    _loss_ws_cache[key] = ws
    while len(_loss_ws_cache) > MAX_CACHED_WORKSPACES:
        old = _loss_ws_cache.pop(next(iter(_loss_ws_cache)))
        old.record_stream(torch.cuda.current_stream(device))
    return ws


def _device_targets(targets, device):
    targets = torch.as_tensor(targets)
    if targets.dim() != 2 or targets.shape[1] != 6:
        raise RuntimeError(f"targets must be [nt, 6] (image, class, x, y, w, h), got {tuple(targets.shape)}")
    return targets.to(device=device, dtype=torch.float32).contiguous()


def _records(workspace, nl, nt):
    """The records at the start of a loss workspace as int32 [nl, nt, LOSS_REC_WORDS] (a view)."""
    return workspace[:nl * nt * K.LOSS_REC_WORDS * 4].view(torch.int32).view(nl, nt, K.LOSS_REC_WORDS)


def _out_of_range_message(n):
    return f"{n} targets outside the batch / grid / class range (the reference raises an IndexError on them)"


def build_targets(model, targets, bs=None, workspace=None):
    """Drop-in for reference ``build_targets`` (utils.py:160-197): ``(txy, twh, tcls, indices)``, per-layer lists with
    ``indices[i] = (b, a, gj, gi)`` int64, ``tcls[i]`` int64, ``txy[i]`` / ``twh[i]`` float32 [n_i, 2], kept targets in the order of
    ``targets``.  ``targets`` ([nt, 6]: image, class, x, y, w, h) may live on the host; the result lives on the device of the model's
    YOLO layers.  Runs the assignment kernel (yolo_build_targets_fwd) and compacts its fixed-slot records with a boolean index:
    THIS SYNCHRONISES with the device (compute_loss does not go through here).  Ties between anchors go to the first maximum.
    ``bs`` bounds the image index (default: the largest image index + 1); a kept target outside the batch / grid / class range raises
    ``RuntimeError``.  ``workspace``: a caller-owned uint8 buffer of ``kernels.loss_workspace_bytes`` bytes."""
    h = _hyper_params(model)
    geom, vecs = _loss_geometry(model)
    device = model.yolo_layers[0].anchor_vec.device
    if device.type != "cuda":
        raise RuntimeError("pytorch_yolo_amd.build_targets runs on a ROCm device only (no CPU fallback)")
    targets = _device_targets(targets, device)
    nt, nl, nc = targets.shape[0], len(geom), int(model.n_class)
    if bs is None:
        bs = max(1, int(targets[:, 0].max()) + 1) if nt else 1
    i64 = lambda: torch.empty((0,), dtype=torch.int64, device=device)
    if nt == 0:
        f2 = lambda: torch.empty((0, 2), dtype=torch.float32, device=device)
        return [f2() for _ in geom], [f2() for _ in geom], [i64() for _ in geom], [(i64(), i64(), i64(), i64()) for _ in geom]
    with torch.cuda.device(device):
        if workspace is None:
            workspace = _loss_workspace(device, geom, bs, nt)
        K.build_targets_fwd(targets, geom, vecs, bs, nc, h["iou_thresh"], workspace)
        rec = _records(workspace, nl, nt)
        bad = int(rec[:, :, 10].amax(0).sum())
        if bad:
            raise RuntimeError("build_targets: " + _out_of_range_message(bad))
        txy, twh, tcls, indices = [], [], [], []
        for i in range(nl):
            r = rec[i][rec[i, :, 0] != 0]
            cols = r.long()
            indices.append((cols[:, 1], cols[:, 2], cols[:, 3], cols[:, 4]))
            tcls.append(cols[:, 5])
            fl = r[:, 6:10].contiguous().view(torch.float32)
            txy.append(fl[:, 0:2].clone())
            twh.append(fl[:, 2:4].clone())
    return txy, twh, tcls, indices


def loss_raw(p, targets, model, class_weight=None, workspace=None, out=None, status=None):
    """Launch only (no host sync once the layers' geometry is cached): returns ``(out, status, workspace)`` device tensors - out
    float32 [5] = (lxy, lwh, lconf, lcls, loss), status int32 [1 + layers] = (targets outside the batch / grid / class range, kept
    targets per layer).  ``workspace`` / ``out`` / ``status`` let a caller pass static buffers (graph capture, guarded tests)."""
    a = _loss_args(p, targets, model, class_weight)
    return _loss_launch(a, workspace, out, status)


def _as_head_tensors(p):
    """The list ``p`` with every tensor float32 and contiguous (torch operations: differentiable where autograd is recording)."""
    p = list(p)
    if not p or not all(isinstance(t, torch.Tensor) for t in p):
        raise RuntimeError("compute_loss: p must be the list of raw head tensors that `io, p = model(x)` returns")
    if not all(t.is_cuda for t in p):
        raise RuntimeError("pytorch_yolo_amd.compute_loss runs on a ROCm device only (no CPU fallback)")
    return [t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous() for t in p]


def _loss_args(p, targets, model, class_weight):
    """What a loss launch needs beside its buffers, read from the model once: a forward and its backward share one of these, so a
    model whose layers move on to another grid in between changes nothing."""
    h = _hyper_params(model)
    p = [t.detach() for t in _as_head_tensors(p)]
    device = p[0].device
    geom, vecs = _loss_geometry(model, [t.shape for t in p])
    targets = _device_targets(targets, device)
    bs = p[0].shape[0]
    if class_weight is not None:
        class_weight = torch.as_tensor(class_weight).to(device=device, dtype=torch.float32).contiguous()
    gains = [bs * h["xy_loss"], bs * h["wh_loss"], bs * h["cls_loss"], bs * h["conf_loss"]]       # k = bs, utils.py:135-136
    return dict(p=p, targets=targets, geom=geom, vecs=vecs, nc=int(model.n_class), bs=bs, nt=targets.shape[0], device=device,
                iou_thresh=h["iou_thresh"], gains=gains, class_weight=class_weight)


def _loss_launch(a, workspace=None, out=None, status=None):
    device = a["device"]
    with torch.cuda.device(device):
        if workspace is None:
            workspace = _loss_workspace(device, a["geom"], a["bs"], a["nt"])
        if out is None:
            out = torch.empty((5,), dtype=torch.float32, device=device)
        if status is None:
            status = torch.empty((1 + len(a["p"]),), dtype=torch.int32, device=device)
        K.loss_fwd(a["p"], a["targets"], a["geom"], a["vecs"], a["nc"], a["iou_thresh"], a["gains"], a["class_weight"], workspace, out,
                   status)
    return out, status, workspace


def _loss_grad_launch(a, grad_loss=None, workspace=None, out=None):
    device = a["device"]
    with torch.cuda.device(device):
        if workspace is None:
            workspace = _loss_workspace(device, a["geom"], a["bs"], a["nt"])
        if grad_loss is None:
            grad_loss = torch.ones((1,), dtype=torch.float32, device=device)
        else:
            grad_loss = grad_loss.detach().to(device=device, dtype=torch.float32).reshape(1)
        if out is None:
            out = [torch.empty_like(t) for t in a["p"]]
        K.loss_bwd(a["p"], a["targets"], a["geom"], a["vecs"], a["nc"], a["iou_thresh"], a["gains"], a["class_weight"], workspace,
                   grad_loss, list(out))
    return list(out)


def loss_grad_raw(p, targets, model, class_weight=None, grad_loss=None, workspace=None, out=None):
    """Launch only: the gradient of ``compute_loss(p, targets, model, class_weight)[0]`` with respect to every ``p[i]``, times
    ``grad_loss`` (a float32 tensor of one element ON THE DEVICE, read there: no host sync; default 1.0).  Returns the list of gradient
    tensors, float32 of the shapes of ``p``; EVERY element is written.  ``out`` (a list of contiguous float32 tensors of those shapes)
    and ``workspace`` (``kernels.loss_workspace_bytes`` bytes) let a caller pass static buffers (graph capture, guarded tests).  The
    call is self-contained: it runs the target assignment itself and uses nothing a forward call left in a workspace.  Targets outside
    the batch / grid / class range are left out, as ``loss_raw`` leaves them out (and counts them in its status array)."""
    return _loss_grad_launch(_loss_args(p, targets, model, class_weight), grad_loss, workspace, out)


class _LossFunction(torch.autograd.Function):
    """loss_raw with a backward: forward(a, *p) returns the five items (out[4] is the loss), backward hands the gradient of out[4] to
    the gradient kernels.  ``p`` are the float32 contiguous head tensors that ``a`` (_loss_args) holds detached.  The gradient of
    items 0-3 is NOT formed: compute_loss hands out only out[4:5] attached.  Once differentiable: a double backward raises."""

    @staticmethod
    def forward(ctx, a, *p):
        ctx.loss_args = dict(a, p=None)
        ctx.save_for_backward(*p)                               # (so that torch notices a p modified in place before the backward)
        out, status, _ = _loss_launch(a)
        ctx.mark_non_differentiable(status)
        return out, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_status):
        a = dict(ctx.loss_args, p=[t.detach() for t in ctx.saved_tensors])
        grads = _loss_grad_launch(a, grad_out.contiguous()[4:5])
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def compute_loss(p, targets, model, class_weight=None, check=True):
    """Drop-in for reference ``compute_loss`` (utils.py:124-157): returns ``(loss, items)`` - ``loss`` float32 [1], ``items`` float32 [5]
    = cat(lxy, lwh, lconf, lcls, loss) - on the device.

    WHAT IS DIFFERENTIABLE: ``loss`` with respect to ``p``, once.  Where autograd is recording (``torch.is_grad_enabled()``) and some
    ``p[i].requires_grad``, ``loss`` carries a ``grad_fn`` and ``loss.backward()`` runs the gradient kernels of csrc/loss.hip
    (``loss_grad_raw``): ``p[i].grad`` is what the reference's ``loss.backward()`` leaves there within 5e-6 of each word group's
    largest element, bit-identical from run to run; a ``p[i]`` that does not require grad gets none.  The forward value has the same
    bits either way; ``items`` is always detached (``:157``).  WHAT IS NOT: nothing propagates through the MODEL's forward -
    the ``p`` of ``io, p = model(x)`` has no ``grad_fn``, so the chain ends at ``p`` unless ``p`` comes from code of the caller's
    (``p = [t.detach().requires_grad_() for t in p]``, heads computed in torch or with ``pytorch_yolo_amd.conv_block``) -, a training-mode forward keeps raising, targets and
    class weights get no gradient, and a double backward raises.  Otherwise (``torch.no_grad()``, or no ``p[i]`` requiring grad)
    ``loss.grad_fn is None`` and nothing can be back-propagated.

    ``p`` is the list of raw head tensors [bs, na, ny, nx, 5 + nc] that ``io, p = model(x)`` returns in eval mode (in the reference the
    same tensors in training and eval mode), on the device (no CPU fallback); tensors that are not float32 or not contiguous are
    converted (by torch operations, which autograd differentiates: such a ``p[i]`` gets a gradient of its own dtype and layout).
    ``targets`` [nt, 6] = image, class, x, y, w, h (normalised) may live on the host; ``nt == 0`` is legal.  ``model`` is
    read for ``hyper_params`` (keys iou_thresh, xy_loss, wh_loss, cls_loss, conf_loss: ``ValueError`` without them), ``n_class`` and,
    per YOLO layer, ``anchor_vec`` / ``n_grids`` / ``n_classes`` - which must describe ``p`` (``RuntimeError`` otherwise: run the
    forward at this input size first).  The reference's quirks are kept: k = bs, a duplicate cell is gathered once per target, and
    with ``n_class == 1`` the class term is BCEWithLogits against the class INDEX.

    Differences from the reference:
      * a kept target whose image, class or grid cell is out of range (the reference raises an IndexError) is left out and counted:
        ``check=True`` reads the count - ONE host sync - and raises ``RuntimeError``; ``check=False`` never syncs and returns the loss
        of the remaining targets (``loss_raw`` also returns the status array);
      * ties between anchors go to the first maximum (torch.max leaves the choice open);
      * the sums are float64 in a fixed order: the value is bit-identical from run to run, within 5e-6 relative of the reference's."""
    p = list(p)
    tracked = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in p)
    if tracked:
        _hyper_params(model)
        p = _as_head_tensors(p)                                 # outside the Function: torch differentiates the conversions
        out, status = _LossFunction.apply(_loss_args(p, targets, model, class_weight), *p)
    else:
        out, status, _ = loss_raw(p, targets, model, class_weight)
    if check:
        bad = int(status[0])
        if bad:
            raise RuntimeError("compute_loss: " + _out_of_range_message(bad))
    return out[4:5], (out.detach() if tracked else out)         # items detached, :157


def _dict_from_results(data, targets, imgs_path, orig_shapes, cur_shape):
    """Drop-in for the reference's ``_dict_from_results`` (utils.py:306-327): the detections of one batch (the list
    ``non_max_suppression`` returns, rows x1 y1 x2 y2 conf cls_conf cls in the network frame ``cur_shape``) are mapped
    back to each original image (``scale_coords(...).round()``, on the device, in place like the reference) and
    appended to ``data[img_path]`` as {'type','score','left','top','right','bottom'} dicts."""
    for i, pred in enumerate(targets):
        if pred is None:
            continue
        scale_coords(cur_shape, pred, orig_shapes[i], round_result=True)
        rows = data.setdefault(imgs_path[i], [])
        for x1, y1, x2, y2, conf, _cls_conf, cls in pred.detach().cpu().numpy():
            rows.append({"type": int(cls), "score": float(conf), "left": int(x1), "top": int(y1), "right": int(x2),
                         "bottom": int(y2)})
    return data


def predict_dataset(model, batches, conf_thresh=0.1, nms_thresh=0.1, nms_style="MERGE", loss=False):
    """The loop of the reference's ``test_model`` (utils.py:357-378) up to its prediction dictionary: for every
    ``(imgs, targets, imgs_path, shapes)`` batch (the reference dataset's collate format): forward, NMS, back-projection.
    The COCO scoring that follows in the reference (``coco_helper`` + pycocotools, utils.py:380-393) is ``test_model`` /
    ``bench_results`` below, on the kernels of csrc/coco_eval.hip.  ``nms_style``: see ``non_max_suppression``.

    ``loss=False`` ignores ``targets`` and returns the dictionary.  ``loss=True`` takes the two-line path per batch
    (``io, p = model(imgs)``, ``non_max_suppression(io, ...)``), computes ``compute_loss(p, targets, model)`` (the model needs
    ``hyper_params``) and returns ``(data, items)``: ``items`` = the batch-size-weighted mean of the five loss items
    (lxy, lwh, lconf, lcls, loss) as a list of floats."""
    was_training = model.training
    model.eval()
    data = {}
    acc, seen = None, 0
    try:
        for imgs, targets, imgs_path, shapes in batches:
            imgs = imgs.to(next(model.parameters()).device)
            with torch.no_grad():
                if loss:
                    io, p = model(imgs)
                    det = non_max_suppression(io, conf_thresh, nms_thresh, nms_style=nms_style)
                    items = compute_loss(p, targets, model)[1].double() * imgs.shape[0]
                    acc = items if acc is None else acc + items
                    seen += imgs.shape[0]
                else:
                    det = model.detect(imgs, conf_thresh, nms_thresh, nms_style=nms_style)
            _dict_from_results(data, det, imgs_path, shapes, tuple(imgs.shape[-2:]))
    finally:
        if was_training:
            model.train()
    if loss:
        return data, ([float("nan")] * 5 if acc is None else (acc / seen).tolist())
    return data


def bench_results(results_path, cocoGt, device="cuda"):
    """Drop-in for the reference's ``bench_results`` (utils.py:330-354): the COCO bbox metrics of a results file (or an in-memory
    results list) against ``cocoGt`` (a pycocotools ``COCO``, any object with a ``.dataset`` dict, or the dataset dict), computed
    by ``coco_eval`` on ``device``.  Prints summarize's twelve lines and the Mean IOU line, returns the reference's dictionary."""
    res = coco_eval(cocoGt, results_path, device)
    for line in res.summary_lines():
        print(line)
    print(f"Mean IOU: {res.mean_iou:.2f}")
    return dict(zip(STAT_NAMES + ("IOU",), [float(v) for v in res.stats] + [res.mean_iou]))


def test_model(model, dataset, batch_size, num_workers, device, conf_thresh=0.1, nms_thresh=0.1):
    """Drop-in for the reference's ``test_model`` (utils.py:357-393): a DataLoader over ``dataset`` with its ``collate_fn``,
    ``predict_dataset``, ``results_from_dict`` against ``dataset.coco.dataset`` and ``bench_results``.  The results list goes to the
    evaluation in memory (the reference writes it to a temporary JSON file for pycocotools).  ``model.training`` is restored."""
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, num_workers=num_workers, shuffle=False, pin_memory=True,
                                         collate_fn=dataset.collate_fn)
    was_training = model.training
    try:
        data = predict_dataset(model, loader, conf_thresh, nms_thresh)
        results = coco_helper.results_from_dict(data, dataset.coco.dataset)
        return bench_results(results, dataset.coco, device)
    finally:
        model.train(was_training)


test_model.__test__ = False        # (a name pytest would otherwise collect wherever it is imported)
