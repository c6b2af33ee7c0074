"""Diagnostics of the plan build, all opt-in by env variable and none of them part of the product path:

* ``YOLO_REDZONE=<bytes>``: guarded allocations (``GuardedAlloc``: Plan's allocator), ``YOLO_REDZONE_BYTE`` the poison byte;
* ``YOLO_SHRINK_OPS="i,j,..."``: launches that process one image (timing only, results wrong);
* ``YOLO_DEPTH_FIRST="a-b:S,..."``: launches [a, b) as S depth-first passes over image sub-batches (bit-equal results).

The last two rewrite the emitted list (``rewrite_list``, called by emit.build_ops)."""
from __future__ import annotations

import os

import torch

from ._lib import OP_CONV, OP_HEAD_DECODE, OP_RESUNIT, OP_STEM, YoloOp

# launches [a, b) of the list as S depth-first passes over image sub-batches ("a-b:S,..."; "" = off): _depth_first
DEPTH_FIRST_DEFAULT = ""


class GuardedAlloc:
    """Plan's allocator.  YOLO_REDZONE=<bytes>: every activation buffer and every packed weight / bias of the plan sits in the
    middle of a larger allocation whose margins are filled with the poison byte: REDZONE_BYTE (0x7f7f... = a large finite bf16 /
    f32 pattern that max pools, MFMAs and decodes would carry into the results) unless YOLO_REDZONE_BYTE names another, such as
    0xFF (NaN in bf16 / f16 / f32: it survives the multiplication by a zero-padded weight that makes 0x7f7f vanish, where a max or
    a compare may drop it); the plan keeps the byte its first guarded allocation was made with.  ``redzone_report()`` then tells
    whether a launch wrote outside its buffer; results that change against a plain plan show reads outside (VERDICT r3 item 2;
    tests/test_gpu_parity.py::test_launch_lists_stay_inside_their_buffers).  Expects ``device``, ``_keep`` and ``_redzones``
    (lists) on the instance."""
    REDZONE_BYTE = 0x7F

    def _redzone(self) -> int:
        return int(os.environ.get("YOLO_REDZONE", "0")) // 256 * 256

    def redzone_byte(self) -> int:
        """The poison byte of this plan's margins: YOLO_REDZONE_BYTE ("0xFF", "255", ...) when the first guarded allocation was made,
        REDZONE_BYTE without it."""
        if getattr(self, "_redzone_byte", None) is None:
            byte = int(os.environ.get("YOLO_REDZONE_BYTE", "") or str(self.REDZONE_BYTE), 0)
            if not 0 <= byte <= 255:
                raise RuntimeError(f"YOLO_REDZONE_BYTE={byte}: not a byte")
            self._redzone_byte = byte
        return self._redzone_byte

    def _guarded(self, nbytes: int):
        """(raw uint8 allocation with poisoned margins, byte offset of the payload)."""
        rz = self._redzone()
        raw = torch.full((nbytes + 2 * rz,), self.redzone_byte(), dtype=torch.uint8, device=self.device)
        self._redzones.append((raw, rz, nbytes))
        return raw, rz

    def _zeros(self, shape, dtype):
        if not self._redzone():
            return torch.zeros(shape, dtype=dtype, device=self.device)
        numel = 1
        for v in shape:
            numel *= v
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        raw, rz = self._guarded(nbytes)
        t = raw[rz:rz + nbytes].view(dtype).view(shape)
        t.zero_()
        return t

    def _dev(self, t):
        """``t`` on the plan's device, kept alive with the plan (packed weights / biases)."""
        if self._redzone() and t.numel():
            nbytes = t.numel() * t.element_size()
            raw, rz = self._guarded(nbytes)
            d = raw[rz:rz + nbytes].view(t.dtype).view(t.shape)
            d.copy_(t)
            t = d
        else:
            t = t.to(self.device)
        self._keep.append(t)
        return t

    def redzone_report(self):
        """Number of margin bytes that no longer hold the poison byte, per guarded allocation: [(index, payload bytes, below, above)]
        for the damaged ones (empty list: every launch stayed inside its buffers)."""
        bad = []
        byte = self.redzone_byte()
        for i, (raw, rz, nbytes) in enumerate(self._redzones):
            lo = int((raw[:rz] != byte).sum())
            hi = int((raw[rz + nbytes:] != byte).sum())
            if lo or hi:
                bad.append((i, nbytes, lo, hi))
        return bad


def rewrite_list(plan, ops, op_launches):
    """The two list rewrites, on the emitted bf16 list (``op_launches``: the Launch record of each op); sets
    ``plan.depth_first`` and ``plan._x_patch``."""
    if plan.f32 or plan.f16:
        return ops, op_launches
    _shrink(plan, ops)
    return _depth_first(plan, ops, op_launches)


def _shrink(plan, ops):
    """Diagnostic only (timing; results wrong): YOLO_SHRINK_OPS="i,j,..." makes launches i, j, ... of the list process ONE image
    instead of the batch - same list, same streams, the launch itself nearly free -, so that `bench.py` can measure what a launch
    family costs INSIDE the pipelined step (tools/marginal_cost.py), as opposed to alone on an idle chip."""
    n = plan.rec.input.n
    for i in (int(v) for v in os.environ.get("YOLO_SHRINK_OPS", "").split(",") if v.strip()):
        op = ops[i]
        if op.kind != OP_HEAD_DECODE and op.splits < 2 and op.conv.n == n and op.conv.n > 1:
            sub = YoloOp.from_buffer_copy(op)      # image 0 only: every batch-major pointer already points at it
            sub.conv.n = 1
            ops[i] = sub


# The first stages of YOLOv3-SPP at 640x640 move 105 MB per 8 images and tensor (320x320x64 bf16) and are bound by memory
# latency, not by the matrix pipe.  A whole-batch launch list runs them breadth-first: every launch streams 0.4-0.8 GB, so by the
# time a consumer launch starts, what its producer wrote has left the 256 MB Infinity Cache.  ``YOLO_DEPTH_FIRST="a-b:S,..."``
# replaces launches [a, b) of the list by S passes over them, pass j on images [j n / S, (j + 1) n / S): same kernels, same tiles
# (a tile never crosses an image), same values - bit for bit -, the producer's sub-batch output still cache-resident when the
# consumer reads it.  Images are independent and the order inside a pass is the list's, so every dependency is kept; buffers
# that share storage (planner.alloc) do so image slice by image slice.
def _depth_first(plan, ops, op_launches):
    n = plan.rec.input.n
    spec = os.environ.get("YOLO_DEPTH_FIRST", DEPTH_FIRST_DEFAULT if n >= 16 else "")
    plan.depth_first = []
    plan._x_patch = [(0, 0)]                            # (op index, byte offset into the caller's NCHW batch) of the ops that read it
    if not spec or spec == "0":
        return ops, op_launches
    segs = []
    for part in spec.split(","):
        rng, s_ = part.split(":")
        a, b = (int(v) for v in rng.split("-"))
        s_ = int(s_)
        b = min(b, len(ops))
        ok = s_ >= 2 and n % s_ == 0 and 0 <= a < b and (not segs or a >= segs[-1][1])
        ok = ok and all(op.kind in (OP_STEM, OP_RESUNIT, OP_CONV) and op.splits < 2 and op.conv.n == n for op in ops[a:b])
        if ok:
            segs.append((a, b, s_))
    if not segs:
        return ops, op_launches
    new_ops, new_launches, pos = [], [], 0
    x_patch = []
    for a, b, s_ in segs:
        new_ops += ops[pos:a]; new_launches += op_launches[pos:a]
        for j in range(s_):
            for i in range(a, b):
                sub, x_off = _sub_op(ops[i], j, s_, plan.rec.c_in)
                if i == 0 and plan.fused_input:
                    x_patch.append((len(new_ops), x_off))
                new_ops.append(sub); new_launches.append(op_launches[i])
        pos = b
        plan.depth_first.append((a, b, s_))
    new_ops += ops[pos:]; new_launches += op_launches[pos:]
    if x_patch:
        plan._x_patch = x_patch
    return new_ops, new_launches


def _sub_op(op, j, s_, c_in):
    """Launch ``op`` restricted to images [j n / s, (j + 1) n / s): batch size and every batch-major pointer moved."""
    sub = YoloOp.from_buffer_copy(op)
    d = sub.conv
    n_sub = d.n // s_
    first = j * n_sub
    d.n = n_sub
    x_off = 0
    if op.kind == OP_STEM:
        x_off = first * c_in * d.h * d.w * 4                               # the caller's float32 NCHW batch (patched per call)
    else:                                               # (a fused unit's x is also its residual: the same batch-major view)
        sub.x = op.x + first * op.conv.h * op.conv.w * op.conv.in_c_total * 2
    up = 4 if op.conv.upsample2x else 1
    m_out = first * op.conv.ho * op.conv.wo
    if op.y:
        sub.y = op.y + m_out * up * op.conv.out_c_total * 2
    if op.residual:
        sub.residual = op.residual + m_out * op.conv.res_c_total * 2
    if op.y_aux:
        sub.y_aux = op.y_aux + m_out * op.conv.aux_c_total * 2
    return sub, x_off
