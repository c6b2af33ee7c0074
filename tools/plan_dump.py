#!/usr/bin/env python3
"""Canonical text of the launch lists the planner builds, for "did this refactor change a plan?" checks.

A plan can be built without a GPU (``torch.device("cpu")``); only its pointers differ from run to run.  This script builds
the plans of a fixed set of configurations (model family, batch, size, precision, planner knobs) and prints, per configuration,
a SHA-256 of a text in which every pointer is rewritten as (ordinal of its allocation by first appearance in the list, byte
offset): every field of every YoloOp / YoloConvDesc in list order, per allocation its size and - for packed weights and biases -
a hash of its bytes, then the heads, the input patches, the shared-buffer count and the FLOP / byte accounting.  Equal pointers
map to equal ordinals, so the text also pins which buffers share storage.  Two commits whose planners agree print the same
hashes; where they do not, ``diff`` the texts:

    python tools/plan_dump.py [OUT_DIR]        # OUT_DIR: also write one text per configuration there

It reads a plan through its public attributes only (op_array, _bufs, _keep, heads, ...), so the same file runs against any
commit's package: PLAN_DUMP_ROOT=<other checkout> python tools/plan_dump.py (with YOLO_HIP_LIB pointing at one built library)."""
import bisect
import hashlib
import os
import sys

import torch

ROOT = os.environ.get("PLAN_DUMP_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cases as CS                                                      # noqa: E402
import pytorch_yolo_amd as P                                             # noqa: E402
from pytorch_yolo_amd import engine                                      # noqa: E402
from pytorch_yolo_amd._lib import YoloConvDesc                           # noqa: E402

PTRS = ("x", "w", "bias", "residual", "y", "y_aux", "w_pre", "bias_pre", "w_dw", "bias_dw", "workspace", "counters")
SCALARS = ("kind", "kpad_pre", "cout_pad_pre", "head_stride_px", "head_na", "head_nc", "io_rows_total", "io_row_offset",
           "head_filter_conf", "ws_bytes", "splits", "head_filter_min_wh")

# (family, batch, size, precision, planner knobs)
CONFIGS = [("spp", 8, 640, "bf16", {}), ("spp", 1, 640, "bf16", {}), ("spp", 1, 640, "fp32", {}), ("tiny", 32, 416, "bf16", {}),
           ("tiny", 4, 416, "fp32", {}), ("mobile", 16, 416, "bf16", {}), ("squeeze", 2, 416, "bf16", {}), ("shuffle", 2, 416, "bf16", {}),
           ("efficient", 2, 416, "bf16", {}), ("yolov3", 2, 416, "bf16", {}), ("lite", 2, 416, "bf16", {}),
           ("spp", 8, 640, "bf16", {"YOLO_DEPTH_FIRST": "0-2:4,2-5:2"}), ("spp", 2, 416, "bf16", {"YOLO_SPLITK": "1"}),
           ("spp", 8, 640, "bf16", {"YOLO_REUSE_BUFFERS": "0"}),
           ("spp", 8, 640, "bf16", {"YOLO_FUSE_RESUNIT": "0", "YOLO_FUSE_STEM": "0", "YOLO_FUSE_HEAD": "0"}),
           ("tiny", 4, 416, "bf16", {"YOLO_FUSE_POOL": "0"}),
           ("mobile", 4, 416, "bf16", {"YOLO_FUSE_MBCONV": "narrow", "YOLO_FUSE_CONV1_S2": "0"}),
           ("mobile", 4, 416, "bf16", {"YOLO_FUSE_MBCONV": "0"}), ("tiny", 4, 416, "bf16", {"YOLO_SHRINK_OPS": "1,3"}),
           ("tiny", 4, 416, "bf16", {"YOLO_REDZONE": "4096"})]


def dump(plan) -> str:
    nbytes = lambda t: t.numel() * t.element_size()
    allocs = {b.tensor.data_ptr(): ("buf", nbytes(b.tensor), None) for b in plan._bufs}
    allocs.update({t.data_ptr(): ("keep", nbytes(t), t) for t in plan._keep if t.numel()})
    for name in ("_splitk_ws", "_splitk_cnt"):                           # split-K workspace / counters (YOLO_SPLITK=1 only)
        t = getattr(plan, name, None)
        if t is not None:
            allocs[t.data_ptr()] = (name, nbytes(t), None)
    starts = sorted(allocs)
    ordinal, lines = {}, []

    def canon(p):
        if not p:
            return "-"
        base = starts[bisect.bisect_right(starts, p) - 1] if p >= starts[0] else None
        if base is None or p - base >= allocs[base][1]:
            raise RuntimeError(f"pointer {p:#x} is outside the plan's allocations")
        kind, size, t = allocs[base]
        if base not in ordinal:
            ordinal[base] = len(ordinal)
            digest = hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16] if t is not None else ""
            lines.append(f"  alloc {ordinal[base]} {kind} {size} {digest}")
        return f"{ordinal[base]}+{p - base}"

    for i in range(plan.n_ops):
        op = plan.op_array[i]
        ptrs = " ".join(f"{n}={canon(getattr(op, n))}" for n in PTRS)
        lines.append(f"op {i} " + " ".join(f"{n}={getattr(op, n)}" for n in SCALARS) + " " + ptrs)
        lines.append("  conv " + " ".join(f"{n}={getattr(op.conv, n)}" for n, _ in YoloConvDesc._fields_))
        lines.append("  anchors " + " ".join(str(v) for v in op.head_anchors_px))
    lines.append(f"heads {[(h['row'], h['na'], h['stride'], h['op']) for h in plan.heads]} rows_total {plan.rows_total}")
    lines.append(f"fused_input {plan.fused_input} x_patch {plan._x_patch} depth_first {plan.depth_first}")
    lines.append(f"shared_buffers {plan.shared_buffers} activation tensors {len({b.tensor.data_ptr() for b in plan._bufs})}")
    lines.append(f"conv_flops {plan.conv_flops()!r} algorithmic_bytes {plan.algorithmic_bytes()!r} detect {plan.algorithmic_bytes(detect=True)!r}")
    if os.environ.get("YOLO_REDZONE"):
        lines.append(f"redzones {[(n, rz) for _, rz, n in getattr(plan, '_redzones', [])]}")
    return "\n".join(lines) + "\n"


def build(family, bs, hw, precision="bf16"):
    torch.manual_seed(0)
    model = {"spp": lambda: P.YOLOv3SPP(anchors=CS.SPP_ANCHORS), "tiny": P.YOLOv3Tiny, "mobile": P.YOLOv3TinyMobile,
             "squeeze": P.YOLOv3TinySqueeze, "shuffle": P.YOLOv3TinyShuffle, "efficient": P.YOLOv3TinyEfficient,
             "yolov3": lambda: P.YOLOv3(kernels_divider=4, anchors=CS.SPP_ANCHORS),
             "lite": lambda: P.LiteYOLOv3(kernels_divider=2, anchors=CS.SPP_ANCHORS)}[family]().eval()
    model.precision = precision
    rec = engine.Recorder(bs, 3, hw, hw)
    model._trace(rec, rec.input)
    return engine.Plan(rec, torch.device("cpu"), model.n_class, hw, model.precision)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    for family, bs, hw, precision, env in CONFIGS:
        os.environ.update(env)
        try:
            text = dump(build(family, bs, hw, precision))
        finally:
            for k in env:
                del os.environ[k]
        tag = f"{family}-{bs}-{hw}-{precision}" + "".join(f"-{k}={v}" for k, v in env.items())
        print(f"{hashlib.sha256(text.encode()).hexdigest()}  {text.count(chr(10) + 'op '):4d} launches  {tag}", flush=True)
        if out:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, tag + ".txt"), "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
