#!/usr/bin/env python3
"""images/s of model.detect() on SPP-640 x 32 in the three precision modes, interleaved in ONE process over several rounds (the chip's
clock and temperature drift between processes: only numbers from the same run compare).  The fp16 mode is timed twice: as shipped
(large 3x3 layers on the 20x20-tile kernels, OP_CONV_T20_F16) and with YOLO_FP16_T20=0 (every layer in the gather kernel: the list
before those kernels existed) - a second model object whose plans are built under that switch.
    python tools/precision_rates.py [rounds] [calls per round]  > profiles/fp16_mode_rates.md
--model mobile times YOLOv3TinyMobile 416 x 64 instead, in the two modes that family has (bf16 and fp32; fp16 raises for its
depthwise layers), same method:
    python tools/precision_rates.py --model mobile [rounds] [calls per round]  > profiles/fp32_encoder_rates.md"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_yolo_amd import YOLOv3SPP, YOLOv3TinyMobile                         # noqa: E402
from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict      # noqa: E402

SPP_ANCHORS = (((10., 13.), (16., 30.), (33., 23.)), ((30., 61.), (62., 45.), (59., 119.)), ((116., 90.), (156., 198.), (373., 326.)))
MODES = ("bf16", "fp16", "fp16 gather-only", "fp32")
GATHER = "fp16 gather-only"


def _op_kinds(plan):
    """{op kind: launches} of the whole-batch list detect() runs (or of the first sub-batch list)."""
    from collections import Counter
    one = (getattr(plan, "_full", None) or getattr(plan, "subs", None) or [plan])[0]
    return Counter(one.op_array[i].kind for i in range(one.n_ops))


def main_mobile(rounds, calls):
    """bf16 and fp32 on YOLOv3TinyMobile 416 x 64: interleaved rounds, one process, one model object (the plan cache is keyed by
    precision)."""
    from pytorch_yolo_amd._lib import OP_DWCONV_F32, OP_MBCONV
    dev = torch.device("cuda", 0)
    bs, hw, conf, iou = 64, 416, 0.1, 0.5
    modes = ("bf16", "fp32")
    model = YOLOv3TinyMobile(n_class=80).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234, n_class=80))
    model = model.to(dev)
    x = torch.cat([synth_images(1, hw, hw, i) for i in range(bs)], 0).to(dev)
    per_mode, n_det, kinds = {m: [] for m in modes}, {}, {}
    with torch.no_grad():
        for m in modes:                                        # plans, packed weights, first-launch costs
            model.precision = m
            for _ in range(2):
                dets = model.detect(x, conf, iou)
            n_det[m] = sum(0 if d is None else len(d) for d in dets)
            kinds[m] = _op_kinds(model.plan_for(x))
        for rnd in range(rounds):
            for m in modes:
                model.precision = m
                n = calls if m != "fp32" else max(3, calls // 5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    model.detect(x, conf, iou)
                torch.cuda.synchronize()
                per_mode[m].append(bs * n / (time.perf_counter() - t0))
    print(f"# model.detect() on YOLOv3TinyMobile 416x416 x {bs}, conf {conf} / iou {iou}: images/s per precision mode")
    print(f"\n{rounds} interleaved rounds in one process, {calls} calls per round (fp32: {max(3, calls // 5)}); "
          f"{torch.cuda.get_device_name(dev)}\n")
    print("| mode | " + " | ".join(f"round {r}" for r in range(rounds)) + " | median | vs bf16 | detections | launches |")
    print("|---|" + "---|" * (rounds + 4))
    med = {m: statistics.median(per_mode[m]) for m in modes}
    for m in modes:
        print(f"| {m} | " + " | ".join(f"{v:.0f}" for v in per_mode[m]) + f" | {med[m]:.0f} | {med[m] / med['bf16']:.3f} | {n_det[m]} | "
              f"{sum(kinds[m].values())} |")
    print(f"\nbf16 / fp32 = {med['bf16'] / med['fp32']:.2f}.  bf16 list: {kinds['bf16'][OP_MBCONV]} fused inverted-residual launches; fp32 list: "
          f"{kinds['fp32'][OP_DWCONV_F32]} OP_DWCONV_F32 launches (one thread per 4 channels of an output pixel: the one form that exists).")


def main():
    if "--model" in sys.argv:
        i = sys.argv.index("--model")
        which = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        if which == "mobile":
            return main_mobile(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
        if which != "spp":
            raise SystemExit(f"--model {which}: spp or mobile")
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    bs, hw, conf, iou = 32, 640, 0.1, 0.5
    model = YOLOv3SPP(n_class=80, anchors=SPP_ANCHORS).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234, n_class=80))
    model = model.to(dev)
    gather = YOLOv3SPP(n_class=80, anchors=SPP_ANCHORS).eval()
    gather.load_state_dict(model.state_dict())
    gather = gather.to(dev)
    gather.precision = "fp16"
    models = {m: (gather if m == GATHER else model) for m in MODES}
    x = torch.cat([synth_images(1, hw, hw, i) for i in range(bs)], 0).to(dev)
    per_mode = {m: [] for m in MODES}
    n_det, kinds = {}, {}
    with torch.no_grad():
        for m in MODES:                                    # plans, packed weights, first-launch costs
            model = models[m]
            if m != GATHER:
                model.precision = m
            old = os.environ.get("YOLO_FP16_T20")
            if m == GATHER:
                os.environ["YOLO_FP16_T20"] = "0"          # read when a plan is built: all of this model's are built in these calls
            try:
                for _ in range(2):
                    dets = model.detect(x, conf, iou)
            finally:
                if m == GATHER:
                    os.environ.pop("YOLO_FP16_T20") if old is None else os.environ.__setitem__("YOLO_FP16_T20", old)
            n_det[m] = sum(0 if d is None else len(d) for d in dets)
            kinds[m] = _op_kinds(model.plan_for(x))
        for rnd in range(rounds):
            for m in MODES:
                model = models[m]
                if m != GATHER:
                    model.precision = m
                n = calls if m != "fp32" else max(3, calls // 5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    model.detect(x, conf, iou)
                torch.cuda.synchronize()
                per_mode[m].append(bs * n / (time.perf_counter() - t0))
    print(f"# model.detect() on YOLOv3-SPP 640x640 x {bs}, conf {conf} / iou {iou}: images/s per precision mode")
    print(f"\n{rounds} interleaved rounds in one process, {calls} calls per round (fp32: {max(3, calls // 5)}); "
          f"{torch.cuda.get_device_name(dev)}\n")
    print("| mode | " + " | ".join(f"round {r}" for r in range(rounds)) + " | median | vs bf16 | detections |")
    print("|---|" + "---|" * (rounds + 3))
    med = {m: statistics.median(per_mode[m]) for m in MODES}
    for m in MODES:
        print(f"| {m} | " + " | ".join(f"{v:.0f}" for v in per_mode[m]) + f" | {med[m]:.0f} | {med[m] / med['bf16']:.3f} | {n_det[m]} |")
    print(f"\nfp16 / fp32 = {med['fp16'] / med['fp32']:.2f}; fp16 / fp16 gather-only = {med['fp16'] / med[GATHER]:.3f} "
          f"(smallest round of fp16 {min(per_mode['fp16']):.0f}, largest of gather-only {max(per_mode[GATHER]):.0f})")
    from pytorch_yolo_amd._lib import OP_CONV_F16, OP_CONV_T20_F16
    for m in ("fp16", GATHER):
        print(f"{m} launch list: {kinds[m][OP_CONV_T20_F16]} OP_CONV_T20_F16 (20x20-tile 3x3 kernels) + {kinds[m][OP_CONV_F16]} OP_CONV_F16 "
              f"(gather kernel) of {sum(kinds[m].values())} launches")
    if not all(a > b for a, b in zip(per_mode["fp16"], per_mode["fp32"])):
        raise SystemExit("fp16 detect() is not faster than the fp32 mode in this run")


if __name__ == "__main__":
    main()
