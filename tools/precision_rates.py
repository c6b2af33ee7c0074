#!/usr/bin/env python3
"""images/s of model.detect() on SPP-640 x 32 in the three precision modes, interleaved in ONE process over several rounds (the chip's
clock and temperature drift between processes: only numbers from the same run compare).
    python tools/precision_rates.py [rounds] [calls per round]  > profiles/fp16_mode_rates.md"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_yolo_amd import YOLOv3SPP                                           # noqa: E402
from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict      # noqa: E402

SPP_ANCHORS = (((10., 13.), (16., 30.), (33., 23.)), ((30., 61.), (62., 45.), (59., 119.)), ((116., 90.), (156., 198.), (373., 326.)))
MODES = ("bf16", "fp16", "fp32")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    bs, hw, conf, iou = 32, 640, 0.1, 0.5
    model = YOLOv3SPP(n_class=80, anchors=SPP_ANCHORS).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234, n_class=80))
    model = model.to(dev)
    x = torch.cat([synth_images(1, hw, hw, i) for i in range(bs)], 0).to(dev)
    per_mode = {m: [] for m in MODES}
    n_det = {}
    with torch.no_grad():
        for m in MODES:                                    # plans, packed weights, first-launch costs
            model.precision = m
            for _ in range(2):
                dets = model.detect(x, conf, iou)
            n_det[m] = sum(0 if d is None else len(d) for d in dets)
        for rnd in range(rounds):
            for m in MODES:
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
    print(f"\nfp16 / fp32 = {med['fp16'] / med['fp32']:.2f}")
    if not all(a > b for a, b in zip(per_mode["fp16"], per_mode["fp32"])):
        raise SystemExit("fp16 detect() is not faster than the fp32 mode in this run")


if __name__ == "__main__":
    main()
