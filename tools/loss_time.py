#!/usr/bin/env python3
"""Time compute_loss(..., check=False) on the head shapes of YOLOv3-SPP at 640 x 640, batch 32, 80 classes, 512 targets.

Device events around ``--calls`` queued calls after a warm-up, repeated ``--repeats`` times; prints a markdown report (and writes it to
``--out``).  Needs a GPU: there is nothing to time without one.

    python tools/loss_time.py --out profiles/loss_time.md
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = (((10., 13.), (16., 30.), (33., 23.)), ((30., 61.), (62., 45.), (59., 119.)), ((116., 90.), (156., 198.), (373., 326.)))
HYPER = dict(iou_thresh=0.2, xy_loss=0.5, wh_loss=0.0625, cls_loss=0.03125, conf_loss=4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--targets", type=int, default=512)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd.utils.utils import compute_loss
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    layers, p, rows = [], [], []
    for i, group in enumerate(ANCHORS):
        n = args.size // (32 >> i)
        stride = args.size / n
        layers.append(types.SimpleNamespace(anchor_vec=torch.tensor(group, dtype=torch.float32, device=dev) / stride,
                                            n_grids=torch.tensor((n, n), dtype=torch.float32, device=dev), n_classes=args.nc))
        p.append((torch.randn((args.bs, 3, n, n, 5 + args.nc), device=dev) * 2.0).contiguous())
        rows.append(args.bs * 3 * n * n)
    model = types.SimpleNamespace(hyper_params=HYPER, n_class=args.nc, yolo_layers=layers)
    t = np.zeros((args.targets, 6), dtype=np.float32)
    t[:, 0] = rng.integers(0, args.bs, args.targets)
    t[:, 1] = rng.integers(0, args.nc, args.targets)
    t[:, 2:4] = rng.uniform(0.01, 0.99, (args.targets, 2))
    for k in range(args.targets):
        w, h = ANCHORS[int(rng.integers(0, 3))][int(rng.integers(0, 3))]
        t[k, 4:6] = np.asarray([w, h]) / args.size * np.exp(rng.uniform(-0.5, 0.5, 2))
    targets = torch.from_numpy(t).to(dev)

    for _ in range(args.warmup):
        loss, items = compute_loss(p, targets, model, check=False)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            loss, items = compute_loss(p, targets, model, check=False)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    total = sum(rows)
    line_bytes = total * 128 + total                  # one 128-byte line per row (word 4 only) + the tconf byte
    row_bytes = total * (5 + args.nc) * 4
    best, med = min(times), float(np.median(times))
    text = "\n".join([
        "# compute_loss(..., check=False): time per call",
        "",
        f"Head shapes of YOLOv3-SPP at {args.size} x {args.size}, batch {args.bs}, {args.nc} classes, {args.targets} targets; "
        f"{torch.cuda.get_device_name(0)}.",
        f"Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows.  Measured once; "
        "there is no threshold on this number.",
        "",
        "| | |",
        "|---|---|",
        f"| time per call, best window | {best:.1f} us |",
        f"| time per call, median window | {med:.1f} us |",
        f"| all windows (us per call) | {', '.join(f'{v:.1f}' for v in times)} |",
        f"| rows of the conf pass (bs x na x ny x nx over the layers) | {total:,} = {' + '.join(f'{r:,}' for r in rows)} |",
        f"| bytes the conf pass must touch (one 128-byte line per row + one tconf byte) | {line_bytes / 1e6:.1f} MB |",
        f"| ... over the best time | {line_bytes / best / 1e6:.2f} TB/s of lines |",
        f"| bytes of the whole ({5 + args.nc}-float) rows, which it does not read | {row_bytes / 1e6:.1f} MB |",
        f"| items of the last call (lxy, lwh, lconf, lcls, loss) | {', '.join(f'{v:.6g}' for v in items.tolist())} |",
        "",
        "The window holds everything a call enqueues: the memset of the tconf map, the assignment, conf, terms and finish kernels, and the",
        "Python between them (the launches are queued, so host time shows only where it exceeds the device time).",
        ""])
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
