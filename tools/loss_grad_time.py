#!/usr/bin/env python3
"""Time the gradient of compute_loss with respect to p (loss_grad_raw: yolo_loss_bwd) on the head shapes of YOLOv3-SPP at 640 x 640,
batch 32, 80 classes, 512 targets - the shapes of tools/loss_time.py - and, on the same device and inputs, torch autograd through a
torch restatement of the loss written below (reference utils/utils.py:124-157 on an assignment taken from build_targets).

Device events around ``--calls`` queued calls after a warm-up, repeated ``--repeats`` times, the two sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU: there is nothing to time without one.

    python tools/loss_grad_time.py --out profiles/loss_grad_time.md
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


def torch_loss(p, assignment, nc, bs):
    """The reference's loss in torch operations (the assignment - txy, twh, tcls, indices - is given: only the differentiable part)."""
    F = torch.nn.functional
    txy, twh, tcls, indices = assignment
    total = 0.0
    for i, pi0 in enumerate(p):
        b, a, gj, gi = indices[i]
        tconf = torch.zeros_like(pi0[..., 0])
        if len(b):
            pi = pi0[b, a, gj, gi]
            tconf[b, a, gj, gi] = 1
            total = total + (bs * HYPER["xy_loss"]) * F.mse_loss(torch.sigmoid(pi[..., 0:2]), txy[i])
            total = total + (bs * HYPER["wh_loss"]) * F.mse_loss(pi[..., 2:4], twh[i])
            if nc > 1:
                total = total + (bs * HYPER["cls_loss"]) * F.cross_entropy(pi[..., 5:], tcls[i])
            else:
                total = total + (bs * HYPER["cls_loss"]) * F.binary_cross_entropy_with_logits(pi[..., 5], tcls[i].float())
        total = total + (bs * HYPER["conf_loss"]) * F.binary_cross_entropy_with_logits(pi0[..., 4], tconf)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--targets", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_grad_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd.utils.utils import build_targets, compute_loss, loss_grad_raw
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
    assignment = build_targets(model, targets, bs=args.bs)
    kept = [len(ix[0]) for ix in assignment[3]]
    grad_loss = torch.ones((1,), dtype=torch.float32, device=dev)
    out = [torch.empty_like(x) for x in p]
    leaves = [x.detach().requires_grad_() for x in p]

    def kernel_call():
        loss_grad_raw(p, targets, model, grad_loss=grad_loss, out=out)

    def kernel_autograd_call():                       # forward + backward through compute_loss's own autograd Function
        for x in leaves:
            x.grad = None
        compute_loss(leaves, targets, model, check=False)[0].backward()

    def torch_backward_call(loss):                    # the backward alone, of a graph recorded before the window
        for x in leaves:
            x.grad = None
        loss.backward(retain_graph=True)

    def torch_call():                                 # forward + backward
        for x in leaves:
            x.grad = None
        torch_loss(leaves, assignment, args.nc, args.bs).backward()

    recorded = torch_loss(leaves, assignment, args.nc, args.bs)
    sides = [("loss_grad_raw (memset, assignment, dense and cells kernels)", kernel_call),
             ("torch autograd, backward only (graph recorded before the window)", lambda: torch_backward_call(recorded)),
             ("compute_loss(...).backward(): forward + backward kernels", kernel_autograd_call),
             ("torch restatement, forward + backward", torch_call)]
    for _, fn in sides:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    # the two gradients agree (the comparison is between two computations of the same thing)
    kernel_call()
    torch_call()
    worst = 0.0
    for g, x in zip(out, leaves):
        for sl in (slice(0, 2), slice(2, 4), slice(4, 5), slice(5, None)):
            top = float(x.grad[..., sl].abs().max())
            worst = max(worst, float((g[..., sl] - x.grad[..., sl]).abs().max()) / top)
    times = {name: [] for name, _ in sides}
    for _ in range(args.repeats):
        for name, fn in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    total = sum(rows)
    no = 5 + args.nc
    written = total * no * 4
    read = total * 128 + total                        # one 128-byte line per row (word 4 only) + the tconf byte
    best = {name: min(v) for name, v in times.items()}
    kbest = best[sides[0][0]]
    lines = [
        "# Gradient of compute_loss with respect to p: time per backward",
        "",
        f"Head shapes of YOLOv3-SPP at {args.size} x {args.size}, batch {args.bs}, {args.nc} classes, {args.targets} targets "
        f"(kept per layer: {kept}); {torch.cuda.get_device_name(0)}.",
        f"Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per side, the sides "
        "alternating window by window.  Measured once; there is no threshold on these numbers.",
        "",
        "| side | best window (us per call) | median | all windows |",
        "|---|---|---|---|"]
    for name, _ in sides:
        v = times[name]
        lines.append(f"| {name} | {min(v):.1f} | {float(np.median(v)):.1f} | {', '.join(f'{x:.1f}' for x in v)} |")
    lines += [
        "",
        "| | |",
        "|---|---|",
        f"| rows (bs x na x ny x nx over the layers) | {total:,} = {' + '.join(f'{r:,}' for r in rows)} |",
        f"| bytes the backward must write: the whole gradient tensors ({no} floats per row) | {written / 1e6:.1f} MB |",
        f"| bytes it must read: one 128-byte line per row (word 4) + one tconf byte | {read / 1e6:.1f} MB |",
        f"| ... together, over the best loss_grad_raw time | {(written + read) / kbest / 1e6:.2f} TB/s |",
        f"| ... the written bytes alone | {written / kbest / 1e6:.2f} TB/s |",
        f"| torch autograd backward only / loss_grad_raw (best windows) | {best[sides[1][0]] / kbest:.2f} x |",
        f"| torch forward + backward / compute_loss(...).backward() | {best[sides[3][0]] / best[sides[2][0]]:.2f} x |",
        f"| largest difference between the two gradients, per layer and word group, over the group's largest element | {worst:.2e} |",
        "",
        "The loss_grad_raw window holds everything a backward enqueues - the memset of the tconf map, the assignment, the dense and the",
        "cells kernels - and the Python between them (the launches are queued, so host time shows only where it exceeds the device",
        "time).  The torch side is handed the assignment (build_targets is not in its windows); its backward-only window replays a graph",
        "recorded once and holds the zero-filled gradient tensors, the index and BCE backward kernels and the accumulation into .grad.",
        ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
