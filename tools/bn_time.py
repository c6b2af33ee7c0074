#!/usr/bin/env python3
"""Time the batch-norm passes of conv_bn_block (csrc/batchnorm.hip) on the three maps of YOLOv3-SPP at 640 x 640, batch 32 - 80x80x256,
40x40x512, 20x20x1024 - each entry on its own: the statistics, the normalise-and-activate pass, the backward's reduction (g = None) and
the whole backward.  The yardstick is what a user does today: torch's native_batch_norm + leaky_relu and their backwards on bf16
channels-last tensors on the same device in the same run.

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  ``--sweep`` also times the two reductions under other compute-unit shares
(yolo_set_launch_cus), i.e. other row-split counts: the table the split rule was chosen from.  Needs a GPU.

    python tools/bn_time.py --out profiles/bn_time.md --sweep 32,64,128,256,512,1024
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("80x80x256", 80, 256), ("40x40x512", 40, 512), ("20x20x1024", 20, 1024)]


def windows(sides, calls, repeats, warmup):
    for _, fn in sides:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {s: [] for s, _ in sides}
    for _ in range(repeats):
        for s, fn in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[s].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01
    dev = "cuda:0"
    bf16, f32 = torch.bfloat16, torch.float32
    aten = torch.ops.aten
    lines = ["# Batch norm of conv_bn_block: time per call on the SPP-640 x %d maps" % args.bs, "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} "
             "windows per side, the sides alternating window by window; best window (median) in microseconds per call, and bytes moved /",
             "best time in TB/s.  Bytes per element: statistics 2 (read z), normalise + activate 4 (read z, write y), backward reduction 4",
             "(read z, dy), whole backward 10 (the reduction, then read z, dy and write g); torch: native_batch_norm 6, leaky_relu 4,",
             "leaky_relu_backward 6, native_batch_norm_backward 10 (each tensor it touches counted once per pass over it).  Measured once;",
             "there is no threshold on these numbers.", "",
             "| map | pick | statistics | normalise + act | bwd reduction | whole backward | torch batch_norm | torch leaky_relu | torch leaky bwd | torch bn bwd | ours fwd / torch fwd | ours bwd / torch bwd |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes, sweep_lines = [], []
    shares = [int(v) for v in args.sweep.split(",") if v]
    for name, m, c in SHAPES:
        gen = torch.Generator().manual_seed(1)
        n, h, w = args.bs, m, m
        pixels, elems = n * h * w, n * h * w * c
        z = (torch.randn((n, h, w, c), generator=gen) + 0.5).to(bf16).to(dev)
        dy = torch.randn((n, h, w, c), generator=gen).to(bf16).to(dev)
        gamma, beta = (1 + 0.1 * torch.randn(c, generator=gen)).to(dev), (0.1 * torch.randn(c, generator=gen)).to(dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        saved = torch.empty((4, c), dtype=f32, device=dev)
        ws = torch.empty((K.bn_workspace_bytes(pixels, c),), dtype=torch.uint8, device=dev)
        y, g = torch.empty_like(z), torch.empty_like(z)
        dgamma, dbeta = torch.empty(c, dtype=f32, device=dev), torch.empty(c, dtype=f32, device=dev)
        K.bn_train_stats(z, gamma, beta, 1e-5, 0.1, rm, rv, saved, ws)
        # the torch side: bf16 channels-last tensors, NCHW-shaped
        tz, tdy = z.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        trm, trv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        tout, tmean, tinv = aten.native_batch_norm(tz, gamma, beta, trm, trv, True, 0.1, 1e-5)
        ty = aten.leaky_relu(tout, 0.1)
        tga = aten.leaky_relu_backward(tdy, tout, 0.1, False)
        sides = [("stats", lambda: K.bn_train_stats(z, gamma, beta, 1e-5, 0.1, rm, rv, saved, ws)),
                 ("act_fwd", lambda: K.bn_act_fwd(z, saved, y, ACT_LEAKY01)),
                 ("bwd_reduce", lambda: K.bn_act_bwd(dy, z, saved, ACT_LEAKY01, True, None, dgamma, dbeta, ws)),
                 ("bwd", lambda: K.bn_act_bwd(dy, z, saved, ACT_LEAKY01, True, g, dgamma, dbeta, ws)),
                 ("torch_bn", lambda: aten.native_batch_norm(tz, gamma, beta, trm, trv, True, 0.1, 1e-5)),
                 ("torch_act", lambda: aten.leaky_relu(tout, 0.1)),
                 ("torch_act_bwd", lambda: aten.leaky_relu_backward(tdy, tout, 0.1, False)),
                 ("torch_bn_bwd", lambda: aten.native_batch_norm_backward(tga, tz, gamma, trm, trv, tmean, tinv, True, 1e-5, [True, True, True]))]
        times = windows(sides, args.calls, args.repeats, args.warmup)
        # the two computations agree (torch's y and dx are bf16 of an fp32 computation with its own statistics: compared at bf16 precision)
        tdx, tdg, tdb = aten.native_batch_norm_backward(aten.leaky_relu_backward(tdy, tout, 0.1, False), tz, gamma, trm, trv, tmean, tinv, True,
                                                        1e-5, [True, True, True])
        agree = (float((y.permute(0, 3, 1, 2).float() - ty.float()).abs().max()), float((g.permute(0, 3, 1, 2).float() - tdx.float()).abs().max()),
                 float((dgamma - tdg.float()).abs().max() / tdg.float().abs().max()), float((dbeta - tdb.float()).abs().max() / tdb.float().abs().max()))
        best = {s: min(v) for s, v in times.items()}
        per = dict(stats=2, act_fwd=4, bwd_reduce=4, bwd=10, torch_bn=6, torch_act=4, torch_act_bwd=6, torch_bn_bwd=10)
        cell = lambda s: f"{best[s]:.1f} ({float(np.median(times[s])):.1f}) {per[s] * elems / best[s] / 1e6:.2f} TB/s"
        ours_f, torch_f = best["stats"] + best["act_fwd"], best["torch_bn"] + best["torch_act"]
        ours_b, torch_b = best["bwd"], best["torch_act_bwd"] + best["torch_bn_bwd"]
        lines.append(f"| {name} | {K.bn_pick(pixels, c)} | " + " | ".join(cell(s) for s, _ in sides) + f" | {ours_f / torch_f:.2f} | {ours_b / torch_b:.2f} |")
        notes.append(f"- {name}: forward ours {ours_f:.1f} us, torch {torch_f:.1f} us; backward ours {ours_b:.1f} us, torch {torch_b:.1f} us; "
                     f"largest |y - torch y| {agree[0]:.3g}, |g - torch dx| {agree[1]:.3g}, relative |dgamma - torch| {agree[2]:.1e}, |dbeta - torch| {agree[3]:.1e}.")
        for share in shares:
            K.set_launch_cus(share)
            try:
                ws_s = torch.empty((K.bn_workspace_bytes(pixels, c),), dtype=torch.uint8, device=dev)
                t = windows([("stats", lambda: K.bn_train_stats(z, gamma, beta, 1e-5, 0.1, rm, rv, saved, ws_s)),
                             ("bwd_reduce", lambda: K.bn_act_bwd(dy, z, saved, ACT_LEAKY01, True, None, dgamma, dbeta, ws_s))],
                            args.calls, args.repeats, args.warmup)
                sweep_lines.append(f"| {name} | {share} | {K.bn_pick(pixels, c)} | {min(t['stats']):.1f} ({float(np.median(t['stats'])):.1f}) | "
                                   f"{min(t['bwd_reduce']):.1f} ({float(np.median(t['bwd_reduce'])):.1f}) |")
            finally:
                K.set_launch_cus(256)
    lines += ["", "Per map (best windows):", ""] + notes
    if sweep_lines:
        lines += ["", "The two reductions (entry = reduction + finalize) under other compute-unit shares, i.e. other numbers of row splits:", "",
                  "| map | launch_cus | pick | statistics | bwd reduction |", "|---|---|---|---|---|"] + sweep_lines
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
