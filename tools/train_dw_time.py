#!/usr/bin/env python3
"""Time the depthwise gradients and the clamp pair of MobileNetV2's inverted residual as it trains (csrc/dw_train.hip, the clamp entries
of csrc/batchnorm.hip) on the depthwise maps of the 416 x 416 model, batch 32, each against what it stands beside on the
same device in the same run:

    yolo_dwconv3x3_bwd_data + yolo_dwconv3x3_bwd_weight   against  torch's autograd backward of F.conv2d(groups=c), bf16 channels-last
    yolo_bn_clamp_fwd / yolo_bn_clamp_bwd                 against  yolo_bn_act_fwd / yolo_bn_act_bwd (LeakyReLU) on the same maps

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window
(the helpers of tools/train_glue_time.py); prints a markdown report (and writes it to ``--out``).  Needs a GPU.

    python tools/train_dw_time.py --out profiles/train_dw_time.md
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from train_glue_time import cell, windows  # noqa: E402

# (input map, channels, stride) of the depthwise layers of MobileNetV2 at 416 x 416
DW_MAPS = [(208, 32, 1), (208, 96, 2), (104, 144, 1), (104, 144, 2), (52, 192, 1), (26, 384, 1), (26, 576, 1), (13, 960, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_dw_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01
    dev, bf16 = "cuda:0", torch.bfloat16
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen).to(bf16).to(dev)
    lines = [f"# Training MobileNetV2's inverted residual: time per call on the depthwise maps of the 416 model, batch {n}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once; these are reported",
             "ratios, not pass marks.", "",
             "## The depthwise gradients against torch's autograd backward of F.conv2d(groups=c)", "",
             "x, g bf16 channels-last in both; torch computes both gradients in one autograd.grad call.  TB/s: the bytes the launch has to move",
             "(data gradient: g and dx; weight gradient: x and g) over its time.", "",
             "| x | stride | bwd_data | TB/s | bwd_weight | TB/s | pick | torch backward | (data + weight) / torch |", "|---|---|---|---|---|---|---|---|---|"]
    for m, c, stride in DW_MAPS:
        mo = (m - 1) // stride + 1
        x, g = rnd(n, m, m, c), rnd(n, mo, mo, c)
        w = (torch.randn((c, 1, 3, 3), generator=gen) / 3).to(bf16).float().to(dev)
        w9c = w.reshape(c, 9).t().contiguous()
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty((K.dwconv3x3_bwd_weight_workspace_bytes(n, m, m, c, stride),), dtype=torch.uint8, device=dev)
        tx, tw = x.permute(0, 3, 1, 2).detach().requires_grad_(), w.to(bf16).requires_grad_()
        ty = F.conv2d(tx, tw, None, stride, 1, 1, c)
        tg = g.permute(0, 3, 1, 2)
        t = windows([("data", lambda: K.dwconv3x3_bwd_data(g, w9c, dx, stride)), ("weight", lambda: K.dwconv3x3_bwd_weight(x, g, dw, ws, stride)),
                     ("torch", lambda: torch.autograd.grad(ty, (tx, tw), tg, retain_graph=True))], args.calls, args.repeats, args.warmup)
        both = min(t["data"]) + min(t["weight"])
        lines.append(f"| {m}x{m}x{c} | {stride} | {cell(t, 'data')} | {2 * (g.numel() + dx.numel()) / min(t['data']) / 1e6:.2f} | {cell(t, 'weight')} | "
                     f"{2 * (x.numel() + g.numel()) / min(t['weight']) / 1e6:.2f} | {K.dwconv3x3_bwd_weight_pick(n, m, m, c, stride)} | {cell(t, 'torch')} | "
                     f"{both / min(t['torch']):.2f} |")
        del x, g, dx, tx, ty, tg, ws
    lines += ["", "## The clamp pair against yolo_bn_act_fwd / yolo_bn_act_bwd (LeakyReLU) on the same maps", "",
              "z, dy bf16; the forward moves z and y, the backward reads z and dy twice and writes g.  The kernels are the same, the activation is",
              "a kernel argument: the pair should cost the same.", "",
              "| z | clamp_fwd | act_fwd | fwd ratio | clamp_bwd | act_bwd | bwd ratio |", "|---|---|---|---|---|---|---|"]
    for m, c, stride in DW_MAPS:
        mo = (m - 1) // stride + 1
        z, dy = rnd(n, mo, mo, c), rnd(n, mo, mo, c)
        y, g = torch.empty_like(z), torch.empty_like(z)
        gamma, beta = torch.ones(c, device=dev), torch.full((c,), 2.0, device=dev)
        saved = torch.empty((4, c), device=dev)
        ws = torch.empty((K.bn_workspace_bytes(n * mo * mo, c),), dtype=torch.uint8, device=dev)
        dgamma, dbeta = torch.empty(c, device=dev), torch.empty(c, device=dev)
        K.bn_train_stats(z, gamma, beta, 1e-5, 0.1, None, None, saved, ws)
        t = windows([("cf", lambda: K.bn_clamp_fwd(z, saved, y, 0.0, 6.0)), ("af", lambda: K.bn_act_fwd(z, saved, y, ACT_LEAKY01)),
                     ("cb", lambda: K.bn_clamp_bwd(dy, z, saved, 0.0, 6.0, True, g, dgamma, dbeta, ws)),
                     ("ab", lambda: K.bn_act_bwd(dy, z, saved, ACT_LEAKY01, True, g, dgamma, dbeta, ws))], args.calls, args.repeats, args.warmup)
        lines.append(f"| {mo}x{mo}x{c} | {cell(t, 'cf')} | {cell(t, 'af')} | {min(t['cf']) / min(t['af']):.2f} | {cell(t, 'cb')} | {cell(t, 'ab')} | "
                     f"{min(t['cb']) / min(t['ab']):.2f} |")
        del z, dy, y, g, ws
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
