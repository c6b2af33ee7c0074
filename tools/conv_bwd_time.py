#!/usr/bin/env python3
"""Time the conv backward (csrc/conv_bwd.hip) on the neck and head shapes of YOLOv3-SPP at 640 x 640, batch 32, each piece on its own -
prepare (g), weight + bias gradient, data gradient - beside this package's forward on the same shape and, as the yardstick, what a user
does today: torch's convolution backward (and leaky_relu backward) on bf16 channels-last tensors on the same device in the same run.

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU: there is nothing to time without one.

    python tools/conv_bwd_time.py --out profiles/conv_bwd_time.md
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, map, cin, cout, k, act, fp32 head)
SHAPES = [("20x20 1024->512 1x1", 20, 1024, 512, 1, "leaky", False),
          ("20x20 512->1024 3x3", 20, 512, 1024, 3, "leaky", False),
          ("40x40 256->512 3x3", 40, 256, 512, 3, "leaky", False),
          ("80x80 128->256 3x3", 80, 128, 256, 3, "leaky", False),
          ("head 20x20 1024->255 1x1", 20, 1024, 255, 1, "none", True),
          ("head 40x40 512->255 1x1", 40, 512, 255, 1, "none", True),
          ("head 80x80 256->255 1x1", 80, 256, 255, 1, "none", True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_bwd_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, DT_BF16, DT_F32
    dev = "cuda:0"
    bf16, f32 = torch.bfloat16, torch.float32
    aten = torch.ops.aten
    lines = ["# Conv backward: time per call on the SPP-640 x %d neck and head shapes" % args.bs, "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} "
             "windows per side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once;",
             "there is no threshold on these numbers.  FLOPs of wgrad = of the forward = 2 n h w cout k k cin.", "",
             "| shape | pick | prepare | bwd_weight | bwd_data | forward | wgrad TFLOP/s | wgrad / forward rate | torch act bwd | torch wgrad + bias | torch dgrad | ours total / torch total |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for name, m, cin, cout, k, act, head in SHAPES:
        gen = torch.Generator().manual_seed(1)
        n, h, w = args.bs, m, m
        ct, cg = (K.roundup(cout, 4) if head else cout), K.roundup(cout, 8)
        d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=ct, out_c_offset=0, ksize=k, stride=1,
                        act=ACT_LEAKY01 if act == "leaky" else ACT_NONE, kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128),
                        out_dtype=DT_F32 if head else DT_BF16)
        odt = f32 if head else bf16
        x = torch.randn((n, h, w, cin), generator=gen).to(bf16).to(dev)
        wt = (torch.randn((cout, cin, k, k), generator=gen) / (cin * k * k) ** 0.5).to(dev)
        bias = torch.zeros((d.cout_pad,), dtype=f32, device=dev)
        dy = torch.randn((n, h, w, cout), generator=gen).to(odt).to(dev)
        packed, _, _ = K.pack_conv_weight_dev(wt, cin)
        packed_t, _, _ = K.pack_conv_weight_dev(wt, cg, transposed=True)
        y = torch.empty((n, h, w, ct), dtype=odt, device=dev)
        g = torch.empty((n, h, w, cg), dtype=bf16, device=dev)
        ws = torch.empty((K.conv2d_bwd_workspace_bytes(d),), dtype=torch.uint8, device=dev)
        dw, db = torch.empty_like(wt), torch.empty((cout,), dtype=f32, device=dev)
        dx = torch.empty_like(x)
        K.conv2d(x, packed, bias, y, d)
        # the torch side: bf16 channels-last tensors, NCHW-shaped
        tx = x.permute(0, 3, 1, 2)
        tw = wt.to(bf16).contiguous(memory_format=torch.channels_last)
        ty = y[..., :cout].permute(0, 3, 1, 2).to(bf16).contiguous(memory_format=torch.channels_last)
        tdy = dy.permute(0, 3, 1, 2).to(bf16).contiguous(memory_format=torch.channels_last)
        tg = tdy.clone()
        conv_args = ([cout], [1, 1], [k // 2, k // 2], [1, 1], False, [0, 0], 1)
        sides = [("prepare", lambda: K.conv2d_bwd_prepare(dy, y, g, d)),
                 ("bwd_weight", lambda: K.conv2d_bwd_weight(x, g, dw, db, ws, d)),
                 ("bwd_data", lambda: K.conv2d_bwd_data(g, packed_t, dx, d)),
                 ("forward", lambda: K.conv2d(x, packed, bias, y, d)),
                 ("torch_act", (lambda: aten.leaky_relu_backward(tdy, ty, 0.1, True)) if act == "leaky" else None),
                 ("torch_wgrad", lambda: aten.convolution_backward(tg, tx, tw, *conv_args, [False, True, True])),
                 ("torch_dgrad", lambda: aten.convolution_backward(tg, tx, tw, *conv_args, [True, False, False]))]
        sides = [(s, fn) for s, fn in sides if fn is not None]
        for _, fn in sides:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the two computations agree (bf16 weight gradient on the torch side: compared at its precision)
        _, tdw, tdb = aten.convolution_backward(g[..., :cout].permute(0, 3, 1, 2), tx, tw, *conv_args, [False, True, True])
        worst = float((dw - tdw.float()).abs().max()) / float(dw.abs().max())
        # ... and so do the data gradients: both sides round dx once to bf16, on the same g and the same bf16 weight
        tdx, _, _ = aten.convolution_backward(g[..., :cout].permute(0, 3, 1, 2), tx, tw, *conv_args, [True, False, False])
        worst_dx = float((dx.float() - tdx.permute(0, 2, 3, 1).float()).abs().max()) / float(dx.float().abs().max())
        times = {s: [] for s, _ in sides}
        for _ in range(args.repeats):
            for s, fn in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[s].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        best = {s: min(v) for s, v in times.items()}
        cell = lambda s: f"{best[s]:.1f} ({float(np.median(times[s])):.1f})" if s in times else "-"
        flops = 2.0 * n * h * w * cout * k * k * cin
        ours = best["prepare"] + best["bwd_weight"] + best["bwd_data"]
        theirs = best.get("torch_act", 0.0) + best["torch_wgrad"] + best["torch_dgrad"]
        lines.append(f"| {name} | {K.conv2d_bwd_pick(d)} | {cell('prepare')} | {cell('bwd_weight')} | {cell('bwd_data')} | {cell('forward')} | "
                     f"{flops / best['bwd_weight'] / 1e6:.1f} | {best['forward'] / best['bwd_weight']:.2f} | {cell('torch_act')} | "
                     f"{cell('torch_wgrad')} | {cell('torch_dgrad')} | {ours / theirs:.2f} |")
        losers = [p for p, a, b in (("prepare", best["prepare"], best.get("torch_act", float("inf"))), ("wgrad", best["bwd_weight"], best["torch_wgrad"]),
                                    ("data gradient", best["bwd_data"], best["torch_dgrad"])) if a > b]
        notes.append(f"- {name}: ours {ours:.1f} us, torch {theirs:.1f} us; " + ("slower than torch in: " + ", ".join(losers) if losers else "no piece slower than torch") +
                     f"; largest |dW - torch dW| / max |dW| = {worst:.1e} (torch's dW is bf16), largest |dx - torch dx| / max |dx| = {worst_dx:.1e} (both bf16).")
    lines += ["", "Per shape, which piece loses to torch (best windows):", ""] + notes + [
        "", "The torch side is handed bf16 channels-last tensors and a bf16 weight (what `F.conv2d` autograd sees under bf16), its wgrad window",
        "includes the bias gradient, and for the heads (act none) it has no activation backward while ours still casts the fp32 dy to g.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
