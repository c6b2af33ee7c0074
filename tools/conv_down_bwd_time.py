#!/usr/bin/env python3
"""Time the backward of the downsample (csrc/conv_down_bwd.hip) on the five 3x3 stride-2 layers of Darknet-53 in YOLOv3-SPP at 640 x 640,
batch 32, each piece on its own - prepare (g), the strided weight + bias gradient, the parity data gradient - beside this package's
forward on the same shape and two yardsticks from the same run on the same device:
  * torch's convolution backward (and leaky_relu backward) on bf16 channels-last tensors: what a user does today;
  * for the data gradient alone, the zero-insertion composition: g written into a zeroed full-resolution map and run through the
    stride-1 data gradient (yolo_conv2d_bwd_data, the forward dispatcher) - 4 x the FLOPs, the thing the parity kernel exists to beat.
    The stride-1 data gradient on the already zero-inserted map is also timed alone: the composition without its memset and copy.

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU: there is nothing to time without one.

    python tools/conv_down_bwd_time.py --out profiles/conv_down_bwd_time.md
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, input map, cin, cout)
SHAPES = [("640x640 32->64", 640, 32, 64),
          ("320x320 64->128", 320, 64, 128),
          ("160x160 128->256", 160, 128, 256),
          ("80x80 256->512", 80, 256, 512),
          ("40x40 512->1024", 40, 512, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_down_bwd_time.py: no GPU - nothing is measured")
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, DT_BF16
    dev = "cuda:0"
    bf16, f32 = torch.bfloat16, torch.float32
    aten = torch.ops.aten
    lines = ["# Downsample backward: time per call on the five 3x3 stride-2 layers of SPP-640 x %d" % args.bs, "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} "
             "windows per side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once;",
             "there is no threshold on these numbers.  FLOPs of wgrad = of dgrad = of the forward = 2 n ho wo cout 9 cin.  dgrad bytes = g + dx +",
             "the weight pack, each once.  zero-insert = memset of a full-resolution g, strided copy of g into it, stride-1 data gradient; conv alone =",
             "that stride-1 data gradient on the zero-inserted map without the memset and the copy (4 x the FLOPs, nothing else).", "",
             "| shape | prepare | wgrad | dgrad (parity) | forward | wgrad TFLOP/s | dgrad TFLOP/s | dgrad GB/s | torch act bwd | torch wgrad + bias | torch dgrad "
             "| zero-insert dgrad | of it: conv alone | wgrad / torch | dgrad / torch | dgrad / zero-insert | dgrad / conv alone | ours total / torch total |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    picks, notes = [], []
    for name, m, cin, cout in SHAPES:
        gen = torch.Generator().manual_seed(1)
        n, h, w = args.bs, m, m
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        common = dict(n=n, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, cout_pad=K.roundup(cout, 128),
                      out_dtype=DT_BF16)
        d = K.conv_desc(h=h, w=w, ksize=3, stride=2, act=ACT_LEAKY01, kpad=K.roundup(9 * cin, 64), **common)
        d1 = K.conv_desc(h=h, w=w, ksize=3, stride=1, act=ACT_LEAKY01, kpad=K.roundup(9 * cin, 64), **common)      # the zero-insertion's conv
        od = K.conv_desc(n=n, h=ho, w=wo, cin=cout, in_c_total=cout, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=1,
                         stride=1, act=ACT_LEAKY01, kpad=K.roundup(cout, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_BF16)
        x = torch.randn((n, h, w, cin), generator=gen).to(bf16).to(dev)
        wt = (torch.randn((cout, cin, 3, 3), generator=gen) / (9 * cin) ** 0.5).to(dev)
        bias = torch.zeros((d.cout_pad,), dtype=f32, device=dev)
        dy = torch.randn((n, ho, wo, cout), generator=gen).to(bf16).to(dev)
        packed, _, _ = K.pack_conv_weight_dev(wt, cin)
        packed_t, _, _ = K.pack_conv_weight_dev(wt, cout, transposed=True)
        packed_d = K.pack_conv_weight_down_dev(wt)
        y = torch.empty((n, ho, wo, cout), dtype=bf16, device=dev)
        g = torch.empty((n, ho, wo, cout), dtype=bf16, device=dev)
        gz = torch.empty((n, h, w, cout), dtype=bf16, device=dev)
        ws = torch.empty((K.conv2d_down_bwd_workspace_bytes(d),), dtype=torch.uint8, device=dev)
        dw, db = torch.empty_like(wt), torch.empty((cout,), dtype=f32, device=dev)
        dx, dxz = torch.empty_like(x), torch.empty_like(x)
        K.conv2d(x, packed, bias, y, d)
        K.conv2d_bwd_prepare(dy, y, g, od)
        tx = x.permute(0, 3, 1, 2)
        tw = wt.to(bf16).contiguous(memory_format=torch.channels_last)
        ty, tdy = y.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        tg = g.permute(0, 3, 1, 2)
        conv_args = ([cout], [2, 2], [1, 1], [1, 1], False, [0, 0], 1)

        def zero_insert():
            gz.zero_()
            gz[:, ::2, ::2] = g
            K.conv2d_bwd_data(gz, packed_t, dxz, d1)
        sides = [("prepare", lambda: K.conv2d_bwd_prepare(dy, y, g, od)),
                 ("wgrad", lambda: K.conv2d_down_bwd_weight(x, g, dw, db, ws, d)),
                 ("dgrad", lambda: K.conv2d_down_bwd_data(g, packed_d, dx, d)),
                 ("forward", lambda: K.conv2d(x, packed, bias, y, d)),
                 ("torch_act", lambda: aten.leaky_relu_backward(tdy, ty, 0.1, True)),
                 ("torch_wgrad", lambda: aten.convolution_backward(tg, tx, tw, *conv_args, [False, True, True])),
                 ("torch_dgrad", lambda: aten.convolution_backward(tg, tx, tw, *conv_args, [True, False, False])),
                 ("zero_insert", zero_insert),
                 ("conv_alone", lambda: K.conv2d_bwd_data(gz, packed_t, dxz, d1))]      # gz holds the zero-inserted g from the side before
        for _, fn in sides:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the computations agree: the parity kernel and the zero-insertion composition round the same sums; torch's dW and dx are bf16
        same = float((dx == dxz).double().mean())
        tdx, tdw, tdb = aten.convolution_backward(tg, tx, tw, *conv_args, [True, True, True])
        worst_w = float((dw - tdw.float()).abs().max()) / float(dw.abs().max())
        worst_x = float((dx.float() - tdx.permute(0, 2, 3, 1).float()).abs().max()) / float(dx.float().abs().max())
        del tdx
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
        cell = lambda s: f"{best[s]:.1f} ({float(np.median(times[s])):.1f})"
        flops = 2.0 * n * ho * wo * cout * 9 * cin
        dbytes = 2.0 * (g.numel() + dx.numel() + packed_d.numel())
        ours = best["prepare"] + best["wgrad"] + best["dgrad"]
        theirs = best["torch_act"] + best["torch_wgrad"] + best["torch_dgrad"]
        lines.append(f"| {name} | {cell('prepare')} | {cell('wgrad')} | {cell('dgrad')} | {cell('forward')} | {flops / best['wgrad'] / 1e6:.1f} | "
                     f"{flops / best['dgrad'] / 1e6:.1f} | {dbytes / best['dgrad'] / 1e3:.0f} | {cell('torch_act')} | {cell('torch_wgrad')} | "
                     f"{cell('torch_dgrad')} | {cell('zero_insert')} | {cell('conv_alone')} | {best['wgrad'] / best['torch_wgrad']:.2f} | "
                     f"{best['dgrad'] / best['torch_dgrad']:.2f} | {best['dgrad'] / best['zero_insert']:.2f} | "
                     f"{best['dgrad'] / best['conv_alone']:.2f} | {ours / theirs:.2f} |")
        picks.append(f"- {name}: `{K.conv2d_down_bwd_pick(d)}`")
        losers = [p for p, a, b in (("prepare (vs torch act bwd)", best["prepare"], best["torch_act"]), ("wgrad (vs torch)", best["wgrad"], best["torch_wgrad"]),
                                    ("dgrad (vs torch)", best["dgrad"], best["torch_dgrad"]),
                                    ("dgrad (vs the zero-insertion composition)", best["dgrad"], best["zero_insert"]),
                                    ("dgrad (vs the stride-1 conv of the composition alone)", best["dgrad"], best["conv_alone"])) if a > b]
        notes.append(f"- {name}: ours {ours:.1f} us, torch {theirs:.1f} us; " + ("slower in: " + ", ".join(losers) if losers else "no piece slower than a yardstick") +
                     f"; parity dx == zero-insertion dx on {100 * same:.3f} % of the elements; largest |dW - torch dW| / max |dW| = {worst_w:.1e}, "
                     f"|dx - torch dx| / max |dx| = {worst_x:.1e} (torch's are bf16 end to end).")
        del x, dy, y, g, gz, dx, dxz, tx, ty, tdy, tg
        torch.cuda.empty_cache()
    lines += ["", "Picks:", ""] + picks + ["", "Per shape, which piece loses to a yardstick (best windows):", ""] + notes + [
        "", "The torch side is handed bf16 channels-last tensors and a bf16 weight (what `F.conv2d` autograd sees under bf16); its wgrad window",
        "includes the bias gradient.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
