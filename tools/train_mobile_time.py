#!/usr/bin/env python3
"""Time expand_dw_bn_block (csrc/dw_train.hip's entries on a batch-normed operand) against the two ops it fuses, and one
training step of YOLOv3-tiny/MobileNetV2 with either op table, on the same device in the same run:

    expand_dw_bn_block                          against  dw_bn_block(conv_bn_relu6_block(..)), the form of models/train.mobile_ops(fused=False)
    forward_train(model, x, ops=mobile_ops())   against  forward_train(model, x, ops=mobile_ops(fused=False)), with compute_loss and backward

The op is timed on the maps of the 16 expanding blocks of the 416 x 416 model, batch 32 (nine distinct shapes): the forward alone (no
graph recorded) and forward + backward with every gradient asked for; beside the times, the bytes the forward has to move on each side
(the backward moves the same bytes on both) and the peak memory of one forward + backward.  Device events around ``--calls`` queued calls
after a warm-up, ``--repeats`` windows per side, the sides alternating window by window (the helpers of tools/train_glue_time.py); prints
a markdown report (and writes it to ``--out``).  Needs a GPU.

    python tools/train_mobile_time.py --out profiles/train_mobile_time.md
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from train_glue_time import HYPER, cell, windows  # noqa: E402

# (input map, cin, hidden, stride of the depthwise conv, blocks of that shape) of the expanding blocks of MobileNetV2 at 416 x 416
BLOCKS = [(208, 16, 96, 2, 1), (104, 24, 144, 1, 1), (104, 24, 144, 2, 1), (52, 32, 192, 1, 2), (52, 32, 192, 2, 1), (26, 64, 384, 1, 4),
          (26, 96, 576, 1, 2), (26, 96, 576, 2, 1), (13, 160, 960, 1, 3)]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2, help="training steps per window of the full-step timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_mobile_time.py: no GPU - nothing is measured")
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    dev, bf16 = "cuda:0", torch.bfloat16
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    fused, composed = MT.mobile_ops().expand_dw_bn_block, MT.mobile_ops(fused=False).expand_dw_bn_block
    lines = [f"# Training YOLOv3-tiny/MobileNetV2: the fused expand + depthwise op and one step, {args.size} x {args.size}, batch {n}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median).  Measured once; these are reported figures, not pass marks.", "",
             "## expand_dw_bn_block against dw_bn_block(conv_bn_relu6_block(..)) on the maps of the 16 expanding blocks", "",
             "Microseconds per call.  MB: what the forward's launches have to move - x + 5 H + 4 Ho composed, x + 3 H + 4 Ho fused, H the hidden",
             "map at the input resolution, Ho at the output resolution (the backward moves the same bytes on both sides: it reads z1 where the",
             "composed form reads y1).  Peak: the largest allocation above the operands during one forward + backward, in MB.", "",
             "| x | hidden | stride | blocks | fwd fused | fwd composed | ratio | fwd+bwd fused | fwd+bwd composed | ratio | MB fused | MB composed | peak fused | peak composed |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    total = dict(ff=0.0, fc=0.0, bf=0.0, bc=0.0, mf=0.0, mc=0.0, saved=0.0)
    for m, cin, hid, stride, count in BLOCKS:
        mo = (m - 1) // stride + 1
        x = torch.randn((n, cin, m, m), generator=gen).to(bf16).to(dev).contiguous(memory_format=torch.channels_last)
        dy = torch.randn((n, hid, mo, mo), generator=gen).to(bf16).to(dev).contiguous(memory_format=torch.channels_last)
        par = lambda t: t.to(dev).requires_grad_()
        we, wd = par(torch.randn((hid, cin, 1, 1), generator=gen) / cin ** 0.5), par(torch.randn((hid, 1, 3, 3), generator=gen) / 3)
        g1, b1, g2, b2 = par(torch.ones(hid)), par(torch.full((hid,), 2.5)), par(torch.ones(hid)), par(torch.full((hid,), 2.5))
        rs = [torch.zeros(hid, device=dev), torch.ones(hid, device=dev), torch.zeros(hid, device=dev), torch.ones(hid, device=dev)]
        xg = x.clone().requires_grad_()

        def fwd(op):
            with torch.no_grad():
                op(x, we, g1, b1, rs[0], rs[1], wd, g2, b2, rs[2], rs[3], stride=stride)

        def both(op):
            for t in (xg, we, g1, b1, wd, g2, b2):
                t.grad = None
            op(xg, we, g1, b1, rs[0], rs[1], wd, g2, b2, rs[2], rs[3], stride=stride).backward(dy)

        t = windows([("ff", lambda: fwd(fused)), ("fc", lambda: fwd(composed)), ("bf", lambda: both(fused)), ("bc", lambda: both(composed))],
                    args.calls, args.repeats, args.warmup)
        xb, hb, hob = 2 * x.numel(), 2 * n * m * m * hid, 2 * n * mo * mo * hid
        mf, mc = (xb + 3 * hb + 4 * hob) / 1e6, (xb + 5 * hb + 4 * hob) / 1e6
        pf, pc = peak_of(lambda: both(fused)) / 1e6, peak_of(lambda: both(composed)) / 1e6
        lines.append(f"| {m}x{m}x{cin} | {hid} | {stride} | {count} | {cell(t, 'ff')} | {cell(t, 'fc')} | {min(t['ff']) / min(t['fc']):.2f} | {cell(t, 'bf')} | "
                     f"{cell(t, 'bc')} | {min(t['bf']) / min(t['bc']):.2f} | {mf:.0f} | {mc:.0f} | {pf:.0f} | {pc:.0f} |")
        for k in ("ff", "fc", "bf", "bc"):
            total[k] += count * min(t[k])
        total["mf"] += count * mf
        total["mc"] += count * mc
        total["saved"] += count * hb / 1e6
        del x, dy, xg, we, wd
    lines += ["", f"Over the 16 blocks (best windows): forward {total['ff'] / 1e3:.2f} ms fused, {total['fc'] / 1e3:.2f} ms composed; forward + backward "
              f"{total['bf'] / 1e3:.2f} ms fused, {total['bc'] / 1e3:.2f} ms composed; the forward moves {total['mf'] / 1e3:.2f} GB fused, "
              f"{total['mc'] / 1e3:.2f} GB composed; the hidden maps not kept for the backward add up to {total['saved'] / 1e3:.2f} GB.", ""]

    # ---- one full step with either table
    from pytorch_yolo_amd.utils.synthetic import synth_images
    torch.manual_seed(0)
    model = Y.YOLOv3TinyMobile(n_class=80)
    model.hyper_params = dict(HYPER)
    with torch.no_grad():
        for mod in model.modules():                        # normalised values around 2.5: both bounds of every ReLU6 are met
            if isinstance(mod, torch.nn.Sequential) and len(mod) == 3 and isinstance(mod[2], torch.nn.ReLU6):
                mod[1].bias.fill_(2.5)
    model = model.to(dev).train()
    x = synth_images(n, args.size, args.size, seed=0).to(dev)
    rng = np.random.default_rng(0)
    targets = torch.from_numpy(np.concatenate([rng.integers(0, n, (40, 1)), rng.integers(0, 80, (40, 1)), rng.uniform(0.2, 0.8, (40, 2)),
                                               rng.uniform(0.05, 0.4, (40, 2))], 1).astype(np.float32)).to(dev)
    tables = {"fused": MT.mobile_ops(), "composed": MT.mobile_ops(fused=False)}

    def step(table):
        model.zero_grad(set_to_none=True)
        p = Y.forward_train(model, x, ops=table)
        loss, _ = Y.compute_loss(p, targets, model)
        loss.backward()

    t = windows([(name, (lambda table: lambda: step(table))(table)) for name, table in tables.items()], args.steps, args.repeats, args.warmup)
    peak = {name: peak_of(lambda: step(table)) for name, table in tables.items()}
    lines += [f"## One training step of YOLOv3TinyMobile(n_class=80), {args.size} x {args.size}, batch {n}: forward_train, compute_loss, backward", "",
              f"Windows of {args.steps} steps; milliseconds per step, best window (median); images/s from the best window; peak: the largest",
              "allocation of one step above the model and its inputs (torch.cuda.max_memory_allocated).", "",
              "| table | ms per step | images/s | windows (ms) | peak GB |", "|---|---|---|---|---|"]
    for name in tables:
        ms = [v / 1e3 for v in t[name]]
        lines.append(f"| {name} | {min(ms):.1f} ({float(np.median(ms)):.1f}) | {n / min(ms) * 1e3:.0f} | {', '.join(f'{v:.1f}' for v in ms)} | {peak[name] / 1e9:.2f} |")
    f_ms, c_ms = (np.asarray(t[k]) / 1e3 for k in ("fused", "composed"))
    spread = max(f_ms.max() - f_ms.min(), c_ms.max() - c_ms.min())
    verdict = "slower than the composed form by more than" if f_ms.min() - c_ms.min() > spread else "not slower than the composed form by more than"
    lines += ["", f"The fused table is {verdict} the spread between the windows of one side ({spread:.2f} ms; best windows {f_ms.min():.1f} against "
              f"{c_ms.min():.1f} ms): DEVICE_OPS_MOBILE is built with fused={'False' if f_ms.min() - c_ms.min() > spread else 'True'}.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
