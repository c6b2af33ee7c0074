#!/usr/bin/env python3
"""Time the ops of a training step of YOLOv3-tiny/ShuffleNetV2 (csrc/shuffle_train.hip) against the forms they replace,
and one training step with either op table, on the same device in the same run:

    max_pool_321                                 against  torch's F.max_pool2d(x, 3, 2, 1), forward and autograd backward, on the model's map
    shuffle_unit_block                           against  the composition on two slices of x, the form of models/train.shuffle_ops(fused=False)
    forward_train(model, x, ops=shuffle_ops())   against  forward_train(model, x, ops=shuffle_ops(fused=False)), with compute_loss and backward

The unit is timed on the maps of the 13 stride-1 units of the 416 x 416 model, batch 32 (three distinct shapes, in the padded physical
layout the wiring runs in): the forward alone (no graph recorded) and forward + backward with every gradient asked for; beside the times,
the peak memory of one forward + backward.  Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side,
the sides alternating window by window (the helpers of tools/train_glue_time.py); prints a markdown report (and writes it to ``--out``).
Needs a GPU.

    python tools/train_shuffle_time.py --out profiles/train_shuffle_time.md
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

# (map, half, slot, units of that shape) of the stride-1 units of ShuffleNetV2 x1.0 at 416 x 416
UNITS = [(52, 58, 64, 3), (26, 116, 128, 7), (13, 232, 256, 3)]
POOL_MAP = (208, 32)                  # conv1's output: 24 channels in 32


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
        raise SystemExit("train_shuffle_time.py: no GPU - nothing is measured")
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    dev, bf16 = "cuda:0", torch.bfloat16
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    cl = lambda t: t.to(bf16).to(dev).contiguous(memory_format=torch.channels_last)
    lines = [f"# Training YOLOv3-tiny/ShuffleNetV2: the pool, the fused stride-1 unit and one step, {args.size} x {args.size}, batch {n}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median).  Measured once; these are reported figures, not pass marks.", ""]

    # ---- the pool
    m, c = POOL_MAP
    x = cl(torch.randn((n, c, m, m), generator=gen))
    mo = (m - 1) // 2 + 1
    dy = cl(torch.randn((n, c, mo, mo), generator=gen))
    xg = x.clone().requires_grad_()

    def pool_fwd(op):
        with torch.no_grad():
            op(x)

    def pool_both(op):
        xg.grad = None
        op(xg).backward(dy)

    ours, theirs = Y.max_pool_321, (lambda t: torch.nn.functional.max_pool2d(t, 3, 2, 1))
    t = windows([("ff", lambda: pool_fwd(ours)), ("fc", lambda: pool_fwd(theirs)), ("bf", lambda: pool_both(ours)), ("bc", lambda: pool_both(theirs))],
                args.calls, args.repeats, args.warmup)
    lines += [f"## max_pool_321 against torch's max_pool2d(3, 2, 1) on the {m} x {m} x {c} map (bf16, channels-last)", "",
              "Microseconds per call; torch's backward is its autograd's.", "",
              "| fwd ours | fwd torch | ratio | fwd+bwd ours | fwd+bwd torch | ratio |", "|---|---|---|---|---|---|",
              f"| {cell(t, 'ff')} | {cell(t, 'fc')} | {min(t['ff']) / min(t['fc']):.2f} | {cell(t, 'bf')} | {cell(t, 'bc')} | {min(t['bf']) / min(t['bc']):.2f} |", ""]
    del x, dy, xg

    # ---- the unit
    fused, composed = MT.shuffle_ops().shuffle_unit_block, MT.shuffle_ops(fused=False).shuffle_unit_block
    lines += ["## shuffle_unit_block against the composition on two slices of x, on the maps of the 13 stride-1 units", "",
              "Microseconds per call.  Peak: the largest allocation above the operands during one forward + backward, in MB.", "",
              "| x | half | units | fwd fused | fwd composed | ratio | fwd+bwd fused | fwd+bwd composed | ratio | peak fused | peak composed |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    total = dict(ff=0.0, fc=0.0, bf=0.0, bc=0.0)
    for m, half, slot, count in UNITS:
        live = torch.zeros(slot)
        live[:half] = 1.0
        x = cl(torch.randn((n, 2 * slot, m, m), generator=gen) * torch.cat([live, live]).reshape(1, -1, 1, 1))
        dy = cl(torch.randn((n, 2 * slot, m, m), generator=gen))
        par = lambda t: t.to(dev).requires_grad_()
        pw = lambda: par(torch.randn((slot, slot, 1, 1), generator=gen) / half ** 0.5 * live.reshape(-1, 1, 1, 1) * live.reshape(1, -1, 1, 1))
        w1, w3, wd = pw(), pw(), par(torch.randn((slot, 1, 3, 3), generator=gen) / 3 * live.reshape(-1, 1, 1, 1))
        vecs = [par(torch.ones(slot)) if i % 2 == 0 else par(0.5 * live) for i in range(6)]
        rs = [torch.zeros(slot, device=dev) if i % 2 == 0 else torch.ones(slot, device=dev) for i in range(6)]
        xg = x.clone().requires_grad_()

        def call(op, xin):
            return op(xin, half, w1, vecs[0], vecs[1], rs[0], rs[1], wd, vecs[2], vecs[3], rs[2], rs[3], w3, vecs[4], vecs[5], rs[4], rs[5])

        def fwd(op):
            with torch.no_grad():
                call(op, x)

        def both(op):
            for p in [xg, w1, w3, wd] + vecs:
                p.grad = None
            call(op, xg).backward(dy)

        t = windows([("ff", lambda: fwd(fused)), ("fc", lambda: fwd(composed)), ("bf", lambda: both(fused)), ("bc", lambda: both(composed))],
                    args.calls, args.repeats, args.warmup)
        pf, pc = peak_of(lambda: both(fused)) / 1e6, peak_of(lambda: both(composed)) / 1e6
        lines.append(f"| {m}x{m}x{2 * slot} | {half} | {count} | {cell(t, 'ff')} | {cell(t, 'fc')} | {min(t['ff']) / min(t['fc']):.2f} | {cell(t, 'bf')} | "
                     f"{cell(t, 'bc')} | {min(t['bf']) / min(t['bc']):.2f} | {pf:.0f} | {pc:.0f} |")
        for k in total:
            total[k] += count * min(t[k])
        del x, dy, xg, w1, w3, wd
    lines += ["", f"Over the 13 units (best windows): forward {total['ff'] / 1e3:.2f} ms fused, {total['fc'] / 1e3:.2f} ms composed; forward + backward "
              f"{total['bf'] / 1e3:.2f} ms fused, {total['bc'] / 1e3:.2f} ms composed.", ""]

    # ---- one full step with either table
    from pytorch_yolo_amd.utils.synthetic import synth_images
    torch.manual_seed(0)
    model = Y.YOLOv3TinyShuffle(n_class=80)
    model.hyper_params = dict(HYPER)
    model = model.to(dev).train()
    x = synth_images(n, args.size, args.size, seed=0).to(dev)
    rng = np.random.default_rng(0)
    targets = torch.from_numpy(np.concatenate([rng.integers(0, n, (40, 1)), rng.integers(0, 80, (40, 1)), rng.uniform(0.2, 0.8, (40, 2)),
                                               rng.uniform(0.05, 0.4, (40, 2))], 1).astype(np.float32)).to(dev)
    tables = {"fused": MT.shuffle_ops(), "composed": MT.shuffle_ops(fused=False)}

    def step(table):
        model.zero_grad(set_to_none=True)
        p = Y.forward_train(model, x, ops=table)
        loss, _ = Y.compute_loss(p, targets, model)
        loss.backward()

    t = windows([(name, (lambda table: lambda: step(table))(table)) for name, table in tables.items()], args.steps, args.repeats, args.warmup)
    peak = {name: peak_of(lambda: step(table)) for name, table in tables.items()}
    lines += [f"## One training step of YOLOv3TinyShuffle(n_class=80), {args.size} x {args.size}, batch {n}: forward_train, compute_loss, backward", "",
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
              f"{c_ms.min():.1f} ms).", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
