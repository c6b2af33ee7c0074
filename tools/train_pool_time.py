#!/usr/bin/env python3
"""Time the max-pool layers of a training step (csrc/pool_train.hip, yolo_bn_act_pool_fwd) on the shapes of YOLOv3-tiny
at 416 x 416, batch 32, each against what it replaces on the same device in the same run:

    yolo_bn_act_pool_fwd                    against  yolo_bn_act_fwd + yolo_maxpool_train_fwd(stride 2)     (the four ConvPoolBlock maps)
    yolo_maxpool_train_fwd / yolo_maxpool_bwd  against  torch max_pool2d forward and autograd backward      (those maps and 26x26x256)

and one whole forward + backward of YOLOv3-tiny at 416 x 32 (compute_loss on 40 seeded targets), split by op: device events at the first
and the last launch of every op call, forward and backward (the method of tools/train_glue_time.py, whose helpers this script uses).

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU.

    python tools/train_pool_time.py --out profiles/train_pool_time.md
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from train_glue_time import HYPER, cell, windows  # noqa: E402

POOL_BN_MAPS = [(416, 16), (208, 32), (104, 64), (52, 128)]          # the four ConvPoolBlocks of sequence_1: the unpooled map and cout
POOL_MAPS = POOL_BN_MAPS + [(26, 256)]                                # ... and max_pool5


def timed_ops(log):
    """DEVICE_OPS_POOL with device events at the start and the end of every call's forward and backward."""
    from pytorch_yolo_amd.models.train import DEVICE_OPS_POOL

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def wrap(family, fn):
        def call(*args, **kw):
            if family == "pool_bn_block":
                family_ = f"pool_bn_block (pool stride {kw.get('pool_stride', 2)})"
            else:
                family_ = family
            rec = dict(family=family_, f0=mark())
            log.append(rec)
            args = list(args)
            for i, t in enumerate(args):                      # aliases of the tensors whose gradient ends this call's backward
                if isinstance(t, torch.Tensor) and t.requires_grad:
                    args[i] = t.view_as(t)
                    args[i].register_hook(lambda g, rec=rec: rec.__setitem__("b1", mark()))
            out = fn(*args, **kw)
            rec["f1"] = mark()

            def begin(g, rec=rec):
                if "b0" not in rec:
                    rec["b0"] = mark()
            out.register_hook(begin)
            return out
        return call
    return SimpleNamespace(**{name: wrap(name, fn) for name, fn in vars(DEVICE_OPS_POOL).items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_pool_time.py: no GPU - nothing is measured")
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01
    from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict
    dev, bf16 = "cuda:0", torch.bfloat16
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen).to(bf16).to(dev)
    lines = [f"# Training max-pools: time per call on the tiny-416 x {n} shapes, and one training step of YOLOv3-tiny at 416 x {n}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once; the only rule on",
             "these numbers is the ship rule of the fused entry: faster than its two-launch composition on each of the four maps.", "",
             "## yolo_bn_act_pool_fwd against yolo_bn_act_fwd + yolo_maxpool_train_fwd", "",
             "Bytes per element of z: fused 2.5 (read z, write the pooled y; 2.75 with the index plane), composition 6.5 + 0.25 (read z, write y,",
             "read y, write the pooled y and idx).  TB/s is 2.5 bytes per element over the fused time.", "",
             "| z | fused | fused TB/s | bn_act_fwd | maxpool_train_fwd | composition | fused / composition | bit-equal |", "|---|---|---|---|---|---|---|---|"]
    ship = True
    for m, c in POOL_BN_MAPS:
        z = rnd(n, m, m, c)
        elems = z.numel()
        saved = torch.stack([torch.zeros(c), torch.ones(c), (1 + 0.1 * torch.randn(c, generator=gen)) * torch.where(torch.arange(c) % 3 == 0, -1.0, 1.0),
                             0.1 * torch.randn(c, generator=gen)]).to(dev)
        full = torch.empty_like(z)
        y, y2 = (torch.empty((n, m // 2, m // 2, c), dtype=bf16, device=dev) for _ in range(2))
        idx, idx2 = (torch.empty((n, m // 2, m // 2, c), dtype=torch.uint8, device=dev) for _ in range(2))
        t = windows([("fused", lambda: K.bn_act_pool_fwd(z, saved, y, idx, ACT_LEAKY01)),
                     ("act", lambda: K.bn_act_fwd(z, saved, full, ACT_LEAKY01)),
                     ("pool", lambda: K.maxpool_train_fwd(full, y2, idx2, 2))], args.calls, args.repeats, args.warmup)
        comp = min(t["act"]) + min(t["pool"])
        equal = bool(torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(idx, idx2))
        ship = ship and min(t["fused"]) < comp
        lines.append(f"| {m}x{m}x{c} | {cell(t, 'fused')} | {2.5 * elems / min(t['fused']) / 1e6:.2f} | {cell(t, 'act')} | {cell(t, 'pool')} | "
                     f"{comp:.1f} | {min(t['fused']) / comp:.2f} | {equal} |")
        del z, full, y, y2, idx, idx2
    lines += ["", f"Ship rule (fused faster than the composition on each of the four maps): {'met' if ship else 'NOT met'}."]
    # ---- the pool pair against torch
    lines += ["", "## The pool pair against torch's max_pool2d with autograd", "",
              "x bf16 channels-last in both; torch's forward keeps int64 indices (8 bytes per pooled element against 1).", "",
              "| x | maxpool_train_fwd | maxpool_bwd | torch forward | torch backward | fwd / torch | bwd / torch | equal |", "|---|---|---|---|---|---|---|---|"]
    for m, c in POOL_MAPS:
        x, dy = rnd(n, m, m, c), rnd(n, m // 2, m // 2, c)
        y, idx, dx = torch.empty_like(dy), torch.empty(dy.shape, dtype=torch.uint8, device=dev), torch.empty_like(x)
        tx = x.permute(0, 3, 1, 2).detach().requires_grad_()
        tdy = dy.permute(0, 3, 1, 2)
        tfwd = lambda: F.max_pool2d(tx, 2, 2)
        ty = tfwd()
        t = windows([("fwd", lambda: K.maxpool_train_fwd(x, y, idx, 2)), ("bwd", lambda: K.maxpool_bwd(dy, idx, dx, 2)), ("torch_fwd", tfwd),
                     ("torch_bwd", lambda: torch.autograd.grad(ty, tx, tdy, retain_graph=True))], args.calls, args.repeats, args.warmup)
        tdx, = torch.autograd.grad(ty, tx, tdy, retain_graph=True)
        equal = bool(torch.equal(y.permute(0, 3, 1, 2), ty.detach()) and torch.equal(dx.permute(0, 3, 1, 2), tdx))
        lines.append(f"| {m}x{m}x{c} | {cell(t, 'fwd')} | {cell(t, 'bwd')} | {cell(t, 'torch_fwd')} | {cell(t, 'torch_bwd')} | "
                     f"{min(t['fwd']) / min(t['torch_fwd']):.2f} | {min(t['bwd']) / min(t['torch_bwd']):.2f} | {equal} |")
        del x, dy, y, idx, dx, tx, ty, tdx
    # ---- one training step, by op
    model = Y.YOLOv3Tiny(n_class=80)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234, n_class=80))
    model.hyper_params = dict(HYPER)
    model = model.to(dev).train()
    x = synth_images(n, 416, 416, seed=0).to(dev)
    rng = np.random.default_rng(0)
    targets = torch.from_numpy(np.concatenate([rng.integers(0, n, (40, 1)), rng.integers(0, 80, (40, 1)), rng.uniform(0.2, 0.8, (40, 2)),
                                               rng.uniform(0.05, 0.4, (40, 2))], 1).astype(np.float32)).to(dev)
    steps = []
    for step in range(3):                                     # the last one is reported
        log = []
        model.zero_grad(set_to_none=True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        p = Y.forward_train(model, x, ops=timed_ops(log))
        loss, _ = Y.compute_loss(p, targets, model)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        steps.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), log))
    fwd_ms, bwd_ms, log = steps[-1]
    fam = {}
    for rec in log:
        f = fam.setdefault(rec["family"], [0, 0.0, 0.0])
        f[0] += 1
        f[1] += rec["f0"].elapsed_time(rec["f1"])
        if "b0" in rec and "b1" in rec:
            f[2] += rec["b0"].elapsed_time(rec["b1"])
    lines += ["", f"## One forward + backward of YOLOv3-tiny at 416 x {n}, by op", "",
              f"Third step of three (milliseconds; device events, so host gaps between launches count where the device waits for the host).  "
              f"Forward + loss {fwd_ms:.2f} ms, backward {bwd_ms:.2f} ms, step {fwd_ms + bwd_ms:.2f} ms = {n / (fwd_ms + bwd_ms) * 1e3:.1f} images/s.  "
              "A call's backward runs from the hook on its output to the hook on its input (the first layer, whose input takes no gradient, has none).", "",
              "| op | calls | forward ms | backward ms |", "|---|---|---|---|"]
    for name, (cnt, f_ms, b_ms) in sorted(fam.items()):
        lines.append(f"| {name} | {cnt} | {f_ms:.2f} | {b_ms:.2f} |")
    tf, tb = sum(v[1] for v in fam.values()), sum(v[2] for v in fam.values())
    lines += [f"| between the ops (casts, pads, reshapes, the loss) | | {fwd_ms - tf:.2f} | {bwd_ms - tb:.2f} |", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
