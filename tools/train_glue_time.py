#!/usr/bin/env python3
"""Time the layers between the convs of a training step (csrc/route.hip, yolo_bn_act_add_fwd) on the SPP-640 x 32 shapes, each against
the torch composition it replaces on the same device in the same run:

    yolo_bn_act_add_fwd               against  yolo_bn_act_fwd + torch add                          (the five residual maps)
    yolo_spp_train_fwd / yolo_spp_bwd against  three max_pool2d + cat, forward and autograd backward (20x20x512)
    yolo_upsample2_concat_fwd / _bwd  against  interpolate + cat, forward and autograd backward      (the two FPN joins)

and one whole forward + backward of YOLOv3-SPP at 640 x 8 (compute_loss on 40 seeded targets), split by op family: device events at the
first and the last launch of every op call, forward and backward (hooks on the op's outputs and inputs).

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU.

    python tools/train_glue_time.py --out profiles/train_glue_time.md
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

ADD_MAPS = [(320, 64), (160, 128), (80, 256), (40, 512), (20, 1024)]
SPP_MAP = (20, 512)
UPCAT = [(20, 256, 512), (40, 128, 256)]          # h of a, ca, cb
ANCHORS = (((10., 13.), (16., 30.), (33., 23.)), ((30., 61.), (62., 45.), (59., 119.)), ((116., 90.), (156., 198.), (373., 326.)))
HYPER = dict(iou_thresh=0.2, xy_loss=0.5, wh_loss=0.0625, cls_loss=0.03125, conf_loss=4.0)


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


def cell(times, s):
    return f"{min(times[s]):.1f} ({float(np.median(times[s])):.1f})"


def timed_ops(log):
    """DEVICE_OPS with device events at the start and the end of every call's forward and backward."""
    from pytorch_yolo_amd.models.train import DEVICE_OPS

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def wrap(family, fn):
        def call(*args, **kw):
            rec = dict(family=family, f0=mark())
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
            for o in (out if isinstance(out, tuple) else (out,)):
                o.register_hook(begin)
            return out
        return call
    return SimpleNamespace(**{name: wrap(name, fn) for name, fn in vars(DEVICE_OPS).items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--model-bs", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_glue_time.py: no GPU - nothing is measured")
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01
    from pytorch_yolo_amd.models.train import forward_train
    from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict
    dev, bf16, f32 = "cuda:0", torch.bfloat16, torch.float32
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen).to(bf16).to(dev)
    lines = [f"# Training glue: time per call on the SPP-640 x {n} shapes, and one training step of YOLOv3-SPP at 640 x {args.model_bs}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once; there is no",
             "threshold on these numbers.", "",
             "## yolo_bn_act_add_fwd against yolo_bn_act_fwd + torch add", "",
             "Bytes per element: fused 6 (read z, residual, write y; 8 with y_preadd), composition 10 (read z, write y, read y, read x, write out).", "",
             "| map | fused | fused TB/s | fused with y_preadd | bn_act_fwd | torch add | composition | fused / composition |", "|---|---|---|---|---|---|---|---|"]
    for m, c in ADD_MAPS:
        z, res = rnd(n, m, m, c), rnd(n, m, m, c)
        elems = z.numel()
        saved = torch.stack([torch.zeros(c), torch.ones(c), 1 + 0.1 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)]).to(dev)
        y, pre, out = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        t = windows([("fused", lambda: K.bn_act_add_fwd(z, saved, res, y, None, ACT_LEAKY01)),
                     ("fused_pre", lambda: K.bn_act_add_fwd(z, saved, res, y, pre, ACT_LEAKY01)),
                     ("act", lambda: K.bn_act_fwd(z, saved, pre, ACT_LEAKY01)),
                     ("add", lambda: torch.add(pre, res, out=out))], args.calls, args.repeats, args.warmup)
        comp = min(t["act"]) + min(t["add"])
        lines.append(f"| {m}x{m}x{c} | {cell(t, 'fused')} | {6 * elems / min(t['fused']) / 1e6:.2f} | {cell(t, 'fused_pre')} | {cell(t, 'act')} | "
                     f"{cell(t, 'add')} | {comp:.1f} | {min(t['fused']) / comp:.2f} |")
        del z, res, y, pre, out
    # ---- SPP
    m, c = SPP_MAP
    x, dy = rnd(n, m, m, c), rnd(n, m, m, 4 * c)
    y, idx, dx = torch.empty((n, m, m, 4 * c), dtype=bf16, device=dev), torch.empty((n, m, m, 3 * c), dtype=torch.uint8, device=dev), torch.empty_like(x)
    tx = x.permute(0, 3, 1, 2).detach().requires_grad_()
    tdy = dy.permute(0, 3, 1, 2)
    tfwd = lambda: torch.cat([F.max_pool2d(tx, k, 1, k // 2) for k in (5, 9, 13)] + [tx], 1)
    ty = tfwd()
    t = windows([("fwd", lambda: K.spp_train_fwd(x, y, idx)), ("bwd", lambda: K.spp_bwd(dy, idx, dx)), ("torch_fwd", tfwd),
                 ("torch_bwd", lambda: torch.autograd.grad(ty, tx, tdy, retain_graph=True))], args.calls, args.repeats, args.warmup)
    tdx, = torch.autograd.grad(ty, tx, tdy, retain_graph=True)
    agree = (bool(torch.equal(y.permute(0, 3, 1, 2), ty.detach())), float((dx.permute(0, 3, 1, 2).float() - tdx.float()).abs().max()))
    lines += ["", "## The SPP pair against three max_pool2d + cat with autograd", "",
              "| map | spp_train_fwd | spp_bwd | torch forward | torch backward | fwd / torch | bwd / torch |", "|---|---|---|---|---|---|---|",
              f"| {m}x{m}x{c} | {cell(t, 'fwd')} | {cell(t, 'bwd')} | {cell(t, 'torch_fwd')} | {cell(t, 'torch_bwd')} | "
              f"{min(t['fwd']) / min(t['torch_fwd']):.2f} | {min(t['bwd']) / min(t['torch_bwd']):.2f} |", "",
              f"Forward equal to torch's: {agree[0]}; largest |dx - torch dx| {agree[1]:.3g} (torch adds the four bf16 gradients pairwise, rounding each sum)."]
    del x, dy, y, idx, dx, tx, ty, tdx
    # ---- upsample + concat
    lines += ["", "## The upsample-concat pair against interpolate + cat with autograd", "",
              "| a, b | fwd | bwd (da and db) | torch forward | torch backward | fwd / torch | bwd / torch |", "|---|---|---|---|---|---|---|"]
    for h, ca, cb in UPCAT:
        a, b, dy = rnd(n, h, h, ca), rnd(n, 2 * h, 2 * h, cb), rnd(n, 2 * h, 2 * h, ca + cb)
        y, da, db = torch.empty_like(dy), torch.empty_like(a), torch.empty_like(b)
        ta, tb = a.permute(0, 3, 1, 2).detach().requires_grad_(), b.permute(0, 3, 1, 2).detach().requires_grad_()
        tdy = dy.permute(0, 3, 1, 2)
        tfwd = lambda: torch.cat([F.interpolate(ta, scale_factor=2, mode="nearest"), tb], 1)
        ty = tfwd()
        t = windows([("fwd", lambda: K.upsample2_concat_fwd(a, b, y)), ("bwd", lambda: K.upsample2_concat_bwd(dy, da, db, n=n, h=h, w=h, ca=ca, cb=cb)),
                     ("torch_fwd", tfwd), ("torch_bwd", lambda: torch.autograd.grad(ty, (ta, tb), tdy, retain_graph=True))],
                    args.calls, args.repeats, args.warmup)
        lines.append(f"| {h}x{h}x{ca}, {2 * h}x{2 * h}x{cb} | {cell(t, 'fwd')} | {cell(t, 'bwd')} | {cell(t, 'torch_fwd')} | {cell(t, 'torch_bwd')} | "
                     f"{min(t['fwd']) / min(t['torch_fwd']):.2f} | {min(t['bwd']) / min(t['torch_bwd']):.2f} |")
        del a, b, dy, y, da, db, ta, tb, ty
    # ---- one training step, by op family
    bs = args.model_bs
    model = Y.YOLOv3SPP(n_class=80, anchors=ANCHORS)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234, n_class=80))
    model.hyper_params = dict(HYPER)
    model = model.to(dev).train()
    x = synth_images(bs, 640, 640, seed=0).to(dev)
    rng = np.random.default_rng(0)
    targets = torch.from_numpy(np.concatenate([rng.integers(0, bs, (40, 1)), rng.integers(0, 80, (40, 1)), rng.uniform(0.2, 0.8, (40, 2)),
                                               rng.uniform(0.05, 0.4, (40, 2))], 1).astype(np.float32)).to(dev)
    steps = []
    for step in range(3):                                     # the last one is reported
        log = []
        model.zero_grad(set_to_none=True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        p = forward_train(model, x, ops=timed_ops(log))
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
    lines += ["", f"## One forward + backward of YOLOv3-SPP at 640 x {bs}, by op family", "",
              f"Third step of three (milliseconds; device events, so host gaps between launches count where the device waits for the host).  "
              f"Forward + loss {fwd_ms:.2f} ms, backward {bwd_ms:.2f} ms, step {fwd_ms + bwd_ms:.2f} ms = {bs / (fwd_ms + bwd_ms) * 1e3:.1f} images/s.  "
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
