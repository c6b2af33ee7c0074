#!/usr/bin/env python3
"""Time the layers of a training step of YOLOv3-tiny/SqueezeNet that are no conv (csrc/fire_train.hip) on the maps of the
full-width model at 416 x 416, batch 32, each against what it replaces on the same device in the same run:

    yolo_maxpool3s2_train_fwd / yolo_maxpool3s2_bwd  against  torch max_pool2d(3, 2, ceil_mode=True) forward and autograd backward
    yolo_fire_bwd_split   against  two .contiguous() channel slices of dy + two yolo_conv2d_bwd_prepare launches (ReLU)
    yolo_fire_bwd_join    against  torch's bf16 add + one yolo_conv2d_bwd_prepare launch (ReLU)

the weight gradient of the unpadded first layer, the conv picks of the step (tests/_train_fire_families.py, no GPU needed for those), and
one whole forward + backward of the model (compute_loss on 40 seeded targets), split by op: device events at the first and the last
launch of every op call, forward and backward (the method of tools/train_glue_time.py, whose helpers this script uses).

Device events around ``--calls`` queued calls after a warm-up, ``--repeats`` windows per side, the sides alternating window by window;
prints a markdown report (and writes it to ``--out``).  Needs a GPU.

    python tools/train_fire_time.py --out profiles/train_fire_time.md
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from train_glue_time import HYPER, cell, windows  # noqa: E402

POOL_MAPS = [(207, 64), (103, 128), (51, 256)]                                   # the three pools: the unpooled map and its channels
FIRE_MAPS = [(103, 16, 64), (51, 32, 128), (25, 48, 192), (25, 64, 256)]          # map, squeeze and expand widths of the four Fire shapes


def timed_ops(log):
    """DEVICE_OPS_FIRE with device events at the start and the end of every call's forward and backward."""
    from pytorch_yolo_amd.models.train import DEVICE_OPS_FIRE

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
            out.register_hook(begin)
            return out
        return call
    return SimpleNamespace(**{name: wrap(name, fn) for name, fn in vars(DEVICE_OPS_FIRE).items()})


def relu_desc(K, pixels, cout, total, offset):
    from pytorch_yolo_amd._lib import ACT_RELU
    return K.conv_desc(n=1, h=pixels, w=1, cin=8, in_c_total=8, in_c_offset=0, cout=cout, out_c_total=total, out_c_offset=offset, ksize=1,
                       stride=1, act=ACT_RELU, kpad=64, cout_pad=K.roundup(cout, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_fire_time.py: no GPU - nothing is measured")
    import _train_fire_families as FF
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_RELU
    from pytorch_yolo_amd.utils.synthetic import synth_images, synth_state_dict
    dev, bf16 = "cuda:0", torch.bfloat16
    n = args.bs
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen).to(bf16).to(dev)
    lines = [f"# Training YOLOv3-tiny/SqueezeNet: time per call on the 416 x {n} maps, and one training step at 416 x {n}", "",
             f"{torch.cuda.get_device_name(0)}.  Device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows per",
             "side, the sides alternating window by window; best window (median) in microseconds per call.  Measured once; these are reported",
             "ratios, not pass marks.", "",
             "## The ceil-mode pool pair against torch's max_pool2d(3, 2, ceil_mode=True) with autograd", "",
             "x bf16 channels-last in both; torch's forward keeps int64 indices (8 bytes per pooled element against 1).  TB/s: the bytes the",
             "launch has to move (forward: x, y and idx; backward: dy, idx and dx) over its time.", "",
             "| x | maxpool3s2_train_fwd | TB/s | maxpool3s2_bwd | TB/s | torch forward | torch backward | fwd / torch | bwd / torch | equal |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for m, c in POOL_MAPS:
        x, dy = rnd(n, m, m, c), rnd(n, m // 2, m // 2, c)
        y, idx, dx = torch.empty_like(dy), torch.empty(dy.shape, dtype=torch.uint8, device=dev), torch.empty_like(x)
        tx = x.permute(0, 3, 1, 2).detach().requires_grad_()
        tdy = dy.permute(0, 3, 1, 2)
        tfwd = lambda: F.max_pool2d(tx, 3, 2, ceil_mode=True)
        ty = tfwd()
        t = windows([("fwd", lambda: K.maxpool3s2_train_fwd(x, y, idx)), ("bwd", lambda: K.maxpool3s2_bwd(dy, idx, dx)), ("torch_fwd", tfwd),
                     ("torch_bwd", lambda: torch.autograd.grad(ty, tx, tdy, retain_graph=True))], args.calls, args.repeats, args.warmup)
        tdx, = torch.autograd.grad(ty, tx, tdy, retain_graph=True)
        # (torch's bf16 backward adds with atomics in an order of its own: equal where a pixel has one term; reported, not required)
        equal = f"y {bool(torch.equal(y.permute(0, 3, 1, 2), ty.detach()))}, dx {100 * float((dx.permute(0, 3, 1, 2) == tdx).float().mean()):.2f} %"
        moved = 2 * x.numel() + 3 * dy.numel()
        lines.append(f"| {m}x{m}x{c} | {cell(t, 'fwd')} | {moved / min(t['fwd']) / 1e6:.2f} | {cell(t, 'bwd')} | {moved / min(t['bwd']) / 1e6:.2f} | "
                     f"{cell(t, 'torch_fwd')} | {cell(t, 'torch_bwd')} | {min(t['fwd']) / min(t['torch_fwd']):.2f} | "
                     f"{min(t['bwd']) / min(t['torch_bwd']):.2f} | {equal} |")
        del x, dy, y, idx, dx, tx, ty, tdx
    # ---- split and join against the compositions they replace
    lines += ["", "## yolo_fire_bwd_split against two .contiguous() slices + two prepare launches", "",
              "dy and y_cat bf16 [pixels][e1 + e3]; the composition copies each half of dy to a dense buffer (torch) and runs",
              "yolo_conv2d_bwd_prepare (ReLU) on it, reading y through its channel view.  TB/s: 6 bytes per element (dy, y, g) over the time.", "",
              "| concat map | split | TB/s | 2 x contiguous | 2 x prepare | composition | split / composition | bit-equal |", "|---|---|---|---|---|---|---|---|"]
    for m, sq, e in FIRE_MAPS:
        pixels = n * m * m
        ycat, dy = torch.relu(rnd(pixels, 2 * e)), rnd(pixels, 2 * e)
        g1, g3, c1, c3 = (torch.empty((pixels, e), dtype=bf16, device=dev) for _ in range(4))
        d1, d3 = relu_desc(K, pixels, e, 2 * e, 0), relu_desc(K, pixels, e, 2 * e, e)
        halves = [dy[:, :e].contiguous(), dy[:, e:].contiguous()]
        t = windows([("split", lambda: K.fire_bwd_split(dy, ycat, g1, g3)),
                     ("copy", lambda: (dy[:, :e].contiguous(), dy[:, e:].contiguous())),
                     ("prep", lambda: (K.conv2d_bwd_prepare(halves[0], ycat, c1, d1), K.conv2d_bwd_prepare(halves[1], ycat, c3, d3)))],
                    args.calls, args.repeats, args.warmup)
        comp = min(t["copy"]) + min(t["prep"])
        equal = bool(torch.equal(g1.view(torch.int16), c1.view(torch.int16)) and torch.equal(g3.view(torch.int16), c3.view(torch.int16)))
        lines.append(f"| {m}x{m}x{2 * e} | {cell(t, 'split')} | {6 * dy.numel() / min(t['split']) / 1e6:.2f} | {cell(t, 'copy')} | {cell(t, 'prep')} | "
                     f"{comp:.1f} | {min(t['split']) / comp:.2f} | {equal} |")
        del ycat, dy, g1, g3, c1, c3, halves
    lines += ["", "## yolo_fire_bwd_join against torch's bf16 add + one prepare launch", "",
              "d1, d3 and the squeeze output bf16 [pixels][sq].  TB/s: 8 bytes per element (d1, d3, s, g_s) over the time.", "",
              "| squeeze map | join | TB/s | add | prepare | composition | join / composition | bit-equal |", "|---|---|---|---|---|---|---|---|"]
    for m, sq, e in FIRE_MAPS:
        pixels = n * m * m
        s, a1, a3 = torch.relu(rnd(pixels, sq)), rnd(pixels, sq), rnd(pixels, sq)
        gs, c = (torch.empty((pixels, sq), dtype=bf16, device=dev) for _ in range(2))
        d = relu_desc(K, pixels, sq, sq, 0)
        tot = a1 + a3
        t = windows([("join", lambda: K.fire_bwd_join(a1, a3, s, gs)), ("add", lambda: a1 + a3), ("prep", lambda: K.conv2d_bwd_prepare(tot, s, c, d))],
                    args.calls, args.repeats, args.warmup)
        comp = min(t["add"]) + min(t["prep"])
        equal = bool(torch.equal(gs.view(torch.int16), c.view(torch.int16)))
        lines.append(f"| {m}x{m}x{sq} | {cell(t, 'join')} | {8 * s.numel() / min(t['join']) / 1e6:.2f} | {cell(t, 'add')} | {cell(t, 'prep')} | "
                     f"{comp:.1f} | {min(t['join']) / comp:.2f} | {equal} |")
        del s, a1, a3, gs, c, tot
    # ---- the first layer's weight gradient
    d = K.conv_desc(n=n, h=416, w=416, cin=8, in_c_total=8, in_c_offset=0, cout=64, out_c_total=64, out_c_offset=0, ksize=3, stride=2, act=ACT_RELU,
                    kpad=128, cout_pad=128, pad=0)
    x, g = rnd(n, 416, 416, 8), rnd(n, d.ho, d.wo, 64)
    dw, db = torch.empty((64, 8, 3, 3), device=dev), torch.empty((64,), device=dev)
    ws = torch.empty((K.conv2d_stem_bwd_workspace_bytes(d),), dtype=torch.uint8, device=dev)
    t = windows([("wgrad", lambda: K.conv2d_stem_bwd_weight(x, g, dw, db, ws, d))], args.calls, args.repeats, args.warmup)
    lines += ["", "## The weight gradient of the unpadded first layer", "",
              f"Conv2d(3 -> 64, 3x3, stride 2, pad 0) on {n} x 416 x 416 (cin padded to 8): {K.conv2d_stem_bwd_pick(d)}; both launches "
              f"{cell(t, 'wgrad')} us; {(x.numel() + g.numel()) * 2 / min(t['wgrad']) / 1e6:.2f} TB/s over the bytes of x and g read once."]
    del x, g
    # ---- the conv picks of the step
    count, rows = FF.enumerate_step()
    cus = K.set_launch_cus(256)
    K.set_launch_cus(cus)
    lines += ["", f"## The conv picks of the step ({cus} compute units)", "",
              "| call | layer (n, h, w, cin, cout, k) | forward | weight gradient | data gradient |", "|---|---|---|---|---|"]
    for kind, layer, stride, p in rows:
        lines.append(f"| {kind} | {layer} | {p['forward']} | {p['wgrad']} | {p.get('dgrad', '-')} |")
    # ---- one training step, by op
    model = Y.YOLOv3TinySqueeze(n_class=80)
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
    lines += ["", f"## One forward + backward of YOLOv3-tiny/SqueezeNet at 416 x {n}, by op", "",
              f"Third step of three (milliseconds; device events, so host gaps between launches count where the device waits for the host).  "
              f"Forward + loss {fwd_ms:.2f} ms, backward {bwd_ms:.2f} ms, step {fwd_ms + bwd_ms:.2f} ms = {n / (fwd_ms + bwd_ms) * 1e3:.1f} images/s; loss "
              f"{float(loss.detach()):.4f}, finite gradients: {all(bool(torch.isfinite(t.grad).all()) for t in model.parameters())}.  "
              "A call's backward runs from the hook on its output to the last hook on one of its inputs.", "",
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
