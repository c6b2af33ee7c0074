#!/usr/bin/env python3
"""Capture tests/golden/train_tiny.npz and train_lite.npz from the REFERENCE itself: one training step of its YOLOv3Tiny and LiteYOLOv3 on
the CPU in float64 - ``p = model.train()(x)``, ``loss, items = compute_loss(p, targets, model)``, ``loss.backward()`` - on the
configuration of tests/_train_pool.py (YOLOv3Tiny kernels_divider 4, LiteYOLOv3 kernels_divider 2, 2 classes, and tests/_train.py's
2 x 3 x 64 x 96 input, synth_state_dict(seed 7), synth_images(seed 3), 8 seeded targets, tests/_loss.py's HYPER).  The last maps are 2 x 3,
the smallest the stride-1 pool takes.

This script holds no reference text: it imports the reference through ``make_golden.import_reference``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_pool.py

Per file, float64, the kinds of arrays of make_golden_train.py:
    p0, p1[, p2]                   the training-mode outputs [bs, 3, ny, nx, 5 + nc]
    gp0, gp1[, gp2]                the gradient of the loss at them (what the backward of the network starts from)
    items [5]                      lxy, lwh, lconf, lcls, loss
    grad/<parameter name>          every BN weight and bias, the first two conv weights, the parameters of the head convs
    rm/<module name>, rv/<...>     every BatchNorm2d's running_mean / running_var after the step
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (also puts the repository root and tests/ on sys.path)


def main():
    import _loss as L
    import _train as T
    import _train_pool as TP
    torch.set_num_threads(8)
    ref = MG.import_reference()
    U = sys.modules["pytorch_yolo.utils.utils"]
    for family, name in TP.MODELS.items():
        x, targets = TP.golden_inputs(family)
        model = T.load_synthetic(ref[family](**TP.CTORS[family])).double().train()
        model.hyper_params = dict(L.HYPER)
        p = model(x.double())
        for t in p:
            t.retain_grad()
        loss, items = U.compute_loss(p, targets.double(), model)
        loss.backward()
        arrs = {f"p{i}": t.detach().numpy() for i, t in enumerate(p)}
        arrs.update({f"gp{i}": t.grad.numpy() for i, t in enumerate(p)})
        arrs["items"] = items.detach().numpy().astype(np.float64)
        params = dict(model.named_parameters())
        for n in TP.stored_gradients(family, list(params)):
            g = params[n].grad
            assert g is not None and torch.isfinite(g).all(), n
            arrs["grad/" + n] = g.numpy()
        for n, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                assert int(m.num_batches_tracked) == 1
                arrs["rm/" + n], arrs["rv/" + n] = m.running_mean.numpy(), m.running_var.numpy()
        assert all(a.dtype == np.float64 for a in arrs.values())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrs)} arrays, loss {float(loss):.6f})")


if __name__ == "__main__":
    main()
