#!/usr/bin/env python3
"""Capture tests/golden/loss_grad.npz from the REFERENCE itself: ``loss.backward()`` of its ``compute_loss`` (utils/utils.py:124-157) on
the CPU, in fp32, on the inputs of tests/golden/loss.npz (cases A-E of tests/_loss.py).

Like make_golden_loss.py this script holds no reference text: it imports the reference through ``make_golden.import_reference``, builds
the reference's own ``YOLOLayer``s (``make_golden_loss.reference_model``), sets ``requires_grad_()`` on p and calls ``loss.backward()``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss_grad.py

Per case <c> and layer <i> the file holds
    <c>_g<i> float32, shaped like p[i]             the gradient, whole                                    (cases A, B, C, E)
    <c>_g<i>_conf float32 [bs, na, ny, nx]         its word-4 plane                                       (case D)
    <c>_g<i>_rows float32 [n_i, 5 + nc]            its rows at the cells of the kept targets, in order    (case D)
    <c>_L<i>_referr float64 [4]                    the reference's own fp32 error against the float64 restatement of
                                                   tests/_loss_grad.py, per word group (xy, wh, conf, class), in the measure defined there
    <c>_items float32 [5]                          the loss items of the same call (they equal those of loss.npz)
Of case D everything outside word 4 and the target rows is asserted to be +0.0 here, so nothing is lost by leaving it out; in every
case the zero pattern of the reference is asserted to equal the restatement's.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (also puts the repository root and tests/ on sys.path)
from make_golden_loss import reference_model  # noqa: E402


def main():
    import _loss as L
    import _loss_grad as LG
    torch.set_num_threads(8)
    MG.import_reference()
    U = sys.modules["pytorch_yolo.utils.utils"]
    from pytorch_yolo.models.yolo_layer import YOLOLayer
    fwd = np.load(os.path.join(HERE, "loss.npz"))
    arrs = {}
    for name, (groups, nc, bs, H, W, nt, seed, weighted) in L.CASES.items():
        layers, p, targets, cw, nc, bs = L.case_inputs(name)
        model = reference_model(YOLOLayer, layers, nc, H, W, L.HYPER)
        pt = [torch.from_numpy(t.copy()).requires_grad_() for t in p]
        loss, items = U.compute_loss(pt, torch.from_numpy(targets.copy()), model,
                                     class_weight=None if cw is None else torch.from_numpy(cw.copy()))
        assert not items.requires_grad and np.array_equal(items.numpy(), fwd[f"{name}_items"])
        loss.backward()
        want, asg = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw)
        arrs[f"{name}_items"] = items.numpy().astype(np.float32)
        for i, (t, w64, A) in enumerate(zip(pt, want, asg)):
            g = t.grad.numpy()
            assert g.dtype == np.float32 and g.shape == p[i].shape and np.isfinite(g).all()
            assert np.array_equal(g != 0, w64 != 0), f"case {name} layer {i}: the zero patterns differ"
            LG.assert_structure(g, A, f"case {name} layer {i} (reference)")
            err = LG.group_errors(g, w64)
            arrs[f"{name}_L{i}_referr"] = err
            print(f"case {name} layer {i}: reference fp32 vs float64 restatement: " +
                  ", ".join(f"{n} {v:.2e}" for (n, _), v in zip(LG.GROUPS, err)))
            if name in LG.FULL_CASES:
                arrs[f"{name}_g{i}"] = g.copy()
            else:
                arrs[f"{name}_g{i}_conf"] = g[..., 4].copy()
                arrs[f"{name}_g{i}_rows"] = g[A["b"], A["a"], A["gj"], A["gi"]].copy()
    path = os.path.join(HERE, "loss_grad.npz")
    np.savez_compressed(path, **arrs)
    print(f"loss_grad.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
