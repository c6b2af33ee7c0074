#!/usr/bin/env python3
"""Capture tests/golden/loss.npz from the REFERENCE itself: its ``compute_loss`` and ``build_targets`` (utils/utils.py:124-197) on the
CPU, and a few answers of its box helpers ``bbox_iou``, ``wh_iou`` and ``xyxy2xywh``.

This script holds no reference text: it imports the reference through ``make_golden.import_reference`` (so it runs only where
make_golden.py runs), takes the functions from the loaded ``pytorch_yolo.utils.utils``, builds the reference's own ``YOLOLayer``s
(``img_size = max(H, W)``, ``n_x_grids`` / ``n_y_grids``, ``create_grids()``) and hangs them on a plain namespace with ``hyper_params``
and ``n_class``.  Inputs come from the seeded generator of tests/_loss.py (cases A-E, seeds in _loss.CASES: seed 0 satisfied the input
conditions in every case, so no seed was skipped).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss.py

Per case <c> the file holds
    <c>_targets [nt, 6]                          the generated targets
    <c>_L<i>_{b,a,gj,gi,tcls} int64 [n_i]        the reference's assignment per layer;  <c>_L<i>_{txy,twh} float32 [n_i, 2]
    <c>_items float32 [5]                        lxy, lwh, lconf, lcls, loss
    <c>_p<i>_sum float64                         the sum of the regenerated p of layer i: a drifted generator fails as such
and, on the 8 fixed boxes below: box_xyxy, xyxy2xywh, bbox_iou_xyxy / bbox_iou_xywh [8, 8] (row i = box i against all), wh_iou [8, 8].
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (also puts the repository root and tests/ on sys.path)

# 8 fixed boxes (x1, y1, x2, y2): overlapping, nested, touching, disjoint, one degenerate
BOXES = np.asarray([[10, 10, 50, 40], [20, 15, 60, 45], [12, 12, 30, 30], [50, 10, 90, 40], [100, 100, 130, 160], [0, 0, 200, 200],
                    [49.5, 39.5, 80.25, 70.75], [70, 70, 70, 90]], dtype=np.float32)


def reference_model(ref_layer_cls, layers, nc, H, W, hyper):
    ys = []
    for L in layers:
        y = ref_layer_cls(list(L["anchors_px"]), nc, None)
        y.img_size, y.n_x_grids, y.n_y_grids = max(H, W), L["nx"], L["ny"]
        y.create_grids()
        assert np.array_equal(y.anchor_vec.numpy(), L["anchor_vec"]), "tests/_loss.make_layers does not form anchor_vec like the reference"
        ys.append(y)
    return types.SimpleNamespace(hyper_params=dict(hyper), n_class=nc, yolo_layers=ys)


def main():
    import _loss as L
    torch.set_num_threads(8)
    MG.import_reference()
    U = sys.modules["pytorch_yolo.utils.utils"]
    from pytorch_yolo.models.yolo_layer import YOLOLayer
    arrs = {}
    for name, (groups, nc, bs, H, W, nt, seed, weighted) in L.CASES.items():
        layers, p, targets, cw, nc, bs = L.case_inputs(name)
        model = reference_model(YOLOLayer, layers, nc, H, W, L.HYPER)
        tt = torch.from_numpy(targets.copy())
        if nt:
            ious = [torch.stack([U.wh_iou(x, tt[:, 4:6] * y.n_grids) for x in y.anchor_vec], 0).numpy() for y in model.yolo_layers]
            cond = L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc, ious=ious)
            L.assert_conditions(cond, f"case {name} (seed {seed})")
            print(f"case {name}: seed {seed}, kept {cond['kept']} of {nt}, duplicate cells {cond['duplicates']}, rejected everywhere "
                  f"{cond['rejected_everywhere']}, threshold margin {cond['thr_gap']:.2e}, anchor margin {cond['top_gap']:.2e}")
        txy, twh, tcls, indices = U.build_targets(model, tt)
        with torch.no_grad():
            loss, items = U.compute_loss([torch.from_numpy(t.copy()) for t in p], tt, model,
                                         class_weight=None if cw is None else torch.from_numpy(cw.copy()))
        assert loss.shape == (1,) and items.shape == (5,) and items.dtype == torch.float32
        arrs[f"{name}_targets"] = targets
        arrs[f"{name}_items"] = items.numpy().astype(np.float32)
        for i in range(len(layers)):
            b, a, gj, gi = indices[i]
            # (with no targets the reference leaves `a` an empty list)
            for k, v in (("b", b), ("a", a), ("gj", gj), ("gi", gi), ("tcls", tcls[i])):
                arrs[f"{name}_L{i}_{k}"] = np.asarray(v if not isinstance(v, torch.Tensor) else v.numpy(), dtype=np.int64).reshape(-1)
            arrs[f"{name}_L{i}_txy"] = txy[i].numpy().astype(np.float32).reshape(-1, 2)
            arrs[f"{name}_L{i}_twh"] = twh[i].numpy().astype(np.float32).reshape(-1, 2)
            arrs[f"{name}_p{i}_sum"] = np.float64(p[i].astype(np.float64).sum())
        print(f"case {name}: items {arrs[f'{name}_items']}")
    box = torch.from_numpy(BOXES.copy())
    xywh = U.xyxy2xywh(box)
    arrs["box_xyxy"] = BOXES
    arrs["xyxy2xywh"] = xywh.numpy()
    arrs["bbox_iou_xyxy"] = torch.stack([U.bbox_iou(b, box) for b in box]).numpy()
    arrs["bbox_iou_xywh"] = torch.stack([U.bbox_iou(b, xywh, x1y1x2y2=False) for b in xywh]).numpy()
    arrs["wh_iou"] = torch.stack([U.wh_iou(b, xywh[:, 2:4]) for b in xywh[:, 2:4]]).numpy()
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **arrs)
    print(f"loss.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
