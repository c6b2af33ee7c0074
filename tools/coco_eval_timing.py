#!/usr/bin/env python3
"""Time ``coco_eval`` on a synthetic set of COCO-val size: 5 000 images, 80 categories, about 100 detections and 7 ground-truth
boxes per image.

Three figures: the two kernel entry points on prepared operands (device events around ``--calls`` queued pairs after a warm-up,
``--repeats`` windows), the whole ``coco_eval`` call (wall clock: host flattening, the device sorts, the kernels, the download),
and - for scale - the numpy restatement of tests/_cocoeval.py on a 1/50 subset of the images.  Prints a markdown report (and
writes it to ``--out``).  Needs a GPU: there is nothing to time without one.

    python tools/coco_eval_timing.py --out profiles/coco_eval_time.md
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic(n_img, n_cat, dets_per_img, gts_per_img, seed=0):
    """Half of the detections are jittered copies of a ground-truth box of their image, the rest are random."""
    rng = np.random.default_rng(seed)
    images = [{"id": i + 1, "file_name": f"{i + 1:012d}.jpg", "height": 480, "width": 640} for i in range(n_img)]
    anns, results = [], []
    for i in range(n_img):
        n_gt = int(rng.poisson(gts_per_img))
        cats = rng.integers(1, n_cat + 1, n_gt)
        xy = rng.uniform(0, 400, (n_gt, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(240), (n_gt, 2)))
        for k in range(n_gt):
            box = [float(xy[k, 0]), float(xy[k, 1]), float(wh[k, 0]), float(wh[k, 1])]
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": int(cats[k]), "bbox": box,
                         "area": box[2] * box[3] * float(rng.uniform(0.4, 1.0)), "iscrowd": int(rng.integers(50) == 0)})
        n_dt = int(rng.poisson(dets_per_img))
        for _ in range(n_dt):
            if n_gt and rng.integers(2):
                k = int(rng.integers(n_gt))
                jit = rng.normal(0, 0.08, 4)
                box = [float(xy[k, 0] + jit[0] * wh[k, 0]), float(xy[k, 1] + jit[1] * wh[k, 1]), float(wh[k, 0] * np.exp(jit[2])),
                       float(wh[k, 1] * np.exp(jit[3]))]
                cat = int(cats[k])
            else:
                box = [float(v) for v in rng.uniform(0, 400, 2)] + [float(v) for v in np.exp(rng.uniform(np.log(8), np.log(240), 2))]
                cat = int(rng.integers(1, n_cat + 1))
            results.append({"image_id": i + 1, "category_id": cat, "bbox": box, "score": float(np.round(rng.uniform(0.1, 1.0), 3))})
    return {"images": images, "categories": [{"id": c, "name": f"c{c}"} for c in range(1, n_cat + 1)], "annotations": anns}, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--cats", type=int, default=80)
    ap.add_argument("--dets", type=float, default=100.0)
    ap.add_argument("--gts", type=float, default=7.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subset", type=int, default=50, help="the restatement runs on images / subset images")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_timing.py: no GPU - nothing is measured")
    import _cocoeval as E
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils import coco_eval as CE
    dev = torch.device("cuda:0")
    dataset, results = synthetic(args.images, args.cats, args.dets, args.gts)

    t0 = time.perf_counter()
    flat = CE.flatten(dataset, results)
    t_flatten = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op = CE.prepare(flat, dev)
    torch.cuda.synchronize()
    t_prepare = time.perf_counter() - t0
    n_img, n_cat, n_dt = len(flat["img_ids"]), len(flat["cat_ids"]), op["dt_box"].shape[0]
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    dt_match, dt_ignore = new((n_dt,), torch.int64), new((n_dt,), torch.int64)
    npig, status = new((n_cat, K.COCO_A), torch.int32), new((1,), torch.int32)
    iou_sum, iou_cnt = new((n_img * n_cat,), torch.float64), new((n_img * n_cat,), torch.int32)
    ws = new((K.coco_workspace_bytes(n_dt),), torch.uint8)
    precision = new((K.COCO_T, K.COCO_R, n_cat, K.COCO_A, K.COCO_M), torch.float64)
    recall = new((K.COCO_T, n_cat, K.COCO_A, K.COCO_M), torch.float64)
    iou_thrs, area_rng, rec_thrs = (torch.from_numpy(v).to(dev) for v in (CE.IOU_THRS, CE.AREA_RNG.reshape(-1), CE.REC_THRS))

    def match():
        K.coco_match_fwd(op["dt_box"], op["dt_off"], op["gt_box"], op["gt_area"], op["gt_crowd"], op["gt_off"], n_img, n_cat, op["max_gt"],
                         iou_thrs, area_rng, dt_match, dt_ignore, npig, iou_sum, iou_cnt, status, ws)

    def accumulate():
        K.coco_accumulate_fwd(op["order"], op["cat_off"], n_cat, dt_match, dt_ignore, npig, rec_thrs, CE.MAX_DETS, CE.EPS, ws, precision, recall)

    def window(fn):
        times = []
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / args.calls)
        return times
    t_match, t_acc = window(match), window(accumulate)
    assert int(status.item()) == 0

    whole = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = CE.coco_eval(dataset, results, dev)
        whole.append(time.perf_counter() - t0)

    n_sub = max(1, args.images // args.subset)
    sub = {"images": dataset["images"][:n_sub], "categories": dataset["categories"],
           "annotations": [a for a in dataset["annotations"] if a["image_id"] <= n_sub]}
    sub_results = [r for r in results if r["image_id"] <= n_sub]
    t0 = time.perf_counter()
    want = E.evaluate(sub, sub_results)
    t_numpy = time.perf_counter() - t0
    got = CE.coco_eval(sub, sub_results, dev)
    same = bool(np.array_equal(got.precision, want["precision"]) and np.array_equal(got.recall, want["recall"]))

    ms = lambda v: f"{v:.3f} ms"
    text = "\n".join([
        "# coco_eval: time on a synthetic set of COCO-val size",
        "",
        f"{n_img:,} images, {n_cat} categories, {len(results):,} results ({n_dt:,} after the cut to 100 per image and category), "
        f"{len(dataset['annotations']):,} annotations; {torch.cuda.get_device_name(0)}.",
        f"Kernel figures: device events around {args.calls} queued calls after {args.warmup} warm-up calls, {args.repeats} windows.  "
        "Measured once; there is no threshold on these numbers.",
        "",
        "| | |",
        "|---|---|",
        f"| yolo_coco_match_fwd (memsets + coco_match), best / median window | {ms(min(t_match))} / {ms(float(np.median(t_match)))} |",
        f"| yolo_coco_accumulate_fwd (coco_sweep, {n_cat * 120:,} workgroups), best / median window | {ms(min(t_acc))} / {ms(float(np.median(t_acc)))} |",
        f"| host flattening (numpy, from the Python dicts), once | {t_flatten:.2f} s |",
        f"| device orderings (four stable torch.sort calls, offsets, gathers; first call), once | {t_prepare * 1e3:.1f} ms |",
        f"| whole coco_eval call, wall clock, three calls | {', '.join(f'{v:.2f} s' for v in whole)} |",
        f"| numpy restatement (tests/_cocoeval.py) on the first {n_sub} images ({len(sub_results):,} results), wall clock | {t_numpy:.2f} s |",
        f"| ... coco_eval on that subset gives bit-equal precision / recall | {same} |",
        f"| stats of the whole set | {', '.join(f'{v:.4f}' for v in res.stats)} |",
        f"| Mean IOU of the whole set | {res.mean_iou:.6f} |",
        "",
        "The whole call is dominated by the host: building float64 arrays out of the result and annotation dictionaries.",
        ""])
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
