"""The oracle of the COCO evaluation tests: an independent numpy restatement of pycocotools' bbox COCOeval (evaluate / accumulate /
summarize, written from the published algorithm with plain loops, image by image, in float64) and of the reference's "Mean IOU"
(utils/utils.py:338-348), a seeded case generator, and hand-derived known answers.

pycocotools itself is not installed where these tests were written: parity with the real library is UNPINNED there
(test_cocoeval_cpu.test_restatement_vs_pycocotools runs wherever the library exists)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
STAT_NAMES = ["AP", "AP50", "AP75", "APS", "APM", "APL", "AR1", "AR10", "AR100", "ARS", "ARM", "ARL"]


def bb_iou(d, g, crowd):
    """maskApi bbIou for one pair of (x, y, w, h) boxes."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    da = d[2] * d[3]
    u = da if crowd else da + g[2] * g[3] - i
    return i / u


def evaluate(dataset, results):
    """Returns a dict: img_ids, cat_ids, precision [T, R, K, A, M], recall [T, K, A, M], stats [12], mean_iou, npig [K, A], and
    ``groups``: {(image index, category index): dict(order = indices into ``results`` in evaluation order,
    matched [A, T, D] bool, ignore [A, T, D] bool, iou_sum, iou_cnt)} for every pair that has detections."""
    img_ids = sorted(set(im["id"] for im in dataset["images"]))
    cat_ids = sorted(set(c["id"] for c in dataset["categories"]))
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    gts, dts = {}, {}
    for ann in dataset.get("annotations", []):
        gts.setdefault((ann["image_id"], ann["category_id"]), []).append(ann)
    for n, r in enumerate(results):
        assert r["image_id"] in set(img_ids), "results do not correspond to the ground truth's images"
        dts.setdefault((r["image_id"], r["category_id"]), []).append((n, r))

    groups, per = {}, {}
    iou_total, n_pairs = 0.0, len(img_ids) * len(cat_ids)
    for ii, img in enumerate(img_ids):
        for kk, cat in enumerate(cat_ids):
            gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
            if not gt and not dt:
                continue
            idx = np.argsort([-float(r["score"]) for _, r in dt], kind="mergesort")
            dt = [dt[i] for i in idx][:MAX_DETS[-1]]
            D, G = len(dt), len(gt)
            crowd = [int(bool(g.get("iscrowd", 0))) for g in gt]
            ious = np.zeros((D, G))
            for di, (_, d) in enumerate(dt):
                for gi, g in enumerate(gt):
                    ious[di, gi] = bb_iou([float(v) for v in d["bbox"]], [float(v) for v in g["bbox"]], crowd[gi])
            s, c = 0.0, 0
            if D and G:
                sel = ious[ious >= 0.3]
                if len(sel):
                    s, c = float(sel.sum()), len(sel)
                    iou_total += sel.mean()
            matched, ignore, gt_ig_all = np.zeros((A, T, D), bool), np.zeros((A, T, D), bool), []
            for ai, (a0, a1) in enumerate(AREA_RNG):
                g_ig = [bool(crowd[gi]) or float(g["area"]) < a0 or float(g["area"]) > a1 for gi, g in enumerate(gt)]
                gorder = [gi for gi in range(G) if not g_ig[gi]] + [gi for gi in range(G) if g_ig[gi]]     # stable sort by ignore
                for ti, thr in enumerate(IOU_THRS):
                    taken = [False] * G
                    for di, (_, d) in enumerate(dt):
                        best, m = min(thr, 1 - 1e-10), -1
                        for gi in gorder:
                            if taken[gi] and not crowd[gi]:
                                continue
                            if m > -1 and not g_ig[m] and g_ig[gi]:
                                break
                            if ious[di, gi] < best:
                                continue
                            best, m = ious[di, gi], gi
                        if m == -1:
                            area = float(d["bbox"][2]) * float(d["bbox"][3])
                            ignore[ai, ti, di] = area < a0 or area > a1
                            continue
                        taken[m] = True
                        matched[ai, ti, di] = True
                        ignore[ai, ti, di] = g_ig[m]
                gt_ig_all.append(g_ig)
            per[(ii, kk)] = dict(scores=[float(r["score"]) for _, r in dt], matched=matched, ignore=ignore, gt_ig=gt_ig_all)
            if D:
                groups[(ii, kk)] = dict(order=[n for n, _ in dt], matched=matched, ignore=ignore, iou_sum=s, iou_cnt=c)

    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    npig_all = np.zeros((K, A), np.int64)
    for kk in range(K):
        for ai in range(A):
            E = [per[(ii, kk)] for ii in range(len(img_ids)) if (ii, kk) in per]
            npig_all[kk, ai] = sum(1 for e in E for v in e["gt_ig"][ai] if not v)
            for mi, max_det in enumerate(MAX_DETS):
                if not E:
                    continue
                scores = np.concatenate([np.asarray(e["scores"][:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["matched"][ai][:, :max_det] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["ignore"][ai][:, :max_det] for e in E], axis=1)[:, inds]
                npig = int(npig_all[kk, ai])
                if npig == 0:
                    continue
                tps, fps = np.logical_and(dtm, ~dtig), np.logical_and(~dtm, ~dtig)
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
                for ti in range(T):
                    tp, fp = tp_sum[ti], fp_sum[ti]
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    recall[ti, kk, ai, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[ti, :, kk, ai, mi] = q

    def summ(ap, iou_thr=None, a=0, m=2):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    stats = np.array([summ(1), summ(1, .5), summ(1, .75), summ(1, a=1), summ(1, a=2), summ(1, a=3),
                      summ(0, m=0), summ(0, m=1), summ(0, m=2), summ(0, a=1), summ(0, a=2), summ(0, a=3)])
    return dict(img_ids=img_ids, cat_ids=cat_ids, precision=precision, recall=recall, stats=stats, mean_iou=float(iou_total) / n_pairs,
                npig=npig_all, groups=groups)


def flags_in_kernel_order(out):
    """The restatement's matched / ignore flags as the kernel packs them: uint64 per detection (bit a * 10 + t), detections in
    (image, category, rank) order; also the indices into ``results`` in that order."""
    order, mbits, ibits = [], [], []
    for key in sorted(out["groups"]):
        g = out["groups"][key]
        A, T, D = g["matched"].shape
        for d in range(D):
            mb = ib = 0
            for a in range(A):
                for t in range(T):
                    mb |= int(g["matched"][a, t, d]) << (a * T + t)
                    ib |= int(g["ignore"][a, t, d]) << (a * T + t)
            order.append(g["order"][d])
            mbits.append(mb)
            ibits.append(ib)
    return np.asarray(order, np.int64), np.asarray(mbits, np.uint64), np.asarray(ibits, np.uint64)


# ---------------------------------------------------------------------------------------------------
def dataset_of(n_img, cat_ids, anns):
    """anns: [(image id, category id, bbox, iscrowd)]; area = w * h; annotation ids from 1."""
    return {"images": [{"id": i, "file_name": f"img{i}.jpg", "height": 512, "width": 512} for i in range(1, n_img + 1)],
            "categories": [{"id": c, "name": f"c{c}"} for c in cat_ids],
            "annotations": [{"id": n + 1, "image_id": i, "category_id": c, "bbox": list(b), "area": b[2] * b[3], "iscrowd": cr}
                            for n, (i, c, b, cr) in enumerate(anns)]}


def res(img, cat, box, score):
    return {"image_id": img, "category_id": cat, "bbox": list(box), "score": score}


GT10 = (0, 0, 10, 10)
FAR = (200, 200, 10, 10)
# name -> (dataset, results, {stat name: expected value}); one image, one category, hand-derived
KNOWN = {
    "perfect_then_fp": (dataset_of(1, [1], [(1, 1, GT10, 0)]), [res(1, 1, GT10, .9), res(1, 1, FAR, .8)], {"AP50": 1.0, "AR100": 1.0}),
    "fp_then_perfect": (dataset_of(1, [1], [(1, 1, GT10, 0)]), [res(1, 1, GT10, .8), res(1, 1, FAR, .9)], {"AP50": 0.5}),
    "two_gt_one_det": (dataset_of(1, [1], [(1, 1, GT10, 0), (1, 1, FAR, 0)]), [res(1, 1, GT10, .9)], {"AP50": 51 / 101, "AR100": 0.5}),
    "iou_exactly_half": (dataset_of(1, [1], [(1, 1, GT10, 0)]), [res(1, 1, (0, 0, 10, 5), .9)], {"AP50": 1.0}),
}


def _box(rng, exact_sizes=True):
    """Coordinates are multiples of 4; sizes from a set that makes areas of exactly 1024 (32 x 32, 16 x 64) and 9216 (96 x 96,
    48 x 192) and IoUs that hit thresholds exactly (a half-height copy of a box has IoU 0.5, a 3/4 one 0.75)."""
    sizes = [(32, 32), (16, 64), (96, 96), (48, 192), (32, 16), (32, 24), (8, 8), (64, 64), (128, 96), (20, 20)]
    w, h = sizes[int(rng.integers(len(sizes)))]
    return (int(rng.integers(0, 24)) * 4, int(rng.integers(0, 24)) * 4, w, h)


def _dets_for(rng, gt_boxes, n, img, cat):
    """n detections: copies of GT boxes (duplicates: the "last equal IoU wins" rule), half- and 3/4-height copies (IoU exactly 0.5
    and 0.75), shifted copies and random boxes; scores are multiples of 1/16."""
    out = []
    for _ in range(n):
        kind = int(rng.integers(5)) if gt_boxes else 4
        if kind < 4:
            x, y, w, h = gt_boxes[int(rng.integers(len(gt_boxes)))]
            box = [(x, y, w, h), (x, y, w, h // 2), (x, y, w, 3 * h // 4), (x + 4, y, w, h)][kind]
        else:
            box = _box(rng)
        out.append(res(img, cat, box, int(rng.integers(1, 16)) / 16))
    return out


def case_S():
    rng = np.random.default_rng(11)
    anns, results = [], []
    for img in (1, 2, 3):
        for cat in (1, 2):
            boxes = [_box(rng) for _ in range(int(rng.integers(1, 5)))]
            boxes.append(boxes[0])                                             # a duplicate GT
            anns += [(img, cat, b, 0) for b in boxes[:4]]
            results += _dets_for(rng, boxes, int(rng.integers(1, 7)), img, cat)
    order = rng.permutation(len(results))
    dataset = dataset_of(3, [1, 2], anns)
    for ann in dataset["annotations"][1::2]:               # an annotation's area is its own number (a mask's), not w * h
        ann["area"] = ann["area"] / 2
    return dataset, [results[i] for i in order]


def case_T():
    """9 images, 5 categories (ids 1, 3, 4, 7, 9): category 7 has no GT, category 9 no detections; image 8 has no detections, image 9
    no GTs; (image 2, category 1) has 130 detections, (image 3, category 3) 70 GTs; crowd GTs; plus a result of a category the
    ground truth does not know (dropped)."""
    rng = np.random.default_rng(23)
    cats = [1, 3, 4, 7, 9]
    anns, results = [], []
    for img in range(1, 10):
        for cat in cats:
            n_gt = 0 if (cat == 7 or img == 9) else int(rng.integers(0, 6))
            n_dt = 0 if (cat == 9 or img == 8) else int(rng.integers(0, 9))
            if (img, cat) == (2, 1):
                n_gt, n_dt = 6, 130
            if (img, cat) == (3, 3):
                n_gt, n_dt = 70, 12
            boxes = [_box(rng) for _ in range(n_gt)]
            if n_gt >= 2:
                boxes[1] = boxes[0]
            anns += [(img, cat, b, int(rng.integers(6) == 0)) for b in boxes]
            results += _dets_for(rng, boxes, n_dt, img, cat)
    results.append(res(1, 1000, (0, 0, 8, 8), .5))
    order = rng.permutation(len(results))
    return dataset_of(9, cats, anns), [results[i] for i in order]


def case_U(chunk):
    """One category, 40 images, more than 2 * chunk + chunk // 2 detections (none of a group beyond rank 100)."""
    rng = np.random.default_rng(37)
    per_img = (2 * chunk + chunk // 2) // 40 + 2
    anns, results = [], []
    for img in range(1, 41):
        boxes = [_box(rng) for _ in range(int(rng.integers(1, 8)))]
        anns += [(img, 1, b, int(rng.integers(10) == 0)) for b in boxes]
        results += _dets_for(rng, boxes, per_img, img, 1)
    order = rng.permutation(len(results))
    return dataset_of(40, [1], anns), [results[i] for i in order]


def case_properties(dataset, results):
    """What a seeded case really contains (the generator's promises, asserted by the tests)."""
    from collections import Counter
    gts, dts = Counter(), Counter()
    for a in dataset["annotations"]:
        gts[(a["image_id"], a["category_id"])] += 1
    score_in_group, score_in_cat = Counter(), {}
    for r in results:
        dts[(r["image_id"], r["category_id"])] += 1
        score_in_group[(r["image_id"], r["category_id"], r["score"])] += 1
        score_in_cat.setdefault((r["category_id"], r["score"]), set()).add(r["image_id"])
    exact = set()
    by_group = {}
    for a in dataset["annotations"]:
        by_group.setdefault((a["image_id"], a["category_id"]), []).append(a)
    for r in results:
        for a in by_group.get((r["image_id"], r["category_id"]), []):
            v = bb_iou(r["bbox"], a["bbox"], a["iscrowd"])
            if v in (0.5, 0.75):
                exact.add(v)
    areas = set(a["area"] for a in dataset["annotations"])
    return dict(max_dt=max(dts.values(), default=0), max_gt=max(gts.values(), default=0),
                ties_in_group=any(v > 1 for v in score_in_group.values()), ties_across_images=any(len(v) > 1 for v in score_in_cat.values()),
                exact_ious=exact, has_1024=1024 in areas, has_9216=9216 in areas, crowd=any(a["iscrowd"] for a in dataset["annotations"]),
                n_results=len(results))
