"""COCO bbox evaluation on the device: what the reference's ``bench_results`` (utils/utils.py:330-354) asks of pycocotools
(``loadRes`` + ``COCOeval(..., 'bbox')``: evaluate, accumulate, summarize) and its "Mean IOU".

Division of work
  host (numpy)   ``flatten``: the ground truth and the results as flat float64 arrays grouped by (image, category), images and
                 categories in ascending id order, each group in its original order; the argument checks of ``loadRes``;
                 ``summarize``: the 12 numbers from the downloaded precision / recall arrays, with pycocotools' expressions
  device (torch) ``prepare``: two orderings, both by a pair of STABLE ``torch.sort`` calls (first by -score, then by the group /
                 category key), which is a total order: the evaluation order inside a group (descending score, ties in results
                 order, cut to maxDets[-1]) and the sweep order of a category (descending score, ties in (image, rank) order)
  device (HIP)   csrc/coco_eval.hip: IoU, matching, the per-group IoU sums, the precision / recall sweep.  No CPU fallback.

pycocotools is not a dependency and parity with it is not pinned by this repository's tests where it is not installed (they compare
with the numpy restatement of tests/_cocoeval.py).  The one known deviation: matched flags are kept per GT slot, so a GT whose
annotation id is 0 can be matched; pycocotools loses such a match."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .. import kernels as K

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # pycocotools Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ("all", "small", "medium", "large")
EPS = float(np.spacing(1))
STAT_NAMES = ("AP", "AP50", "AP75", "APS", "APM", "APL", "AR1", "AR10", "AR100", "ARS", "ARM", "ARL")


class CocoEvalResult:
    """``stats``: the 12 numbers of COCOeval.summarize in its order; ``precision`` [10, 101, K, 4, 3] and ``recall`` [10, K, 4, 3]
    (float64 numpy, pycocotools' layout); ``mean_iou``: the reference's "Mean IOU"; ``cat_ids`` / ``img_ids``: the axes."""

    def __init__(self, stats, precision, recall, mean_iou, cat_ids, img_ids, npig):
        self.stats, self.precision, self.recall, self.mean_iou = stats, precision, recall, mean_iou
        self.cat_ids, self.img_ids, self.npig = cat_ids, img_ids, npig

    def summary_lines(self):
        out = []
        rows = [(1, None, 0, 2), (1, .5, 0, 2), (1, .75, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
                (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2)]
        for value, (ap, thr, a, m) in zip(self.stats, rows):
            title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
            iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else "{:0.2f}".format(thr)
            out.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(title, kind, iou, AREA_LBL[a], MAX_DETS[m],
                                                                                                 value))
        return out


def _load_results(results):
    if isinstance(results, (str, os.PathLike)):
        with open(results) as f:
            results = json.load(f)
    if not isinstance(results, list):
        raise ValueError("coco_eval: results must be a list of result dicts or the path of a JSON file that holds one")
    return results


def flatten(gt, results):
    """Host flattening.  Returns a dict of numpy arrays: ``img_ids`` / ``cat_ids`` (sorted), detections ``dt_box`` f64 [nD, 4],
    ``dt_score`` f64 [nD], ``dt_group`` int64 [nD] and ground truth ``gt_box`` f64 [nG, 4], ``gt_area`` f64 [nG], ``gt_crowd`` u8 [nG],
    ``gt_group`` int64 [nG], ``gt_off`` int32 [I * K + 1]; group = image index * K + category index, groups ascending and each in its
    original (results list / annotation list) order.  Results of a category the ground truth does not have are dropped; a result
    for an unknown image raises ValueError (loadRes' assertion), and so does a non-finite box or score."""
    dataset = getattr(gt, "dataset", gt)
    img_ids = np.unique(np.asarray([im["id"] for im in dataset["images"]], dtype=np.int64))
    cat_ids = np.unique(np.asarray([c["id"] for c in dataset["categories"]], dtype=np.int64))
    if len(img_ids) == 0 or len(cat_ids) == 0:
        raise ValueError("coco_eval: the ground truth has no images or no categories")
    n_cat = len(cat_ids)

    def index_of(ids, values):
        pos = np.clip(np.searchsorted(ids, values), 0, len(ids) - 1)
        return pos, ids[pos] == values

    def grouped(img, cat, columns):
        """Rows of known image and category, sorted by group (stable)."""
        ii, ok_i = index_of(img_ids, img)
        kk, ok_k = index_of(cat_ids, cat)
        keep = ok_i & ok_k
        group = (ii * n_cat + kk)[keep]
        order = np.argsort(group, kind="stable")
        return group[order], [np.ascontiguousarray(c[keep][order]) for c in columns], ok_i

    results = _load_results(results)
    for r in results:
        if "bbox" not in r or len(r["bbox"]) != 4:
            raise ValueError("coco_eval: every result needs a 'bbox' of four numbers (bbox evaluation only)")
    n = len(results)
    box = np.asarray([r["bbox"] for r in results], dtype=np.float64).reshape(n, 4)
    score = np.asarray([r["score"] for r in results], dtype=np.float64).reshape(n)
    if not (np.isfinite(box).all() and np.isfinite(score).all()):
        raise ValueError("coco_eval: non-finite box or score in the results")
    dt_group, (dt_box, dt_score), known = grouped(np.asarray([r["image_id"] for r in results], dtype=np.int64).reshape(n),
                                                  np.asarray([r["category_id"] for r in results], dtype=np.int64).reshape(n), (box, score))
    if not known.all():
        raise ValueError("coco_eval: results do not correspond to the ground truth's images (image ids "
                         f"{sorted(set(int(r['image_id']) for r, k in zip(results, known) if not k))[:5]} ...)")

    anns = dataset.get("annotations", [])
    n = len(anns)
    box = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(n, 4)
    area = np.asarray([a["area"] for a in anns], dtype=np.float64).reshape(n)
    crowd = np.asarray([1 if a.get("iscrowd", 0) else 0 for a in anns], dtype=np.uint8).reshape(n)
    if not (np.isfinite(box).all() and np.isfinite(area).all()):
        raise ValueError("coco_eval: non-finite box or area in the ground truth")
    gt_group, (gt_box, gt_area, gt_crowd), _ = grouped(np.asarray([a["image_id"] for a in anns], dtype=np.int64).reshape(n),
                                                       np.asarray([a["category_id"] for a in anns], dtype=np.int64).reshape(n),
                                                       (box, area, crowd))
    n_groups = len(img_ids) * n_cat
    if max(len(dt_group), len(gt_group), n_groups) >= 2 ** 31 - 1:
        raise ValueError("coco_eval: more than 2^31 detections, annotations or (image, category) pairs")
    gt_off = np.zeros(n_groups + 1, dtype=np.int32)
    np.cumsum(np.bincount(gt_group, minlength=n_groups), out=gt_off[1:])
    return dict(img_ids=img_ids, cat_ids=cat_ids, dt_box=dt_box, dt_score=dt_score, dt_group=dt_group, gt_box=gt_box, gt_area=gt_area,
                gt_crowd=gt_crowd, gt_group=gt_group, gt_off=gt_off)


def _offsets(keys, n):
    off = torch.zeros(n + 1, dtype=torch.int64, device=keys.device)
    off[1:] = torch.cumsum(torch.bincount(keys, minlength=n), 0)
    return off


def prepare(flat, device, max_det=MAX_DETS[-1]):
    """The device operands of the kernels (a dict of tensors on ``device``; index plumbing only, runs on any torch device):
    the detections in evaluation order cut to ``max_det`` per group (``dt_box``, ``dt_score``, ``dt_off``), the ground truth, and the
    sweep order (``order``, ``cat_off``).  Each ordering is two stable sorts: by -score, then by the key - ties keep their order."""
    n_cat, n_groups = len(flat["cat_ids"]), len(flat["img_ids"]) * len(flat["cat_ids"])
    score = torch.from_numpy(flat["dt_score"]).to(device)
    group = torch.from_numpy(flat["dt_group"]).to(device)
    by_score = torch.sort(-score, stable=True).indices
    perm = by_score[torch.sort(group[by_score], stable=True).indices]
    rank = torch.arange(len(perm), device=device) - _offsets(group, n_groups)[group]      # (group is ascending: group[perm] == group)
    perm = perm[rank < max_det]
    group, score = group[perm], score[perm]
    cat = group % n_cat
    by_score = torch.sort(-score, stable=True).indices
    order = by_score[torch.sort(cat[by_score], stable=True).indices]
    return dict(dt_box=torch.from_numpy(flat["dt_box"]).to(device)[perm].contiguous(), dt_score=score, dt_perm=perm,
                dt_off=_offsets(group, n_groups).to(torch.int32), order=order.to(torch.int32), cat_off=_offsets(cat, n_cat).to(torch.int32),
                gt_box=torch.from_numpy(flat["gt_box"]).to(device), gt_area=torch.from_numpy(flat["gt_area"]).to(device),
                gt_crowd=torch.from_numpy(flat["gt_crowd"]).to(device), gt_off=torch.from_numpy(flat["gt_off"]).to(device),
                max_gt=int(np.diff(flat["gt_off"]).max()) if len(flat["gt_group"]) else 0)


def summarize(precision, recall):
    """COCOeval.summarize's 12 numbers from the arrays, with its expressions: the mean of the entries > -1 of a slice, -1 without any."""
    def one(ap, iou_thr=None, a=0, m=2):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1), one(1, iou_thr=.5), one(1, iou_thr=.75), one(1, a=1), one(1, a=2), one(1, a=3),
                     one(0, m=0), one(0, m=1), one(0, m=2), one(0, a=1), one(0, a=2), one(0, a=3)])


def mean_iou(iou_sum, iou_cnt):
    """Reference utils.py:338-348: the mean, over ALL (image, category) pairs, of each pair's mean IoU entry >= 0.3 (pairs without
    such an entry add 0)."""
    has = iou_cnt > 0
    ratios = iou_sum[has] / iou_cnt[has]
    return float(np.cumsum(ratios)[-1]) / len(iou_cnt) if len(ratios) else 0.0


def coco_eval(gt, results, device="cuda"):
    """Evaluate ``results`` (a list of COCO result dicts or the path of a JSON file) against ``gt`` (a COCO dataset dict, or any
    object with a ``.dataset`` dict such as a pycocotools ``COCO``) on ``device``.  Returns a CocoEvalResult."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("pytorch_yolo_amd.coco_eval runs on a ROCm device only (no CPU fallback)")
    flat = flatten(gt, results)
    n_img, n_cat = len(flat["img_ids"]), len(flat["cat_ids"])
    with torch.cuda.device(device):
        op = prepare(flat, device)
        if op["max_gt"] > K.coco_max_gt():
            raise RuntimeError(f"coco_eval: an (image, category) pair with {op['max_gt']} ground-truth boxes exceeds the cap of {K.coco_max_gt()}")
        n_dt = op["dt_box"].shape[0]
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
        dt_match, dt_ignore = new((n_dt,), i64), new((n_dt,), i64)
        npig, status = new((n_cat, K.COCO_A), i32), new((1,), i32)
        iou_sum, iou_cnt = new((n_img * n_cat,), f64), new((n_img * n_cat,), i32)
        ws = new((K.coco_workspace_bytes(n_dt),), torch.uint8)
        precision = new((K.COCO_T, K.COCO_R, n_cat, K.COCO_A, K.COCO_M), f64)
        recall = new((K.COCO_T, n_cat, K.COCO_A, K.COCO_M), f64)
        iou_thrs, area_rng, rec_thrs = (torch.from_numpy(v).to(device) for v in (IOU_THRS, AREA_RNG.reshape(-1), REC_THRS))
        K.coco_match_fwd(op["dt_box"], op["dt_off"], op["gt_box"], op["gt_area"], op["gt_crowd"], op["gt_off"], n_img, n_cat, op["max_gt"],
                         iou_thrs, area_rng, dt_match, dt_ignore, npig, iou_sum, iou_cnt, status, ws)
        K.coco_accumulate_fwd(op["order"], op["cat_off"], n_cat, dt_match, dt_ignore, npig, rec_thrs, MAX_DETS, EPS, ws, precision, recall)
        if int(status.item()):
            raise RuntimeError(f"coco_eval: {int(status.item())} (image, category) pairs exceed the cap of {K.coco_max_gt()} ground-truth boxes")
        precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
        miou = mean_iou(iou_sum.cpu().numpy(), iou_cnt.cpu().numpy())
        npig = npig.cpu().numpy()
    return CocoEvalResult(summarize(precision, recall), precision, recall, miou, flat["cat_ids"], flat["img_ids"], npig)
