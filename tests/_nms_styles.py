"""The reference's other suppression styles, restated.  TEST INFRASTRUCTURE (the companion of oracle/nms.py, which restates 'MERGE').

numpy float32 restatement of the 'OR' (:253-259), 'AND' (:260-265) and 'SOFT' (:277-287) branches of the reference's
``non_max_suppression`` (utils/utils.py:200-293).  Everything around the per-class loop is what oracle/nms.py does, in its order:
conf product and the three filters (:212-218), ``xywh2xyxy`` (:231), the sort by conf (:237), the loop over ascending class ids
(:241), a class of one row kept as it is (:244-246, the length BEFORE the cap), the cap of 100 (:247-250) and the final sort (:291).
Every arithmetic step is one IEEE fp32 operation in the reference's order; the IoU is oracle.nms._iou_1_to_n itself.

Rules fixed where the reference is under-specified (the same as oracle/nms.py):
  * both argsorts are stable: (conf descending, then earlier row / earlier emission);
  * ``torch.max(1)`` tie -> lowest class index.
'SOFT' only: ``exp`` is taken in float64 and rounded once to fp32 (<= 0.5 ulp), ``iou ** 2`` is ``iou * iou`` (what torch's pow does for
the exponent 2) and the division by 0.5 is exact.  SOFT_RTOL / SOFT_ATOL is the one tolerance of the style tests: per factor the two
sides differ by at most 1 ulp of each side's exp plus half an ulp of each side's multiply = 3 * 2^-23 relative, over a chain of at most
99 factors 99 * 3 * 2^-23 = 3.6e-5 -> rtol 4e-5; atol is the smallest normal, so no side's handling of denormals matters.
"""
import numpy as np

from oracle.nms import AREA_EPS, F32, MAX_PER_CLASS, MIN_WH, _iou_1_to_n  # noqa: F401

STYLES = ("OR", "AND", "SOFT")
AND_MIN_IOU = F32(0.5)          # utils.py:263: a constant of the reference, not nms_thres
SOFT_SIGMA = F32(0.5)           # utils.py:278
SOFT_RTOL = 4e-5
SOFT_ATOL = 2.0 ** -126


def candidates(pred, conf_thres):
    """The style-independent front of one image (utils.py:212-237): (input row, corners [n,4], conf, class_conf, class) of the rows
    that pass the filters, sorted by conf descending (stable), or None.  ``pred`` is not modified."""
    assert pred.dtype == np.float32 and pred.ndim == 2
    cls = pred[:, 5:]
    class_pred = np.argmax(cls, axis=1)
    class_conf = cls[np.arange(len(cls)), class_pred]
    conf = pred[:, 4] * class_conf                                           # :213
    row = np.concatenate([pred[:, :4], conf[:, None], pred[:, 5:]], 1)
    keep = conf > F32(conf_thres)                                            # :216
    keep &= (pred[:, 2] > MIN_WH) & (pred[:, 3] > MIN_WH)                    # :217
    keep &= np.isfinite(row).all(1)                                          # :218
    idx = np.nonzero(keep)[0]
    if idx.size == 0:
        return None
    x, y, w, h = (pred[idx, k] for k in range(4))
    half = F32(2)
    boxes = np.stack([x - w / half, y - h / half, x + w / half, y + h / half], 1)   # :57-60
    conf, cconf, cpred = conf[idx], class_conf[idx], class_pred[idx]
    order = np.argsort(-conf, kind="stable")                                 # :237
    return idx[order], boxes[order], conf[order], cconf[order], cpred[order]


def nms_image(pred, conf_thres, nms_thres, style, max_per_class=MAX_PER_CLASS):
    """One image in style 'OR' | 'AND' | 'SOFT': (dets [n,7] float32, kept input rows [n] int64) or (None, None).  ``max_per_class``:
    the cap of :247-250, the reference's 100 by default."""
    assert style in STYLES
    nms_thres = F32(nms_thres)
    cand = candidates(pred, conf_thres)
    if cand is None:
        return None, None
    idx, boxes, conf, cconf, cpred = cand
    out_rows, out_idx = [], []

    def emit(b, s, cc, c, i):
        out_rows.append(np.array([*b, s, cc, F32(c)], dtype=F32))
        out_idx.append(i)

    for c in np.unique(cpred):                                               # ascending, :241
        sel = np.nonzero(cpred == c)[0]
        n = len(sel)
        if n == 1:                                                           # :244-246
            k = sel[0]
            emit(boxes[k], conf[k], cconf[k], c, idx[k])
            continue
        sel = sel[:max_per_class]                                            # :247-250
        b, s, cc, ii = boxes[sel], conf[sel].copy(), cconf[sel], idx[sel]
        left = np.arange(len(sel))                                           # dc, as positions in the capped class list
        if style == "OR":
            while left.size:                                                 # :254
                emit(b[left[0]], s[left[0]], cc[left[0]], c, ii[left[0]])    # :255
                if left.size == 1:                                           # :256-257
                    break
                iou = _iou_1_to_n(b[left[0]], b[left[1:]])                   # :258
                left = left[1:][iou < nms_thres]                             # :259
        elif style == "AND":
            while left.size > 1:                                             # :261
                iou = _iou_1_to_n(b[left[0]], b[left[1:]])                   # :262
                if np.max(iou) > AND_MIN_IOU:                                # :263 (a NaN maximum compares false, like torch's)
                    emit(b[left[0]], s[left[0]], cc[left[0]], c, ii[left[0]])
                left = left[1:][iou < nms_thres]                             # :265
        else:
            while left.size:                                                 # :279
                emit(b[left[0]], s[left[0]], cc[left[0]], c, ii[left[0]])    # :280-283
                if left.size == 1:
                    break
                iou = _iou_1_to_n(b[left[0]], b[left[1:]])                   # :284
                left = left[1:]                                              # :285
                arg = (-(iou * iou)) / SOFT_SIGMA                            # :287, fp32 (the division by 0.5 is exact)
                assert arg.dtype == np.float32
                s[left] = s[left] * np.exp(arg.astype(np.float64)).astype(F32)
    if not out_rows:                                                         # :289 ('AND' can erase every class)
        return None, None
    dets = np.stack(out_rows).astype(F32)
    kept = np.asarray(out_idx, dtype=np.int64)
    final = np.argsort(-dets[:, 4], kind="stable")                           # :291
    return dets[final], kept[final]


def non_max_suppression(prediction, conf_thres, nms_thres, style, max_per_class=MAX_PER_CLASS):
    """Batch wrapper: (list of dets or None, list of kept-index arrays or None)."""
    dets, kept = [], []
    for pred in prediction:
        d, k = nms_image(pred, conf_thres, nms_thres, style, max_per_class)
        dets.append(d)
        kept.append(k)
    return dets, kept


def corners(pred_rows):
    """xywh2xyxy (utils.py:57-60) of input rows [n, >=4], fp32."""
    x, y, w, h = (pred_rows[:, k] for k in range(4))
    half = F32(2)
    return np.stack([x - w / half, y - h / half, x + w / half, y + h / half], 1)


def assert_same(style, dets, idx, want_dets, want_idx, tag=""):
    """The comparison of the style tests, for one image.  'OR' / 'AND': kept indices equal and all seven columns bit-equal.  'SOFT':
    kept-index SETS equal, columns 0-3, 5, 6 bit-equal after pairing rows by kept index, conf within SOFT_RTOL / SOFT_ATOL, and the
    conf column of ``dets`` non-increasing.  Returns the largest relative conf difference seen (0.0 where bit-equality is asked)."""
    if want_dets is None:
        assert dets is None, f"{tag}: detections where none are expected"
        return 0.0
    assert dets is not None, f"{tag}: no detections, {len(want_dets)} expected"
    dets, idx = np.asarray(dets), np.asarray(idx).astype(np.int64)
    assert dets.dtype == np.float32 and dets.shape == want_dets.shape, f"{tag}: {dets.shape} against {want_dets.shape}"
    if style != "SOFT":
        assert np.array_equal(idx, want_idx), f"{tag}: kept indices differ"
        assert np.array_equal(dets.view(np.uint32), want_dets.view(np.uint32)), f"{tag}: detections differ (bit-exact expected)"
        return 0.0
    assert len(set(idx.tolist())) == len(idx) and len(set(want_idx.tolist())) == len(want_idx), f"{tag}: a row was emitted twice"
    assert set(idx.tolist()) == set(want_idx.tolist()), f"{tag}: kept-index sets differ"
    a, b = dets[np.argsort(idx)], want_dets[np.argsort(want_idx)]
    cols = [0, 1, 2, 3, 5, 6]
    assert np.array_equal(a[:, cols].view(np.uint32), b[:, cols].view(np.uint32)), f"{tag}: boxes / class_conf / class differ"
    diff = np.abs(a[:, 4].astype(np.float64) - b[:, 4].astype(np.float64))
    rel = float(np.max(diff / np.maximum(np.abs(b[:, 4].astype(np.float64)), SOFT_ATOL)))
    assert bool(np.all(diff <= SOFT_ATOL + SOFT_RTOL * np.abs(b[:, 4].astype(np.float64)))), \
        f"{tag}: SOFT conf differs by up to {rel:.3e} relative (bound {SOFT_RTOL:.1e})"
    assert bool(np.all(dets[1:, 4] <= dets[:-1, 4])), f"{tag}: SOFT conf column is not non-increasing"
    return rel
