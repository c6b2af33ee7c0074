"""Inputs of the NMS edge tests (tests/test_nms_edges_cpu.py, tests/test_nms_edges_gpu.py).  TEST INFRASTRUCTURE.

The other NMS tests draw their inputs from _cases.synth_predictions, whose survivor counts and class segment lengths fall wherever the
seed puts them.  Here both are EXACT BY CONSTRUCTION: ``edge_predictions(spec)`` builds [bs, rows, 5 + nc] float32 from a per-image
list {class: number of surviving rows}, so a table row can sit on a boundary of csrc/nms.hip on purpose:

  key sort (survivors n of an image)    n <= 1024 / 2048 / 4096 / 8192: block_sort_regs<1 | 2 | 4 | 8> on keys in LDS; above: the bitonic
                                        network in the global workspace                                       -> key_sort_branch(n)
  final order (kept rows n_out)         f_pad <= 512: the wave-local LDS network; up to 8192: block_sort_regs; above: the bitonic
                                        network in the image's key row of the workspace                       -> final_sort_branch(n_out)
  per-class loop                        two candidates per lane (q, q + 64), alive masks with special cases at 64 and 128
  filter                                four lanes per row scan ceil(nc / 4) classes each; 16-byte loads only for aligned tiles

Conf values.  A surviving row has ONE class score of exactly 1.0 (the others 0, or an equal 1.0 further right where a tie of the class
maximum is asked for), so conf = obj * 1.0 = obj, and obj = 1 - k * 2^-20 with a different k in 1 .. n for every survivor of an image
(a seeded permutation): n < 2^20 distinct fp32 values in (0.98, 1) - fp32 spacing there is 2^-24 -, all above conf_thres = 0.5.
Filler rows have objectness 0 and never survive.  The tie cases (TIE_CASES) are hand-made rows and say where their ties are.

Boxes.  'clustered': centres from a small seeded set plus a jitter of a few pixels, 30-pixel boxes: MERGE and OR have groups to merge.
'disjoint': 20-pixel boxes on a 40-pixel grid, one cell per surviving row: every IoU is 0, so OR keeps min(segment, cap) rows of a
class, SOFT's factors are exp(0) = 1 exactly (its conf column is then bit-defined) and AND emits classes of one row only.
"""
import functools

import numpy as np

import _nms_styles as S
from oracle import nms as onms

F32 = np.float32
CONF_THRES = 0.5
NMS_THRES = 0.5
LDS_KEYS = 8192              # csrc/nms_common.h kLdsKeys
MERGE_THREADS = 1024         # csrc/nms.hip kMergeThreads
MAX_PER_CLASS_CAP = 128      # csrc/nms_common.h kMaxPerClassCap
ALL_STYLES = ("MERGE", "OR", "AND", "SOFT")


def _pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def key_sort_branch(n):
    """Which sort of nms_merge_kernel the keys of an image with n survivors take (read off the kernel's n_pad rule)."""
    if n == 0:
        return "none (empty image)"
    n_pad = max(MERGE_THREADS, _pow2_at_least(n))
    return f"LDS, registers KPT {n_pad // MERGE_THREADS}" if n_pad <= LDS_KEYS else f"global bitonic ({n_pad} keys)"


def final_sort_branch(n_out):
    """Which sort the final order of an image with n_out kept rows takes (the kernel's f_pad rule)."""
    if n_out == 0:
        return "none"
    f_pad = _pow2_at_least(n_out)
    if f_pad <= 512:
        return f"LDS wave-local network ({f_pad} keys)"
    if n_out <= LDS_KEYS:
        return f"LDS, registers KPT {max(MERGE_THREADS, f_pad) // MERGE_THREADS}"
    return f"global bitonic ({max(2 * LDS_KEYS, f_pad)} keys)"


def edge_predictions(spec):
    """[bs, rows, 5 + nc] float32 of ``spec``:
      nc, rows        class count, rows per image
      images          per image a dict {class: number of surviving rows}
      layout          'clustered' (default) | 'disjoint'
      tie_with        optional {class: later class}: the surviving rows of ``class`` carry the same score 1.0 in the later column too -
                      a tie of the class maximum, which the first column wins (torch.max semantics)
      pin_last        optional: the last row of every non-empty image is a survivor
      seed            positions, conf permutation and boxes
    Survivor count and segment lengths depend on ``images`` alone."""
    nc, rows, images = spec["nc"], spec["rows"], spec["images"]
    layout = spec.get("layout", "clustered")
    tie_with = spec.get("tie_with", {})
    rng = np.random.default_rng(spec.get("seed", 0))
    pred = np.zeros((len(images), rows, 5 + nc), dtype=F32)
    centres = rng.uniform(60.0, 560.0, (12, 2))
    for b, segs in enumerate(images):
        # filler: plausible boxes and class scores, objectness 0
        pred[b, :, 0:2] = rng.uniform(20.0, 600.0, (rows, 2))
        pred[b, :, 2:4] = rng.uniform(10.0, 60.0, (rows, 2))
        pred[b, :, 5:] = rng.uniform(0.1, 0.9, (rows, nc))
        n = sum(segs.values())
        assert n <= rows and all(0 <= c < nc and m > 0 for c, m in segs.items())
        if n == 0:
            continue
        if spec.get("pin_last"):
            where = np.sort(np.append(rng.choice(rows - 1, n - 1, replace=False), rows - 1))
        else:
            where = np.sort(rng.choice(rows, n, replace=False))
        cls = rng.permutation(np.repeat(np.fromiter(segs.keys(), dtype=np.int64), np.fromiter(segs.values(), dtype=np.int64)))
        k = rng.permutation(n) + 1
        pred[b, where, 4] = (1.0 - k.astype(np.float64) * 2.0 ** -20).astype(F32)
        pred[b, where, 5:] = 0.0
        pred[b, where, 5 + cls] = 1.0
        for c, later in tie_with.items():
            assert c < later < nc
            pred[b, where[cls == c], 5 + later] = 1.0
        if layout == "disjoint":
            cell = rng.permutation(n)
            pred[b, where, 0] = 30.0 + 40.0 * (cell % 100)
            pred[b, where, 1] = 30.0 + 40.0 * (cell // 100)
            pred[b, where, 2:4] = 20.0
        else:
            assert layout == "clustered"
            pred[b, where, 0:2] = centres[rng.integers(0, len(centres), n)] + rng.uniform(-4.0, 4.0, (n, 2))
            pred[b, where, 2:4] = rng.uniform(27.0, 33.0, (n, 2))
    return pred


def spread(n, nc):
    """n surviving rows over nc classes, as evenly as they go: {class: count} without empty classes."""
    return {c: n // nc + (1 if c < n % nc else 0) for c in range(nc) if n // nc + (1 if c < n % nc else 0) > 0}


def kept_soft(segs, max_per_class=100):
    """Rows 'SOFT' keeps (it removes nothing), and 'OR' / 'MERGE' on disjoint boxes: sum of min(segment, cap)."""
    return sum(min(m, max_per_class) for m in segs.values())


# ---- case 1: key-sort boundaries: one image, nc = 4, rows = n + 37 ------------------------------------------------------------------
KEY_SORT_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16385)


def key_sort_spec(n):
    return {"nc": 4, "rows": n + 37, "images": [spread(n, 4)], "seed": 100 + n}


# ---- case 2: final-sort boundaries: 'SOFT' on clustered boxes, 'OR' on disjoint ones; n_out = sum of min(segment, 100) ---------------
FINAL_SORT_N_OUT = (1, 511, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8000)


def final_sort_spec(n_out, style):
    """q = n_out // 100 classes of 101 surviving rows (one more than the cap: 100 take part) and one class of n_out % 100."""
    q, r = divmod(n_out, 100)
    segs = {c: 101 for c in range(q)}
    if r:
        segs[q] = r
    nc = max(4, len(segs))
    assert nc <= 80 and kept_soft(segs) == n_out
    return {"nc": nc, "rows": sum(segs.values()) + 37, "images": [segs], "seed": 200 + n_out,
            "layout": "disjoint" if style == "OR" else "clustered"}


# ---- case 3: the mixed batch ---------------------------------------------------------------------------------------------------------
MIXED_COUNTS = (0, 1, 1025, 8193, 300)
MIXED_SPEC = {"nc": 4, "rows": 8193 + 37, "images": [spread(n, 4) for n in MIXED_COUNTS], "seed": 300}

# ---- case 4: images that start off a 16-byte boundary; the last tile is the single row 64 --------------------------------------------
UNALIGNED_NC = (1, 2, 4)


def unaligned_spec(nc):
    return {"nc": nc, "rows": 65, "images": [spread(n, nc) for n in (40, 23, 65)], "seed": 400 + nc, "pin_last": True}


# ---- case 5: ties.  Hand-made rows (x, y, w, h, obj, class); the class score is 1.0, so conf = obj ------------------------------------
def tie_rows(rows, nc):
    out = np.zeros((len(rows), 5 + nc), dtype=F32)
    for i, (x, y, w, h, obj, cls) in enumerate(rows):
        out[i, :5] = (x, y, w, h, obj)
        if cls is not None:
            out[i, 5 + cls] = 1.0
    return out[None]


def _tie_a():
    """One class, conf 0.75 on five different boxes: an overlapping pair (IoU 0.67), another (IoU 0.82), a lone box; one row above and
    one below them, filler between."""
    return tie_rows([(300, 300, 20, 20, .75, 0), (50, 50, 20, 20, .75, 0), (10, 10, 20, 20, 0., None), (54, 50, 20, 20, .75, 0),
                     (152, 150, 20, 20, .75, 0), (150, 150, 20, 20, .75, 0), (52, 50, 20, 20, .875, 0), (400, 50, 20, 20, .625, 0)], 2)


def _tie_b():
    """Equal conf across two classes (0.75: classes 2 and 0) and three (0.5625: classes 3, 1, 0), input rows in descending class order,
    disjoint boxes and one overlapping pair per class."""
    rows = []
    for j, (conf, classes) in enumerate(((.75, (2, 0)), (.5625, (3, 1, 0)))):
        for i, c in enumerate(classes):
            rows.append((40 + 60 * i, 40 + 120 * j, 20, 20, conf, c))
            rows.append((43 + 60 * i, 40 + 120 * j, 20, 20, conf, c))
            rows.append((40 + 60 * i, 90 + 120 * j, 20, 20, conf, c))
    return tie_rows(rows, 4)


def _tie_c():
    """Exact duplicate rows (IoU 1): three copies in class 0, two in class 1 of the same box and conf, and a copy with a lower conf."""
    r = (100, 100, 30, 30, .75)
    return tie_rows([r + (0,), r + (1,), r + (0,), (300, 300, 30, 30, .75, 1), r + (1,), r + (0,), (100, 100, 30, 30, .5625, 0)], 2)


def _tie_d():
    """A whole class of 130 rows of conf 0.75 on disjoint boxes, interleaved with filler and with rows of class 1: under the cap of 100
    the first 100 BY INPUT ROW take part."""
    rows = []
    for j in range(130):
        rows.append((30 + 40 * (j % 20), 30 + 40 * (j // 20), 20, 20, .75, 0))
        if j % 3 == 0:
            rows.append((30 + 40 * (j % 20), 530 + 40 * (j // 20), 20, 20, .75 if j % 2 else .625, 1))
        if j % 5 == 0:
            rows.append((5, 5, 20, 20, 0., None))
    return tie_rows(rows, 2)


TIE_CASES = {"a_one_class": _tie_a, "b_across_classes": _tie_b, "c_duplicates": _tie_c, "d_class_of_130": _tie_d}

# ---- case 6: max_per_class.  Per value the segments (one class each, one image): the set's largest below, the value itself, the
# set's smallest above (set = 1, 2, 64, 65, 128, 129, 200; the value itself is added where the set lacks it) ---------------------------
MAX_PER_CLASS_TABLE = {
    1: (1, 2, 200),              # (no segment can be below 1)
    2: (1, 2, 64),
    63: (2, 63, 64, 65),
    64: (2, 64, 65, 129),
    65: (64, 65, 128),
    100: (65, 100, 128, 200),
    127: (65, 127, 128, 129),
    128: (65, 128, 129, 200),
}
MAX_PER_CLASS_REFUSED = (0, 129)


def max_per_class_spec(mpc):
    segs = dict(enumerate(MAX_PER_CLASS_TABLE[mpc]))
    return {"nc": len(segs), "rows": sum(segs.values()) + 37, "images": [segs], "seed": 600 + mpc}


AND_CAP1_SPEC = {"nc": 2, "rows": 5 + 37, "images": [{1: 5}], "seed": 666}          # 'AND', max_per_class 1: nothing is emitted

# ---- case 7: the caller's cap below the kept count: image 0 keeps 57, image 1 keeps 3 -------------------------------------------------
SMALL_CAP = 10
SMALL_CAP_KEPT = (57, 3)
SMALL_CAP_SPECS = {
    # MERGE / OR / SOFT: three classes of ten disjoint rows and 27 classes of one
    "disjoint": {"nc": 32, "rows": 57 + 37, "layout": "disjoint", "seed": 700,
                 "images": [{**{c: 10 for c in range(3)}, **{c: 1 for c in range(3, 30)}}, {0: 1, 5: 2}]},
    # AND keeps classes of one row only: 57 of them (and three)
    "singles": {"nc": 60, "rows": 57 + 37, "layout": "disjoint", "seed": 701,
                "images": [{c: 1 for c in range(57)}, {c: 1 for c in (2, 30, 59)}]},
}


def small_cap_spec(style):
    return SMALL_CAP_SPECS["singles" if style == "AND" else "disjoint"]


# ---- case 8: more kept rows than the LDS key buffer holds ----------------------------------------------------------------------------
MANY_KEPT = 90 * 95
MANY_KEPT_SPEC = {"nc": 90, "rows": 9000, "layout": "disjoint", "seed": 800, "images": [{c: 95 for c in range(90)}]}
MANY_KEPT_BATCH_SPEC = {"nc": 90, "rows": 9000, "layout": "disjoint", "seed": 801,
                        "images": [{c: 3 + c % 5 for c in range(0, 90, 2)}, {c: 95 for c in range(90)}]}
MANY_KEPT_STYLES = ("SOFT", "OR")

# ---- case 9: wide rows: the four lanes of a row scan ceil(nc / 4) classes each, the last one fewer ------------------------------------
WIDE_NC = (81, 128, 250, 251)
TOO_WIDE_NC = 252            # 64 rows x (5 + nc) floats no longer fit the filter's 64 KiB tile


def wide_spec(nc):
    """Classes on both sides of every quarter boundary; ties of the class maximum between the first and the last class and across the
    first quarter boundary.  300 rows, 210 of them survive."""
    cps = (nc + 3) // 4
    classes = sorted({0, cps - 1, cps, 2 * cps, 3 * cps - 1, 3 * cps, nc - 1})
    assert len(classes) == 7
    return {"nc": nc, "rows": 300, "images": [{c: 30 for c in classes}, {c: 10 + i for i, c in enumerate(classes)}], "seed": 900 + nc,
            "tie_with": {0: nc - 1, cps - 1: cps}}


# ---- the cases by name: inputs and restatements are computed once per session and handed out read-only --------------------------------
_SPECS = {
    "key_sort": key_sort_spec, "final_sort": final_sort_spec, "mixed": lambda: MIXED_SPEC, "unaligned": unaligned_spec,
    "max_per_class": max_per_class_spec, "and_cap1": lambda: AND_CAP1_SPEC, "small_cap": small_cap_spec, "many": lambda: MANY_KEPT_SPEC,
    "many_batch": lambda: MANY_KEPT_BATCH_SPEC, "wide": wide_spec,
}


def case_spec(kind, *args):
    return _SPECS[kind](*args)


@functools.lru_cache(maxsize=None)
def case_pred(kind, *args):
    """The input of a case, [bs, rows, 5 + nc] float32, read-only."""
    pred = TIE_CASES[args[0]]() if kind == "tie" else edge_predictions(case_spec(kind, *args))
    pred.setflags(write=False)
    return pred


@functools.lru_cache(maxsize=None)
def case_want(style, max_per_class, kind, *args):
    """(dets, kept) lists of the restatement (oracle/nms.py for 'MERGE', tests/_nms_styles.py for the others)."""
    pred = case_pred(kind, *args)
    if style == "MERGE":
        return onms.non_max_suppression(pred, CONF_THRES, NMS_THRES, mutate=False, max_per_class=max_per_class)
    return S.non_max_suppression(pred, CONF_THRES, NMS_THRES, style, max_per_class)


def survivors(pred_image):
    """(input rows, conf, class) of the rows of one image that pass the filter, in input order."""
    cand = S.candidates(np.asarray(pred_image), CONF_THRES)
    if cand is None:
        return np.zeros(0, np.int64), np.zeros(0, F32), np.zeros(0, np.int64)
    idx, _, conf, _, cpred = cand
    o = np.argsort(idx)
    return idx[o], conf[o], cpred[o]


def segments(pred_image):
    """{class: number of surviving rows} of one image, from the restatement's filter."""
    _, _, cls = survivors(pred_image)
    c, m = np.unique(cls, return_counts=True)
    return dict(zip(c.tolist(), m.tolist()))


# ---- case 10: the compact form (head conv + decode + filter -> nms_styled_compact).  Crafted LOGITS: an identity head conv feeds
# bf16-exact values straight through, so the plain head (io -> nms_styled) and the filter epilogue decode the same numbers ---------------
LOGIT_LADDER = np.array([2.0 ** e * (1.0 + m / 128.0) for e in range(3) for m in range(128)], dtype=F32)       # 384 bf16 values in [1, 8)
COMPACT_CONF_THRES = 0.5     # a surviving row has obj and class logits >= 1: conf >= sigmoid(1)^2 = 0.534; filler: obj logit -88
COMPACT_ANCHORS = {3: [(10., 10.), (12., 12.), (9., 9.)],      # x e^0.5: 16.5 / 19.8 / 14.8 px at stride 16: rows of a cell overlap
                   2: [(6., 6.), (9., 9.)]}                     # 9.9 / 14.8 px: the two rows of a cell have IoU 0.44, cells are disjoint


def edge_logits(spec):
    """Logits [n, na, h, w, 5 + nc] float32, bf16-exact, of ``spec`` = nc, na, h, w, images [{class: surviving rows}], seed and
    optionally tied_classes: the rows of these classes all carry the same objectness and class logit (equal conf inside a class and
    across the classes).  io row of (anchor a, y, x) = (a * h + y) * w + x.  Survivor counts and segments are exact by construction;
    conf values of the untied rows are drawn from a 384 x 384 ladder and MAY repeat: the compact form is compared with the plain form
    on the same numbers, both of which promise the total order."""
    nc, na, h, w = spec["nc"], spec["na"], spec["h"], spec["w"]
    rng = np.random.default_rng(spec["seed"])
    lg = np.zeros((len(spec["images"]), na * h * w, 5 + nc), dtype=F32)
    lg[..., 2:4] = 0.5
    lg[..., 4] = -88.0
    lg[..., 5:] = -6.0
    for b, segs in enumerate(spec["images"]):
        n = sum(segs.values())
        assert n <= na * h * w
        where = np.sort(rng.choice(na * h * w, n, replace=False))
        cls = rng.permutation(np.repeat(np.fromiter(segs.keys(), dtype=np.int64), np.fromiter(segs.values(), dtype=np.int64)))
        obj, score = rng.choice(LOGIT_LADDER, n), rng.choice(LOGIT_LADDER, n)
        tied = np.isin(cls, spec.get("tied_classes", ()))
        obj[tied], score[tied] = 3.0, 2.0
        lg[b, where, 4] = obj
        lg[b, where, 5 + cls] = score
    return lg.reshape(len(spec["images"]), na, h, w, 5 + nc)


COMPACT_KEY_SORT_N = (1024, 1025, 8192, 8193)


def compact_key_sort_spec(n):
    return {"nc": 4, "na": 3, "h": 53, "w": 53, "images": [spread(n, 4)], "seed": 1000 + n}            # 8427 rows


COMPACT_TIE_SPEC = {"nc": 4, "na": 3, "h": 8, "w": 8, "images": [{0: 30, 1: 30, 2: 30, 3: 20}, {0: 50, 3: 1}], "seed": 1100,
                    "tied_classes": (0, 1, 2)}
COMPACT_MANY_SPEC = {"nc": 90, "na": 2, "h": 68, "w": 68, "images": [{c: 95 for c in range(90)}], "seed": 1200}      # 9248 rows
