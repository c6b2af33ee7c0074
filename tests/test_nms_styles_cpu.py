"""Host-side tests of the NMS styles 'OR', 'AND' and 'SOFT' (``nms_style=``): the numpy restatement of the reference's three branches
(tests/_nms_styles.py) against what the reference itself returned (tests/golden/nms_styles.npz, captured by
tests/golden/make_golden_nms_styles.py), its properties on the six NMS cases, and the plumbing that needs no GPU (the style names, the
two new C-ABI symbols).  The GPU tests (tests/test_nms_styles_gpu.py) compare the kernels with this restatement.

The one tolerance: 'SOFT' conf, rtol 4e-5 / atol 2^-126 (derivation: tests/_nms_styles.py); everything else is bit-equality."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import _cases as C
import _nms_styles as S
from helpers import load_golden
from oracle import nms as onms
from pytorch_yolo_amd import YOLOv3Tiny, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_INPUTS = ("kat", "nms_small_nc2", "nms_none_pass")


def golden_input(name):
    if name == "kat":
        return C.NMS_KAT_ROWS[None].copy(), C.NMS_KAT_ARGS["conf_thres"], C.NMS_KAT_ARGS["nms_thres"]
    return C.nms_case_inputs(name)


@functools.lru_cache(maxsize=None)
def restated(name, style):
    """The restatement's (dets, kept) lists of a golden input or an NMS case, computed once per session."""
    pred, conf, iou = golden_input(name)
    if style == "MERGE":
        return onms.non_max_suppression(pred.copy(), conf, iou, mutate=False)
    return S.non_max_suppression(pred, conf, iou, style)


def golden_image(g, style, name, b):
    key = f"{style}_{name}"
    if int(g[f"{key}_count_{b}"]) == 0:
        return None, None
    return g[f"{key}_dets_{b}"], g[f"{key}_kept_{b}"]


@pytest.mark.parametrize("name", GOLDEN_INPUTS)
@pytest.mark.parametrize("style", S.STYLES)
def test_restatement_vs_reference_golden(style, name):
    g = load_golden("nms_styles")
    dets, kept = restated(name, style)
    worst = 0.0
    for b in range(len(dets)):
        gd, gk = golden_image(g, style, name, b)
        worst = max(worst, S.assert_same(style, dets[b], kept[b], gd, gk, f"{style} {name} image {b}"))
    if style == "SOFT":
        print(f"[nms styles] SOFT {name}: restatement vs reference, largest relative conf difference {worst:.3e} (bound {S.SOFT_RTOL:.1e})")


@pytest.mark.parametrize("name", list(C.NMS_CASES))
def test_or_keeps_what_merge_keeps_with_the_input_corners(name):
    """'OR' and 'MERGE' walk the same pivots: they differ only where an IoU equals nms_thres exactly (OR removes it, MERGE keeps it
    as a pivot of its own), which the continuous synthetic boxes never produce.  Every OR box is its input row's corners."""
    pred, _, _ = golden_input(name)
    dets, kept = restated(name, "OR")
    _, mkept = restated(name, "MERGE")
    for b in range(len(dets)):
        assert (dets[b] is None) == (mkept[b] is None)
        if dets[b] is None:
            continue
        assert np.array_equal(kept[b], mkept[b])
        assert np.array_equal(dets[b][:, :4], S.corners(pred[b][kept[b]]))


def test_or_counts_on_the_six_cases():
    counts = [0 if k is None else len(k) for name in C.NMS_CASES for k in restated(name, "OR")[1]]
    assert counts == [11, 672, 639, 40, 42, 25, 12, 0, 21, 86]


def test_styles_are_not_vacuous():
    """On the dense case 'AND' erases rows that 'OR' keeps but not all of them, and 'SOFT' fills the cap of every class; an image
    without survivors is None in every style."""
    n_or = [len(k) for k in restated("nms_dense_nc3", "OR")[1]]
    n_and = [len(k) for k in restated("nms_dense_nc3", "AND")[1]]
    n_soft = [len(k) for k in restated("nms_dense_nc3", "SOFT")[1]]
    assert n_or == [40, 42] and n_and == [22, 22]
    assert all(0 < a < o for a, o in zip(n_and, n_or))
    assert n_soft == [3 * onms.MAX_PER_CLASS] * 2
    for style in S.STYLES:
        dets, kept = restated("nms_none_pass", style)
        assert dets[1] is None and kept[1] is None and dets[0] is not None and dets[2] is not None


def test_known_answers():
    dets, kept = restated("kat", "OR")
    assert kept[0].tolist() == [0, 2]
    dets, kept = restated("kat", "AND")
    assert kept[0].tolist() == [0, 2]                    # row 2 is its class's only row: the n == 1 shortcut
    dets, kept = restated("kat", "SOFT")
    assert kept[0].tolist() == [0, 2, 1, 3]
    np.testing.assert_allclose(dets[0][:, 4], [0.81, 0.63, 0.16778, 0.04359], rtol=2e-4)
    assert np.array_equal(dets[0][:, 5], C.NMS_KAT_ROWS[[0, 2, 1, 3]][:, [5, 6]].max(1))       # class_conf untouched


def test_and_drops_the_last_row_and_may_erase_an_image():
    """Hand-made rows through the restatement: two disjoint boxes of one class -> None; the cap is taken before the loop."""
    rows = np.array([[50, 50, 20, 20, .9, .9], [150, 150, 20, 20, .8, .9]], dtype=np.float32)
    assert S.nms_image(rows, 0.1, 0.5, "AND") == (None, None)
    d, k = S.nms_image(rows, 0.1, 0.5, "OR")
    assert k.tolist() == [0, 1]
    d, k = S.nms_image(rows, 0.1, 0.5, "SOFT")
    assert k.tolist() == [0, 1] and np.array_equal(d[:, 4], (rows[:, 4] * rows[:, 5]))         # iou 0: the factor is exp(0) = 1


def test_unknown_style_raises_value_error():
    """Style names are the reference's, case-sensitive; the check comes first, so it needs neither a GPU nor the library."""
    from pytorch_yolo_amd.utils.utils import nms_launch, nms_raw, non_max_suppression, predict_dataset
    pred = torch.zeros(1, 4, 7)
    for bad in ("or", "HARD", "", None, 1):
        with pytest.raises(ValueError) as e:
            non_max_suppression(pred, 0.5, 0.5, nms_style=bad)
        assert all(s in str(e.value) for s in ("'MERGE'", "'OR'", "'AND'", "'SOFT'"))
    with pytest.raises(ValueError):
        nms_raw(pred, 0.5, 0.5, nms_style="soft")
    with pytest.raises(ValueError):
        nms_launch(pred, 0.5, 0.5, None, nms_style="Merge")
    model = YOLOv3Tiny().eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError):
        model.detect(x, 0.5, 0.5, nms_style="and")
    with pytest.raises(ValueError):
        next(model.detect_stream([x], 0.5, 0.5, nms_style="and"))
    with pytest.raises(ValueError):
        predict_dataset(model, [(x, None, ["a"], [(64, 64)])], nms_style="x")
    assert [_lib.nms_style_id(s) for s in ("MERGE", "OR", "AND", "SOFT")] == [0, 1, 2, 3]


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yolo_nms_styled", "yolo_nms_styled_compact"):
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name)
    # the styled entry points take their neighbours' arguments plus one int
    for new, old in (("yolo_nms_styled", "yolo_nms_merge"), ("yolo_nms_styled_compact", "yolo_nms_merge_compact")):
        (res_n, args_n), (res_o, args_o) = _lib.SIGNATURES[new], _lib.SIGNATURES[old]
        assert res_n is res_o is ctypes.c_int and args_n == args_o[:-1] + [ctypes.c_int, ctypes.c_void_p]
    enum = re.search(r"enum \{ YOLO_NMS_MERGE = (\d), YOLO_NMS_OR = (\d), YOLO_NMS_AND = (\d), YOLO_NMS_SOFT = (\d) \};", text)
    assert enum and [int(v) for v in enum.groups()] == [_lib.NMS_MERGE, _lib.NMS_OR, _lib.NMS_AND, _lib.NMS_SOFT] == [0, 1, 2, 3]
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2
