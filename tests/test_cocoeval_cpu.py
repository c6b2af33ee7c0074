"""CPU-only checks of the COCO evaluation (utils/coco_eval.py, csrc/coco_eval.hip): the numpy restatement of tests/_cocoeval.py
against hand-derived known answers (bar 1e-12: the precision carries np.spacing(1)), what the seeded cases promise,
``results_from_dict`` against the reference's own answers (tests/golden/coco_results.json), the host flattening and orderings, the
C entry points (declared, exported, argument errors without a device), and - wherever pycocotools is installed - the restatement
against the real library (skipped elsewhere: parity with pycocotools is unpinned there)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import _cocoeval as E
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.utils import coco_eval as CE
from pytorch_yolo_amd.utils import coco_helper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_coco_sweep_chunk", "yolo_coco_max_gt", "yolo_coco_workspace_bytes", "yolo_coco_match_fwd", "yolo_coco_accumulate_fwd")
BAR = 1e-12


def stats_of(dataset, results):
    out = E.evaluate(dataset, results)
    return dict(zip(E.STAT_NAMES, out["stats"])), out


@pytest.mark.parametrize("name", list(E.KNOWN))
def test_known_answers(name):
    dataset, results, want = E.KNOWN[name]
    stats, out = stats_of(dataset, results)
    for key, value in want.items():
        assert abs(stats[key] - value) <= BAR, (name, key, stats[key], value)
    if name == "two_gt_one_det":
        assert E.REC_THRS[50] == 0.5
    if name == "iou_exactly_half":                         # IoU exactly 0.5: matched at threshold 0.5, not at 0.55
        g = out["groups"][(0, 0)]
        assert E.bb_iou((0, 0, 10, 5), E.GT10, 0) == 0.5
        assert g["matched"][0, :, 0].tolist() == [True] + [False] * 9
        assert out["precision"][1, 0, 0, 0, 2] == 0.0


def test_crowd_absorbs_two_detections():
    dataset = E.dataset_of(1, [1], [(1, 1, E.GT10, 0), (1, 1, (100, 100, 40, 40), 1)])
    results = [E.res(1, 1, E.GT10, .9), E.res(1, 1, (100, 100, 20, 20), .8), E.res(1, 1, (110, 110, 20, 20), .7)]
    stats, out = stats_of(dataset, results)
    g = out["groups"][(0, 0)]
    assert g["matched"][0, 0].tolist() == [True, True, True] and g["ignore"][0, 0].tolist() == [False, True, True]
    assert abs(stats["AP50"] - 1.0) <= BAR and stats["AR100"] == 1.0 and out["npig"][0, 0] == 1


def test_area_exactly_1024_is_small_and_medium():
    dataset = E.dataset_of(1, [1], [(1, 1, (0, 0, 32, 32), 0)])
    stats, out = stats_of(dataset, [E.res(1, 1, (0, 0, 32, 32), .9)])
    assert out["npig"][0].tolist() == [1, 1, 1, 0]
    assert abs(stats["APS"] - 1.0) <= BAR and abs(stats["APM"] - 1.0) <= BAR and stats["APL"] == -1.0


def test_category_without_gt_and_category_without_detections():
    dataset = E.dataset_of(1, [1, 2, 3], [(1, 1, E.GT10, 0), (1, 3, E.GT10, 0)])
    _, out = stats_of(dataset, [E.res(1, 1, E.GT10, .9), E.res(1, 2, E.GT10, .9)])
    assert (out["precision"][:, :, 1] == -1).all() and (out["recall"][:, 1] == -1).all()              # category 2: no GT
    assert (out["precision"][:, :, 2, :2] == 0).all() and (out["recall"][:, 2, :2] == 0).all()        # category 3: no detections
    assert (out["precision"][:, :, 2, 2:] == -1).all()                                                # ... and no medium / large GT


def test_seeded_cases_keep_their_promises():
    chunk = K.coco_sweep_chunk()
    s, t, u = E.case_properties(*E.case_S()), E.case_properties(*E.case_T()), E.case_properties(*E.case_U(chunk))
    assert s["max_dt"] <= 6 and s["max_gt"] <= 4 and len(E.case_S()[0]["images"]) == 3
    assert t["max_dt"] == 130 > 100 and t["max_gt"] == 70 > 64 and t["crowd"]
    for p in (s, t, u):
        assert p["ties_in_group"] and p["ties_across_images"] and p["exact_ious"] == {0.5, 0.75} and p["has_1024"] and p["has_9216"]
    assert u["n_results"] > 2 * chunk and u["n_results"] % chunk != 0 and u["max_dt"] <= 100 and len(E.case_U(chunk)[0]["images"]) == 40
    dataset, results = E.case_T()
    out = E.evaluate(dataset, results)
    cats = out["cat_ids"]
    assert (out["npig"][cats.index(7)] == 0).all() and (out["recall"][:, cats.index(9), 0] == 0).all()
    # duplicate GT boxes: a detection equal to both matches the LATER one
    dataset = E.dataset_of(1, [1], [(1, 1, E.GT10, 0), (1, 1, E.GT10, 0), (1, 1, E.FAR, 0)])
    assert abs(stats_of(dataset, [E.res(1, 1, E.GT10, .9)])[0]["AR100"] - 1 / 3) <= BAR


@pytest.mark.parametrize("name", ["some", "none", "only_empty_lists"])
def test_results_from_dict_vs_golden(name):
    with open(os.path.join(ROOT, "tests", "golden", "coco_results.json")) as f:
        g = json.load(f)[name]
    data = {file_name: preds for file_name, preds in g["data"]}              # (stored as pairs: the dictionary's order matters)
    got = coco_helper.results_from_dict(data, g["annotations"])
    assert got == g["results"] and [list(r) for r in got] == [list(r) for r in g["results"]]
    if name != "some":
        assert got == [{"image_id": 1, "category_id": 0, "bbox": [0, 0, 0, 0], "score": 0}]
    with pytest.raises(KeyError):
        coco_helper.results_from_dict({"unknown.jpg": []}, g["annotations"])


def test_flatten_order_and_dropped_categories():
    dataset, results = E.case_T()
    flat = CE.flatten(dataset, results)
    assert flat["img_ids"].tolist() == list(range(1, 10)) and flat["cat_ids"].tolist() == [1, 3, 4, 7, 9]
    known = [r for r in results if r["category_id"] in (1, 3, 4, 7, 9)]
    assert len(known) == len(results) - 1 == len(flat["dt_score"])
    assert (np.diff(flat["dt_group"]) >= 0).all() and (np.diff(flat["gt_group"]) >= 0).all()
    # inside a group: the order of the results list
    group_of = lambda r: (r["image_id"] - 1) * 5 + [1, 3, 4, 7, 9].index(r["category_id"])
    want = sorted(range(len(known)), key=lambda i: group_of(known[i]))                  # (sorted is stable)
    assert np.array_equal(flat["dt_box"], np.asarray([known[i]["bbox"] for i in want], dtype=np.float64))
    assert np.array_equal(flat["dt_score"], np.asarray([known[i]["score"] for i in want]))
    anns = dataset["annotations"]
    want = sorted(range(len(anns)), key=lambda i: group_of(anns[i]))
    assert np.array_equal(flat["gt_box"], np.asarray([anns[i]["bbox"] for i in want], dtype=np.float64))
    assert np.array_equal(flat["gt_crowd"], np.asarray([anns[i]["iscrowd"] for i in want], dtype=np.uint8))
    assert flat["gt_off"][-1] == len(anns) and flat["gt_off"].dtype == np.int32 and len(flat["gt_off"]) == 46
    # a .dataset attribute and a JSON path are accepted
    holder = type("Coco", (), {"dataset": dataset})()
    assert np.array_equal(CE.flatten(holder, results)["dt_box"], flat["dt_box"])


def test_flatten_accepts_a_json_path(tmp_path):
    dataset, results = E.case_S()
    path = tmp_path / "results.json"
    path.write_text(json.dumps(results))
    a, b = CE.flatten(dataset, str(path)), CE.flatten(dataset, results)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_flatten_refusals():
    dataset, results = E.case_S()
    with pytest.raises(ValueError, match="images"):
        CE.flatten(dataset, results + [E.res(99, 1, E.GT10, .5)])
    for bad in (E.res(1, 1, (0, 0, float("nan"), 4), .5), E.res(1, 1, (0, 0, float("inf"), 4), .5), E.res(1, 1, E.GT10, float("nan"))):
        with pytest.raises(ValueError, match="non-finite"):
            CE.flatten(dataset, results + [bad])
    with pytest.raises(ValueError, match="bbox"):
        CE.flatten(dataset, [{"image_id": 1, "category_id": 1, "score": .5, "segmentation": []}])
    with pytest.raises(ValueError):
        CE.flatten(dataset, {"not": "a list"})
    with pytest.raises(RuntimeError, match="ROCm device only"):
        CE.coco_eval(dataset, results, "cpu")


@pytest.mark.parametrize("case", ["S", "T", "U"])
def test_orderings_equal_the_restatement(case):
    """prepare() - index plumbing, run here on the CPU - yields pycocotools' evaluation order (stable, cut to 100) and sweep order."""
    dataset, results = {"S": E.case_S, "T": E.case_T, "U": lambda: E.case_U(K.coco_sweep_chunk())}[case]()
    flat = CE.flatten(dataset, results)
    op = CE.prepare(flat, "cpu")
    out = E.evaluate(dataset, results)
    order, _, _ = E.flags_in_kernel_order(out)
    known = [r for r in results if r["category_id"] in set(out["cat_ids"])]
    index_in_known = {id(r): i for i, r in enumerate(known)}
    want_box = np.asarray([results[n]["bbox"] for n in order], dtype=np.float64).reshape(-1, 4)
    assert np.array_equal(op["dt_box"].numpy(), want_box)
    assert np.array_equal(op["dt_score"].numpy(), np.asarray([results[n]["score"] for n in order], dtype=np.float64))
    counts = np.diff(op["dt_off"].numpy())
    assert counts.max() <= 100 and counts.sum() == len(order) and op["dt_off"].dtype == torch.int32
    if case == "T":
        assert counts.max() == 100 and len(known) - len(order) == 30 and op["max_gt"] == 70
    # sweep order: category by category, descending score, ties in (image, rank) order = ascending flat index
    sweep, cat_off, K_ = op["order"].numpy(), op["cat_off"].numpy(), len(out["cat_ids"])
    score = op["dt_score"].numpy()
    cat = np.repeat(np.arange(len(counts)), counts) % K_
    assert sorted(sweep.tolist()) == list(range(len(order))) and cat_off[-1] == len(order)
    for k in range(K_):
        part = sweep[cat_off[k]:cat_off[k + 1]]
        assert (cat[part] == k).all()
        mine = np.nonzero(cat == k)[0]
        assert np.array_equal(part, mine[np.argsort(-score[mine], kind="mergesort")])
    assert index_in_known


def test_summarize_and_mean_iou_expressions():
    dataset, results = E.case_T()
    out = E.evaluate(dataset, results)
    assert np.array_equal(CE.summarize(out["precision"], out["recall"]), out["stats"])
    assert np.array_equal(CE.IOU_THRS, E.IOU_THRS) and np.array_equal(CE.REC_THRS, E.REC_THRS) and CE.AREA_RNG.tolist() == E.AREA_RNG
    assert CE.EPS == np.spacing(1) and tuple(CE.MAX_DETS) == tuple(E.MAX_DETS)
    n = len(out["img_ids"]) * len(out["cat_ids"])
    s, c = np.zeros(n), np.zeros(n, np.int32)
    for (ii, kk), g in out["groups"].items():
        s[ii * len(out["cat_ids"]) + kk], c[ii * len(out["cat_ids"]) + kk] = g["iou_sum"], g["iou_cnt"]
    assert abs(CE.mean_iou(s, c) - out["mean_iou"]) <= 1e-12
    assert CE.mean_iou(np.zeros(4), np.zeros(4, np.int32)) == 0.0


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    declared = re.findall(r"YOLO_API\s+[\w\s\*]+?\b(yolo_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert declared.count(name) == 1 and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.load().yolo_abi_version() == _lib.ABI_VERSION == 2            # no new struct, no changed meaning
    import pytorch_yolo_amd as pkg
    from pytorch_yolo_amd.utils import utils as U
    for name in ("bench_results", "test_model"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(U, name)
    assert "coco_eval" in pkg.__all__ and pkg.coco_eval is CE.coco_eval
    assert K.coco_sweep_chunk() >= 64 and K.coco_max_gt() >= 128
    assert K.coco_workspace_bytes(0) > 0 and K.coco_workspace_bytes(1000) >= 4000
    assert K.coco_workspace_bytes(2000) - K.coco_workspace_bytes(1000) <= 4 * 1000 + 256        # linear in nD


def test_argument_errors_without_a_device():
    """Every bad-argument path returns before any launch: fake non-null pointers are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    big = 1 << 30
    md = (ctypes.c_int32 * 3)(1, 10, 100)

    def match(**kw):
        a = dict(dt_box=fake, dt_off=fake, n_dt=5, gt_box=fake, gt_area=fake, gt_crowd=fake, gt_off=fake, n_gt=2000, n_img=2, n_cat=3, max_gt=4,
                 iou_thrs=fake, area_rng=fake, dt_match=fake, dt_ignore=fake, npig=fake, iou_sum=fake, iou_cnt=fake, status=fake, ws=fake,
                 ws_bytes=big)
        a.update(kw)
        return lib.yolo_coco_match_fwd(*a.values(), None)

    def accumulate(**kw):
        a = dict(order=fake, cat_off=fake, n_dt=5, n_cat=3, dt_match=fake, dt_ignore=fake, npig=fake, rec_thrs=fake, max_dets=md,
                 eps=float(np.spacing(1)), ws=fake, ws_bytes=big, precision=fake, recall=fake)
        a.update(kw)
        return lib.yolo_coco_accumulate_fwd(*a.values(), None)

    def failed(rc, code, text):
        msg = lib.yolo_last_error().decode()
        assert rc == code and text in msg, (rc, msg)

    for key in ("dt_box", "dt_off", "gt_box", "gt_area", "gt_crowd", "gt_off", "iou_thrs", "area_rng", "dt_match", "dt_ignore", "npig", "iou_sum",
                "iou_cnt", "status", "ws"):
        failed(match(**{key: None}), -1, "null")
    failed(match(n_dt=-1), -1, "negative")
    failed(match(n_gt=-1), -1, "negative")
    failed(match(n_img=0), -1, "unsupported")
    failed(match(n_cat=0), -1, "unsupported")
    failed(match(n_img=1 << 20, n_cat=1 << 12), -1, "unsupported")
    failed(match(max_gt=-1), -1, "max_gt")
    failed(match(max_gt=2001), -1, "max_gt")
    failed(match(max_gt=K.coco_max_gt() + 1), -2, "cap")                       # above the cap: an error, never a truncation
    failed(match(ws_bytes=8), -3, "workspace")
    for key in ("order", "cat_off", "dt_match", "dt_ignore", "npig", "rec_thrs", "max_dets", "ws", "precision", "recall"):
        failed(accumulate(**{key: None}), -1, "null")
    failed(accumulate(n_dt=-1), -1, "negative")
    failed(accumulate(n_cat=0), -1, "unsupported")
    failed(accumulate(max_dets=(ctypes.c_int32 * 3)(10, 1, 100)), -1, "ascending")
    failed(accumulate(eps=0.0), -1, "spacing")
    failed(accumulate(ws_bytes=8), -3, "workspace")
    assert lib.yolo_coco_workspace_bytes(-1) == 0 and "negative" in lib.yolo_last_error().decode()
    # the Python wrappers refuse host tensors and wrong dtypes before the FFI crossing
    with pytest.raises(RuntimeError, match="ROCm device"):
        K.coco_accumulate_fwd(*[torch.zeros(4, dtype=torch.int32)] * 2, 1, *[torch.zeros(4)] * 4, (1, 10, 100), 1e-16, *[torch.zeros(4)] * 3)


def test_restatement_vs_pycocotools(tmp_path):
    """Wherever the real library is installed: the restatement's arrays equal pycocotools' on every seeded case."""
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    for dataset, results in (E.case_S(), E.case_T(), E.case_U(K.coco_sweep_chunk())) + tuple(v[:2] for v in E.KNOWN.values()):
        results = [r for r in results if r["category_id"] in set(c["id"] for c in dataset["categories"])]
        gt = COCO()
        gt.dataset = dataset
        gt.createIndex()
        ev = COCOeval(gt, gt.loadRes(results), "bbox")
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        out = E.evaluate(dataset, results)
        assert np.array_equal(ev.eval["precision"], out["precision"]) and np.array_equal(ev.eval["recall"], out["recall"])
        assert np.array_equal(ev.stats, out["stats"])
