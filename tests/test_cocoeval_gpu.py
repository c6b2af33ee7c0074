"""GPU tests of the COCO bbox evaluation (csrc/coco_eval.hip through the C ABI wrappers of kernels.py, ``coco_eval``, ``bench_results``
and ``test_model``) against the numpy restatement of tests/_cocoeval.py.

Bars: matched / ignore flags and npig equal; precision and recall BIT-equal float64 (the same IEEE operations in
the same order over exact integer counts); the 12 stats equal; the per-group IoU sums and the Mean IOU within 1e-9 absolute (any
summation order of n <= 100 * G values in [0.3, 1] is within n * 2^-53 relative); two GPU runs of the same call ``torch.equal``.

Every device operand of the kernels, the workspace and the outputs sit between the poisoned bands of tests/_guard.py (0xFF and
0x7F); outputs are pre-filled with NaN or a sentinel; the bands are checked after each run."""
import numpy as np
import pytest
import torch

import _cases as C
import _cocoeval as E
import _guard as G
from helpers import build_case
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.utils import coco_eval as CE
from pytorch_yolo_amd.utils import coco_helper
from pytorch_yolo_amd.utils import utils as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, I32, I64 = torch.float64, torch.int32, torch.int64
SENTINEL = -7
_cache = {}


def case(name):
    """(dataset, results, restatement output), computed once per session and never modified."""
    if name not in _cache:
        if name in E.KNOWN:
            dataset, results = E.KNOWN[name][:2]
        else:
            dataset, results = {"S": E.case_S, "T": E.case_T, "U": lambda: E.case_U(K.coco_sweep_chunk())}[name]()
        _cache[name] = (dataset, results, E.evaluate(dataset, results))
    return _cache[name]


class Operands:
    """The device operands of one evaluation, allocated through ``a`` (a _guard.Guard or _guard.Plain)."""

    def __init__(self, a, dataset, results, max_gt=None):
        flat = CE.flatten(dataset, results)
        op = CE.prepare(flat, DEV)
        self.n_img, self.n_cat, self.n_dt = len(flat["img_ids"]), len(flat["cat_ids"]), op["dt_box"].shape[0]
        self.max_gt = op["max_gt"] if max_gt is None else max_gt
        ng = self.n_img * self.n_cat
        for key in ("dt_box", "dt_off", "gt_box", "gt_area", "gt_crowd", "gt_off", "order", "cat_off"):
            setattr(self, key, a.like(key, op[key]))
        self.iou_thrs = a.like("iou_thrs", torch.from_numpy(CE.IOU_THRS))
        self.area_rng = a.like("area_rng", torch.from_numpy(CE.AREA_RNG.reshape(-1)))
        self.rec_thrs = a.like("rec_thrs", torch.from_numpy(CE.REC_THRS))
        self.dt_match = a.alloc("dt_match", (self.n_dt,), I64, SENTINEL)
        self.dt_ignore = a.alloc("dt_ignore", (self.n_dt,), I64, SENTINEL)
        self.npig = a.alloc("npig", (self.n_cat, K.COCO_A), I32, SENTINEL)
        self.iou_sum = a.alloc("iou_sum", (ng,), F64, float("nan"))
        self.iou_cnt = a.alloc("iou_cnt", (ng,), I32, SENTINEL)
        self.status = a.alloc("status", (1,), I32, SENTINEL)
        self.ws = a.alloc("workspace", (K.coco_workspace_bytes(self.n_dt),), torch.uint8, 0xCD)
        self.precision = a.alloc("precision", (K.COCO_T, K.COCO_R, self.n_cat, K.COCO_A, K.COCO_M), F64, float("nan"))
        self.recall = a.alloc("recall", (K.COCO_T, self.n_cat, K.COCO_A, K.COCO_M), F64, float("nan"))

    def match(self):
        K.coco_match_fwd(self.dt_box, self.dt_off, self.gt_box, self.gt_area, self.gt_crowd, self.gt_off, self.n_img, self.n_cat, self.max_gt,
                         self.iou_thrs, self.area_rng, self.dt_match, self.dt_ignore, self.npig, self.iou_sum, self.iou_cnt, self.status, self.ws)

    def accumulate(self):
        K.coco_accumulate_fwd(self.order, self.cat_off, self.n_cat, self.dt_match, self.dt_ignore, self.npig, self.rec_thrs, CE.MAX_DETS, CE.EPS,
                              self.ws, self.precision, self.recall)

    def run(self):
        self.match()
        self.accumulate()
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("dt_match", "dt_ignore", "npig", "iou_sum", "iou_cnt", "status", "precision",
                                                                    "recall")}


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def assert_against_restatement(got, want, label):
    _, mbits, ibits = E.flags_in_kernel_order(want)
    assert got["status"].tolist() == [0], label
    assert np.array_equal(got["dt_match"].view(np.uint64), mbits), f"{label}: matched flags"
    assert np.array_equal(got["dt_ignore"].view(np.uint64), ibits), f"{label}: ignore flags"
    assert np.array_equal(got["npig"], want["npig"]), f"{label}: npig"
    n_cat = len(want["cat_ids"])
    s, c = np.zeros(len(got["iou_sum"])), np.zeros(len(got["iou_cnt"]), np.int32)
    for (ii, kk), g in want["groups"].items():
        s[ii * n_cat + kk], c[ii * n_cat + kk] = g["iou_sum"], g["iou_cnt"]
    assert np.array_equal(got["iou_cnt"], c), f"{label}: IoU entries >= 0.3"
    worst = float(np.abs(got["iou_sum"] - s).max())
    miou = CE.mean_iou(got["iou_sum"], got["iou_cnt"])
    print(f"[coco] {label}: largest IoU-sum difference {worst:.3e}, mean IOU {miou!r} vs {want['mean_iou']!r}")
    assert worst <= 1e-9 and abs(miou - want["mean_iou"]) <= 1e-9, f"{label}: IoU sums"
    assert not np.isnan(got["precision"]).any() and not np.isnan(got["recall"]).any(), f"{label}: an output element was not written"
    assert np.array_equal(bits(got["precision"]), bits(want["precision"])), f"{label}: precision is not bit-equal"
    assert np.array_equal(bits(got["recall"]), bits(want["recall"])), f"{label}: recall is not bit-equal"
    assert np.array_equal(CE.summarize(got["precision"], got["recall"]), want["stats"]), f"{label}: stats"


@pytest.mark.parametrize("name", list(E.KNOWN) + ["S", "T", "U"])
def test_kernels_vs_restatement(name):
    dataset, results, want = case(name)
    if name == "U":
        assert max(np.diff(CE.prepare(CE.flatten(dataset, results), "cpu")["cat_off"].numpy())) > 2 * K.coco_sweep_chunk()
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, dataset, results)
        got = op.run()
        assert_against_restatement(got, want, f"case {name} (poison 0x{poison:02X})")
        again = op.run()                                                      # the same call on the same buffers
        assert all(np.array_equal(bits(got[k]) if got[k].dtype == np.float64 else got[k], bits(again[k]) if again[k].dtype == np.float64 else again[k])
                   for k in got), f"case {name}: two runs differ"
        a.assert_intact()
    if name in E.KNOWN:
        stats = dict(zip(E.STAT_NAMES, CE.summarize(got["precision"], got["recall"])))
        for key, value in E.KNOWN[name][2].items():
            assert abs(stats[key] - value) <= 1e-12, (name, key, stats[key])


@pytest.mark.parametrize("name", ["T", "U"])
def test_two_runs_are_equal(name):
    dataset, results, _ = case(name)
    runs = []
    for _ in range(2):
        op = Operands(G.Plain(DEV), dataset, results)
        op.match()
        op.accumulate()
        runs.append(op)
    torch.cuda.synchronize()
    for key in ("dt_match", "dt_ignore", "npig", "iou_sum", "iou_cnt", "precision", "recall"):
        assert torch.equal(getattr(runs[0], key), getattr(runs[1], key)), key


def test_coco_eval_object():
    dataset, results, want = case("T")
    res = CE.coco_eval(dataset, results, DEV)
    assert np.array_equal(res.stats, want["stats"]) and res.stats.shape == (12,)
    assert np.array_equal(bits(res.precision), bits(want["precision"])) and np.array_equal(bits(res.recall), bits(want["recall"]))
    assert abs(res.mean_iou - want["mean_iou"]) <= 1e-9
    assert res.cat_ids.tolist() == want["cat_ids"] and res.img_ids.tolist() == want["img_ids"]
    holder = type("Coco", (), {"dataset": dataset})()
    assert np.array_equal(CE.coco_eval(holder, results, DEV).stats, res.stats)


def test_more_gts_than_the_cap_is_an_error_not_a_truncation():
    cap = K.coco_max_gt()
    dataset = E.dataset_of(1, [1], [(1, 1, (4 * (n % 100), 4 * (n // 100), 8, 8), 0) for n in range(cap + 1)])
    results = [E.res(1, 1, (0, 0, 8, 8), .5)]
    with pytest.raises(RuntimeError, match="cap"):
        CE.coco_eval(dataset, results, DEV)
    a = G.Guard(G.POISONS[0], DEV)
    op = Operands(a, dataset, results)
    with pytest.raises(RuntimeError, match="cap"):                           # the C entry point refuses the stated maximum
        op.match()
    op = Operands(a, dataset, results, max_gt=1)                             # a caller that misstates it: the kernel reports the group
    op.match()
    torch.cuda.synchronize()
    assert op.status.tolist() == [1] and op.dt_match.tolist() == [SENTINEL]
    a.assert_intact()


class _Dataset(torch.utils.data.Dataset):
    """A synthetic in-memory dataset in the reference's format: items (image, targets, path, original shape), ``collate_fn``, and
    ``.coco.dataset``."""

    def __init__(self, imgs, shape, nc):
        self.imgs, self.shape = imgs, shape
        self.paths = [f"img{i}.jpg" for i in range(len(imgs))]
        self.coco = type("Coco", (), {})()
        self.coco.dataset = {"images": [{"id": 10 + i, "file_name": p, "height": shape[0], "width": shape[1]} for i, p in enumerate(self.paths)],
                             "categories": [{"id": c, "name": f"c{c}"} for c in range(nc)], "annotations": []}

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        return self.imgs[i], torch.zeros((0, 6)), self.paths[i], self.shape

    @staticmethod
    def collate_fn(batch):
        imgs, targets, paths, shapes = zip(*batch)
        return torch.stack(imgs), torch.cat(targets), list(paths), list(shapes)


def test_test_model_end_to_end(capsys):
    from pytorch_yolo_amd.utils.synthetic import synth_images
    spec = C.MODEL_CASES["tiny_small"]
    model, _, x = build_case(spec)
    model = model.to(DEV)
    nc = spec[1]["n_class"]
    with torch.no_grad():
        io, _ = model(x.to(DEV))
    conf = float((io[..., 4] * io[..., 5:].max(-1).values).flatten().median())     # a threshold this random-weight model clears
    dataset = _Dataset(synth_images(5, 64, 96, 70), (128, 192), nc)
    loader = [dataset.collate_fn([dataset[i] for i in idx]) for idx in ((0, 1), (2, 3), (4,))]
    data = U.predict_dataset(model, loader, conf, 0.5)
    first = coco_helper.results_from_dict(data, dataset.coco.dataset)
    assert len(first) >= 10, "the comparison is vacuous"
    # ground truth: every third detection as it is, every third shrunk to 3/4 of its height, plus a crowd box per image
    anns = []
    for n, r in enumerate(first):
        if n % 3 == 2:
            continue
        x0, y0, w, h = r["bbox"]
        box = [x0, y0, w, h] if n % 3 == 0 else [x0, y0, w, max(1, 3 * h // 4)]
        anns.append({"id": len(anns) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": box, "area": box[2] * box[3],
                     "iscrowd": 0})
    for im in dataset.coco.dataset["images"]:
        anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": 0, "bbox": [0, 0, 96, 64], "area": 96 * 64, "iscrowd": 1})
    dataset.coco.dataset["annotations"] = anns

    model.train()
    metrics = U.test_model(model, dataset, 2, 0, DEV, conf, 0.5)
    printed = capsys.readouterr().out
    assert model.training
    model.eval()
    assert U.test_model(model, dataset, 2, 0, DEV, conf, 0.5) == metrics and not model.training
    assert printed.count("Average Precision") == 6 and printed.count("Average Recall") == 6 and "Mean IOU:" in printed
    assert list(metrics) == ["AP", "AP50", "AP75", "APS", "APM", "APL", "AR1", "AR10", "AR100", "ARS", "ARM", "ARL", "IOU"]
    assert all(isinstance(v, float) for v in metrics.values())
    want = E.evaluate(dataset.coco.dataset, first)
    assert [metrics[k] for k in E.STAT_NAMES] == want["stats"].tolist()
    assert abs(metrics["IOU"] - want["mean_iou"]) <= 1e-9
    assert metrics["AP50"] > 0 and metrics["AR100"] > 0 and metrics["IOU"] > 0, "the comparison is vacuous"
    assert U.bench_results(first, dataset.coco, DEV) == metrics
