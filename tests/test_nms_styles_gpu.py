"""GPU tests of the NMS styles 'OR', 'AND' and 'SOFT' (``nms_style=``; csrc/nms.hip, one instantiation of nms_merge_kernel per style)
against the numpy restatement of the reference's three branches (tests/_nms_styles.py) and, on the three captured inputs, against the
reference itself (tests/golden/nms_styles.npz).

Comparisons (tests/_nms_styles.assert_same):
  * 'OR', 'AND': kept indices equal, all seven columns bit-equal;
  * 'SOFT': kept-index sets equal; boxes, class_conf and class bit-equal after pairing rows by kept index; conf within rtol 4e-5 /
    atol 2^-126 (99 factors x (1 ulp per side's exp + 1/2 ulp per side's multiply); derivation in tests/_nms_styles.py); the conf
    column non-increasing.  Every 'SOFT' test prints the largest relative conf difference it saw.
Where two GPU runs of the same kernel on the same input are compared (detect() against the composition, the guarded runs, MERGE through
the old and the new entry point) the comparison is bit-equality in every style."""
import numpy as np
import pytest
import torch

import _cases as C
import _guard as G
import _nms_styles as S
from helpers import build_case, load_golden
from oracle import nms as onms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
GOLDEN_INPUTS = ("kat", "nms_small_nc2", "nms_none_pass")


def _inputs(name):
    if name == "kat":
        return C.NMS_KAT_ROWS[None].copy(), C.NMS_KAT_ARGS["conf_thres"], C.NMS_KAT_ARGS["nms_thres"]
    return C.nms_case_inputs(name)


def _run(pred_np, conf, iou, style):
    from pytorch_yolo_amd.utils.utils import non_max_suppression
    pred = torch.from_numpy(pred_np.copy()).to(DEV)
    dets, idx = non_max_suppression(pred, conf, iou, with_indices=True, nms_style=style)
    assert np.array_equal(pred.cpu().numpy(), pred_np, equal_nan=True)                        # the input is left alone
    to_np = lambda t: None if t is None else t.cpu().numpy()
    return [to_np(d) for d in dets], [to_np(i) for i in idx]


def _check_vs_restatement(pred, conf, iou, style, tag):
    dets, idx = _run(pred, conf, iou, style)
    want, want_idx = S.non_max_suppression(pred, conf, iou, style)
    worst = 0.0
    for b in range(pred.shape[0]):
        worst = max(worst, S.assert_same(style, dets[b], idx[b], want[b], want_idx[b], f"{style} {tag} image {b}"))
    if style == "SOFT":
        print(f"[nms styles] SOFT {tag}: kernel vs restatement, largest relative conf difference {worst:.3e} (bound {S.SOFT_RTOL:.1e})")
    return dets, idx, want, want_idx


@pytest.mark.parametrize("name", list(C.NMS_CASES) + ["kat"])
@pytest.mark.parametrize("style", S.STYLES)
def test_styles_vs_restatement(style, name):
    pred, conf, iou = _inputs(name)
    dets, idx, want, _ = _check_vs_restatement(pred, conf, iou, style, name)
    if name in GOLDEN_INPUTS:
        g = load_golden("nms_styles")
        worst = 0.0
        for b in range(pred.shape[0]):
            key = f"{style}_{name}"
            n = int(g[f"{key}_count_{b}"])
            gd, gk = (g[f"{key}_dets_{b}"], g[f"{key}_kept_{b}"]) if n else (None, None)
            worst = max(worst, S.assert_same(style, dets[b], idx[b], gd, gk, f"{style} {name} image {b} vs the reference"))
        if style == "SOFT":
            print(f"[nms styles] SOFT {name}: kernel vs reference golden, largest relative conf difference {worst:.3e}")
    if name == "nms_dense_nc3":                          # the cap is reached: the loops run at their longest
        n = [len(d) for d in want]
        assert n == ([300, 300] if style == "SOFT" else n) and all(v > 0 for v in n)


@pytest.mark.parametrize("seed", range(8))
def test_styles_random_sweep(seed):
    """The generator of test_nms_random_sweep_vs_oracle (random batch sizes, row counts, class counts incl. 1, 2, 3, 5, 7, thresholds,
    forced ties of the class maximum), the style drawn from the seed."""
    rng = np.random.default_rng(1000 + seed)
    bs = int(rng.integers(1, 4))
    rows = int(rng.choice([17, 64, 65, 300, 1000]))
    nc = int(rng.choice([1, 2, 3, 5, 7, 20, 80]))
    conf, iou = float(rng.choice([0.05, 0.1, 0.3])), float(rng.choice([0.3, 0.5, 0.7]))
    pred = C.synth_predictions(2000 + seed, bs, rows, nc)
    if nc > 1:                                   # exact ties between two classes on a tenth of the rows
        tie = rng.random((bs, rows)) < 0.1
        a, b2 = rng.integers(0, nc, 2)
        top = pred[..., 5:].max(-1)
        for cls in (int(a), int(b2)):
            pred[..., 5 + cls] = np.where(tie, top, pred[..., 5 + cls])
    style = S.STYLES[seed % len(S.STYLES)]
    _check_vs_restatement(pred, conf, iou, style, f"sweep seed {seed} (bs {bs}, rows {rows}, nc {nc})")


def _rows(*rows, nc=2):
    """Hand-made prediction rows (x, y, w, h, obj, class, class score) -> [n, 5 + nc] float32, the other class scores 0."""
    out = np.zeros((len(rows), 5 + nc), dtype=np.float32)
    for i, (x, y, w, h, obj, cls, score) in enumerate(rows):
        out[i, :5] = (x, y, w, h, obj)
        out[i, 5 + cls] = score
    return out


def test_styles_edges_iou_equal_to_the_threshold():
    """Two 20x20 boxes shifted by 10: IoU = 200 / 600 in fp32; with exactly that value as nms_thres 'OR' removes the second box
    (it keeps iou < nms_thres only), 'MERGE' leaves it alone (it merges iou > nms_thres only) and emits it as a pivot of its own."""
    pred = _rows((50, 50, 20, 20, .9, 0, .9), (60, 50, 20, 20, .8, 0, .9))[None]
    thr = np.float32(200) / ((np.float32(400) + np.float32(1e-16)) + np.float32(400) - np.float32(200))
    assert S._iou_1_to_n(S.corners(pred[0])[0], S.corners(pred[0])[1:])[0] == thr
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, float(thr), "OR", "iou == thres")
    assert idx[0].tolist() == [0]
    _, midx = _run(pred, 0.1, float(thr), "MERGE")
    assert midx[0].tolist() == [0, 1]
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, float(np.nextafter(thr, np.float32(1))), "OR", "iou just below thres")
    assert idx[0].tolist() == [0, 1]


def test_styles_edges_and_erases():
    """'AND': two disjoint boxes of one class -> the image is None; a pair with IoU 0.40 at nms_thres 0.3 is neither emitted (0.40 is
    not > 0.5) nor kept (0.40 is not < 0.3); a lone box of another class is kept (the n == 1 shortcut)."""
    filler = (300, 300, 20, 20, 0., 1, .5)
    img0 = _rows((50, 50, 20, 20, .9, 0, .9), (150, 150, 20, 20, .8, 0, .9), filler)
    img1 = _rows((50, 50, 20, 20, .9, 0, .9), (58.5, 50, 20, 20, .8, 0, .9), (200, 200, 30, 30, .7, 1, .9))
    pred = np.stack([img0, img1])
    iou = S._iou_1_to_n(S.corners(img1)[0], S.corners(img1)[1:2])[0]
    assert 0.3 < iou < 0.5
    dets, idx, _, _ = _check_vs_restatement(pred, 0.1, 0.3, "AND", "erase")
    assert dets[0] is None and idx[1].tolist() == [2]
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, 0.3, "OR", "erase")
    assert idx[0].tolist() == [0, 1] and idx[1].tolist() == [0, 2]


def test_styles_edges_cap_of_100():
    """A class of 130 rows, conf descending with the row index, every box 40 px from the next except where said:
      rows 0..97   49 pairs (2k, 2k + 1) of boxes shifted by 2 px (IoU 0.82): the head of each pair is emitted, its partner removed;
      row 98       alone: 'OR' emits it, 'AND' does not;
      row 99       the 100th: its only overlap partner is row 100, the 101st, which the cap cuts off.  So under 'AND' it is the last
                   row left and is NOT emitted (without the cap, row 100 would make it a head with max iou > 0.5); 'OR' emits it;
      rows 101..129 alone: beyond the cap in both styles ('OR' without the cap would emit them).
    A class of one row (n == 1) is kept in both styles."""
    rows = []
    for k in range(130):
        cell = k // 2 if k < 98 else k - 49              # a 40 px grid cell per pair, then one per row (rows 99 and 100 share one)
        if k >= 100:
            cell -= 1
        x, y = 30 + 40 * (cell % 13), 30 + 40 * (cell // 13)
        if (k < 98 and k % 2) or k == 100:
            x += 2
        rows.append((x, y, 20, 20, 0.99 - 0.005 * k, 0, .9))
    rows.append((30, 700, 20, 20, .5, 1, .9))
    pred = _rows(*rows)[None]
    xy = pred[0, :130, :2]
    d = np.abs(xy[:, None] - xy[None]).max(-1) + np.eye(130) * 1e3
    assert sorted(map(tuple, np.argwhere(d < 20))) == sorted([(2 * k, 2 * k + 1) for k in range(49)] + [(2 * k + 1, 2 * k) for k in range(49)] + [(99, 100), (100, 99)])
    heads = list(range(0, 98, 2))
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, 0.5, "AND", "cap")
    assert sorted(idx[0].tolist()) == heads + [130]
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, 0.5, "OR", "cap")
    assert sorted(idx[0].tolist()) == heads + [98, 99, 130]
    _, idx, _, _ = _check_vs_restatement(pred, 0.1, 0.5, "SOFT", "cap")
    assert sorted(idx[0].tolist()) == list(range(100)) + [130]


def test_styles_edges_threshold_of_one():
    """nms_thres = 1.0: 'OR', 'AND' and 'SOFT' terminate for any threshold; 'MERGE' would not, and is still refused."""
    pred, conf, _ = _inputs("nms_small_nc2")
    for style in S.STYLES:
        _check_vs_restatement(pred, conf, 1.0, style, "nms_thres 1.0")
    with pytest.raises(RuntimeError, match="nms_thres must be < 1"):
        _run(pred, conf, 1.0, "MERGE")


@pytest.mark.parametrize("style", ["OR", "SOFT"])
def test_many_survivors_styles(style):
    """> 8192 survivors in one image (the input of test_nms_many_survivors_global_sort_path): the keys are sorted in the global
    workspace ahead of the new loops."""
    pred = C.synth_predictions(77, 1, 12000, 4)
    pred[0, :, 4] = np.maximum(pred[0, :, 4], np.float32(0.5))
    assert len(S.candidates(pred[0], 0.001)[0]) > 8192
    _check_vs_restatement(pred, 0.001, 0.5, style, "12000 rows")


def _lists_equal(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v))


@pytest.mark.parametrize("name", ["tiny_small", "spp_kd2_nc80"])
@pytest.mark.parametrize("style", S.STYLES)
def test_detect_equals_composition(style, name):
    """model.detect(x, c, t, nms_style=s) - the per-launch path: the one-call pipeline step is MERGE-only - is bit-equal to
    non_max_suppression(model(x)[0], c, t, nms_style=s), indices included, and so is every batch of detect_stream().  Both plans take
    the compact NMS form (yolo_nms_styled_compact); launch_detect(compact=False) runs the plain one on io as well.  Thresholds: those of
    test_detect_without_raw_head_tensors (0.05 / 0.5), at which these random-weight models detect nothing (scores stay below 0.01),
    and - so that the comparison is not vacuous - the median score of the model's own rows, a rule on the data like
    test_fp16_gpu.py's.  Afterwards detect() / detect_stream() without the keyword are still the MERGE composition: a ring built for
    one style is never handed to another."""
    from pytorch_yolo_amd.utils.utils import nms_capacity, non_max_suppression, split_detections
    model, sd, x = build_case(C.MODEL_CASES[name])
    model = model.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        io, _ = model(xd)
        plan = model.plan_for(xd)
        assert plan.compact_ok
        score = io[..., 4] * io[..., 5:].max(-1).values
        for conf, iou in ((0.05, 0.5), (float(score.flatten().median()), 0.5)):
            want, want_idx = non_max_suppression(io, conf, iou, with_indices=True, nms_style=style)
            _lists_equal(model.detect(xd, conf, iou, nms_style=style), want)
            cap = nms_capacity(plan.rows_total, model.n_class)
            out = (torch.empty((xd.shape[0], cap, 7), dtype=F32, device=DEV), torch.empty((xd.shape[0], cap), dtype=torch.int32, device=DEV),
                   torch.empty((xd.shape[0],), dtype=torch.int32, device=DEV))
            io2, ps = plan.new_outputs(want_p=False)
            for compact in (True, False):
                plan.launch_detect(xd, io2, ps, out, conf, iou, compact=compact, nms_style=style)
                torch.cuda.synchronize()
                got, got_idx = split_detections(*out, with_indices=True)
                _lists_equal(got, want)
                _lists_equal(got_idx, want_idx)
            streamed = list(model.detect_stream([xd] * 4, conf, iou, nms_style=style))
            assert len(streamed) == 4
            for lst in streamed:
                _lists_equal(lst, want)
        assert max(0 if d is None else len(d) for d in want) >= 5, "the comparison is vacuous"
        merged = non_max_suppression(io, conf, iou)
        assert any(m is not None and (w is None or m.shape != w.shape or not torch.equal(m, w)) for m, w in zip(merged, want))
        _lists_equal(model.detect(xd, conf, iou), merged)
        for lst in model.detect_stream([xd] * 4, conf, iou):
            _lists_equal(lst, merged)
        for lst in model.detect_stream([xd] * 4, conf, iou, nms_style=style):      # ... and back: the style's own ring is reused
            _lists_equal(lst, want)


def _kept(dets, idx, cnt):
    torch.cuda.synchronize()
    c = cnt.cpu().tolist()
    cap = dets.shape[1]
    return {"count": cnt, "dets": torch.cat([dets[b, :min(m, cap)] for b, m in enumerate(c)]),
            "idx": torch.cat([idx[b, :min(m, cap)] for b, m in enumerate(c)])}


@pytest.mark.parametrize("style", S.STYLES)
def test_styled_guarded(style):
    """yolo_nms_styled with pred, the workspace (pre-filled with 0xCD) and the three outputs between the poisoned bands of
    tests/_guard.py: the guarded outputs are bit-equal to a plain run, every margin keeps its poison, pred is not written."""
    from pytorch_yolo_amd import _lib
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import MAX_PER_CLASS, MIN_WH, nms_capacity
    pred, conf, iou = _inputs("nms_none_pass")
    bs, rows, no = pred.shape
    nc = no - 5
    cap = nms_capacity(rows, nc)
    pred_t = torch.from_numpy(pred.copy())

    def body(a):
        p = a.like("pred", pred_t, plane=rows * no)
        ws = a.alloc("workspace", (K.nms_workspace_bytes(bs, rows, nc),), torch.uint8, 0xCD)
        dets = a.alloc("dets", (bs, cap, 7), F32, -3.0, plane=cap * 7)
        idx = a.alloc("idx", (bs, cap), torch.int32, -3, plane=cap)
        cnt = a.alloc("count", (bs,), torch.int32, -3)
        K.nms_styled(p, conf, iou, dets, idx, cnt, ws, style=_lib.NMS_STYLES[style], min_wh=MIN_WH, max_per_class=MAX_PER_CLASS)
        out = _kept(dets, idx, cnt)
        out["pred"] = p
        return out

    want = body(G.Plain(DEV))
    want = {k: v.detach().clone() for k, v in want.items()}
    rd, rk = S.non_max_suppression(pred, conf, iou, style)
    counts = want["count"].cpu().tolist()
    assert counts == [0 if d is None else len(d) for d in rd] and sum(counts) > 0
    off = 0
    for b, n in enumerate(counts):
        if n:
            S.assert_same(style, want["dets"][off:off + n].cpu().numpy(), want["idx"][off:off + n].cpu().numpy(), rd[b], rk[b], f"{style} image {b}")
        off += n
    assert np.array_equal(want["pred"].cpu().numpy(), pred, equal_nan=True), "pred is read-only without mutate_conf"
    for poison in G.POISONS:
        g = G.Guard(poison, DEV)
        got = body(g)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k].cpu().contiguous().view(-1).view(torch.uint8), want[k].cpu().contiguous().view(-1).view(torch.uint8)), \
                f"{k} (poison 0x{poison:02X}) differs from the plain run: a read outside an operand"
        g.assert_intact()


def test_merge_unchanged_through_new_entry():
    """yolo_nms_styled(..., YOLO_NMS_MERGE) and yolo_nms_merge: byte-identical dets, idx and count; an unknown style is refused."""
    from pytorch_yolo_amd import _lib
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import MAX_PER_CLASS, MIN_WH, nms_capacity
    pred, conf, iou = _inputs("nms_mid_nc80")
    bs, rows, no = pred.shape
    nc = no - 5
    cap = nms_capacity(rows, nc)
    p = torch.from_numpy(pred).to(DEV)
    ws = torch.empty(K.nms_workspace_bytes(bs, rows, nc), dtype=torch.uint8, device=DEV)
    mk = lambda: (torch.zeros((bs, cap, 7), device=DEV), torch.zeros((bs, cap), dtype=torch.int32, device=DEV),
                  torch.zeros((bs,), dtype=torch.int32, device=DEV))
    a, b = mk(), mk()
    K.nms_merge(p, conf, iou, *a, ws, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS)
    torch.cuda.synchronize()
    K.nms_styled(p, conf, iou, *b, ws, style=_lib.NMS_MERGE, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS)
    torch.cuda.synchronize()
    assert torch.equal(a[2], b[2]) and int(a[2].min()) > 0
    for i, n in enumerate(a[2].tolist()):
        assert torch.equal(a[0][i, :n].view(torch.int32), b[0][i, :n].view(torch.int32)) and torch.equal(a[1][i, :n], b[1][i, :n])
    odets, okept = onms.non_max_suppression(pred.copy(), conf, iou)
    for i, n in enumerate(a[2].tolist()):
        assert np.array_equal(b[0][i, :n].cpu().numpy(), odets[i]) and np.array_equal(b[1][i, :n].cpu().numpy(), okept[i])
    for bad in (-1, 4):
        with pytest.raises(RuntimeError, match="unknown style"):
            K.nms_styled(p, conf, iou, *b, ws, style=bad, min_wh=MIN_WH, max_per_class=MAX_PER_CLASS)
