"""Shared by the loss tests (test_loss_cpu.py, test_loss_gpu.py) and tests/golden/make_golden_loss.py:

  * a numpy restatement of reference build_targets / compute_loss (utils/utils.py:99-197): the target assignment fp32 operation for
    fp32 operation in the reference's order (so indices and txy are THE answer in every bit), the loss terms and their sums in
    float64 from the fp32 inputs, each layer's contribution formed like the reference's (mean rounded to fp32, times the fp32 gain,
    accumulated in fp32);
  * the seeded input generator and the case table of tests/golden/loss.npz;
  * the conditions every generated input must satisfy, and the comparison helpers with the tolerances.

Tolerances (derivation: DESIGN.md 3.6a).  twh: the division is the same IEEE operation on both sides, logf is within 1 ulp on either
side: 2 ulp = 2.4e-7 relative; the bar is rtol 1e-6 / atol 1e-7.  Loss items: every summed term is non-negative and O(1) on these
inputs (logit scale 2), a term costs a handful of fp32 transcendental roundings (<= ~8 ulp = 5e-7 relative), float64 sums add
nothing, and the reference's own fp32 result is within 1.3e-7 of an exact evaluation: 5e-6 relative on every non-zero item; an item
the other side reports as exactly 0.0 must be exactly 0.0."""
import types

import numpy as np
import torch

import _cases as C
from pytorch_yolo_amd.utils.synthetic import key_rng

F32 = np.float32
HYPER = dict(iou_thresh=0.2, xy_loss=0.5, wh_loss=0.0625, cls_loss=0.03125, conf_loss=4.0)
HYPER_KEYS = ("iou_thresh", "xy_loss", "wh_loss", "cls_loss", "conf_loss")
TWH_RTOL, TWH_ATOL = 1e-6, 1e-7
LOSS_RTOL = 5e-6
MARGIN = 1e-4                 # distance of every best IoU from iou_thresh, and of the two best anchors of a target from each other
ITEM_NAMES = ("lxy", "lwh", "lconf", "lcls", "loss")

# name -> (anchor groups, n_class, bs, H, W, nt, seed, class_weight).  Seeds: the first of 0, 1, 2, ... at which the conditions
# below hold for the case (make_golden_loss.py asserts them on the reference's own IoUs).
CASES = {
    "A": (C.TINY_ANCHORS, 3, 2, 64, 96, 40, 0, False),      # non-square grids (gi / gj, n_grids order), rows << one workgroup
    "B": (C.TINY_ANCHORS, 1, 1, 64, 64, 12, 0, False),      # the nc == 1 BCE branch
    "C": (C.SPP_ANCHORS, 80, 3, 96, 64, 60, 0, True),       # three layers, weighted CE, 864 rows in the last layer: a tail
    "D": (C.SPP_ANCHORS, 3, 8, 320, 320, 300, 0, False),    # a 38,400-row layer: many workgroups, the partial-sum pass
    "E": (C.TINY_ANCHORS, 3, 2, 64, 96, 0, 0, False),       # case A's p, no targets: only lconf; no launch with an empty grid
}
SWEEP_SEEDS = {"A": (101, 102, 103), "C": (201, 202, 203)}  # candidates of the restatement sweep; see sweep_inputs


def make_layers(anchor_groups, H, W):
    """Per YOLO layer (coarsest grid first, stride 32, 16, 8): dict(anchor_vec float32 [na, 2], nx, ny, na, stride) with anchor_vec
    formed like YOLOLayer.create_grids forms it (yolo_layer.py:102,109: torch's float32 anchors / the Python float stride)."""
    img_size = max(H, W)
    layers = []
    for i, group in enumerate(anchor_groups):
        s = 32 >> i
        ny, nx = H // s, W // s
        stride = img_size / max(nx, ny)
        vec = (torch.tensor(group, dtype=torch.float32) / stride).numpy()
        layers.append(dict(anchor_vec=vec, nx=nx, ny=ny, na=len(group), stride=stride, anchors_px=group))
    return layers


def make_p(seed, layers, bs, nc):
    """The raw head tensors: normals x 2, one keyed generator per layer."""
    return [(key_rng(seed, f"loss_p{i}").standard_normal((bs, L["na"], L["ny"], L["nx"], 5 + nc)) * 2.0).astype(F32)
            for i, L in enumerate(layers)]


def make_targets(seed, layers, bs, nc, nt):
    """[nt, 6] float32: image and class uniform, xy in [0.01, 0.99], wh = a random anchor of a random layer in normalised units times
    exp(U(-0.5, 0.5)) per axis; target 1 copies target 0's image and box (a duplicate cell), target 3's wh is multiplied by (8, 0.1)
    (a shape no anchor fits: rejected on every layer)."""
    rng = key_rng(seed, "loss_targets")
    t = np.zeros((nt, 6), dtype=F32)
    if nt == 0:
        return t
    t[:, 0] = rng.integers(0, bs, nt)
    t[:, 1] = rng.integers(0, nc, nt)
    t[:, 2:4] = rng.uniform(0.01, 0.99, (nt, 2))
    li = rng.integers(0, len(layers), nt)
    for k in range(nt):
        L = layers[int(li[k])]
        a = int(rng.integers(0, L["na"]))
        t[k, 4:6] = L["anchor_vec"][a] / np.asarray([L["nx"], L["ny"]], dtype=F32) * np.exp(rng.uniform(-0.5, 0.5, 2))
    if nt > 1:
        t[1, 0] = t[0, 0]
        t[1, 2:6] = t[0, 2:6]
    if nt > 3:
        t[3, 4:6] *= np.asarray([8.0, 0.1], dtype=F32)
    return t


def case_inputs(name):
    """(layers, p, targets, class_weight or None, nc, bs) of a golden case."""
    groups, nc, bs, H, W, nt, seed, weighted = CASES[name]
    layers = make_layers(groups, H, W)
    p = make_p(seed if name != "E" else CASES["A"][6], layers, bs, nc)
    targets = make_targets(seed, layers, bs, nc, nt)
    cw = np.linspace(0.5, 2.0, nc).astype(F32) if weighted else None
    return layers, p, targets, cw, nc, bs


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def layer_ious(L, targets):
    """wh_iou of every anchor of the layer with every target (utils.py:116-121), float32 [na, nt]."""
    ng = np.asarray([L["nx"], L["ny"]], dtype=F32)
    gwh = targets[:, 4:6] * ng
    out = []
    for aw, ah in L["anchor_vec"]:
        inter = np.minimum(aw, gwh[:, 0]) * np.minimum(ah, gwh[:, 1])
        uni = ((aw * ah + F32(1e-16)) + gwh[:, 0] * gwh[:, 1]) - inter
        out.append(inter / uni)
    return np.stack(out, 0).astype(F32) if out else np.zeros((0, len(targets)), F32)


def build_targets(layers, targets, iou_thresh, bs, nc):
    """Per layer: dict(b, a, gj, gi, tcls int64 [n]; txy, twh float32 [n, 2]; kept: bool [nt]; bad: bool [nt] = kept but outside the
    batch / grid / class range (left out of the arrays))."""
    targets = np.asarray(targets, dtype=F32)
    out = []
    with np.errstate(all="ignore"):
        for L in layers:
            ng = np.asarray([L["nx"], L["ny"]], dtype=F32)
            nt = len(targets)
            if nt == 0:
                z = np.zeros(0, np.int64)
                out.append(dict(b=z, a=z, gj=z, gi=z, tcls=z, txy=np.zeros((0, 2), F32), twh=np.zeros((0, 2), F32),
                                kept=np.zeros(0, bool), bad=np.zeros(0, bool)))
                continue
            iou = layer_ious(L, targets)
            a = np.argmax(iou, 0)                                     # first maximum
            best = iou[a, np.arange(nt)]
            kept = best > F32(iou_thresh)
            gwh = targets[:, 4:6] * ng
            gxy = targets[:, 2:4] * ng
            bf, cf = np.trunc(targets[:, 0]), np.trunc(targets[:, 1])
            gif, gjf = np.trunc(gxy[:, 0]), np.trunc(gxy[:, 1])
            ok = (bf >= 0) & (bf < bs) & (cf >= 0) & (cf < nc) & (gif >= 0) & (gif < L["nx"]) & (gjf >= 0) & (gjf < L["ny"])
            v = kept & ok
            txy = (gxy - np.floor(gxy)).astype(F32)
            twh = np.log(gwh / L["anchor_vec"][a]).astype(F32)
            i64 = lambda x: x[v].astype(np.int64)
            out.append(dict(b=i64(bf), a=a[v].astype(np.int64), gj=i64(gjf), gi=i64(gif), tcls=i64(cf), txy=txy[v], twh=twh[v],
                            kept=kept, bad=kept & ~ok))
    return out


def _bce(x, t):
    return np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))


def compute_loss(p, targets, layers, hyper, nc, class_weight=None):
    """(items float32 [5] = lxy, lwh, lconf, lcls, loss; assignment = build_targets(...); n_bad = targets flagged on some layer)."""
    bs = p[0].shape[0]
    asg = build_targets(layers, targets, hyper["iou_thresh"], bs, nc)
    gain = {k: F32(bs * hyper[k]) for k in ("xy_loss", "wh_loss", "cls_loss", "conf_loss")}
    lxy = lwh = lconf = lcls = F32(0)
    for pi0, A in zip(p, asg):
        pi0 = np.asarray(pi0, dtype=F32)
        tconf = np.zeros(pi0.shape[:4], dtype=np.float64)
        n = len(A["b"])
        if n:
            idx = (A["b"], A["a"], A["gj"], A["gi"])
            tconf[idx] = 1.0
            pi = pi0[idx].astype(np.float64)
            sig = 1.0 / (1.0 + np.exp(-pi[:, 0:2]))
            lxy = F32(lxy + gain["xy_loss"] * F32(np.mean((sig - A["txy"].astype(np.float64)) ** 2)))
            lwh = F32(lwh + gain["wh_loss"] * F32(np.mean((pi[:, 2:4] - A["twh"].astype(np.float64)) ** 2)))
            if nc > 1:
                z = pi[:, 5:]
                m = z.max(1)
                ce = np.log(np.exp(z - m[:, None]).sum(1)) + m - z[np.arange(n), A["tcls"]]
                w = np.ones(n) if class_weight is None else np.asarray(class_weight, dtype=F32).astype(np.float64)[A["tcls"]]
                cls_mean = (w * ce).sum() / w.sum()
            else:
                cls_mean = np.mean(_bce(pi[:, 5], A["tcls"].astype(np.float64)))
            lcls = F32(lcls + gain["cls_loss"] * F32(cls_mean))
        lconf = F32(lconf + gain["conf_loss"] * F32(np.mean(_bce(pi0[..., 4].astype(np.float64), tconf))))
    loss = F32(F32(F32(lxy + lwh) + lconf) + lcls)
    n_bad = int(np.any([A["bad"] for A in asg], 0).sum()) if len(targets) else 0
    return np.asarray([lxy, lwh, lconf, lcls, loss], dtype=F32), asg, n_bad


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------------------
def input_conditions(layers, targets, iou_thresh, bs, nc, ious=None):
    """dict(kept per layer, duplicate cells, rejected on every layer, smallest |best iou - iou_thresh|, smallest gap between the two
    best anchors); ``ious`` = per-layer [na, nt] arrays from another source (the reference's wh_iou) instead of layer_ious."""
    asg = build_targets(layers, targets, iou_thresh, bs, nc)
    nt = len(targets)
    dup, thr_gap, top_gap = 0, np.inf, np.inf
    rejected = np.ones(nt, bool)
    for i, (L, A) in enumerate(zip(layers, asg)):
        iou = (layer_ious(L, targets) if ious is None else np.asarray(ious[i], dtype=F32)).astype(np.float64)
        srt = np.sort(iou, 0)
        thr_gap = min(thr_gap, float(np.abs(srt[-1] - float(F32(iou_thresh))).min()))
        if iou.shape[0] > 1:
            top_gap = min(top_gap, float((srt[-1] - srt[-2]).min()))
        cells = list(zip(A["b"], A["a"], A["gj"], A["gi"]))
        dup += len(cells) - len(set(cells))
        rejected &= ~A["kept"]
    return dict(kept=[len(A["b"]) for A in asg], duplicates=dup, rejected_everywhere=int(rejected.sum()), thr_gap=thr_gap, top_gap=top_gap,
                bad=int(np.any([A["bad"] for A in asg], 0).sum()))


def conditions_hold(cond):
    return (min(cond["kept"]) >= 4 and cond["duplicates"] >= 1 and cond["rejected_everywhere"] >= 1 and cond["thr_gap"] >= MARGIN
            and cond["top_gap"] >= MARGIN and cond["bad"] == 0)


def assert_conditions(cond, tag):
    assert min(cond["kept"]) >= 4, f"{tag}: a layer keeps fewer than 4 targets: {cond['kept']}"
    assert cond["duplicates"] >= 1, f"{tag}: no duplicate cell"
    assert cond["rejected_everywhere"] >= 1, f"{tag}: no target is rejected on every layer"
    assert cond["thr_gap"] >= MARGIN, f"{tag}: a best IoU lies {cond['thr_gap']:.3e} from iou_thresh"
    assert cond["top_gap"] >= MARGIN, f"{tag}: the two best anchors of a target are {cond['top_gap']:.3e} apart"
    assert cond["bad"] == 0, f"{tag}: {cond['bad']} targets are out of range"


def good_targets(seed, layers, bs, nc, nt):
    """(targets, seed used): the generator's targets at the first of seed, seed + 1000, seed + 2000, ... at which the conditions hold
    (the caller asserts them)."""
    for _ in range(50):
        targets = make_targets(seed, layers, bs, nc, nt)
        if conditions_hold(input_conditions(layers, targets, HYPER["iou_thresh"], bs, nc)):
            break
        seed += 1000
    return targets, seed


def sweep_inputs(geometry, k):
    """Input k (0..2) of the restatement sweep at the geometry of case 'A' or 'C': fresh targets (good_targets from
    SWEEP_SEEDS[geometry][k]) and fresh p from the seed that was used."""
    groups, nc, bs, H, W, nt, _, weighted = CASES[geometry]
    layers = make_layers(groups, H, W)
    targets, seed = good_targets(SWEEP_SEEDS[geometry][k], layers, bs, nc, nt)
    cw = np.linspace(0.5, 2.0, nc).astype(F32) if weighted else None
    return layers, make_p(seed, layers, bs, nc), targets, cw, nc, bs, seed


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
def assert_assignment(got, want, tag, txy_exact=True):
    """got / want: per-layer dicts with b, a, gj, gi, tcls, txy, twh (numpy).  Returns the largest relative twh difference."""
    worst = 0.0
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("b", "a", "gj", "gi", "tcls"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(w[k])), f"{tag} layer {i}: {k} differs"
        gt, wt = np.asarray(g["txy"], dtype=F32), np.asarray(w["txy"], dtype=F32)
        assert gt.shape == wt.shape == (len(w["b"]), 2), f"{tag} layer {i}: txy shape"
        if txy_exact:
            assert np.array_equal(gt.view(np.int32), wt.view(np.int32)), f"{tag} layer {i}: txy is not bit-equal"
        else:
            assert np.array_equal(gt, wt), f"{tag} layer {i}: txy differs"
        gw, ww = np.asarray(g["twh"], dtype=F32), np.asarray(w["twh"], dtype=F32)
        assert gw.shape == ww.shape
        assert np.allclose(gw, ww, rtol=TWH_RTOL, atol=TWH_ATOL), f"{tag} layer {i}: twh differs by {np.abs(gw - ww).max():.3e}"
        if gw.size:
            worst = max(worst, float((np.abs(gw.astype(np.float64) - ww) / np.maximum(np.abs(ww), 1e-3)).max()))
    return worst


def assert_items(got, want, tag):
    """Five loss items within LOSS_RTOL where ``want`` is non-zero, exactly 0.0 where it is 0.0.  Prints and returns the relative
    differences."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == (5,), tag
    rel = np.where(want != 0, np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0), 0.0)
    print(f"[loss] {tag}: " + ", ".join(f"{n} {g:.7g} vs {w:.7g} (rel {r:.2e})" for n, g, w, r in zip(ITEM_NAMES, got, want, rel)))
    for n, g, w, r in zip(ITEM_NAMES, got, want, rel):
        if w == 0.0:
            assert g == 0.0, f"{tag}: {n} is {g!r} where the other side is exactly 0.0"
        else:
            assert np.isfinite(g) and r <= LOSS_RTOL, f"{tag}: {n} = {g!r} vs {w!r}: relative difference {r:.3e} > {LOSS_RTOL:.0e}"
    return rel


def namespace_model(layers, nc, hyper=HYPER, device=None):
    """A plain namespace with what compute_loss / build_targets read from a model: hyper_params, n_class and yolo_layers carrying
    anchor_vec, n_grids, n_classes (tensors on ``device``)."""
    ys = [types.SimpleNamespace(anchor_vec=torch.from_numpy(L["anchor_vec"].copy()).to(device or "cpu"),
                                n_grids=torch.tensor((L["nx"], L["ny"]), dtype=torch.float32, device=device or "cpu"), n_classes=nc)
          for L in layers]
    return types.SimpleNamespace(hyper_params=None if hyper is None else dict(hyper), n_class=nc, yolo_layers=ys)
