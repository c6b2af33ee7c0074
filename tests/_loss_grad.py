"""Shared by the loss-gradient tests (test_loss_grad_cpu.py, test_loss_grad_gpu.py) and tests/golden/make_golden_loss_grad.py:

  * a float64 numpy restatement of d loss / d p of reference compute_loss (utils/utils.py:124-157), built on the assignment of
    tests/_loss.py; it returns dense arrays shaped like p;
  * the comparison measure and its bar;
  * the layout of tests/golden/loss_grad.npz.

The measure.  Per layer and per word group - xy (words 0-1), wh (2-3), conf (4), class (5..) -

    err = max |g - g64| / max |g64|        over the elements of the group,

and a group whose g64 is all zero must be all zero in g.  A per-element relative error says nothing here: sigmoid(x) - t cancels, and
the reference's own fp32 autograd is off by up to 5e-4 relative on single elements.  In this measure the reference's fp32 autograd
lies within 7.9e-7 of a float64 evaluation on cases A-E (conf <= 1.2e-7; the figures are stored in the golden file and printed by the
tests).  The bar for the kernels is LOSS_RTOL = 5e-6: an element is a handful of fp32 transcendental roundings of an O(1) quantity,
times a scale both sides share exactly - about 8 ulp -, and the device's expf is not ATen's.

The zero pattern is exact on both sides: an element outside word 4 and outside the assigned cells is +0.0 bit for bit."""
import numpy as np

import _loss as L

F64 = np.float64
GROUPS = (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf", slice(4, 5)), ("class", slice(5, None)))
GRAD_RTOL = L.LOSS_RTOL
FULL_CASES = ("A", "B", "C", "E")      # the golden file holds their gradients whole; of case D the word-4 planes and the target rows


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def loss_grad(p, targets, layers, hyper, nc, class_weight=None, G=1.0):
    """(d (G * loss) / d p as float64 arrays shaped like p, assignment).  The gains are the fp32 values k * h[...] the kernels and the
    reference use; everything else is float64 from the fp32 inputs.  A cell shared by several targets gets the sum of their terms:
    the reference gathers the cell once per target (:143), so its index backward adds."""
    bs = p[0].shape[0]
    asg = L.build_targets(layers, targets, hyper["iou_thresh"], bs, nc)
    gain = {k: float(L.F32(bs * hyper[k])) * float(G) for k in ("xy_loss", "wh_loss", "cls_loss", "conf_loss")}
    grads = []
    for pi0, A in zip(p, asg):
        x = np.asarray(pi0, dtype=L.F32).astype(F64)
        g = np.zeros_like(x)
        tconf = np.zeros(x.shape[:4], dtype=F64)
        n = len(A["b"])
        idx = (A["b"], A["a"], A["gj"], A["gi"])
        if n:
            tconf[idx] = 1.0
        g[..., 4] = gain["conf_loss"] / tconf.size * (_sigmoid(x[..., 4]) - tconf)                 # BCEWithLogits, mean, :154
        if n:
            pi = x[idx]
            d = np.zeros_like(pi)
            s = _sigmoid(pi[:, 0:2])
            d[:, 0:2] = gain["xy_loss"] * (s - A["txy"].astype(F64)) * s * (1.0 - s) / n           # MSE of the sigmoid, :146
            d[:, 2:4] = gain["wh_loss"] * (pi[:, 2:4] - A["twh"].astype(F64)) / n                  # :147
            if nc > 1:                                                                             # CrossEntropyLoss(weight=), :150
                z = pi[:, 5:]
                e = np.exp(z - z.max(1, keepdims=True))
                sm = e / e.sum(1, keepdims=True)
                sm[np.arange(n), A["tcls"]] -= 1.0
                w = np.ones(n) if class_weight is None else np.asarray(class_weight, dtype=L.F32).astype(F64)[A["tcls"]]
                d[:, 5:] = gain["cls_loss"] * w[:, None] * sm / w.sum()
            else:                                                                                  # BCE against the class INDEX, :152
                d[:, 5] = gain["cls_loss"] * (_sigmoid(pi[:, 5]) - A["tcls"].astype(F64)) / n
            np.add.at(g, idx, d)
        grads.append(g)
    return grads, asg


def cell_mask(shape, A):
    """bool [bs, na, ny, nx]: the cells of the assignment A."""
    m = np.zeros(shape[:4], dtype=bool)
    if len(A["b"]):
        m[A["b"], A["a"], A["gj"], A["gi"]] = True
    return m


def group_errors(g, g64):
    """float64 [4]: the measure per word group (xy, wh, conf, class); 0.0 for a group that is all zero on both sides, inf where g64 is
    all zero and g is not."""
    g, g64 = np.asarray(g, dtype=F64), np.asarray(g64, dtype=F64)
    assert g.shape == g64.shape
    out = []
    for _, sl in GROUPS:
        a, b = g[..., sl], g64[..., sl]
        top = float(np.abs(b).max()) if b.size else 0.0
        diff = float(np.abs(a - b).max()) if b.size else 0.0
        out.append(diff / top if top > 0 else (0.0 if diff == 0 else np.inf))
    return np.asarray(out, dtype=F64)


def assert_grads(got, want, tag, ref_err=None):
    """got / want: per-layer arrays.  Every group of every layer within GRAD_RTOL in the measure, every element finite.  Prints the
    errors - beside the reference's own (``ref_err`` [layers, 4]) where given - and returns them as [layers, 4]."""
    assert len(got) == len(want), tag
    errs = np.stack([group_errors(g, w) for g, w in zip(got, want)])
    for i, e in enumerate(errs):
        line = ", ".join(f"{name} {v:.2e}" + (f" (reference {ref_err[i][k]:.2e})" if ref_err is not None else "")
                         for k, ((name, _), v) in enumerate(zip(GROUPS, e)))
        print(f"[loss grad] {tag} layer {i}: {line}")
    for i, (g, e) in enumerate(zip(got, errs)):
        assert np.isfinite(np.asarray(g)).all(), f"{tag} layer {i}: a gradient element is not finite"
        for (name, _), v in zip(GROUPS, e):
            assert v <= GRAD_RTOL, f"{tag} layer {i}: {name} differs by {v:.3e} of the group's largest element > {GRAD_RTOL:.0e}"
    return errs


def assert_structure(g, A, tag):
    """g float32 shaped like p: every element outside word 4 and outside the cells of A is +0.0 bit for bit; word 4 is non-zero in
    every row."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    bits = g.view(np.int32)
    cells = cell_mask(g.shape, A)
    rest = np.ones(g.shape[-1], dtype=bool)
    rest[4] = False
    outside = bits[~cells][:, rest]
    assert not outside.any(), f"{tag}: {int((outside != 0).sum())} elements outside word 4 and the assigned cells are not +0.0"
    assert (g[..., 4] != 0).all(), f"{tag}: word 4 is zero in {int((g[..., 4] == 0).sum())} rows"


def golden_grads(gold, name, p_shapes, asg):
    """The reference's gradients of case ``name`` from tests/golden/loss_grad.npz as dense float32 arrays.  Case D is put together
    from its word-4 planes and the rows of its target cells (everything else was +0.0 in the reference: the capture script asserts it)."""
    out = []
    for i, (shape, A) in enumerate(zip(p_shapes, asg)):
        if name in FULL_CASES:
            g = gold[f"{name}_g{i}"]
        else:
            g = np.zeros(shape, dtype=np.float32)
            g[..., 4] = gold[f"{name}_g{i}_conf"]
            rows = gold[f"{name}_g{i}_rows"]
            assert len(rows) == len(A["b"])
            if len(rows):
                g[A["b"], A["a"], A["gj"], A["gi"]] = rows
        assert g.shape == tuple(shape) and g.dtype == np.float32
        out.append(g)
    return out


def golden_ref_err(gold, name, nl):
    return np.stack([gold[f"{name}_L{i}_referr"] for i in range(nl)])
