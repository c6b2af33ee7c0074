"""Restatement of the training ops of MobileNetV2's inverted residual (csrc/dw_train.hip, the clamp entries of
csrc/batchnorm.hip; include/yolo_hip.h) in numpy, and the cases.

Maps are NHWC numpy arrays, the depthwise weight is [c, 3, 3] (the parameter without its singleton).  With ``rounding`` every operation
is the kernels': float32 operations one at a time (numpy rounds each on its own, as the library built without contraction does), float64
sums, bf16 roundings through torch's RNE cast.  With ``rounding=False`` every value stays float64: the form that has to equal torch's
float64 autograd.

    clamp        a = f32(z) scale + shift; y = bf16(min(max(a, lo), hi)); slope = (a > lo and a < hi) ? 1 : 0 (torch's hardtanh_backward:
                 zero AT both bounds); ga = f32(dy) slope; from there tests/_bn.py (xh, B, G, c1, c2, g)
    depthwise    z[n, oh, ow] = bf16(chain over the taps (kh, kw) in row-major order of fmaf(f32(x[n, s oh + kh - 1, s ow + kw - 1]),
                 w[kh, kw], acc)), acc = 0 first; a tap outside the map adds nothing
    data         dx[n, ih, iw] = bf16(the same chain over the taps whose oh = (ih + 1 - kh) / s, ow = (iw + 1 - kw) / s are integral and
                 inside the map, of fmaf(f32(g[n, oh, ow]), w[kh, kw], acc))
    weight       dw[ch, kh, kw] = f32(sum over (n, oh, ow) of f32(g) f32(x tap)): exact fp32 products, a float64 sum
With w holding bf16 values every product of the two chains is exact in fp32, so fmaf(a, b, acc) is numpy's float32 acc + a * b.
Bound of the weight gradient (tests/_bn.py's): |dw - S| <= 2^-24 |S| + T 2^-53 A, T terms, A the float64 sum of |terms|.
"""
import re

import numpy as np
import torch

import _bn as N

F32, F64 = np.float32, np.float64
RELU6 = (0.0, 6.0)

# (n, h, w, c, stride) of the kernel tests: each the smallest shape of one path
CASES = [
    (2, 5, 7, 8, 1),           # odd map, one chunk
    (2, 6, 8, 16, 2),          # even map at stride 2: the last row and column of x meet only the taps 0 and 1
    (2, 7, 9, 24, 2),          # odd map at stride 2, three chunks: 85 pixel slots, one idle thread a kernel row
    (1, 1, 1, 8, 1),           # one pixel: only the centre tap is in bounds
    (1, 2, 1, 8, 2),           # two rows, one column, one output pixel
    (1, 3, 40, 136, 1),        # 17 chunks: 15 pixel slots, 8 passes in 3 splits, the last pass ragged
    (2, 100, 100, 16, 1),      # the weight gradient splits: 157 passes, one a split, the last of 32 pixels
    (2, 100, 100, 16, 2),      # 40 passes, one a split
]
SPLIT_CASES = (6, 7)
CU_SHARES = (8, 64)            # yolo_set_launch_cus values the split cases also run under
# what yolo_dwconv3x3_bwd_weight_pick / _workspace_bytes say for the cases at the default 256 compute units
PICKS = [
    ("dw_wgrad<3x256x1,s1> grid 1x1 passes 1 last 1", 576),
    ("dw_wgrad<3x128x2,s2> grid 1x1 passes 1 last 1", 1152),
    ("dw_wgrad<3x85x3,s2> grid 1x1 passes 1 last 1", 1728),
    ("dw_wgrad<3x256x1,s1> grid 1x1 passes 1 last 1", 576),
    ("dw_wgrad<3x256x1,s2> grid 1x1 passes 1 last 1", 576),
    ("dw_wgrad<3x15x17,s1> grid 3x1 passes 3 last 2", 29376),
    ("dw_wgrad<3x128x2,s1> grid 157x1 passes 1 last 1", 180864),
    ("dw_wgrad<3x128x2,s2> grid 40x1 passes 1 last 1", 46080),
]
SPLIT_PICKS = {(6, 8): "dw_wgrad<3x128x2,s1> grid 8x1 passes 20 last 17", (6, 64): "dw_wgrad<3x128x2,s1> grid 53x1 passes 3 last 1",
               (7, 8): "dw_wgrad<3x128x2,s2> grid 8x1 passes 5 last 5", (7, 64): "dw_wgrad<3x128x2,s2> grid 40x1 passes 1 last 1"}
# (n, h, w, c, stride) of the float64 comparisons with autograd: both strides on even and odd maps, a 1x1 and a 2x1 map
SMALL_CASES = [(2, 5, 7, 8, 1), (2, 6, 8, 8, 1), (2, 5, 7, 8, 2), (2, 6, 8, 16, 2), (2, 1, 1, 8, 1), (2, 2, 1, 8, 2), (2, 2, 1, 8, 1)]


def case_id(c):
    return "%dx%dx%d_c%d_s%d" % c


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def parse_pick(s):
    m = re.fullmatch(r"dw_wgrad<3x(\d+)x(\d+),s(\d)> grid (\d+)x(\d+) passes (\d+) last (\d+)", s)
    assert m, s
    return dict(zip(("rows", "width", "stride", "splits", "tiles", "passes", "last"), map(int, m.groups())))


def split_ranges(m_out, pick):
    """[(first output pixel, end)] of the pixel splits of a pick on m_out output pixels."""
    p = parse_pick(pick)
    step = p["rows"] * p["passes"]
    return [(s * step, min(m_out, (s + 1) * step)) for s in range(p["splits"])]


bf16 = N.bf16


def _ft(rounding):
    return F32 if rounding else F64


# ---- the clamp ------------------------------------------------------------------------------------------------------------------------
def clamp_forward(z, saved, lo=0.0, hi=6.0, rounding=True):
    ft = _ft(rounding)
    y = np.minimum(np.maximum(N.pre_act(z, saved, rounding), ft(lo)), ft(hi))
    return bf16(y) if rounding else y


def clamp_terms(dy, z, saved, lo=0.0, hi=6.0, rounding=True, inject=None):
    """tests/_bn.py's backward_terms with the clamp's slope.  inject="hi": the slope at a == hi taken as 1 (the fault the tests must see)."""
    ft = _ft(rounding)
    a = N.pre_act(z, saved, rounding)
    inside = (a > ft(lo)) & ((a <= ft(hi)) if inject == "hi" else (a < ft(hi)))
    ga = np.asarray(dy).astype(ft) * np.where(inside, ft(1), ft(0))
    xh = (np.asarray(z).astype(ft) - saved[0]) * saved[1]
    t = ga * xh
    return dict(ga=ga, xh=xh, B=ga.astype(F64).sum(0), G=t.astype(F64).sum(0), Ba=np.abs(ga).astype(F64).sum(0),
                Ga=np.abs(t).astype(F64).sum(0), clamped=float((~inside).mean()))


# ---- the depthwise conv -----------------------------------------------------------------------------------------------------------------
def _tap(p, kh, kw, stride, ho, wo):
    """The view of the padded map ``p`` [n, h + 2, w + 2, c] that tap (kh, kw) pairs with the output map."""
    return p[:, kh:kh + stride * (ho - 1) + 1:stride, kw:kw + stride * (wo - 1) + 1:stride]


def _inside(shape, stride):
    """1.0 where a pixel of the padded map is inside the map, as float64 [n, h + 2, w + 2, 1]."""
    n, h, w, _ = shape
    m = np.zeros((n, h + 2, w + 2, 1))
    m[:, 1:-1, 1:-1] = 1.0
    return m


def dw_forward(x, w, stride, rounding=True):
    """z [n, ho, wo, c]: the chain in tap order, then one rounding to bf16."""
    ft = _ft(rounding)
    x, w = np.asarray(x).astype(ft), np.asarray(w).astype(ft)
    n, h, wd, c = x.shape
    ho, wo = out_hw(h, wd, stride)
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    ok = _inside(x.shape, stride)
    acc = np.zeros((n, ho, wo, c), dtype=ft)
    for kh in range(3):
        for kw in range(3):
            t, m = _tap(p, kh, kw, stride, ho, wo), _tap(ok, kh, kw, stride, ho, wo) > 0
            acc = np.where(m, acc + t * w[:, kh, kw], acc)          # a tap outside the map adds nothing (not even + 0)
    return bf16(acc) if rounding else acc


def dw_bwd_data(g, w, shape, stride, rounding=True, inject=None):
    """dx [n, h, w, c] of the map ``shape``.  inject="parity": at stride 2 the taps are paired with the pixels of the other parity
    (ih = s oh + kh instead of s oh + kh - 1), the fault the tests must see."""
    ft = _ft(rounding)
    g, w = np.asarray(g).astype(ft), np.asarray(w).astype(ft)
    n, h, wd, c = shape
    ho, wo = out_hw(h, wd, stride)
    off = 1 if inject == "parity" else 0
    acc = np.zeros((n, h + 3, wd + 3, c), dtype=ft)                  # the padded map (one spare row and column for the injection)
    for kh in range(3):
        for kw in range(3):
            v = acc[:, kh + off:kh + off + stride * (ho - 1) + 1:stride, kw + off:kw + off + stride * (wo - 1) + 1:stride]
            v += g * w[:, kh, kw]                                    # one term a pixel and tap: the chain's order is the taps' order
    dx = acc[:, 1:h + 1, 1:wd + 1]
    return bf16(dx) if rounding else dx.copy()


def dw_bwd_weight(x, g, stride, rounding=True, drop=None):
    """dict(dw [c, 3, 3], S the float64 sums, A the sums of |terms|, T the in-bounds terms per tap).  drop = (a, b): the output pixels
    [a, b) of the flattened (n, oh, ow) range are left out, as a dropped split's partial would."""
    x, g = np.asarray(x).astype(F64), np.asarray(g).astype(F64)
    n, h, wd, c = x.shape
    ho, wo = out_hw(h, wd, stride)
    if drop is not None:
        keep = np.ones(n * ho * wo)
        keep[drop[0]:drop[1]] = 0.0
        g = g * keep.reshape(n, ho, wo, 1)
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    ok = _inside(x.shape, stride)
    s, a, t = np.zeros((c, 3, 3)), np.zeros((c, 3, 3)), np.zeros((3, 3))
    for kh in range(3):
        for kw in range(3):
            terms = g * _tap(p, kh, kw, stride, ho, wo)
            s[:, kh, kw], a[:, kh, kw] = terms.sum((0, 1, 2)), np.abs(terms).sum((0, 1, 2))
            t[kh, kw] = _tap(ok, kh, kw, stride, ho, wo).sum()
    return dict(dw=s.astype(F32) if rounding else s, S=s, A=a, T=t)


def dw_weight_bound(r):
    return N.bound_sum(r["S"], r["T"][None], r["A"])


def torch_dw_reference(x, w, g, stride):
    """float64 autograd of F.conv2d(groups=c): z, dx, dw as NHWC / [c, 3, 3] numpy arrays."""
    import torch.nn.functional as F
    xt = torch.from_numpy(np.asarray(x, dtype=F64)).permute(0, 3, 1, 2).contiguous().requires_grad_()
    wt = torch.from_numpy(np.asarray(w, dtype=F64)).unsqueeze(1).contiguous().requires_grad_()
    z = F.conv2d(xt, wt, None, stride, 1, 1, wt.shape[0])
    z.backward(torch.from_numpy(np.asarray(g, dtype=F64)).permute(0, 3, 1, 2))
    return z.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy(), wt.grad[:, 0].numpy()


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def integer_operands(case, seed=0):
    """x, g: integers in [-7, 7]; w: integers in [-2, 2], asymmetric under every flip: every product and every sum is exact in fp32 and
    in bf16 (|dx| <= 9 * 14 = 126 < 256)."""
    n, h, wd, c, stride = case
    ho, wo = out_hw(h, wd, stride)
    rng = np.random.default_rng(8000 + seed)
    x = rng.integers(-7, 8, (n, h, wd, c)).astype(F32)
    g = rng.integers(-7, 8, (n, ho, wo, c)).astype(F32)
    w = rng.integers(-2, 3, (c, 3, 3)).astype(F32)
    w[0] = np.array([[1, -2, 0], [2, 1, -1], [-2, 0, 2]], dtype=F32)                        # no flip or transpose maps it to itself
    return x, w, g


def random_operands(case, seed=0):
    """x, g ~ N(0, 1) rounded to bf16, w ~ N(0, 1/9) rounded to bf16 (what the ops hand to the kernels); float32 arrays."""
    n, h, wd, c, stride = case
    ho, wo = out_hw(h, wd, stride)
    rng = np.random.default_rng(9000 + seed)
    x = bf16(rng.standard_normal((n, h, wd, c)).astype(F32))
    g = bf16(rng.standard_normal((n, ho, wo, c)).astype(F32))
    w = bf16((rng.standard_normal((c, 3, 3)) / 3.0).astype(F32))
    return x, w, g


def clamp_edge_operands(case, lo=0.0, hi=6.0, seed=0):
    """Operands of a BN case (tests/_bn.py CASES) on which a = z + shift is an integer that hits lo, hi and the values beside them: z
    integers in [-4, 4], saved = (mean 0, invstd 1, scale 1, integer shifts in [1, 4]), dy integers in [-3, 3].  Every sum is exact."""
    m, c = N.rows_of(case), case[3]
    assert m >= 6
    rng = np.random.default_rng(9500 + seed)
    z = rng.integers(-4, 5, (m, c)).astype(F32)
    shift = rng.integers(1, 5, c).astype(F32)
    for row, a in enumerate((lo, hi, hi + 1, lo - 1, lo + 1, hi - 1)):    # every channel holds a == lo, a == hi and the values beside them
        z[row] = a - shift
    dy = rng.integers(-3, 4, (m, c)).astype(F32)
    dy[dy == 0] = 1.0
    saved = np.stack([np.zeros(c, F32), np.ones(c, F32), np.ones(c, F32), shift])
    return z, dy, saved


# ---- the ops in float64 (rounding off) or with the device's rounding points, forward and backward, on NHWC arrays -------------------------
def _rows(a):
    return a.reshape(-1, a.shape[-1])


def bn_forward(z, gamma, beta, act, rm=None, rv=None, rounding=True):
    """Batch statistics and the activation (a (lo, hi) clamp or "none") of the NHWC map z: (y, cache)."""
    st = N.stats(_rows(z), gamma, beta, rm=rm, rv=rv, rounding=rounding)
    y = clamp_forward(_rows(z), st["saved"], act[0], act[1], rounding) if isinstance(act, tuple) else N.forward(_rows(z), st["saved"], "none", rounding)
    return y.reshape(z.shape), dict(z=z, saved=st["saved"], act=act, rm=st["rm"], rv=st["rv"])


def bn_backward(dy, cache, rounding=True, inject=None):
    """(g, dgamma, dbeta) of bn_forward's cache."""
    z, saved, act = _rows(cache["z"]), cache["saved"], cache["act"]
    tr = clamp_terms(_rows(dy), z, saved, act[0], act[1], rounding, inject) if isinstance(act, tuple) else N.backward_terms(_rows(dy), z, saved, "none", rounding)
    c1, c2 = N.centre(tr, z.shape[0], True, rounding)
    ft = _ft(rounding)
    return N.backward_apply(tr, saved, c1, c2, rounding).reshape(cache["z"].shape), tr["G"].astype(ft), tr["B"].astype(ft)


def pw_forward(x, w, rounding=True):
    """1x1 conv of the NHWC x with w [cout, cin] rounded to bf16: z (bf16 values with rounding; the sum itself is float64)."""
    wq = bf16(np.asarray(w, dtype=F32)).astype(F64) if rounding else np.asarray(w, dtype=F64)
    z = np.asarray(x, dtype=F64) @ wq.T
    return bf16(z.astype(F32)) if rounding else z


def pw_backward(x, w, g, rounding=True):
    """(dx, dw) of the 1x1 conv: float64 sums, dx rounded once to bf16, dw to fp32."""
    wq = bf16(np.asarray(w, dtype=F32)).astype(F64) if rounding else np.asarray(w, dtype=F64)
    g64 = np.asarray(g, dtype=F64)
    dx = g64 @ wq
    dw = _rows(g64).T @ _rows(np.asarray(x, dtype=F64))
    return (bf16(dx.astype(F32)), dw.astype(F32)) if rounding else (dx, dw)


def inverted_residual(x, p, stride, residual, dy, rounding=False):
    """An inverted residual from the restated ops, forward and backward: expand (conv_bn_relu6_block, 1x1), depthwise (dw_bn_block),
    project (project_bn_block, with x as the residual where ``residual``).  p: dict(w_exp [hid, cin], w_dw [hid, 3, 3], w_proj [cout,
    hid], g1, b1, g2, b2, g3, b3 and rm1.. rv3).  Returns dict(y, dx, the parameter gradients by name, the running statistics)."""
    z1 = pw_forward(x, p["w_exp"], rounding)
    y1, c1 = bn_forward(z1, p["g1"], p["b1"], RELU6, p["rm1"], p["rv1"], rounding)
    wq = bf16(np.asarray(p["w_dw"], dtype=F32)) if rounding else p["w_dw"]
    z2 = dw_forward(y1, wq, stride, rounding)
    y2, c2 = bn_forward(z2, p["g2"], p["b2"], RELU6, p["rm2"], p["rv2"], rounding)
    z3 = pw_forward(y2, p["w_proj"], rounding)
    y3, c3 = bn_forward(z3, p["g3"], p["b3"], "none", p["rm3"], p["rv3"], rounding)
    if rounding:
        y = bf16(y3 + np.asarray(x, dtype=F32)) if residual else y3                      # y3 = bf16(a): rounded, then the add, rounded once
    else:
        y = y3 + x if residual else y3
    out = dict(y=y)
    g3, out["g3"], out["b3"] = bn_backward(dy, c3, rounding)
    d2, out["w_proj"] = pw_backward(y2, p["w_proj"], g3, rounding)
    g2, out["g2"], out["b2"] = bn_backward(d2, c2, rounding)
    d1 = dw_bwd_data(g2, wq, y1.shape, stride, rounding)
    out["w_dw"] = dw_bwd_weight(y1, g2, stride, rounding)["dw"]
    g1, out["g1"], out["b1"] = bn_backward(d1, c1, rounding)
    dx, out["w_exp"] = pw_backward(x, p["w_exp"], g1, rounding)
    if residual:
        dx = bf16(dx + np.asarray(dy, dtype=F32)) if rounding else dx + dy
    out["dx"] = dx
    for i, c in ((1, c1), (2, c2), (3, c3)):
        out["rm%d" % i], out["rv%d" % i] = c["rm"], c["rv"]
    return out


# ---- dense convs of any kernel size and stride (the first layer), and the chain of the op tests ---------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=F64))).permute(0, 3, 1, 2).contiguous()


def _a(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def dense_forward(x, w, stride=1, rounding=True):
    """conv2d(x, bf16(w), stride, padding=k // 2) of the NHWC x with w [cout, cin, k, k]: float64 sums, z rounded once to bf16."""
    import torch.nn.functional as F
    wq = torch.from_numpy(bf16(np.asarray(w, dtype=F32)).astype(F64) if rounding else np.asarray(w, dtype=F64))
    z = _a(F.conv2d(_t(x), wq, None, stride, wq.shape[-1] // 2))
    return bf16(z.astype(F32)) if rounding else z


def dense_sums(x, w, g, stride=1):
    """The float64 sums of a dense conv's two gradients from the values as given: dict(dw, dx)."""
    wt = torch.from_numpy(np.asarray(w, dtype=F64))
    xt, gt = _t(x), _t(g)
    pad = wt.shape[-1] // 2
    return dict(dw=torch.nn.grad.conv2d_weight(xt, wt.shape, gt, stride, pad).numpy(), dx=_a(torch.nn.grad.conv2d_input(xt.shape, wt, gt, stride, pad)))


def dense_backward(x, w, g, stride=1, rounding=True):
    """(dx, dw) of the dense conv on bf16(w): float64 sums, dx rounded once to bf16, dw to fp32; with the bound quantities
    dict(dw, dw_abs, dw_terms, dx, dx_abs, dx_terms) as the third result."""
    wq = bf16(np.asarray(w, dtype=F32)).astype(F64) if rounding else np.asarray(w, dtype=F64)
    s = dense_sums(x, wq, g, stride)
    a = dense_sums(np.abs(x), np.abs(wq), np.abs(g), stride)
    t = dense_sums(np.ones_like(np.asarray(x, dtype=F64)), np.ones_like(wq), np.ones_like(np.asarray(g, dtype=F64)), stride)
    q = dict(dw=s["dw"], dw_abs=a["dw"], dw_terms=t["dw"], dx=s["dx"], dx_abs=a["dx"], dx_terms=t["dx"])
    if rounding:
        return bf16(s["dx"].astype(F32)), s["dw"].astype(F32), q
    return s["dx"], s["dw"], q


# chain of the op tests (x0 [2, 3, 12, 20], NHWC here):
#   stem   conv_bn_relu6_block 3x3 stride 2, 3 -> 32      e1  conv_bn_relu6_block 1x1 32 -> 192      d1  dw_bn_block stride 2
#   p1     project_bn_block 192 -> 24                     e2  conv_bn_relu6_block 1x1 24 -> 144      d2  dw_bn_block stride 1
#   p2     project_bn_block 144 -> 24 with p1's output as the residual        head  conv_block 1x1 24 -> 21, act none, float32; loss = sum(h R)
CHAIN_X = (2, 12, 20, 3)
CHAIN = [("stem", "dense", 3, 32, 3, 2), ("e1", "dense", 32, 192, 1, 1), ("d1", "dw", 192, 192, 3, 2), ("p1", "project", 192, 24, 1, 1),
         ("e2", "dense", 24, 144, 1, 1), ("d2", "dw", 144, 144, 3, 1), ("p2", "project", 144, 24, 1, 1)]
CHAIN_HEAD = (24, 21)


def chain_operands(seed=0):
    """float64 numpy operands: x0 (bf16 values), per layer W (dense [cout, cin, k, k]; depthwise [c, 3, 3]), gamma, beta; Wh, bh, R."""
    rng = np.random.default_rng(9900 + seed)
    ops = dict(x0=bf16(rng.standard_normal(CHAIN_X).astype(F32)).astype(F64), W={}, gamma={}, beta={})
    for name, kind, cin, cout, k, stride in CHAIN:
        shape = (cout, 3, 3) if kind == "dw" else (cout, cin, k, k)
        fan = 9 if kind == "dw" else cin * k * k
        ops["W"][name] = (rng.standard_normal(shape) / fan ** 0.5).astype(F32).astype(F64)
        ops["gamma"][name] = rng.uniform(1.0, 2.0, cout).astype(F32).astype(F64)
        ops["beta"][name] = ((0.0 if kind == "project" else 2.0) + 0.5 * rng.standard_normal(cout)).astype(F32).astype(F64)
    ops["Wh"] = (rng.standard_normal((CHAIN_HEAD[1], CHAIN_HEAD[0], 1, 1)) / CHAIN_HEAD[0] ** 0.5).astype(F32).astype(F64)
    ops["bh"] = (0.5 * rng.standard_normal(CHAIN_HEAD[1])).astype(F32).astype(F64)
    ops["R"] = rng.standard_normal((2, 3, 5, CHAIN_HEAD[1]))
    return ops


def chain_param_names():
    return [f"{what}_{name}" for name, *_ in CHAIN for what in ("W", "gamma", "beta")] + ["Wh", "bh"]


def chain_autograd64(ops):
    """The chain in float64 torch without any rounding: the gradients of chain_param_names() as numpy arrays."""
    import torch.nn.functional as F
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=F64).copy()).requires_grad_()
    W, ga, be = ({n: leaf(v) for n, v in ops[k].items()} for k in ("W", "gamma", "beta"))
    wh, bh = leaf(ops["Wh"]), leaf(ops["bh"])
    x, res = _t(ops["x0"]), None
    for name, kind, cin, cout, k, stride in CHAIN:
        if kind == "dw":
            z = F.conv2d(x, W[name].unsqueeze(1), None, stride, 1, 1, cout)
        else:
            z = F.conv2d(x, W[name], None, stride, k // 2)
        y = F.batch_norm(z, None, None, ga[name], be[name], True, N.MOMENTUM, N.EPS)
        if kind == "project":
            y = y if res is None else res + y
            res = y
        else:
            y = F.hardtanh(y, 0.0, 6.0)
        x = y
    (F.conv2d(x, wh, bh) * _t(ops["R"])).sum().backward()
    out = {f"{what}_{n}": t[n].grad.numpy() for n, *_ in CHAIN for what, t in (("W", W), ("gamma", ga), ("beta", be))}
    out.update(Wh=wh.grad.numpy(), bh=bh.grad.numpy())
    return out


def chain_restated(ops, rounding=True):
    """The chain from this module's functions with every rounding point of the device chain (or none): the same gradients."""
    caches, x, res = [], ops["x0"], None
    for name, kind, cin, cout, k, stride in CHAIN:
        w = ops["W"][name]
        if kind == "dw":
            wq = bf16(w.astype(F32)) if rounding else w
            z = dw_forward(x, wq, stride, rounding)
        else:
            z = dense_forward(x, w, stride, rounding)
        y, c = bn_forward(z, ops["gamma"][name], ops["beta"][name], "none" if kind == "project" else RELU6, rounding=rounding)
        if kind == "project":
            if res is not None:
                y = bf16(y + res) if rounding else y + res                                # y = bf16(a) here: rounded before the add
            c["res"] = res is not None
            res = y
        caches.append((x, c))
        x = y
    r = bf16(np.asarray(ops["R"], dtype=F32)) if rounding else ops["R"]        # the head's g = bf16(dy)
    dy, dwh, _ = dense_backward(x, ops["Wh"], r, 1, rounding)
    out = dict(Wh=dwh, bh=np.asarray(r, dtype=F64).sum((0, 1, 2)).astype(_ft(rounding)))
    pending = None                                                       # the residual's gradient on its way to p1's output
    for (name, kind, cin, cout, k, stride), (xin, c) in zip(reversed(CHAIN), reversed(caches)):
        if pending is not None and name == "p1":
            dy = bf16(dy + pending) if rounding else dy + pending
            pending = None
        g, out["gamma_" + name], out["beta_" + name] = bn_backward(dy, c, rounding)
        if kind == "project" and c["res"]:
            pending = dy
        if kind == "dw":
            wq = bf16(ops["W"][name].astype(F32)) if rounding else ops["W"][name]
            out["W_" + name] = dw_bwd_weight(xin, g, stride, rounding)["dw"]
            dy = dw_bwd_data(g, wq, xin.shape, stride, rounding)
        else:
            dy, out["W_" + name], _ = dense_backward(xin, ops["W"][name], g, stride, rounding)
    return {k_: np.asarray(v, dtype=F64) for k_, v in out.items()}


def rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=F64) - want) / np.linalg.norm(want))
