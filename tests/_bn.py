"""Restatement of the batch norm of conv_bn_block (csrc/batchnorm.hip; include/yolo_hip.h) in numpy, and the cases.

z is [M, C] (M = n h w rows, C channels).  With ``rounding`` every operation is the kernels': float64 sums, the listed float64
operations, everything else one float32 operation at a time (numpy rounds each float32 operation on its own, as the library built
without contraction does).  With ``rounding=False`` every value stays float64 and eps, momentum are taken as given: the form that has to
equal torch.nn.functional.batch_norm + leaky_relu under float64 autograd.

    statistics   S1 = sum z, S2 = sum z z (float64); mean64 = S1 / M; var64 = max(S2 / M - mean64 mean64, 0); mean = f32(mean64);
                 var = f32(var64); invstd = f32(1 / sqrt(var64 + (double)eps)); scale = gamma invstd; shift = beta - mean scale;
                 rm <- rm (1 - m) + m mean; rv <- rv (1 - m) + m f32(var64 M / (M - 1))
    forward      a = f32(z) scale + shift; y = bf16(a > 0 ? a : 0.1f a)
    backward     slope = a > 0 ? 1 : 0.1f; ga = f32(dy) slope; xh = (f32(z) - mean) invstd; B = sum ga, G = sum ga xh (float64 sums of
                 fp32 terms); dbeta = f32(B), dgamma = f32(G); c1 = f32(B / M), c2 = f32(G / M) (running statistics: 0);
                 g = bf16(scale ((ga - c1) - xh c2))
Bounds (T terms, S the float64 value, A the float64 sum of |terms|; 2^-24 is half an fp32 ulp, 2^-53 half a float64 one, and a sum of T
terms in any order is within (T - 1) 2^-53 A of S):
    |mean - S| <= 2^-24 |S| + T 2^-53 A / M       |var - S| likewise with the terms z z       |dgamma - S|, |dbeta - S| <= 2^-24 |S| + T 2^-53 A
"""
import re

import numpy as np
import torch

F32, F64 = np.float32, np.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53

# (n, h, w, C): each the smallest shape of one path
CASES = [
    (1, 3, 5, 8),          # one chunk column, fewer rows than one pass
    (2, 8, 16, 32),
    (2, 7, 9, 136),        # 17 chunk columns: 15 rows a pass, one idle thread, ragged passes, two splits
    (1, 5, 5, 1024),       # 2 rows per pass, three splits
    (2, 3, 3, 2056),       # two column tiles, the second one chunk wide
    (2, 100, 100, 16),     # 157 passes in 32 splits, the last of two passes and the very last pass of 32 rows
]
SPLIT_CASE = 5
CU_SHARES = (8, 64)        # yolo_set_launch_cus values the split case also runs under: 8 splits and 32
# what yolo_bn_pick / yolo_bn_workspace_bytes say for the cases at the default 256 compute units
PICKS = [
    ("bn_reduce<256x1> grid 1x1 passes 1 last 1", 192),
    ("bn_reduce<64x4> grid 1x1 passes 4 last 4", 768),
    ("bn_reduce<15x17> grid 2x1 passes 5 last 4", 5440),
    ("bn_reduce<2x128> grid 3x1 passes 5 last 3", 57344),
    ("bn_reduce<1x256> grid 4x2 passes 5 last 3", 148032),
    ("bn_reduce<128x2> grid 32x1 passes 5 last 2", 8320),
]
SPLIT_PICKS = {8: "bn_reduce<128x2> grid 8x1 passes 20 last 17", 64: "bn_reduce<128x2> grid 32x1 passes 5 last 2"}
EPS, MOMENTUM = 1e-5, 0.1


def case_id(c):
    return "%dx%dx%d_c%d" % c


def rows_of(c):
    return c[0] * c[1] * c[2]


def parse_pick(s):
    """dict(rows, width, splits, tiles, passes, last) of a yolo_bn_pick string."""
    m = re.fullmatch(r"bn_reduce<(\d+)x(\d+)> grid (\d+)x(\d+) passes (\d+) last (\d+)", s)
    assert m, s
    return dict(zip(("rows", "width", "splits", "tiles", "passes", "last"), map(int, m.groups())))


def split_ranges(m, pick):
    """[(first row, end row)] of the row splits of a pick on m rows."""
    p = parse_pick(pick)
    step = p["rows"] * p["passes"]
    return [(s * step, min(m, (s + 1) * step)) for s in range(p["splits"])]


def bf16(a):
    """RNE to bf16 of a float32 array, as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).to(torch.float32).numpy()


def _ft(rounding):
    return F32 if rounding else F64


def stats(z, gamma, beta, eps=EPS, momentum=MOMENTUM, rm=None, rv=None, rounding=True, drop=None):
    """Training statistics of z [M, C].  drop = (a, b): the rows [a, b) are left out of both sums (M stays), as a dropped row or a
    dropped split's partial would.  Returns dict(mean, var, invstd, scale, shift, saved [4, C], rm, rv, and the bound quantities
    s1, a1, s2 (= a2), mean64, var64)."""
    ft = _ft(rounding)
    z = np.asarray(z, dtype=F64)
    m = z.shape[0]
    keep = z
    if drop is not None:
        keep = np.concatenate([z[:drop[0]], z[drop[1]:]], 0)
    s1, s2 = keep.sum(0), (keep * keep).sum(0)
    mean64 = s1 / m
    var64 = np.maximum(s2 / m - mean64 * mean64, 0.0)
    mean, var = mean64.astype(ft), var64.astype(ft)
    eps64 = float(F32(eps)) if rounding else float(eps)
    invstd = (1.0 / np.sqrt(var64 + eps64)).astype(ft)
    scale = np.asarray(gamma).astype(ft) * invstd
    shift = np.asarray(beta).astype(ft) - mean * scale
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, saved=np.stack([mean, invstd, scale, shift]),
               s1=s1, a1=np.abs(keep).sum(0), s2=s2, mean64=mean64, var64=var64, rm=None, rv=None)
    mom = ft(momentum)
    if rm is not None:
        out["rm"] = np.asarray(rm).astype(ft) * (ft(1) - mom) + mom * mean
    if rv is not None:
        out["rv"] = np.asarray(rv).astype(ft) * (ft(1) - mom) + mom * (var64 * float(m) / (float(m) - 1.0)).astype(ft)
    return out


def eval_saved(gamma, beta, rm, rv, eps=EPS, rounding=True):
    """saved [4, C] from the running statistics."""
    ft = _ft(rounding)
    eps64 = float(F32(eps)) if rounding else float(eps)
    mean = np.asarray(rm).astype(ft)
    invstd = (1.0 / np.sqrt(np.asarray(rv).astype(ft).astype(F64) + eps64)).astype(ft)
    scale = np.asarray(gamma).astype(ft) * invstd
    return np.stack([mean, invstd, scale, np.asarray(beta).astype(ft) - mean * scale])


def pre_act(z, saved, rounding=True):
    """a = f32(z) scale + shift."""
    ft = _ft(rounding)
    return np.asarray(z).astype(ft) * saved[2] + saved[3]


def forward(z, saved, act="leaky", rounding=True):
    """y (float32 holding bf16 values; float64 and unrounded with rounding=False)."""
    ft = _ft(rounding)
    a = pre_act(z, saved, rounding)
    y = np.where(a > 0, a, ft(0.1) * a) if act == "leaky" else a
    return bf16(y) if rounding else y


def backward_terms(dy, z, saved, act="leaky", rounding=True):
    """ga, xh and the two reductions: dict(ga, xh, B, G float64 sums, Ba, Ga sums of |terms|)."""
    ft = _ft(rounding)
    a = pre_act(z, saved, rounding)
    slope = np.where(a > 0, ft(1), ft(0.1)) if act == "leaky" else ft(1)
    ga = np.asarray(dy).astype(ft) * slope
    xh = (np.asarray(z).astype(ft) - saved[0]) * saved[1]
    t = ga * xh
    return dict(ga=ga, xh=xh, B=ga.astype(F64).sum(0), G=t.astype(F64).sum(0), Ba=np.abs(ga).astype(F64).sum(0),
                Ga=np.abs(t).astype(F64).sum(0), nonpositive=float((a <= 0).mean()))


def centre(terms, m, batch_stats, rounding=True):
    """c1, c2 of the float64 sums."""
    ft = _ft(rounding)
    if not batch_stats:
        return np.zeros_like(terms["B"], dtype=ft), np.zeros_like(terms["G"], dtype=ft)
    return (terms["B"] / float(m)).astype(ft), (terms["G"] / float(m)).astype(ft)


def backward_apply(terms, saved, c1, c2, rounding=True):
    """g = bf16(scale ((ga - c1) - xh c2))."""
    g = saved[2] * ((terms["ga"] - c1) - terms["xh"] * c2)
    return bf16(g) if rounding else g


def bound_mean(s, terms, abs_sum, m):
    return U24 * np.abs(s) + terms * U53 * abs_sum / m


def bound_sum(s, terms, abs_sum):
    return U24 * np.abs(s) + terms * U53 * abs_sum


def ratio(got, want, bound):
    """Largest |got - want| / bound; an element whose bound is 0 must be met exactly."""
    err = np.abs(np.asarray(got, dtype=F64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def ulps32(a, b):
    """Distance of two positive float32 arrays in units in the last place."""
    return np.abs(np.ascontiguousarray(a, dtype=F32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, dtype=F32).view(np.int32).astype(np.int64))


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _vectors(rng, c):
    gamma = rng.uniform(0.5, 1.5, c).astype(F32)
    beta = (0.5 * rng.standard_normal(c)).astype(F32)
    rm = rng.standard_normal(c).astype(F32)
    rv = rng.uniform(0.5, 2.0, c).astype(F32)
    return gamma, beta, rm, rv


def exact_operands(case, seed=0):
    """z of odd integers in [-7, 7] (float32 [M, C]): S1 and S2 are exact in float64 in any order, every element adds at least 1 to S2,
    and every channel holds at least two distinct values (its variance is not 0).  gamma, beta, rm, rv: random float32."""
    m, c = rows_of(case), case[3]
    rng = np.random.default_rng(4000 + seed)
    z = (2 * rng.integers(-4, 4, (m, c)) + 1).astype(F32)
    z[0], z[1] = 3.0, -5.0                                        # the guard: two distinct values in every channel
    # leaving out a row of value v keeps var where S1 == v (M + 1) / 2: move such a channel's S1 by 2 (the grid of those sums has
    # spacing M + 1 >= 16), so that EVERY single dropped row shows in var of every channel
    hidden = np.isin(2.0 * z.sum(0, dtype=F64) / (m + 1), np.arange(-7.0, 8.0, 2.0))
    z[2, hidden] += np.where(z[2, hidden] == 7.0, -2.0, 2.0)
    assert not np.isin(2.0 * z.sum(0, dtype=F64) / (m + 1), np.arange(-7.0, 8.0, 2.0)).any() and m + 1 >= 16
    assert z.min() >= -7 and z.max() <= 7 and bool((np.abs(z) % 2 == 1).all()) and bool((z.max(0) > z.min(0)).all())
    return (z,) + _vectors(rng, c)


def random_operands(case, dy_dtype=torch.bfloat16, seed=0):
    """z = bf16(offset_c + sigma_c N(0, 1)) with |offset_c| up to 4 sigma_c, so that S2 / M - mean^2 cancels; dy ~ N(0, 1) rounded to
    ``dy_dtype``; float32 arrays.  gamma in [0.5, 1.5], beta ~ N(0, 1/4): a good share of a = z scale + shift is non-positive."""
    m, c = rows_of(case), case[3]
    rng = np.random.default_rng(5000 + seed)
    sigma = rng.uniform(0.5, 2.0, c)
    offset = rng.uniform(-4.0, 4.0, c) * sigma
    z = bf16((offset + sigma * rng.standard_normal((m, c))).astype(F32))
    dy = torch.from_numpy(rng.standard_normal((m, c)).astype(F32)).to(dy_dtype).to(torch.float32).numpy()
    return (z, dy) + _vectors(rng, c)


# ---- float64 torch reference (CPU tests) and the chain of the op tests -----------------------------------------------------------------
def torch_reference(z, dy, gamma, beta, rm, rv, training, act, eps=EPS, momentum=MOMENTUM):
    """F.batch_norm + leaky_relu under float64 autograd on [M, C] (batch_norm's [N, C] form): y, dz, dgamma, dbeta, rm, rv."""
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64).copy())
    zt, gt, bt = t(z).requires_grad_(), t(gamma).requires_grad_(), t(beta).requires_grad_()
    rmt, rvt = t(rm), t(rv)
    y = F.batch_norm(zt, rmt, rvt, gt, bt, training, momentum, eps)
    if act == "leaky":
        y = F.leaky_relu(y, 0.1)
    y.backward(t(dy))
    return dict(y=y.detach().numpy(), dz=zt.grad.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy(), rm=rmt.numpy(), rv=rvt.numpy())


def restated_block(z, dy, gamma, beta, rm, rv, training, act, rounding=True, eps=EPS, momentum=MOMENTUM):
    """The same from the functions above: y, dz (= g), dgamma, dbeta, rm, rv."""
    ft = _ft(rounding)
    if training:
        st = stats(z, gamma, beta, eps, momentum, rm, rv, rounding)
        saved, rm2, rv2 = st["saved"], st["rm"], st["rv"]
    else:
        saved, rm2, rv2 = eval_saved(gamma, beta, rm, rv, eps, rounding), np.asarray(rm), np.asarray(rv)
    tr = backward_terms(dy, z, saved, act, rounding)
    c1, c2 = centre(tr, np.asarray(z).shape[0], training, rounding)
    return dict(y=forward(z, saved, act, rounding), dz=backward_apply(tr, saved, c1, c2, rounding), dgamma=tr["G"].astype(ft),
                dbeta=tr["B"].astype(ft), rm=rm2, rv=rv2, saved=saved, terms=tr, c1=c1, c2=c2)


# chain of the op tests:  c1 = conv_bn_block(x0 [2,16,6,10], 3x3 16 -> 32)   c2 = conv_bn_block(c1, 1x1 32 -> 24)
#                         h = conv_block(c2, 1x1 24 -> 21, act none, float32)    loss = sum(h R)
CHAIN_X = (2, 16, 6, 10)
CHAIN_BN = [(16, 32, 3), (32, 24, 1)]
CHAIN_HEAD = (24, 21, 1)


def chain_operands(seed=0):
    """float64 torch tensors: x0 (bf16 values), W and gamma / beta of the two layers, head Wh and bh, R."""
    gen = torch.Generator().manual_seed(6000 + seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    ops = dict(x0=rn(*CHAIN_X).to(torch.bfloat16).to(torch.float64), W=[], gamma=[], beta=[])
    for cin, cout, k in CHAIN_BN:
        ops["W"].append((rn(cout, cin, k, k) / (cin * k * k) ** 0.5).to(torch.float64))
        ops["gamma"].append((1.0 + 0.25 * rn(cout)).to(torch.float32).to(torch.float64))
        ops["beta"].append((0.5 * rn(cout)).to(torch.float32).to(torch.float64))
    cin, cout, k = CHAIN_HEAD
    ops["Wh"] = (rn(cout, cin, k, k) / cin ** 0.5).to(torch.float64)
    ops["bh"] = (0.5 * rn(cout)).to(torch.float64)
    ops["R"] = rn(CHAIN_X[0], cout, CHAIN_X[2], CHAIN_X[3]).to(torch.float64)
    return ops


CHAIN_PARAMS = ("W1", "gamma1", "beta1", "W2", "gamma2", "beta2", "Wh", "bh")


def chain_autograd64(ops):
    """conv -> batch_norm(training=True) -> leaky_relu twice, then the head, in float64 torch without any rounding: the gradients of
    CHAIN_PARAMS as a dict."""
    import torch.nn.functional as F
    leaf = lambda t: t.clone().requires_grad_()
    W, ga, be = [leaf(t) for t in ops["W"]], [leaf(t) for t in ops["gamma"]], [leaf(t) for t in ops["beta"]]
    wh, bh = leaf(ops["Wh"]), leaf(ops["bh"])
    x = ops["x0"]
    for i, (cin, cout, k) in enumerate(CHAIN_BN):
        x = F.leaky_relu(F.batch_norm(F.conv2d(x, W[i], None, padding=k // 2), None, None, ga[i], be[i], True, MOMENTUM, EPS), 0.1)
    (F.conv2d(x, wh, bh) * ops["R"]).sum().backward()
    return dict(W1=W[0].grad, gamma1=ga[0].grad, beta1=be[0].grad, W2=W[1].grad, gamma2=ga[1].grad, beta2=be[1].grad, Wh=wh.grad, bh=bh.grad)


def _rows(t):
    """NCHW torch tensor -> [M, C] numpy."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _nchw(a, like):
    n, _, h, w = like.shape
    return torch.from_numpy(np.asarray(a, dtype=F64)).reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def chain_restated(ops, rounding=True):
    """The chain from this module's functions and tests/_conv_bwd.py's: float64 sums with every rounding point of the device chain
    (bf16 weights in the products, z, y, g and dx rounded to bf16, the batch norm's float32 operations).  Returns the gradients of
    CHAIN_PARAMS and, per batch-norm layer, dict(x, z, y, dy, block = restated_block's result, conv = grads() of the conv)."""
    import _conv_bwd as B
    layers, x = [], ops["x0"]
    for i, (cin, cout, k) in enumerate(CHAIN_BN):
        z = B.bf16(B.forward(x, ops["W"][i], None, k, "none", rounding), rounding)
        st = stats(_rows(z), ops["gamma"][i].numpy(), ops["beta"][i].numpy(), rounding=rounding)
        y = _nchw(forward(_rows(z), st["saved"], "leaky", rounding), z)
        layers.append(dict(x=x, z=z, y=y, saved=st["saved"]))
        x = y
    cin, cout, k = CHAIN_HEAD
    h = B.forward(x, ops["Wh"], ops["bh"], k, "none", rounding)
    head = B.grads(x, ops["Wh"], ops["R"], h, k, "none", rounding)
    out = dict(Wh=head["dw"], bh=head["db"], layers=layers)
    dy = head["dx"]
    for i in (1, 0):
        lay = layers[i]
        k = CHAIN_BN[i][2]
        tr = backward_terms(_rows(dy), _rows(lay["z"]), lay["saved"], "leaky", rounding)
        c1, c2 = centre(tr, tr["ga"].shape[0], True, rounding)
        g = _nchw(backward_apply(tr, lay["saved"], c1, c2, rounding), lay["z"])
        conv = B.grads(lay["x"], ops["W"][i], g, None, k, "none", rounding)
        ft = _ft(rounding)
        out["W%d" % (i + 1)] = conv["dw"]
        out["gamma%d" % (i + 1)] = torch.from_numpy(tr["G"].astype(ft).astype(F64))
        out["beta%d" % (i + 1)] = torch.from_numpy(tr["B"].astype(ft).astype(F64))
        lay.update(dy=dy, g=g, conv=conv)
        dy = conv["dx"]
    return out
