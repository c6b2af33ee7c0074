"""Restatements of the ops of a training step of YOLOv3-tiny/SqueezeNet (csrc/fire_train.hip, the ReLU slope of
csrc/conv_bwd.hip, yolo_conv2d_stem_bwd_* of csrc/conv_down_bwd.hip; include/yolo_hip.h), the CPU op table of tests/_train_pool.py
extended by them, the golden-size configuration of the model and its float64 reference.

Convs: NCHW float64 torch tensors, as tests/_conv_bwd.py; the pool: NHWC numpy arrays, as tests/_train_pool.py.  ``rounding=False`` keeps
float64 everywhere (what has to equal torch's float64 autograd).

    relu_forward    y = relu(conv2d(x, bf16(W), stride, padding) + bias) in float64, before the output's own rounding
    relu_upstream   g = bf16_rne(f32(dy) * (y > 0 ? 1 : 0))
    relu_grads      tests/_conv_bwd.grads on that g with act none (g is a bf16 value already: its rounding is the identity)
    stem_grads      dW[co][ci][kh][kw] = sum g[n,co,oh,ow] x[n,ci,2oh+kh,2ow+kw], db = sum g, with A = sum |terms| and T = the term count
    pool3_forward   MaxPool2d(3, 2, ceil_mode=True), pad 0: tap 3i + j of the window at (oy, ox) is (2oy + i, 2ox + j), -inf beyond the map;
                    idx: the tap of the FIRST maximum among the in-bounds taps in row-major order
    pool3_backward  acc = 0; for the windows oy in [ceil((py - 2) / 2), py // 2] and [0, ho), ox likewise, in row-major (oy, ox) order:
                    acc += dy[q] where idx[q] == 3 (py - 2oy) + (px - 2ox); dx = bf16(acc)
    fire_restated   the Fire module from the pieces above with every rounding point of ops.fire_block: the squeeze and the two expand
                    outputs rounded to bf16, g1 | g3 = relu_upstream per half of dy, the two expand data gradients rounded to bf16 each, g_s =
                    bf16((f32(d1) + f32(d3)) * (s > 0))
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import _bn as N
import _conv_bwd as B
import _train as T
import _train_pool as TP

F32, F64 = np.float32, np.float64
TF64 = torch.float64

# ---- the golden-size configuration: tests/_train.py's input size, seeds and target count -----------------------------------------------
CLASS = "YOLOv3TinySqueeze"
CTOR = dict(n_class=2, kernels_divider=4)
FIRE_KEYS = ("squeeze.weight", "squeeze.bias", "expand1x1.weight", "expand1x1.bias", "expand3x3.weight", "expand3x3.bias")


def golden_inputs(model):
    """(x float32 [BS, 3, H, W], targets float32 [N_TARGETS, 6]) of the step; the targets are drawn for the model's own anchors and grids
    (3 x 5 on a 64 x 96 input: the encoder's stride is not 32)."""
    from pytorch_yolo_amd.utils.synthetic import synth_images
    rng = np.random.default_rng(T.TARGET_SEED)
    t = np.zeros((T.N_TARGETS, 6), dtype=F32)
    t[:, 0] = rng.integers(0, T.BS, T.N_TARGETS)
    t[:, 1] = rng.integers(0, model.n_class, T.N_TARGETS)
    t[:, 2:4] = rng.uniform(0.1, 0.9, (T.N_TARGETS, 2))
    t[:, 4:6] = rng.uniform(0.1, 0.6, (T.N_TARGETS, 2))
    return synth_images(T.BS, T.H, T.W, seed=T.IMAGE_SEED), torch.from_numpy(t)


# ---- convs with ReLU, NCHW float64 torch ----------------------------------------------------------------------------------------------------
def relu_forward(x, w, b, rounding=True, stride=1, pad=None):
    k = w.shape[2]
    return F.relu(F.conv2d(x.to(TF64), B.bf16(w, rounding), None if b is None else b.to(TF64), stride=stride, padding=k // 2 if pad is None else pad))


def relu_upstream(dy, y, rounding=True):
    """g (float64).  With rounding: one fp32 multiply by 0 or 1, then RNE to bf16."""
    mask = (y > 0)
    if not rounding:
        return dy.to(TF64) * mask.to(TF64)
    return (dy.to(torch.float32) * mask.to(torch.float32)).to(torch.bfloat16).to(TF64)


def relu_grads(x, w, dy, y, rounding=True):
    """tests/_conv_bwd.grads of the stride-1 conv with ReLU: the same dict (dw, db, dx, dx_sum and the bound quantities), plus g."""
    g = relu_upstream(dy, y, rounding)
    return B.grads(x, w, g, None, w.shape[2], "none", rounding)


def stem_grads(x, w, dy, y, rounding=True, act="relu"):
    """The weight and bias gradient of Conv2d(cin, cout, 3, stride=2, padding=0) and their bound quantities (tests/_conv_bwd.bound_sum)."""
    x = x.to(TF64)
    n, cin = x.shape[:2]
    g = relu_upstream(dy, y, rounding) if act == "relu" else B.upstream(dy, y, act, rounding)
    cout = g.shape[1]
    cols, ones = F.unfold(x, 3, stride=2), F.unfold(torch.ones_like(x), 3, stride=2)          # [n, cin 9, ho wo]
    sums = lambda a, c: torch.einsum("nop,ncp->oc", a.reshape(n, cout, -1), c).reshape(cout, cin, 3, 3)
    return dict(g=g, dw=sums(g, cols), dw_abs=sums(g.abs(), cols.abs()), dw_terms=sums(torch.ones_like(g), ones), db=g.sum((0, 2, 3)),
                db_abs=g.abs().sum((0, 2, 3)), db_terms=torch.full((cout,), float(g.numel() // cout), dtype=TF64))


# ---- the ceil-mode pool, NHWC numpy ------------------------------------------------------------------------------------------------------------
def pool3_out(n):
    return -(-(n - 3) // 2) + 1            # == n // 2 for n >= 2


def pool3_forward(x, tie="first"):
    """(y, idx uint8) of x [n,h,w,c], h and w >= 2.  tie: "first" (the rule) or "last" (the fault injection)."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    ho, wo = pool3_out(h), pool3_out(w)
    assert h >= 2 and w >= 2 and (ho, wo) == (h // 2, w // 2)
    xp = np.full((n, 2 * ho + 1, 2 * wo + 1, c), -np.inf, dtype=x.dtype)
    xp[:, :h, :w] = x
    valid = np.zeros((2 * ho + 1, 2 * wo + 1), dtype=bool)
    valid[:h, :w] = True
    best = np.full((n, ho, wo, c), -np.inf, dtype=x.dtype)
    arg = np.full(best.shape, -1, dtype=np.int64)
    for k in range(9):
        i, j = divmod(k, 3)
        cand, ok = xp[:, i:i + 2 * ho:2, j:j + 2 * wo:2], valid[i:i + 2 * ho:2, j:j + 2 * wo:2][None, :, :, None]
        take = ok & ((arg < 0) | ((cand > best) if tie == "first" else (cand >= best)))
        best, arg = np.where(take, cand, best), np.where(take, k, arg)
    assert arg.min() >= 0
    return best, arg.astype(np.uint8)


def pool3_backward(dy, idx, shape, rounding=True, drop=None):
    """dx of ``shape`` [n,h,w,c].  The up to four windows of a pixel are visited in row-major (oy, ox) order.  drop: the index (0..3) of one
    of the four (earlier | own row) x (earlier | own column) terms that is left out (the fault injection)."""
    ft = F32 if rounding else F64
    dy, idx = np.asarray(dy).astype(ft), np.asarray(idx).astype(np.int64)
    n, h, w, c = shape
    ho, wo = h // 2, w // 2
    acc = np.zeros(shape, dtype=ft)
    py, px = np.arange(h), np.arange(w)
    # the earlier window first: an even pixel row > 0 is tap row 2 of window py / 2 - 1 and tap row 0 of window py / 2 (-1: there is none)
    rows = [np.where((py > 0) & (py % 2 == 0), py // 2 - 1, -1), py // 2]
    cols = [np.where((px > 0) & (px % 2 == 0), px // 2 - 1, -1), px // 2]
    for t, (oy, ox) in enumerate((oy, ox) for oy in rows for ox in cols):
        if t == drop:
            continue
        ok = ((oy >= 0) & (oy < ho))[:, None] & ((ox >= 0) & (ox < wo))[None, :]              # [h, w]; an odd map's last row: py // 2 == ho
        oyc, oxc = np.clip(oy, 0, ho - 1), np.clip(ox, 0, wo - 1)
        me = (3 * (py - 2 * oyc))[:, None] + (px - 2 * oxc)[None, :]
        hit = (idx[:, oyc][:, :, oxc] == me[None, :, :, None]) & ok[None, :, :, None]
        acc = acc + np.where(hit, dy[:, oyc][:, :, oxc], ft(0))
    return N.bf16(acc) if rounding else acc


# ---- the Fire module ----------------------------------------------------------------------------------------------------------------------------
def fire_restated(x, p, dy, rounding=True):
    """Fire forward and backward.  x [n,cin,h,w], p = (squeeze_w, squeeze_b, e1_w, e1_b, e3_w, e3_b), dy [n,e1+e3,h,w]; float64 tensors.
    Returns dict(y, s, r1, r3, rs (the three convs' tests/_conv_bwd.grads dicts), gs, d1, d3)."""
    sw, sb, w1, b1, w3, b3 = p
    s = B.bf16(relu_forward(B.bf16(x, rounding), sw, sb, rounding), rounding)
    y1, y3 = B.bf16(relu_forward(s, w1, b1, rounding), rounding), B.bf16(relu_forward(s, w3, b3, rounding), rounding)
    e1 = w1.shape[0]
    r1 = relu_grads(s, w1, dy[:, :e1], y1, rounding)
    r3 = relu_grads(s, w3, dy[:, e1:], y3, rounding)
    tot = r1["dx"] + r3["dx"]                                              # two bf16 values: the float64 sum is exact
    gs = relu_upstream(tot.to(torch.float32) if rounding else tot, s, rounding)     # (the fp32 add, then the factor, then bf16)
    rs = B.grads(B.bf16(x, rounding), sw, gs, None, 1, "none", rounding)
    return dict(y=torch.cat([y1, y3], 1), s=s, r1=r1, r3=r3, rs=rs, gs=gs)


# ---- the CPU op table -------------------------------------------------------------------------------------------------------------------------
class _Stem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rounding):
        x, w = B.bf16(x.detach(), rounding), w.detach().to(TF64)
        y = B.bf16(relu_forward(x, w, b.detach(), rounding, stride=2, pad=0), rounding)
        ctx.keep = (x, w, y, rounding)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, rounding = ctx.keep
        r = stem_grads(x, w, dy, y, rounding)
        return None, r["dw"], r["db"], None


class _Fire(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sw, sb, w1, b1, w3, b3, rounding):
        ctx.keep = (x.detach(), tuple(t.detach().to(TF64) for t in (sw, sb, w1, b1, w3, b3)), rounding)
        x, p, _ = ctx.keep
        return fire_restated(x, p, torch.zeros((x.shape[0], w1.shape[0] + w3.shape[0]) + tuple(x.shape[2:]), dtype=TF64), rounding)["y"]

    @staticmethod
    def backward(ctx, dy):
        x, p, rounding = ctx.keep
        r = fire_restated(x, p, dy, rounding)
        return (r["rs"]["dx"], r["rs"]["dw"], r["rs"]["db"], r["r1"]["dw"], r["r1"]["db"], r["r3"]["dw"], r["r3"]["db"], None)


class _Pool3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rounding):
        xn = T._nhwc(B.bf16(x, rounding))
        y, ctx.idx = pool3_forward(xn)
        ctx.keep = (xn.shape, rounding)
        return T._nchw(y)

    @staticmethod
    def backward(ctx, dy):
        shape, rounding = ctx.keep
        return T._nchw(pool3_backward(T._nhwc(dy), ctx.idx, shape, rounding)), None


def cpu_ops(rounding):
    """tests/_train_pool.cpu_ops(rounding) plus stem_block, fire_block, max_pool_ceil and concat: the CPU mirror of DEVICE_OPS_FIRE."""
    def stem_block(x, w, b=None, *, act="relu"):
        assert act == "relu" and b is not None
        return _Stem.apply(x, w, b, rounding)

    table = dict(vars(TP.cpu_ops(rounding)))
    table.update(stem_block=stem_block, fire_block=lambda x, *p: _Fire.apply(x, *p, rounding), max_pool_ceil=lambda x: _Pool3.apply(x, rounding),
                 concat=lambda xs: torch.cat(list(xs), 1))
    return SimpleNamespace(**table)


# ---- the float64 reference of the model: oracle.squeezenet's encoder and the head with F.batch_norm(training=True) -------------------------------
def reference_step(sd, x, momentum=0.1, eps=1e-5):
    """The raw head maps [bs, 3 (5 + nc), ny, nx] of YOLOv3TinySqueeze as it trains, by torch float64 autograd.  ``sd``: a dict of float64
    tensors with the model's state_dict keys (the parameters require grad).  Returns (branch1, branch2, stats): stats[prefix] = the batch
    mean and UNBIASED variance of each ConvBlock's conv output, what the running statistics are updated with."""
    from oracle.squeezenet import squeezenet_routes
    route1, route2 = squeezenet_routes(sd, x)
    stats = {}

    def block(prefix, t, k):
        z = F.conv2d(t, sd[prefix + ".sequence.conv.weight"], None, padding=k // 2)
        m = z.numel() // z.shape[1]
        stats[prefix] = (z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False) * m / (m - 1))
        bn = prefix + ".sequence.batch_norm."
        return F.leaky_relu(F.batch_norm(z, None, None, sd[bn + "weight"], sd[bn + "bias"], True, momentum, eps), 0.1)

    def plain(prefix, t):
        return F.conv2d(t, sd[prefix + ".weight"], sd[prefix + ".bias"])
    b1 = block("sequence_branch1_1.branch1_conv1", route2, 1)
    b1 = block("sequence_branch1_2.branch1_conv2", torch.cat([route1, b1], 1), 3)
    b2 = block("sequence_branch2.branch2_conv1", route2, 3)
    return plain("sequence_branch1_2.branch1_conv3", b1), plain("sequence_branch2.branch2_conv2", b2), stats
