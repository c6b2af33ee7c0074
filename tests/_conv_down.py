"""Float64 restatement of the backward of the downsample, ConvBlock(3x3, stride 2, pad 1) (csrc/conv_down_bwd.hip;
include/yolo_hip.h), with its rounding points, and the test cases.  What it shares with the stride-1 backward comes from
tests/_conv_bwd.py (upstream(), bf16(), the bounds, the structured-sign generator) and tests/_bn.py (the batch norm).

For y = act(conv(x, bf16(W), stride 2, pad 1) + bias), ho = (h - 1) // 2 + 1, wo likewise:
    g  = bf16_rne(fp32(dy) * (y > 0 ? 1 : 0.1f)), [n, cout, ho, wo]                                  (_conv_bwd.upstream)
    dW[co][ci][kh][kw] = sum_{n,oh,ow} g[n,co,oh,ow] * x[n,ci,2 oh + kh - 1,2 ow + kw - 1]           taps outside the image add nothing
    db[co] = sum g
    dx[n,ci,ih,iw] = bf16_rne(sum g[n,co,oh,ow] * bf16(W)[co][ci][kh][kw])  over co and the (kh, kw) with ih + 1 - kh = 2 oh,
                     iw + 1 - kw = 2 ow, 0 <= oh < ho, 0 <= ow < wo
dx is computed the way the kernel does it, one parity class of (ih, iw) at a time: a pixel (2 a + p) of a class has, along one axis,
    p = 0: kernel index 1 from output index a         p = 1: kernel index 0 from output index a + 1 (if it exists) and 2 from a
so 1, 2, 2 or 4 taps.  ``rounding=False`` switches every rounding point off (the form that must equal float64 autograd).  Beside each
sum S: A = sum |terms| and T = the number of in-bounds terms, for the bounds of _conv_bwd.py:
    |dW - S| <= 2 T 2^-24 A        |db - S| <= 2 T 2^-24 A        |dx - S| <= 2^-8 |S| + 2 T 2^-24 A
"""
import torch
import torch.nn.functional as F

import _conv_bwd as B

F64 = torch.float64

# (n, h, w, cin, cout, view of x and dx: None or (channels of the buffer, offset)); act is LeakyReLU(0.1) everywhere
CASES = [
    (2, 5, 7, 8, 16, None),          # 1 odd map, unequal classes
    (2, 6, 8, 24, 40, None),         # 2 even map, ragged column tile
    (1, 1, 9, 16, 8, None),          # 3 one-row map: two classes empty
    (3, 2, 2, 8, 8, None),           # 4 ho = wo = 1, image boundaries every pixel
    (2, 7, 10, 16, 136, None),       # 5 128x128 wgrad tile, ragged both ways
    (1, 9, 9, 136, 72, None),        # 6 dgrad N tile ragged, K = 4 x 72
    (4, 32, 32, 16, 24, None),       # 7 1024 output pixels: the split path with partial db
    (2, 6, 8, 24, 40, (48, 16)),     # 8 case 2 with x / dx as the view [16, 40) of a 48-channel buffer
    (2, 6, 6, 32, 64, None),         # 9 Darknet's channel ratio
    (2, 8, 8, 64, 128, None),        # 10 ... and with the 128x128 wgrad tile
]
SPLIT_CASE = 6
CU_SHARES = (8, 64)
ACT = "leaky"
# what yolo_conv2d_down_bwd_pick says for the cases at the default 256 compute units
PICKS = [
    "wgrad<64x128,BK64,tr_b16,s2> grid 1x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<64x128,BK64,tr_b16,s2> grid 2x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<64x128,BK64,tr_b16,s2> grid 2x1 splits 1; dgrad<128x64,BK64,parity> grid 2x1 tiles 0+0+1+1",
    "wgrad<64x128,BK64,tr_b16,s2> grid 1x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<128x128,BK64,tr_b16,s2> grid 2x2 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<128x128,BK64,tr_b16,s2> grid 10x1 splits 1; dgrad<128x128,BK64,parity> grid 4x2 tiles 1+1+1+1",
    "wgrad<64x128,BK64,tr_b16,s2> grid 2x1 splits 2; dgrad<128x64,BK64,parity> grid 32x1 tiles 8+8+8+8",
    "wgrad<64x128,BK64,tr_b16,s2> grid 2x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<64x128,BK64,tr_b16,s2> grid 3x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
    "wgrad<128x128,BK64,tr_b16,s2> grid 5x1 splits 1; dgrad<128x64,BK64,parity> grid 4x1 tiles 1+1+1+1",
]
SPLIT_PICKS = {8: "splits 2", 64: "splits 2"}       # 16 stages: the 8-stage minimum of a split decides, whatever the share
# ... so a larger case, beside the ten, whose split count does follow the compute-unit share: 5120 output pixels are 80 stages on two
# column tiles - ten splits of 8 stages at 256 and at 64 compute units, eight of 10 at 8
CU_CASE = (5, 64, 64, 16, 24, None)
CU_CASE_SPLITS = {256: 10, 64: 10, 8: 8}


def case_id(c):
    n, h, w, cin, cout, view = c
    return f"{n}x{h}x{w}_{cin}to{cout}" + ("_view" if view else "")


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def fwd_desc(case, **over):
    """The FORWARD's stride-2 descriptor of a case (what every down_bwd entry takes); ``over`` replaces conv_desc arguments."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, DT_BF16
    n, h, w, cin, cout, view = case
    total, off = view or (cin, 0)
    kw = dict(n=n, h=h, w=w, cin=cin, in_c_total=total, in_c_offset=off, cout=cout, out_c_total=cout, out_c_offset=0, ksize=3, stride=2,
              act=ACT_LEAKY01, kpad=K.roundup(9 * cin, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_BF16)
    kw.update(over)
    return K.conv_desc(**kw)


def out_desc(case, act=None):
    """The stride-1 descriptor of the OUTPUT map: what yolo_conv2d_bwd_prepare takes to make g."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, DT_BF16
    n, h, w, cin, cout, view = case
    ho, wo = out_hw(h, w)
    return K.conv_desc(n=n, h=ho, w=wo, cin=cout, in_c_total=cout, in_c_offset=0, cout=cout, out_c_total=cout, out_c_offset=0, ksize=1,
                       stride=1, act=ACT_LEAKY01 if act is None else act, kpad=K.roundup(cout, 64), cout_pad=K.roundup(cout, 128),
                       out_dtype=DT_BF16)


def forward(x, w, b, act=ACT, rounding=True):
    """y in float64 (before the output's own rounding): act(conv(x, bf16(W), stride 2, pad 1) + bias)."""
    y = F.conv2d(x.to(F64), B.bf16(w, rounding), None if b is None else b.to(F64), stride=2, padding=1)
    return F.leaky_relu(y, 0.1) if act == "leaky" else y


def _axis_taps(p):
    """[(kernel index, output offset)] of the pixels of parity p along one axis."""
    return [(0, 1), (2, 0)] if p else [(1, 0)]


def _class_sums(g, wb, h, w, ph, pw, tph, tpw):
    """S, A, T of the pixels of class (ph, pw) computed with the taps of class (tph, tpw) (the same class unless a fault is injected):
    [n, cin, class rows, class columns]."""
    n, cout, ho, wo = g.shape
    cin = wb.shape[1]
    hc, wc = (h + 1 - ph) // 2, (w + 1 - pw) // 2
    s, a, t = (torch.zeros((n, cin, hc, wc), dtype=F64) for _ in range(3))
    for kh, dh in _axis_taps(tph):
        for kw, dw in _axis_taps(tpw):
            ha, wa = min(hc, ho - dh), min(wc, wo - dw)         # class rows a whose output row a + dh exists
            if ha <= 0 or wa <= 0:
                continue
            gs = g[:, :, dh:dh + ha, dw:dw + wa]
            s[:, :, :ha, :wa] += torch.einsum("nohw,oc->nchw", gs, wb[:, :, kh, kw])
            a[:, :, :ha, :wa] += torch.einsum("nohw,oc->nchw", gs.abs(), wb[:, :, kh, kw].abs())
            t[:, :, :ha, :wa] += cout
    return s, a, t


def grads(x, w, dy, y, act=ACT, rounding=True, inject=None, g=None):
    """The gradients and their bound quantities.  x [n,cin,h,w], w [cout,cin,3,3], dy and y [n,cout,ho,wo] (any float dtype); ``g``
    given: it is the upstream gradient (the batch norm's), dy / y / act are not looked at.
    inject: ("tap", t) - tap t of dW reads the pixel one column to the right of its own; ("pixels", a, b) - the output pixels [a, b) of
    the flattened (n, ho, wo) range are left out of dW, as a dropped split would; ("parity",) - the classes (odd, even) and (even, odd)
    of dx use each other's taps."""
    x = x.to(F64)
    n, cin, h, wd = x.shape
    if g is None:
        g = B.upstream(dy, y, act, rounding)
    g = g.to(F64)
    cout, ho, wo = g.shape[1:]
    assert (ho, wo) == out_hw(h, wd)
    cols = F.unfold(x, 3, padding=1, stride=2)                          # [n, cin 9, ho wo], rows ordered (ci, kh, kw)
    ones = F.unfold(torch.ones_like(x), 3, padding=1, stride=2)
    if inject and inject[0] == "tap":
        t = inject[1]
        shifted = F.unfold(torch.roll(x, -1, 3), 3, padding=1, stride=2).reshape(n, cin, 9, -1)
        cols = cols.reshape(n, cin, 9, -1).clone()
        cols[:, :, t] = shifted[:, :, t]
        cols = cols.reshape(n, cin * 9, -1)
    gw = g
    if inject and inject[0] == "pixels":
        keep = torch.ones(n * ho * wo, dtype=F64)
        keep[inject[1]:inject[2]] = 0
        gw = g * keep.reshape(n, 1, ho, wo)
    out = dict(g=g)
    out["dw"], out["dw_abs"] = B._dw_sums(gw, cols, cin, 3), B._dw_sums(gw.abs(), cols.abs(), cin, 3)
    out["dw_terms"] = B._dw_sums(torch.ones_like(g), ones, cin, 3)
    out["db"], out["db_abs"] = g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))
    out["db_terms"] = torch.full_like(out["db"], n * ho * wo)
    wb = B.bf16(w, rounding)
    s, a, t = (torch.zeros((n, cin, h, wd), dtype=F64) for _ in range(3))
    for ph in (0, 1):
        for pw in (0, 1):
            tph, tpw = (pw, ph) if inject and inject[0] == "parity" and ph != pw else (ph, pw)
            cs, ca, ct = _class_sums(g, wb, h, wd, ph, pw, tph, tpw)
            s[:, :, ph::2, pw::2], a[:, :, ph::2, pw::2], t[:, :, ph::2, pw::2] = cs, ca, ct
    out["dx_sum"], out["dx_abs"], out["dx_terms"] = s, a, t
    out["dx"] = B.bf16(s, rounding)
    return out


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _as_bwd_case(case):
    n, h, w, cin, cout, view = case
    return (n, h, w, cin, cout, 3, ACT, torch.bfloat16, view, None)


def _crop(dy, case):
    ho, wo = out_hw(case[1], case[2])
    return dy[:, :, :ho, :wo].contiguous()


def exact_operands(case, seed=0):
    """_conv_bwd.exact_operands (integer x, structured signs of w and dy so that the terms of dx over co share a sign and dx grows past
    256), dy cropped to the output map: the structure is per pixel and per channel, so it survives the crop."""
    x, w, b, dy = B.exact_operands(_as_bwd_case(case), seed)
    return x, w, b, _crop(dy, case)


def random_operands(case, seed=0):
    x, w, b, dy = B.random_operands(_as_bwd_case(case), seed)
    return x, w, b, _crop(dy, case)


# The rounding guard of dx binds from _conv_bwd.DX_ROUNDING_FROM_TERMS = 128 terms on.  A pixel has cout, 2 cout or 4 cout terms, so cases
# 1, 3, 4 and 7 (at most 64, 16, 8 and 96 terms) have no such element, and cases 2 and 8 (40 couts) only their (odd, odd) pixels
def exact_conditions(case, seed=0):
    """The float64 witnesses of exactness (every operand and sum an integer, every sum of |terms| below 2^24), the share of y that is
    non-positive, and the share of dx that needs rounding to bf16 among the elements with 128 or more terms (None if there are none)."""
    x, w, b, dy = exact_operands(case, seed)
    y = forward(x, w, b)
    r = grads(x, w, dy, y)
    ints = all(bool((t == t.round()).all()) for t in (x, w, b, dy, r["g"], r["dw"], r["db"], r["dx_sum"]))
    y_pre = F.conv2d(x, w, b, stride=2, padding=1)
    many = r["dx_terms"] >= B.DX_ROUNDING_FROM_TERMS
    rounded = float((B.bf16(r["dx_sum"][many]) != r["dx_sum"][many]).double().mean()) if bool(many.any()) else None
    return dict(integers=ints, largest_abs_sum=float(max(r["dw_abs"].max(), r["db_abs"].max(), r["dx_abs"].max(),
                                                         F.conv2d(x.abs(), w.abs(), b.abs(), stride=2, padding=1).max())),
                y_nonpositive=float((y_pre <= 0).double().mean()), dx_rounded=rounded, dx_terms=int(r["dx_terms"].max()))


# ---- the chain of the op tests ----------------------------------------------------------------------------------------------
#   a = conv_bn_block(x0 [2,8,16,20], 3x3 8 -> 16)      u = down_bn_block(a, 16 -> 32)  [2,32,8,10]
#   r = u + conv_bn_block(conv_bn_block(u, 1x1 32 -> 16), 3x3 16 -> 32)                 (Darknet's residual unit; torch's add)
#   v = down_bn_block(r, 32 -> 64)  [2,64,4,5]          h = conv_block(v, 1x1 64 -> 21, act none, float32)      loss = sum(h R)
CHAIN_X = (2, 8, 16, 20)
CHAIN_BN = [(8, 16, 3, 1), (16, 32, 3, 2), (32, 16, 1, 1), (16, 32, 3, 1), (32, 64, 3, 2)]      # cin, cout, k, stride
CHAIN_HEAD = (64, 21, 1)
CHAIN_PARAMS = tuple(f"{p}{i + 1}" for i in range(5) for p in ("W", "gamma", "beta")) + ("Wh", "bh")


def chain_operands(seed=0):
    gen = torch.Generator().manual_seed(7000 + seed)
    rn = lambda *s: torch.randn(s, generator=gen)
    ops = dict(x0=rn(*CHAIN_X).to(torch.bfloat16).to(F64), W=[], gamma=[], beta=[])
    for cin, cout, k, stride in CHAIN_BN:
        ops["W"].append((rn(cout, cin, k, k) / (cin * k * k) ** 0.5).to(F64))
        ops["gamma"].append((1.0 + 0.25 * rn(cout)).to(torch.float32).to(F64))
        ops["beta"].append((0.5 * rn(cout)).to(torch.float32).to(F64))
    cin, cout, k = CHAIN_HEAD
    ops["Wh"] = (rn(cout, cin, k, k) / cin ** 0.5).to(F64)
    ops["bh"] = (0.5 * rn(cout)).to(F64)
    ops["R"] = rn(CHAIN_X[0], cout, 4, 5).to(F64)
    return ops


def chain_autograd64(ops):
    """The network in float64 torch without any rounding: the gradients of CHAIN_PARAMS as a dict."""
    import _bn as N
    leaf = lambda t: t.clone().requires_grad_()
    W, ga, be = [leaf(t) for t in ops["W"]], [leaf(t) for t in ops["gamma"]], [leaf(t) for t in ops["beta"]]
    wh, bh = leaf(ops["Wh"]), leaf(ops["bh"])

    def layer(i, x):
        cin, cout, k, stride = CHAIN_BN[i]
        z = F.conv2d(x, W[i], None, stride=stride, padding=k // 2)
        return F.leaky_relu(F.batch_norm(z, None, None, ga[i], be[i], True, N.MOMENTUM, N.EPS), 0.1)
    u = layer(1, layer(0, ops["x0"]))
    r = u + layer(3, layer(2, u))
    v = layer(4, r)
    (F.conv2d(v, wh, bh) * ops["R"]).sum().backward()
    out = dict(Wh=wh.grad, bh=bh.grad)
    for i in range(5):
        out[f"W{i + 1}"], out[f"gamma{i + 1}"], out[f"beta{i + 1}"] = W[i].grad, ga[i].grad, be[i].grad
    return out


def conv_grads(i, x, w, g, rounding=True):
    """The conv gradients of chain layer i on the upstream gradient g (the batch norm's): _conv_bwd.grads at stride 1, grads() at 2."""
    cin, cout, k, stride = CHAIN_BN[i]
    if stride == 2:
        return grads(x, w, None, None, "none", rounding, g=g)
    return B.grads(x, w, g, None, k, "none", rounding)


def chain_restated(ops, rounding=True):
    """The same network in float64 with every rounding point of the device chain: bf16 weights in the products; z, y, g, dx rounded to
    bf16; the batch norm's float32 operations (_bn); the residual add and the sum of u's two gradients rounded once to bf16 (torch's
    bf16 kernels add in fp32 and round once).  Returns the gradients of CHAIN_PARAMS."""
    import _bn as N

    def fwd(i, x):
        cin, cout, k, stride = CHAIN_BN[i]
        z64 = forward(x, ops["W"][i], None, "none", rounding) if stride == 2 else B.forward(x, ops["W"][i], None, k, "none", rounding)
        z = B.bf16(z64, rounding)
        st = N.stats(N._rows(z), ops["gamma"][i].numpy(), ops["beta"][i].numpy(), rounding=rounding)
        y = N._nchw(N.forward(N._rows(z), st["saved"], "leaky", rounding), z)
        return dict(x=x, z=z, y=y, saved=st["saved"])

    def bwd(i, lay, dy):
        tr = N.backward_terms(N._rows(dy), N._rows(lay["z"]), lay["saved"], "leaky", rounding)
        c1, c2 = N.centre(tr, tr["ga"].shape[0], True, rounding)
        g = N._nchw(N.backward_apply(tr, lay["saved"], c1, c2, rounding), lay["z"])
        conv = conv_grads(i, lay["x"], ops["W"][i], g, rounding)
        ft = N._ft(rounding)
        out[f"W{i + 1}"] = conv["dw"]
        out[f"gamma{i + 1}"] = torch.from_numpy(tr["G"].astype(ft).astype("float64"))
        out[f"beta{i + 1}"] = torch.from_numpy(tr["B"].astype(ft).astype("float64"))
        return conv["dx"]
    lays = [None] * 5
    lays[0] = fwd(0, ops["x0"])
    lays[1] = fwd(1, lays[0]["y"])
    u = lays[1]["y"]
    lays[2] = fwd(2, u)
    lays[3] = fwd(3, lays[2]["y"])
    r = B.bf16(u + lays[3]["y"], rounding)
    lays[4] = fwd(4, r)
    v = lays[4]["y"]
    h = B.forward(v, ops["Wh"], ops["bh"], 1, "none", rounding)
    head = B.grads(v, ops["Wh"], ops["R"], h, 1, "none", rounding)
    out = dict(Wh=head["dw"], bh=head["db"])
    dr = bwd(4, lays[4], head["dx"])
    du_unit = bwd(2, lays[2], bwd(3, lays[3], dr))
    du = B.bf16(dr + du_unit, rounding)
    out["x0_grad"] = bwd(0, lays[0], bwd(1, lays[1], du))
    return out
