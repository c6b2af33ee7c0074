"""Float64 restatement of the conv backward (csrc/conv_bwd.hip) with its rounding points, and the test cases.

The arithmetic, for y = act(conv(x, bf16(W)) + bias) at stride 1, pad k // 2, act none or LeakyReLU(0.1):
    g  = bf16_rne(fp32(dy) * (y > 0 ? 1 : 0.1f))          (act none: bf16_rne(dy)); one fp32 multiply, done here in torch fp32
    dW[co][ci][kh][kw] = sum_{n,oh,ow} g[n,co,oh,ow] * x[n,ci,oh+kh-pad,ow+kw-pad]      taps outside the image add nothing
    db[co] = sum g
    dx = bf16_rne(conv(g, Wt)),  Wt[ci][co][kh][kw] = bf16(W)[co][ci][k-1-kh][k-1-kw], same pad
bf16 rounding is torch's RNE cast.  Tensors are NCHW / OIHW float64 here; ``rounding=False`` switches every rounding point off (the
form that must equal float64 autograd).  Beside each sum S the restatement returns A = sum |terms| and T = the number of in-bounds
terms, the two quantities of the error bounds:
    |dW - S| <= 2 T 2^-24 A        |db - S| <= 2 T 2^-24 A        |dx - S| <= 2^-8 |S| + 2 T 2^-24 A
(products of bf16 values are exact in fp32, (T - 1) 2^-24 A bounds an fp32 sum in any order, the factor 2 covers the MFMA's internal
order, 2^-8 is one bf16 ulp).
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
U24 = 2.0 ** -24

# (n, h, w, cin, cout, k, act, dtype of y and dy, view of x: None or (channels of the buffer, offset), view of y: None or the same)
CASES = [
    (2, 13, 17, 24, 40, 3, "leaky", torch.bfloat16, None, None),      # 1 odd map, 442 pixels, ragged channel counts below one tile
    (1, 1, 9, 8, 8, 3, "none", torch.bfloat16, None, None),           # 2 one-row map: only centre-row taps are in bounds
    (2, 20, 20, 64, 128, 1, "leaky", torch.bfloat16, None, None),     # 3 1x1
    (2, 8, 8, 32, 255, 1, "none", torch.float32, None, None),         # 4 head: g padded 255 -> 256, fp32 y and dy
    (1, 4, 4, 16, 18, 1, "none", torch.float32, None, None),          # 5 nc = 1 head, padded 18 -> 24
    (2, 80, 80, 16, 32, 3, "leaky", torch.bfloat16, None, None),      # 6 12,800 pixels: the split path
    (3, 5, 7, 136, 8, 3, "none", torch.bfloat16, None, None),         # 7 1224 columns: ten 128-wide tiles, the last ragged; cout below a tile
    (2, 13, 17, 24, 40, 3, "leaky", torch.bfloat16, (48, 16), None),  # 8 case 1 with x as the view [16, 40) of a 48-channel buffer
    # the 128x128 tile (cout > 64) on the grids the neck layers take
    (2, 6, 7, 16, 136, 3, "leaky", torch.bfloat16, None, None),       # 9 2x2 tiles, both edges ragged (144 columns, 136 couts); 84 pixels = one full + one partial stage
    (2, 9, 9, 32, 72, 3, "leaky", torch.bfloat16, None, None),        # 10 ragged 128-tile (72 couts: no g chunk from chunk 9 on), three column tiles
    (1, 10, 13, 256, 128, 1, "none", torch.bfloat16, None, None),     # 11 1x1 with two FULL column tiles: all four waves of the tile in range
    (5, 20, 20, 32, 136, 3, "leaky", torch.bfloat16, None, None),     # 12 the split path in the 128-wide tile: 32 stages, 3x2 tiles, 4 splits, with db
    (2, 5, 6, 16, 24, 1, "none", torch.float32, None, None),          # 13 fp32 head with cout % 8 == 0: whole 8-channel loads of fp32 dy
    (1, 7, 9, 16, 100, 3, "leaky", torch.bfloat16, None, None),       # 14 bf16 output with cout % 8 != 0 (element loads of bf16); dx is a conv with 104 input channels
    (1, 7, 9, 16, 100, 3, "leaky", torch.bfloat16, None, (112, 4)),   # 15 case 14 with y as the view [4, 104) of a 112-channel buffer (the "v4" view of _exact_cases.py; the forward accepts it as it is)
]
SPLIT_CASE = 5          # index of case 6 in CASES
WIDE_SPLIT_CASE = 11    # index of case 12
# compute-unit shares (yolo_set_launch_cus) the two split cases also run under: 8 gives case 6 eight splits instead of 25 and case 12
# three (11, 11 and 10 stages) instead of 4; 64 leaves both counts as they are (CPU test: test_split_count_follows_the_cu_share)
CU_SHARES = (8, 64)


def case_id(c):
    n, h, w, cin, cout, k, act, dt, view, oview = c
    return f"{n}x{h}x{w}_{cin}to{cout}_k{k}_{act}_{'bf16' if dt == torch.bfloat16 else 'f32'}" + ("_view" if view else "") + ("_yview" if oview else "")


def fwd_desc(case, **over):
    """The FORWARD's descriptor of a case (what every backward entry point takes); ``over`` replaces conv_desc arguments."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, DT_BF16, DT_F32
    n, h, w, cin, cout, k, act, dt, view, oview = case
    total, off = view or (cin, 0)
    f32 = dt == torch.float32
    ototal, ooff = oview or (K.roundup(cout, 4) if f32 else cout, 0)
    kw = dict(n=n, h=h, w=w, cin=cin, in_c_total=total, in_c_offset=off, cout=cout, out_c_total=ototal,
              out_c_offset=ooff, ksize=k, stride=1, act=ACT_LEAKY01 if act == "leaky" else ACT_NONE, kpad=K.roundup(k * k * cin, 64),
              cout_pad=K.roundup(cout, 128), out_dtype=DT_F32 if f32 else DT_BF16)
    kw.update(over)
    return K.conv_desc(**kw)


def bf16(t, rounding=True):
    """RNE to bf16 of an fp32-representable float64 tensor, back in float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64) if rounding else t.to(F64)


def forward(x, w, b, k, act, rounding=True):
    """y in float64 (before the output's own rounding): act(conv(x, bf16(W)) + bias)."""
    y = F.conv2d(x.to(F64), bf16(w, rounding), None if b is None else b.to(F64), padding=k // 2)
    return F.leaky_relu(y, 0.1) if act == "leaky" else y


def upstream(dy, y, act, rounding=True):
    """g (float64 NCHW).  With rounding the product is the kernel's single fp32 multiply by 0.1f, then RNE to bf16."""
    if not rounding:
        one, slope = torch.tensor(1.0, dtype=F64), torch.tensor(0.1, dtype=F64)
        return dy.to(F64) * (torch.where(y > 0, one, slope) if act == "leaky" else 1.0)
    d = dy.to(torch.float32)
    if act == "leaky":
        d = d * torch.where(y > 0, torch.tensor(1.0, dtype=torch.float32), torch.tensor(0.1, dtype=torch.float32))
    return d.to(torch.bfloat16).to(F64)


def _dw_sums(g, cols, cin, k):
    n, cout = g.shape[:2]
    return torch.einsum("nop,ncp->oc", g.reshape(n, cout, -1), cols).reshape(cout, cin, k, k)


def grads(x, w, dy, y, k, act, rounding=True, inject=None):
    """The gradients and their bound quantities.  x [n,cin,h,w], w [cout,cin,k,k], dy and y [n,cout,h,w] (any float dtype).
    inject (the generators' guards): ("tap", t) - tap t reads the pixel one column to the right of its own; ("pixels", a, b) - the
    pixels [a, b) of the flattened (n, h, w) range are left out of dW, as a dropped split would."""
    x = x.to(F64)
    n, cin, h, wd = x.shape
    g = upstream(dy, y, act, rounding)
    cols = F.unfold(x, k, padding=k // 2)                                # [n, cin k k, h w], rows ordered (ci, kh, kw)
    ones = F.unfold(torch.ones_like(x), k, padding=k // 2)
    if inject and inject[0] == "tap":
        t = inject[1]
        shifted = F.unfold(torch.roll(x, -1, 3), k, padding=k // 2).reshape(n, cin, k * k, -1)
        cols = cols.reshape(n, cin, k * k, -1).clone()
        cols[:, :, t] = shifted[:, :, t]
        cols = cols.reshape(n, cin * k * k, -1)
    gw = g
    if inject and inject[0] == "pixels":
        keep = torch.ones(n * h * wd, dtype=F64)
        keep[inject[1]:inject[2]] = 0
        gw = g * keep.reshape(n, 1, h, wd)
    out = dict(g=g)
    out["dw"], out["dw_abs"] = _dw_sums(gw, cols, cin, k), _dw_sums(gw.abs(), cols.abs(), cin, k)
    out["dw_terms"] = _dw_sums(torch.ones_like(g), ones, cin, k)
    out["db"], out["db_abs"] = g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))
    out["db_terms"] = torch.full_like(out["db"], n * h * wd)
    wt = bf16(w, rounding).flip(2, 3).transpose(0, 1)                     # the data gradient is a FORWARD conv with these weights
    s = F.conv2d(g, wt, padding=k // 2)
    out["dx_sum"], out["dx_abs"] = s, F.conv2d(g.abs(), wt.abs(), padding=k // 2)
    out["dx_terms"] = F.conv2d(torch.ones_like(g), torch.ones_like(wt), padding=k // 2)
    out["dx"] = bf16(s, rounding)
    return out


def bound_sum(terms, abs_sum):
    return 2.0 * terms * U24 * abs_sum


def bound_dx(s, terms, abs_sum):
    return 2.0 ** -8 * s.abs() + bound_sum(terms, abs_sum)


def ratio(got, want, bound):
    """Largest |got - want| / bound; an element whose bound is 0 must be met exactly."""
    err = (got.to(F64) - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(F64))
    return float(r.max())


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_operands(case, seed=0):
    """Integer operands on which every product and every partial sum is exact in fp32 in any order: x, |w| and |dy| (/ 10 for
    LeakyReLU, where 0.1f * 10k == k in fp32) in {-3..3}.  The signs of w and dy are structured - w = u_co v_ci m, dy = a_p u_co m'
    with random signs u, v, a and random magnitudes m, m' - so that the terms of dx[p, ci] share the sign a_p v_ci and dx grows to
    ~2.9 cout k^2 and beyond 256, where bf16 has to round; x is plain random, so y, dW and db see random signs.
    Returns x [n,cin,h,w], w, b, dy [n,cout,h,w] as float64 tensors of integers."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    gen = _gen(1000 + seed)
    r = lambda *s: torch.randint(-3, 4, s, generator=gen).to(F64)
    sign = lambda *s: (torch.randint(0, 2, s, generator=gen) * 2 - 1).to(F64)
    x = r(n, cin, h, wd)
    u, v, a = sign(cout), sign(cin), sign(n, 1, h, wd)
    w = r(cout, cin, k, k).abs() * u.reshape(-1, 1, 1, 1) * v.reshape(1, -1, 1, 1)
    b = r(cout)
    dy = r(n, cout, h, wd).abs() * a * u.reshape(1, -1, 1, 1) * (10.0 if act == "leaky" else 1.0)
    return x, w, b, dy


def random_operands(case, seed=0):
    """x, dy ~ N(0, 1) rounded to their storage types, w ~ N(0, 1 / fan_in) fp32 (it is NOT bf16-representable: the pack rounds it),
    b ~ N(0, 1) fp32; float64 tensors."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    gen = _gen(2000 + seed)
    x = torch.randn((n, cin, h, wd), generator=gen).to(torch.bfloat16).to(F64)
    w = (torch.randn((cout, cin, k, k), generator=gen) / (cin * k * k) ** 0.5).to(F64)
    b = torch.randn((cout,), generator=gen).to(F64)
    dy = torch.randn((n, cout, h, wd), generator=gen).to(dt).to(F64)
    return x, w, b, dy


def needs_rounding(t):
    """Fraction of the elements of a float64 tensor that are not bf16 values."""
    return float((bf16(t) != t).double().mean())


def exact_conditions(case, seed=0):
    """What makes an exact case a test (asserted by the CPU tests, relied on by the GPU ones): the float64 witnesses of exactness -
    every operand an integer, every sum of |terms| below 2^24 -, the share of y that is non-positive and the share of dx that needs
    rounding to bf16."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = exact_operands(case, seed)
    y = forward(x, w, b, k, act)
    r = grads(x, w, dy, y, k, act)
    ints = all(bool((t == t.round()).all()) for t in (x, w, b, dy, r["g"], r["dw"], r["db"], r["dx_sum"]))
    y_pre = F.conv2d(x, w, b, padding=k // 2)
    return dict(integers=ints, largest_abs_sum=float(max(r["dw_abs"].max(), r["db_abs"].max(), r["dx_abs"].max(), F.conv2d(x.abs(), w.abs(), b.abs(), padding=k // 2).max())),
                y_nonpositive=float((y_pre <= 0).double().mean()), dx_rounded=needs_rounding(r["dx_sum"]),
                dx_terms=cout * k * k)


# dx can only leave the bf16 integers (|v| <= 256) where it has terms to grow on: with |g w| <= 9 and a mean of ~2.9 per term the
# rounding guard binds from 128 terms on; below that (cases 2, 5, 7: 24, 18 and 72 terms) dx is exact in bf16 whatever the operands.
DX_ROUNDING_FROM_TERMS = 128


# ---- a chain of conv_blocks (torch's max-pool, upsample and concat between the layers) -------------------------------------
#   f  = conv(x0 [2,32,8,10], W1)      a = conv(f, W2)      c = cat([upsample2x(a), r [2,48,16,20]], 1)      m = conv(c, W3)
#   h1 = conv(m, W4)                   h2 = conv(max_pool2d(f, 2, 2), W5)          loss = sum(h1 R1) + sum(h2 R2)
# f has two consumers (its gradient is a bf16 sum), the gradient of c arrives at a and r as channel slices, every dx is the next dy.
CHAIN_BS, CHAIN_HW, CHAIN_SKIP = 2, (8, 10), 48
CHAIN_LAYERS = [                         # cin, cout, k, act, dtype of y
    (32, 64, 3, "leaky", torch.bfloat16),
    (64, 32, 1, "leaky", torch.bfloat16),
    (80, 136, 3, "leaky", torch.bfloat16),
    (136, 21, 1, "none", torch.float32),
    (64, 21, 1, "none", torch.float32),
]


def chain_operands(seed=0):
    """x0, r: N(0, 1) bf16 values; W1..W5 ~ N(0, 1 / fan_in) fp32 master weights, b1..b5 ~ N(0, 1/4) fp32; R1, R2 ~ N(0, 1) fp32.
    float64 NCHW tensors: dict(x0, r, R=[R1, R2], W=[...], b=[...])."""
    gen = _gen(3000 + seed)
    h, w = CHAIN_HW
    rn = lambda *s: torch.randn(s, generator=gen)
    ops = dict(x0=rn(CHAIN_BS, 32, h, w).to(torch.bfloat16).to(F64), r=rn(CHAIN_BS, CHAIN_SKIP, 2 * h, 2 * w).to(torch.bfloat16).to(F64), W=[], b=[])
    for cin, cout, k, act, dt in CHAIN_LAYERS:
        ops["W"].append((rn(cout, cin, k, k) / (cin * k * k) ** 0.5).to(F64))
        ops["b"].append((rn(cout) * 0.5).to(F64))
    ops["R"] = [rn(CHAIN_BS, 21, 2 * h, 2 * w).to(F64), rn(CHAIN_BS, 21, h // 2, w // 2).to(F64)]
    return ops


def chain_autograd64(ops):
    """The network in float64 torch without any rounding: (dW list, db list, gradient of x0, gradient of r)."""
    x0, r = ops["x0"].clone().requires_grad_(), ops["r"].clone().requires_grad_()
    W = [t.clone().requires_grad_() for t in ops["W"]]
    b = [t.clone().requires_grad_() for t in ops["b"]]

    def conv(i, x):
        y = F.conv2d(x, W[i], b[i], padding=CHAIN_LAYERS[i][2] // 2)
        return F.leaky_relu(y, 0.1) if CHAIN_LAYERS[i][3] == "leaky" else y
    f = conv(0, x0)
    a = conv(1, f)
    m = conv(2, torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), r], 1))
    loss = (conv(3, m) * ops["R"][0]).sum() + (conv(4, F.max_pool2d(f, 2, 2)) * ops["R"][1]).sum()
    loss.backward()
    return [t.grad for t in W], [t.grad for t in b], x0.grad, r.grad


def _pool_backward(x, dy):
    """Gradient of max_pool2d(x, 2, 2) in float64: dy at the maximum of each window (torch's choice among equal values)."""
    leaf = x.clone().requires_grad_()
    return torch.autograd.grad(F.max_pool2d(leaf, 2, 2), leaf, dy)[0]


def chain_restated(ops, rounding=True):
    """The same network from forward() / grads(): float64 sums with every rounding point of the device chain - bf16 weights in the
    product, y rounded to its storage type, g and dx rounded to bf16 by grads(), the upsample's 2x2 sum and the sum of f's two
    gradients rounded once to bf16 (torch's bf16 kernels add in fp32 and round once).  Returns dict(calls=[per layer: x, y, dy and
    the result of grads()], dw, db, x0_grad, r_grad, f_grads=(the two consumers' gradients of f))."""
    W, b = ops["W"], ops["b"]

    def store(y, dt):
        if not rounding:
            return y
        return bf16(y) if dt == torch.bfloat16 else y.to(torch.float32).to(F64)

    def fwd(i, x):
        cin, cout, k, act, dt = CHAIN_LAYERS[i]
        return store(forward(x, W[i], b[i], k, act, rounding), dt)

    def bwd(i, x, y, dy):
        cin, cout, k, act, dt = CHAIN_LAYERS[i]
        return dict(x=x, y=y, dy=dy, r=grads(x, W[i], dy, y, k, act, rounding))
    f = fwd(0, ops["x0"])
    a = fwd(1, f)
    c = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), ops["r"]], 1)
    m = fwd(2, c)
    pooled = F.max_pool2d(f, 2, 2)
    h1, h2 = fwd(3, m), fwd(4, pooled)
    calls = [None] * 5
    calls[3] = bwd(3, m, h1, ops["R"][0])
    calls[4] = bwd(4, pooled, h2, ops["R"][1])
    calls[2] = bwd(2, c, m, calls[3]["r"]["dx"])
    dc = calls[2]["r"]["dx"]
    calls[1] = bwd(1, f, a, bf16(F.avg_pool2d(dc[:, :32], 2) * 4, rounding))
    f_grads = (calls[1]["r"]["dx"], _pool_backward(f, calls[4]["r"]["dx"]))
    calls[0] = bwd(0, ops["x0"], f, bf16(f_grads[0] + f_grads[1], rounding))
    return dict(calls=calls, dw=[c_["r"]["dw"] for c_ in calls], db=[c_["r"]["db"] for c_ in calls], x0_grad=calls[0]["r"]["dx"],
                r_grad=dc[:, 32:], f_grads=f_grads)


def rel_l2(got, want):
    return float((got.to(F64) - want).norm() / want.norm())
