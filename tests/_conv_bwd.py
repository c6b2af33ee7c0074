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

# (n, h, w, cin, cout, k, act, dtype of y and dy, view of x: None or (channels of the buffer, offset))
CASES = [
    (2, 13, 17, 24, 40, 3, "leaky", torch.bfloat16, None),      # 1 odd map, 442 pixels, ragged channel counts below one tile
    (1, 1, 9, 8, 8, 3, "none", torch.bfloat16, None),           # 2 one-row map: only centre-row taps are in bounds
    (2, 20, 20, 64, 128, 1, "leaky", torch.bfloat16, None),     # 3 1x1
    (2, 8, 8, 32, 255, 1, "none", torch.float32, None),         # 4 head: g padded 255 -> 256, fp32 y and dy
    (1, 4, 4, 16, 18, 1, "none", torch.float32, None),          # 5 nc = 1 head, padded 18 -> 24
    (2, 80, 80, 16, 32, 3, "leaky", torch.bfloat16, None),      # 6 12,800 pixels: the split path
    (3, 5, 7, 136, 8, 3, "none", torch.bfloat16, None),         # 7 1224 columns: ten 128-wide tiles, the last ragged; cout below a tile
    (2, 13, 17, 24, 40, 3, "leaky", torch.bfloat16, (48, 16)),  # 8 case 1 with x as the view [16, 40) of a 48-channel buffer
]
SPLIT_CASE = 5          # index of case 6 in CASES


def case_id(c):
    n, h, w, cin, cout, k, act, dt, view = c
    return f"{n}x{h}x{w}_{cin}to{cout}_k{k}_{act}_{'bf16' if dt == torch.bfloat16 else 'f32'}" + ("_view" if view else "")


def fwd_desc(case, **over):
    """The FORWARD's descriptor of a case (what every backward entry point takes); ``over`` replaces conv_desc arguments."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, DT_BF16, DT_F32
    n, h, w, cin, cout, k, act, dt, view = case
    total, off = view or (cin, 0)
    f32 = dt == torch.float32
    kw = dict(n=n, h=h, w=w, cin=cin, in_c_total=total, in_c_offset=off, cout=cout, out_c_total=K.roundup(cout, 4) if f32 else cout,
              out_c_offset=0, ksize=k, stride=1, act=ACT_LEAKY01 if act == "leaky" else ACT_NONE, kpad=K.roundup(k * k * cin, 64),
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
