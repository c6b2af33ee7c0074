"""GPU tests of the conv backward (csrc/conv_bwd.hip through pytorch_yolo_amd.kernels and pytorch_yolo_amd.ops.conv_block) against the
float64 restatement of tests/_conv_bwd.py.

Every case runs the whole chain on the device - device weight pack, the FORWARD (yolo_conv2d_fwd), prepare (g), weight / bias gradient,
transposed pack, data gradient - with every operand, g, the workspace, dW, db and dx between the poisoned bands of tests/_guard.py and
the outputs and the workspace pre-filled with NaN.  The slope of LeakyReLU is taken from the y the device's forward wrote.

Exact cases (integer operands, tests/_conv_bwd.exact_operands): torch.equal.  Random cases: per element
    |dW - S| <= 2 T 2^-24 A,   |db - S| <= 2 T 2^-24 A,   |dx - S| <= 2^-8 |S| + 2 T 2^-24 A
(T in-bounds terms, S the float64 sum, A the float64 sum of |terms|); each test prints its largest error / bound ratio.

Measured on an MI355X, largest error / bound over the fifteen cases: dW 0.0335 (the one-row map; 0.0000-0.0179 elsewhere), db 0.0009,
dx 0.98 - dx is one RNE away from its fp32 sum and half a bf16 spacing IS 2^-8 |S| right above a power of two, so the dx ratio reaches
~1 by construction of the bound; dx == bf16_rne(S) on 99.90-100 % of the elements.  End to end: dW 0.0586, db 0.0000; the five-layer
chain: dW 0.0158, db 0.0002, dx 0.995.

Beside the cases: the forms of prepare no case launches (test_prepare_forms), the dbias == NULL launch (test_weight_gradient_without_bias),
other compute-unit shares and with them other split counts (test_exact_under_other_cu_shares), and conv_block in composition - five
layers with torch's max-pool, upsample and concat between them, layer by layer against the restatement and as a whole against float64
autograd (test_chain_*)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _conv_bwd as B
import _guard as G
import _loss as L
from pytorch_yolo_amd import YOLOv3Tiny, compute_loss, conv_block, loss_grad_raw
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype)


def nchw64(t):
    return t.permute(0, 3, 1, 2).to(F64)


def device_chain(a, case, x, w, b, dy, fill=NAN, want_db=True):
    """The whole chain of one case on allocations of ``a`` (a _guard.Guard or _guard.Plain); float64 NCHW results on the host, the
    channels of the dx and y buffers outside their views and the workspace as raw bits.  want_db=False: the dbias == NULL launch."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    total, off = view or (cin, 0)
    d = B.fwd_desc(case)
    cg, ct, yo = K.roundup(cout, 8), d.out_c_total, d.out_c_offset
    xbuf = a.alloc("x", (n, h, wd, total), BF16, NAN)                 # channels outside the view hold NaN
    xbuf[..., off:off + cin] = nhwc(x, BF16).to(DEV)
    w_dev = a.like("w", w.to(F32))
    bias = a.alloc("bias", (d.cout_pad,), F32)
    bias[:cout] = b.to(F32).to(DEV)
    packed = a.alloc("w_packed", (d.cout_pad, d.kpad), BF16, fill)
    K.pack_conv_weight_dev(w_dev, cin, out=packed)
    ybuf = a.alloc("y", (n, h, wd, ct), dt, fill)
    K.conv2d(xbuf, packed, bias, ybuf, d)
    dy_dev = a.like("dy", nhwc(dy, dt))
    g = a.alloc("g", (n, h, wd, cg), BF16, fill)
    K.conv2d_bwd_prepare(dy_dev, ybuf, g, d)
    ws = a.alloc("workspace", (K.conv2d_bwd_workspace_bytes(d) // 4,), F32, fill)
    dw = a.alloc("dw", (cout, cin, k, k), F32, fill)
    db = a.alloc("db", (cout,), F32, fill) if want_db else None
    K.conv2d_bwd_weight(xbuf, g, dw, db, ws, d)
    packed_t = a.alloc("w_packed_t", (K.roundup(cin, 128), K.roundup(k * k * cg, 64)), BF16, fill)
    K.pack_conv_weight_dev(w_dev, cg, transposed=True, out=packed_t)
    dxbuf = a.alloc("dx", (n, h, wd, total), BF16, NAN)
    K.conv2d_bwd_data(g, packed_t, dxbuf, d)
    torch.cuda.synchronize()
    outside = torch.cat([dxbuf[..., :off], dxbuf[..., off + cin:]], -1).cpu().view(torch.int16)
    assert torch.equal(xbuf[..., off:off + cin].cpu(), nhwc(x, BF16))                              # the operands are read-only
    if oview:                                                                                      # the forward kept to its view of y
        y_out = torch.cat([ybuf[..., :yo], ybuf[..., yo + cout:]], -1).cpu()
        assert torch.equal(y_out.view(torch.int16), torch.full_like(y_out, fill).view(torch.int16))
    outs = (g, dw, db, dxbuf[..., off:off + cin]) if want_db else (g, dw, dxbuf[..., off:off + cin])
    return dict(y=nchw64(ybuf[..., yo:yo + cout].cpu()), g=nchw64(g[..., :cout].cpu()), g_pad=g[..., cout:].cpu(), dw=dw.cpu().to(F64),
                db=db.cpu().to(F64) if want_db else None, dx=nchw64(dxbuf[..., off:off + cin].cpu()), dx_outside=outside,
                ws=ws.cpu().view(torch.int32), raw=[t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32) for t in outs])


def same_bits(r1, r2):
    return all(torch.equal(p, q) for p, q in zip(r1["raw"], r2["raw"]))


def check_untouched(r):
    assert not r["g_pad"].any(), "the pad channels of g must be zero"
    nan_bits = torch.full((), NAN, dtype=BF16).view(torch.int16)
    assert bool((r["dx_outside"] == nan_bits).all()), "dx wrote outside its channel view"


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_exact(case):
    """Integer operands: dW and db have ONE right value and dx is that integer rounded once to bf16 - torch.equal.  Run between 0xFF
    bands with NaN-filled outputs, and on plain zero-filled allocations: the same bits."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.exact_operands(case)
    a = G.Guard(G.POISONS[0], DEV)
    r = device_chain(a, case, x, w, b, dy)
    a.assert_intact()
    check_untouched(r)
    y64 = B.forward(x, w, b, k, act)
    assert torch.equal(r["y"] > 0, y64 > 0) and (act != "none" or torch.equal(r["y"], B.bf16(y64) if dt == BF16 else y64))
    want = B.grads(x, w, dy, r["y"], k, act)
    for name in ("g", "dw", "db", "dx"):
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ"
    assert want["dw"].any() and want["db"].any() and want["dx"].any()
    assert same_bits(r, device_chain(G.Plain(DEV), case, x, w, b, dy, fill=0.0))


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_random_within_bounds(case):
    """Random operands against the restatement, once per poison; the two runs are bit-equal (no atomics, nothing read before it is
    written)."""
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    runs = []
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        runs.append(device_chain(a, case, x, w, b, dy))
        a.assert_intact()
        check_untouched(runs[-1])
    assert same_bits(*runs)
    r = runs[0]
    want = B.grads(x, w, dy, r["y"], k, act)
    assert torch.equal(r["g"], want["g"])                                                        # one fp32 multiply, one RNE: exact
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  dx=B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    # dx is one RNE away from its fp32 sum: half a bf16 spacing is 2^-8 |S| right above a power of two, so its ratio reaches ~1 by
    # design of the bound; what the summation itself contributes shows in the share of elements that ARE bf16_rne(S)
    same = float((r["dx"] == want["dx"]).double().mean())
    print(f"conv_bwd {B.case_id(case)}: largest error / bound  dW {ratios['dw']:.4f}  db {ratios['db']:.4f}  dx {ratios['dx']:.4f}"
          f"  (dx == bf16_rne(S) on {100 * same:.2f} % of the elements)")
    assert (act == "none" or 0.15 < float((r["y"] <= 0).double().mean()) < 0.85) and want["dw"].any()
    for name, v in ratios.items():
        assert v <= 1.0, f"{name}: error / bound = {v}"


@functools.lru_cache(maxsize=None)
def exact_reference(index):
    """The exact operands of CASES[index] and their gradients from the float64 forward (computed once, shared, left unchanged): on
    integer operands the device's y has the float64 y's signs, which every user asserts."""
    n, h, wd, cin, cout, k, act, dt, view, oview = B.CASES[index]
    x, w, b, dy = B.exact_operands(B.CASES[index])
    y64 = B.forward(x, w, b, k, act)
    return (x, w, b, dy), y64, B.grads(x, w, dy, y64, k, act)


def assert_exact(r, y64, want, names=("g", "dw", "db", "dx")):
    assert torch.equal(r["y"] > 0, y64 > 0)
    for name in names:
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ"


@pytest.mark.parametrize("form", ["f32_dy_bf16_y", "bf16_dy_no_y", "bf16_dy_f32_y", "bf16_dy_f32_y_leaky"])
def test_prepare_forms(form):
    """The instantiations of bwd_prepare_kernel that the cases do not launch: dy and y of different dtypes, and y == NULL (act none)
    with a bf16 dy.  Exact operands, guarded allocations with g NaN-filled, g against the restatement's upstream(): torch.equal.
    The last form is case 13's shape with LeakyReLU, so that the fp32 y is read, not only typed."""
    index, act, dy_dt, pass_y = dict(f32_dy_bf16_y=(0, "leaky", F32, True), bf16_dy_no_y=(0, "none", BF16, False),
                                     bf16_dy_f32_y=(12, "none", BF16, True), bf16_dy_f32_y_leaky=(12, "leaky", BF16, True))[form]
    case = B.CASES[index][:6] + (act,) + B.CASES[index][7:]
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.exact_operands(case)
    d = B.fwd_desc(case)
    a = G.Guard(G.POISONS[0], DEV)
    xbuf = a.like("x", nhwc(x, BF16))
    packed, bias, kpad, cout_pad = K.pack_conv_weight(w.to(F32), b.to(F32), cin)
    ybuf = a.alloc("y", (n, h, wd, d.out_c_total), dt, NAN)
    K.conv2d(xbuf, a.like("w_packed", packed), a.like("bias", bias), ybuf, d)
    dy_dev = a.like("dy", nhwc(dy, dy_dt))
    g = a.alloc("g", (n, h, wd, K.roundup(cout, 8)), BF16, NAN)
    K.conv2d_bwd_prepare(dy_dev, ybuf if pass_y else None, g, d)
    torch.cuda.synchronize()
    a.assert_intact()
    y = nchw64(ybuf[..., :cout].cpu())
    assert torch.equal(y > 0, B.forward(x, w, b, k, act) > 0) and torch.equal(dy_dev.cpu(), nhwc(dy, dy_dt))
    want = B.upstream(dy, y, act)
    assert torch.equal(nchw64(g[..., :cout].cpu()), want) and want.any() and not g[..., cout:].cpu().any()
    if act == "leaky":
        assert 0.15 < float((want != dy).double().mean()) < 0.85         # the slope was applied, and not everywhere


@pytest.mark.parametrize("index", [8, B.WIDE_SPLIT_CASE], ids=lambda i: B.case_id(B.CASES[i]))
def test_weight_gradient_without_bias(index):
    """dbias == NULL on the 128x128 tile, unsplit (case 9) and split (case 12): dW has the bits of the run with a bias gradient - and
    the exact value -, and the workspace behind the splits' partial dW matrices, where the partial db rows would go, keeps its NaN fill
    bit for bit."""
    case = B.CASES[index]
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    (x, w, b, dy), y64, want = exact_reference(index)
    a = G.Guard(G.POISONS[0], DEV)
    r = device_chain(a, case, x, w, b, dy, want_db=False)
    a.assert_intact()
    check_untouched(r)
    assert_exact(r, y64, want, ("g", "dw", "dx"))
    with_db = device_chain(G.Plain(DEV), case, x, w, b, dy)
    assert torch.equal(r["raw"][1], with_db["raw"][1]) and torch.equal(with_db["db"], want["db"])
    splits = int(K.conv2d_bwd_pick(B.fwd_desc(case)).rsplit(" ", 1)[1])
    used = splits * cout * k * k * cin
    assert r["ws"].numel() == used + splits * cout and (splits >= 2) == (index == B.WIDE_SPLIT_CASE)
    nan_bits = torch.full((), NAN, dtype=F32).view(torch.int32)
    assert bool((r["ws"][used:] == nan_bits).all()), "the dbias == NULL launch wrote partial db rows"
    assert not bool((r["ws"][:used] == nan_bits).any()) and not bool((with_db["ws"] == nan_bits).any())


@pytest.mark.parametrize("index", [B.SPLIT_CASE, B.WIDE_SPLIT_CASE], ids=lambda i: B.case_id(B.CASES[i]))
def test_exact_under_other_cu_shares(index):
    """The split count follows the thread's compute-unit share (yolo_set_launch_cus): under 8 and 64 CUs - other split counts, for
    case 12 three splits of 11, 11 and 10 stages - the integer sums are what they are under 256.  The workspace is re-queried after
    each change (device_chain does); the old share comes back whatever happens."""
    case = B.CASES[index]
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    (x, w, b, dy), y64, want = exact_reference(index)
    d = B.fwd_desc(case)
    base = K.conv2d_bwd_pick(d)
    picks = []
    for cus in B.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            picks.append(K.conv2d_bwd_pick(d))
            a = G.Guard(G.POISONS[0], DEV)
            r = device_chain(a, case, x, w, b, dy)
            a.assert_intact()
        finally:
            K.set_launch_cus(old)
        assert old == 256 and r["ws"].numel() == int(picks[-1].rsplit(" ", 1)[1]) * cout * (k * k * cin + 1)
        check_untouched(r)
        assert_exact(r, y64, want)
    assert K.conv2d_bwd_pick(d) == base and any(p != base for p in picks), (base, picks)


def test_device_packer_equals_host_packer():
    """Both orientations, bit for bit against yolo_pack_conv_weight_f32 (for the transposed one: applied to w.flip(2, 3).transpose(0, 1)):
    half-way cases in both directions, values that round to zero, fp32 subnormals, cin_w < cin."""
    lib = _lib.load()
    for k, cout, cin_w, cin in ((3, 21, 12, 16), (1, 255, 32, 32), (3, 8, 136, 136), (1, 5, 3, 8)):
        w = torch.randn((cout, cin_w, k, k), generator=torch.Generator().manual_seed(7 + k + cout))
        flat = w.view(-1)
        special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 2.0 ** -134, 2.0 ** -133, 1e-45, -1e-45,
                                2.0 ** -134 * 1.5, 3.3895e38, 0.0, -0.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -20])
        flat[:special.numel()] = special
        flat[-special.numel():] = special.flip(0)
        for transposed in (False, True):
            a = G.Guard(G.POISONS[0], DEV)
            w_dev = a.like("w", w)
            src = w.flip(2, 3).transpose(0, 1).contiguous() if transposed else w
            rows, chans, c_pad = (cin_w, cout, K.roundup(cout, 8)) if transposed else (cout, cin_w, cin)
            kpad, cout_pad = K.roundup(k * k * c_pad, 64), K.roundup(rows, 128)
            want = torch.full((cout_pad, kpad), NAN, dtype=BF16)
            assert lib.yolo_pack_conv_weight_f32(src.data_ptr(), rows, chans, k, c_pad, cout_pad, kpad, want.data_ptr()) == 0
            out = a.alloc("packed", (cout_pad, kpad), BF16, NAN)
            got, kp, cp = K.pack_conv_weight_dev(w_dev, c_pad, transposed=transposed, out=out)
            torch.cuda.synchronize()
            a.assert_intact()
            assert (kp, cp) == (kpad, cout_pad) and got.data_ptr() == out.data_ptr()
            assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), (k, cout, cin_w, cin, transposed)
            assert bool((want.float() == 0).any()) and bool((want.float() != 0).any())


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    """NCHW-shaped, dense channels-last (the package's NHWC layout)."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("index", [0, 3], ids=lambda i: B.case_id(B.CASES[i]))
def test_conv_block_forward_and_backward(index):
    """conv_block's forward is bit-equal to K.conv2d on the HOST-packed weight, and .backward() gives the kernels' gradients
    (device_chain on plain allocations) bit for bit."""
    case = B.CASES[index]
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    chain = device_chain(G.Plain(DEV), case, x, w, b, dy)
    xd = _cl(x.to(BF16).to(DEV)).requires_grad_()
    wp, bp = torch.nn.Parameter(w.to(F32).to(DEV)), torch.nn.Parameter(b.to(F32).to(DEV))
    out = conv_block(xd, wp, bp, act=act, out_dtype=dt)
    assert out.dtype == dt and tuple(out.shape) == (n, cout, h, wd) and out.grad_fn is not None
    packed, bias, kpad, cout_pad = K.pack_conv_weight(w.to(F32), b.to(F32), cin)
    d = B.fwd_desc(case)
    y_ref = torch.full((n, h, wd, d.out_c_total), NAN, dtype=dt, device=DEV)
    K.conv2d(xd.detach().permute(0, 2, 3, 1), packed.to(DEV), bias.to(DEV), y_ref, d)
    assert torch.equal(out.detach().permute(0, 2, 3, 1), y_ref[..., :cout])
    out.backward(_cl(dy.to(dt).to(DEV)))
    torch.cuda.synchronize()
    assert xd.grad.dtype == BF16 and wp.grad.dtype == F32 and bp.grad.dtype == F32 and wp.grad.shape == wp.shape
    assert torch.equal(xd.grad.cpu().to(F64), chain["dx"]) and torch.equal(wp.grad.cpu().to(F64), chain["dw"])
    assert torch.equal(bp.grad.cpu().to(F64), chain["db"])


def test_conv_block_autograd_contract():
    case = B.CASES[0]
    n, h, wd, cin, cout, k, act, dt, view, oview = case
    x, w, b, dy = B.random_operands(case)
    xd = _cl(x.to(BF16).to(DEV))
    wd_, bd = w.to(F32).to(DEV), b.to(F32).to(DEV)
    # nothing requires grad / no_grad: the forward only
    assert conv_block(xd, wd_, bd).grad_fn is None
    wp = torch.nn.Parameter(wd_.clone())
    with torch.no_grad():
        plain = conv_block(xd, wp, bd)
    assert plain.grad_fn is None and not plain.requires_grad
    # only the weight requires grad: x and bias get None, and the forward value is the same
    out = conv_block(xd, wp, bd)
    assert torch.equal(out.detach(), plain)
    out.backward(_cl(dy.to(BF16).to(DEV)))
    assert wp.grad is not None and xd.grad is None and bd.grad is None
    chain = device_chain(G.Plain(DEV), case, x, w, b, dy)                  # the dbias == NULL launch: the kernels' dW, bit for bit
    assert torch.equal(wp.grad.cpu().to(F64), chain["dw"]) and chain["dw"].any()
    y64 = plain.cpu().to(F64)
    want = B.grads(x, w, dy, y64, k, act)                                  # (the two lambdas read ``want`` when called: the 12-channel part below rebinds it)
    within = lambda got, name: B.ratio(got.cpu(), want[name], B.bound_sum(want[name + "_terms"], want[name + "_abs"]))
    within_dx = lambda got, sel=slice(None): B.ratio(got.cpu(), want["dx_sum"][:, sel], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])[:, sel])
    assert within(wp.grad, "dw") <= 1.0
    # only x requires grad
    xr = xd.clone().requires_grad_()
    gx, = torch.autograd.grad(conv_block(xr, wd_, bd), xr, _cl(dy.to(BF16).to(DEV)))
    assert gx.dtype == BF16 and gx.shape == xr.shape and within_dx(gx) <= 1.0 and bool(gx.any())
    # only the bias requires grad
    bp = torch.nn.Parameter(bd.clone())
    gb, = torch.autograd.grad(conv_block(xd, wd_, bp), bp, _cl(dy.to(BF16).to(DEV)))
    assert gb.dtype == F32 and gb.shape == bp.shape and within(gb, "db") <= 1.0 and bool(gb.any())
    # one weight shared by two calls in one graph: its gradient is the fp32 sum of the two calls' dW (autograd's addition)
    xb = _cl(x.flip(2).to(BF16).to(DEV))
    dyd = _cl(dy.to(BF16).to(DEV))
    ga, = torch.autograd.grad(conv_block(xd, wp, bd), wp, dyd)
    gb2, = torch.autograd.grad(conv_block(xb, wp, bd), wp, dyd)
    wp.grad = None
    torch.autograd.backward([conv_block(xd, wp, bd), conv_block(xb, wp, bd)], [dyd, dyd])
    assert torch.equal(ga.cpu().to(F64), chain["dw"]) and not torch.equal(ga, gb2) and torch.equal(wp.grad, ga + gb2)
    # a double backward raises
    xr2 = xd.clone().requires_grad_()
    g1, = torch.autograd.grad(conv_block(xr2, wp, bd).float().sum(), xr2, create_graph=True)
    with pytest.raises(RuntimeError, match="does not require grad"):       # an upstream gradient that does not require grad: detached
        g1.float().sum().backward()
    scale = torch.tensor(2.0, device=DEV, requires_grad=True)              # one that does: a node that refuses to be differentiated
    g1, = torch.autograd.grad((conv_block(xr2, wp, bd).float() * scale).sum(), xr2, create_graph=True)
    assert g1.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g1.float().sum().backward()
    # a float32 NCHW-contiguous x gets a float32 gradient of its own layout, the bf16 gradient widened
    x32 = x.to(F32).to(DEV).contiguous().requires_grad_()
    conv_block(x32, wd_, bd).backward(_cl(dy.to(BF16).to(DEV)))
    assert x32.grad.dtype == F32 and x32.grad.is_contiguous() and torch.equal(x32.grad, gx.float())
    assert within_dx(x32.grad) <= 1.0                                      # against the restatement, not only the op's other path
    # 12 input channels are zero-padded to 16 by torch: gradients of the 12-channel shapes
    x12 = xd[:, :12].float().contiguous().requires_grad_()
    w12 = torch.nn.Parameter(wd_[:, :12].clone())
    b12 = torch.nn.Parameter(bd.clone())
    o12 = conv_block(x12, w12, b12)
    o12.backward(_cl(dy.to(BF16).to(DEV)))
    assert x12.grad.shape == x12.shape and w12.grad.shape == w12.shape and bool(w12.grad.any())
    # ... by value: the restatement on the zero-padded 16-channel operands, the pad channels' slice dropped
    pad4 = lambda t: F.pad(t[:, :12], (0, 0, 0, 0, 0, 4))
    want = B.grads(pad4(x), pad4(w), dy, o12.detach().cpu().to(F64), k, act)
    assert not want["dw"][:, 12:].any() and not want["dx_sum"][:, 12:].any() and want["dw"][:, :12].any()   # the slice drops zeros only
    assert x12.grad.dtype == F32 and within_dx(x12.grad, slice(0, 12)) <= 1.0 and bool(x12.grad.any()) and bool(b12.grad.any())
    assert B.ratio(w12.grad.cpu(), want["dw"][:, :12], B.bound_sum(want["dw_terms"], want["dw_abs"])[:, :12]) <= 1.0 and within(b12.grad, "db") <= 1.0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv_block(xd.cpu(), wd_.cpu())


# ---- conv_block in composition (the chain of tests/_conv_bwd.py) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference():
    """Operands, float64 autograd and the float64 chain with the rounding points: computed once, shared, left unchanged."""
    ops = B.chain_operands()
    return ops, B.chain_autograd64(ops), B.chain_restated(ops)


def run_chain(ops):
    """The chain on the device.  Each conv_block call reads an alias of its input (x.view_as(x)) whose hook sees that call's dx apart
    from what autograd adds up for a tensor with two consumers; a hook on each output sees the dy the call received.  Returns
    dict(calls=[x, y, dy, dx per layer], dw, db, x0_grad, r_grad, f_pool = the gradient of f that came through the max-pool)."""
    x0, r = (_cl(ops[name].to(BF16).to(DEV)).requires_grad_() for name in ("x0", "r"))
    W = [torch.nn.Parameter(t.to(F32).to(DEV)) for t in ops["W"]]
    b = [torch.nn.Parameter(t.to(F32).to(DEV)) for t in ops["b"]]
    R = [t.to(F32).to(DEV) for t in ops["R"]]
    calls = [dict() for _ in B.CHAIN_LAYERS]
    out = dict(calls=calls)

    def keep(store, key):
        return lambda grad: store.__setitem__(key, grad.detach().clone())

    def call(i, x):
        cin, cout, k, act, dt = B.CHAIN_LAYERS[i]
        alias = x.view_as(x)
        alias.register_hook(keep(calls[i], "dx"))
        y = conv_block(alias, W[i], b[i], act=act, out_dtype=dt)
        y.register_hook(keep(calls[i], "dy"))
        calls[i].update(x=alias.detach(), y=y.detach())
        return y

    f = call(0, x0)
    a = call(1, f)
    m = call(2, torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), r], 1))
    h1 = call(3, m)
    f_pool = f.view_as(f)
    f_pool.register_hook(keep(out, "f_pool"))
    h2 = call(4, F.max_pool2d(f_pool, 2, 2))
    ((h1 * R[0]).sum() + (h2 * R[1]).sum()).backward()
    torch.cuda.synchronize()
    out.update(dw=[t.grad for t in W], db=[t.grad for t in b], x0_grad=x0.grad, r_grad=r.grad)
    return out


@functools.lru_cache(maxsize=None)
def chain_on_device():
    return run_chain(chain_reference()[0])


def _chain_tensors(run):
    return [c[key] for c in run["calls"] for key in ("y", "dy", "dx")] + run["dw"] + run["db"] + [run["x0_grad"], run["r_grad"], run["f_pool"]]


def test_chain_layer_by_layer():
    """Five conv_blocks with torch's max-pool, upsample and concat between them, bf16 channels-last: every call, fed to the restatement
    with the device's own x, dy and y, has an exact g (yolo_conv2d_bwd_prepare on the same tensors) and dW, db, dx within the three
    bounds of test_random_within_bounds; the glue is autograd's: the gradient of the concat arrives at r and - through the upsample's
    2x2 sum, one bf16 rounding - at a; f's gradient is torch's bf16 sum of its two consumers'; each dx is the next dy.  A second run
    gives the same bits everywhere.  Layer 3 (80 -> 136 on 640 pixels) is a 6x2 grid of the 128x128 tile.

    Measured on an MI355X, largest error / bound of layers 1-5: dW 0.0070 0.0049 0.0022 0.0014 0.0158, db 0.0002 0.0000 0.0001 0.0000
    0.0000, dx 0.8984 0.9920 0.8117 0.9950 0.9941 (dx reaches ~1 by the bound's own bf16 term: the module docstring); the upsample's
    2x2 sum against its float64 value 0.9960."""
    ops = chain_reference()[0]
    run = chain_on_device()
    calls = run["calls"]
    for i, (c, (cin, cout, k, act, dt)) in enumerate(zip(calls, B.CHAIN_LAYERS)):
        n, _, h, wd = c["x"].shape
        assert c["dy"].dtype == dt and c["dx"].dtype == BF16 and c["dx"].shape == c["x"].shape
        want = B.grads(c["x"].cpu().to(F64), ops["W"][i], c["dy"].cpu(), c["y"].cpu().to(F64), k, act)
        d = B.fwd_desc((n, h, wd, cin, cout, k, act, dt, None, None))
        g = torch.full((n, h, wd, K.roundup(cout, 8)), NAN, dtype=BF16, device=DEV)
        K.conv2d_bwd_prepare(c["dy"].permute(0, 2, 3, 1).contiguous(), c["y"].permute(0, 2, 3, 1), g, d)
        assert torch.equal(nchw64(g[..., :cout].cpu()), want["g"]) and not g[..., cout:].cpu().any()
        ratios = dict(dw=B.ratio(run["dw"][i].cpu(), want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                      db=B.ratio(run["db"][i].cpu(), want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                      dx=B.ratio(c["dx"].cpu(), want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
        print(f"conv_bwd chain layer {i + 1} ({cin} -> {cout}, k{k}): largest error / bound  dW {ratios['dw']:.4f}  db {ratios['db']:.4f}"
              f"  dx {ratios['dx']:.4f}")
        for name, v in ratios.items():
            assert v <= 1.0, f"layer {i + 1} {name}: error / bound = {v}"
        assert all(bool(t.any()) for t in (run["dw"][i], run["db"][i], c["dx"], c["dy"]))
        assert act == "none" or 0.15 < float((c["y"] <= 0).double().mean()) < 0.85
    # the glue.  One layer's dx is the next layer's dy:
    assert torch.equal(calls[2]["dy"], calls[3]["dx"]) and torch.equal(run["x0_grad"], calls[0]["dx"])
    # the concat's gradient: channels 32.. are r's, channels ..32 go through the upsample's backward (a 2x2 sum, rounded once) to a
    dc = calls[2]["dx"]
    assert torch.equal(run["r_grad"], dc[:, 32:]) and run["r_grad"].shape == (B.CHAIN_BS, B.CHAIN_SKIP, 16, 20)
    s = F.avg_pool2d(dc[:, :32].cpu().to(F64), 2) * 4
    up = B.ratio(calls[1]["dy"].cpu(), s, B.bound_dx(s, torch.full_like(s, 4.0), F.avg_pool2d(dc[:, :32].cpu().to(F64).abs(), 2) * 4))
    print(f"conv_bwd chain, upsample backward (2x2 bf16 sum): largest error / bound {up:.4f}")
    assert up <= 1.0, up
    # f has two consumers: the 1x1 layer's dx and what the max-pool hands on of layer 5's dx (each dx value at one place of its window)
    pooled = run["f_pool"].cpu().to(F64)
    assert torch.equal(F.avg_pool2d(pooled, 2) * 4, calls[4]["dx"].cpu().to(F64))
    assert int((pooled != 0).sum()) == int((calls[4]["dx"] != 0).sum())
    assert torch.equal(calls[0]["dy"], calls[1]["dx"] + run["f_pool"]) and not torch.equal(calls[0]["dy"], calls[1]["dx"])
    again = run_chain(ops)
    for t1, t2 in zip(_chain_tensors(run), _chain_tensors(again)):
        assert t1.dtype == t2.dtype and torch.equal(t1.view(torch.int16 if t1.dtype == BF16 else torch.int32),
                                                    t2.view(torch.int16 if t2.dtype == BF16 else torch.int32))


def test_chain_vs_float64_autograd():
    """The chain's parameter gradients against float64 autograd of the same network without any rounding (F.conv2d, leaky_relu, the
    same pool, upsample and concat on the fp32 master weights), by relative L2 error.  The yardstick for that number is the float64
    chain WITH every documented rounding point (chain_restated; tests/test_conv_bwd_cpu.py keeps it equal to autograd with the
    rounding off): the device shares every rounding point and differs in fp32 summation order only, so its error has to be within
    1.5 x the yardstick's for each of W1..W5 and b1..b5 - a dropped tensor or a wrong slice is off by order one.

    Measured on an MI355X, device / float64 chain with the rounding points: dW1 4.9003e-02 / 4.9003e-02, dW2 3.1797e-02 / 3.1798e-02,
    dW3 2.8633e-02 / 2.8633e-02, dW4 3.0690e-03 / 3.0689e-03, dW5 2.8789e-03 / 2.8789e-03, db1 3.1400e-02 / 3.1403e-02, db2 3.0485e-02 /
    3.0486e-02, db3 3.2234e-02 / 3.2234e-02, db4 1.6887e-03 / 1.6887e-03, db5 1.6103e-03 / 1.6103e-03 (quotients 0.9999-1.00002).  Both
    are the 0.02-0.06 % of LeakyReLU outputs that the bf16 roundings moved across zero (tests/test_conv_bwd_cpu.py counts them)."""
    ops, (dw64, db64, _, _), cpu = chain_reference()
    run = chain_on_device()
    rows = []
    for kind, dev, ref, want in (("W", run["dw"], cpu["dw"], dw64), ("b", run["db"], cpu["db"], db64)):
        for i in range(len(B.CHAIN_LAYERS)):
            rows.append((f"{kind}{i + 1}", B.rel_l2(dev[i].cpu(), want[i]), B.rel_l2(ref[i], want[i])))
            print("conv_bwd chain vs float64 autograd, relative L2 of d%s: device %.4e  float64 chain with the rounding points %.4e" % rows[-1]
                  + "  device / chain %.5f" % (rows[-1][1] / rows[-1][2]))
    for name, e_dev, e_cpu in rows:
        assert e_cpu > 0 and e_dev <= 1.5 * e_cpu, (name, e_dev, e_cpu)


def test_end_to_end_head_training_step():
    """compute_loss(p, targets, model)[0].backward() fills weight.grad / bias.grad of two conv_block heads (out_dtype float32) whose
    outputs are shaped into p by torch: equal to the restatement fed with loss_grad_raw's output, within the bounds, non-zero, and
    bit-equal across two runs.  The model's own forward stays without a grad_fn."""
    nc, bs = 2, 2
    model = YOLOv3Tiny(n_class=nc).eval()
    model.hyper_params = dict(L.HYPER)
    model = model.to(DEV)
    with torch.no_grad():
        io, p0 = model(torch.rand((bs, 3, 64, 64), generator=torch.Generator().manual_seed(3)).to(DEV))
    assert model(torch.rand((bs, 3, 64, 64)).to(DEV))[1][0].grad_fn is None
    layers = [dict(anchor_vec=y.anchor_vec.cpu().numpy().astype("float32"), nx=int(y.n_grids[0]), ny=int(y.n_grids[1]), na=int(y.anchor_vec.shape[0]))
              for y in model.yolo_layers]
    targets, _ = L.good_targets(77, layers, bs, nc, 24)
    targets = torch.from_numpy(targets)
    gen = torch.Generator().manual_seed(11)
    feats, params = [], []
    for t, cin in zip(p0, (512, 256)):
        _, na, ny, nx, no = t.shape
        feats.append(_cl(torch.randn((bs, cin, ny, nx), generator=gen).to(BF16).to(DEV)))
        params.append((torch.nn.Parameter((torch.randn((na * no, cin, 1, 1), generator=gen) / cin ** 0.5).to(DEV)),
                       torch.nn.Parameter(torch.randn((na * no,), generator=gen).to(DEV))))

    def step():
        for w, b in params:
            w.grad = b.grad = None
        p = []
        for f, (w, b), t in zip(feats, params, p0):
            _, na, ny, nx, no = t.shape
            out = conv_block(f, w, b, act="none", out_dtype=F32)
            p.append(out.reshape(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous())
        compute_loss(p, targets, model)[0].backward()
        torch.cuda.synchronize()
        return [t.detach() for t in p], [(w.grad.clone(), b.grad.clone()) for w, b in params]

    p, grads = step()
    _, again = step()
    upstream = loss_grad_raw(p, targets, model)
    for (f, (w, b), gp, (gw, gb), (gw2, gb2)) in zip(feats, params, upstream, grads, again):
        _, na, ny, nx, no = gp.shape
        dy = gp.permute(0, 1, 4, 2, 3).reshape(bs, na * no, ny, nx).cpu()
        want = B.grads(f.cpu(), w.detach().cpu(), dy, None, 1, "none")
        rw = B.ratio(gw.cpu(), want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"]))
        rb = B.ratio(gb.cpu(), want["db"], B.bound_sum(want["db_terms"], want["db_abs"]))
        print(f"conv_bwd end to end {ny}x{nx}: largest error / bound  dW {rw:.4f}  db {rb:.4f}")
        assert rw <= 1.0 and rb <= 1.0
        assert bool(gw.any()) and bool(gb.any()) and gw.dtype == F32 and gw.shape == w.shape
        assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32)) and torch.equal(gb.view(torch.int32), gb2.view(torch.int32))
