"""GPU tests of the downsample's backward (csrc/conv_down_bwd.hip through pytorch_yolo_amd.kernels and pytorch_yolo_amd.ops.down_block /
down_bn_block) against the float64 restatement of tests/_conv_down.py.

Every case runs the whole chain on the device - device weight pack, the FORWARD (yolo_conv2d_fwd at stride 2), prepare (g, on the
stride-1 descriptor of the output map), the strided weight / bias gradient, the dgrad pack, the parity data gradient - with every operand,
g, the workspace, dW, db and dx between the poisoned bands of tests/_guard.py and the outputs and the workspace pre-filled with NaN.

Exact cases (integer operands): torch.equal.  Random cases: per element
    |dW - S| <= 2 T 2^-24 A,   |db - S| <= 2 T 2^-24 A,   |dx - S| <= 2^-8 |S| + 2 T 2^-24 A
(T in-bounds terms, S the float64 sum, A the float64 sum of |terms|); each test prints its largest error / bound ratio (DESIGN.md 3.6e
holds the measured values)."""
import functools

import numpy as np
import pytest
import torch

import _bn as N
import _conv_bwd as B
import _conv_down as D
import _guard as G
from pytorch_yolo_amd import _lib, conv_block, conv_bn_block, down_block, down_bn_block
from pytorch_yolo_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype)


def nchw64(t):
    return t.permute(0, 3, 1, 2).to(F64)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def device_chain(a, case, x, w, b, dy, fill=NAN, want_db=True):
    """The whole chain of one case on allocations of ``a`` (a _guard.Guard or _guard.Plain); float64 NCHW results on the host, the
    channels of the dx buffer outside its view and the workspace as raw bits.  want_db=False: the dbias == NULL launch."""
    n, h, wd, cin, cout, view = case
    total, off = view or (cin, 0)
    ho, wo = D.out_hw(h, wd)
    d = D.fwd_desc(case)
    xbuf = a.alloc("x", (n, h, wd, total), BF16, NAN)                 # channels outside the view hold NaN
    xbuf[..., off:off + cin] = nhwc(x, BF16).to(DEV)
    w_dev = a.like("w", w.to(F32))
    bias = a.alloc("bias", (d.cout_pad,), F32)
    bias[:cout] = b.to(F32).to(DEV)
    packed = a.alloc("w_packed", (d.cout_pad, d.kpad), BF16, fill)
    K.pack_conv_weight_dev(w_dev, cin, out=packed)
    ybuf = a.alloc("y", (n, ho, wo, cout), BF16, fill)
    K.conv2d(xbuf, packed, bias, ybuf, d)
    dy_dev = a.like("dy", nhwc(dy, BF16))
    g = a.alloc("g", (n, ho, wo, cout), BF16, fill)
    K.conv2d_bwd_prepare(dy_dev, ybuf, g, D.out_desc(case))
    ws = a.alloc("workspace", (K.conv2d_down_bwd_workspace_bytes(d) // 4,), F32, fill)
    dw = a.alloc("dw", (cout, cin, 3, 3), F32, fill)
    db = a.alloc("db", (cout,), F32, fill) if want_db else None
    K.conv2d_down_bwd_weight(xbuf, g, dw, db, ws, d)
    packed_d = a.alloc("w_packed_d", (3, 3, cin, cout), BF16, fill)
    K.pack_conv_weight_down_dev(w_dev, out=packed_d)
    dxbuf = a.alloc("dx", (n, h, wd, total), BF16, NAN)
    K.conv2d_down_bwd_data(g, packed_d, dxbuf, d)
    torch.cuda.synchronize()
    outside = torch.cat([dxbuf[..., :off], dxbuf[..., off + cin:]], -1).cpu().view(torch.int16)
    assert torch.equal(xbuf[..., off:off + cin].cpu(), nhwc(x, BF16))                              # the operands are read-only
    assert torch.equal(packed_d.cpu().view(torch.int16), w.to(F32).to(BF16).permute(2, 3, 1, 0).contiguous().view(torch.int16))
    outs = (g, dw, db, dxbuf[..., off:off + cin]) if want_db else (g, dw, dxbuf[..., off:off + cin])
    return dict(y=nchw64(ybuf.cpu()), g=nchw64(g.cpu()), dw=dw.cpu().to(F64), db=db.cpu().to(F64) if want_db else None,
                dx=nchw64(dxbuf[..., off:off + cin].cpu()), dx_outside=outside, ws=ws.cpu().view(torch.int32),
                raw=[bits(t.contiguous().cpu()) for t in outs])


def same_bits(r1, r2):
    return all(torch.equal(p, q) for p, q in zip(r1["raw"], r2["raw"]))


def check_untouched(r):
    nan_bits = torch.full((), NAN, dtype=BF16).view(torch.int16)
    assert bool((r["dx_outside"] == nan_bits).all()), "dx wrote outside its channel view"


def run_guarded(case, x, w, b, dy, poison, **kw):
    a = G.Guard(poison, DEV)
    r = device_chain(a, case, x, w, b, dy, **kw)
    a.assert_intact()
    check_untouched(r)
    return r


@functools.lru_cache(maxsize=None)
def exact_reference(index):
    """The exact operands of CASES[index] and their gradients from the float64 forward (computed once, shared, left unchanged): on
    integer operands the device's y has the float64 y's signs, which every user asserts."""
    x, w, b, dy = D.exact_operands(D.CASES[index])
    y64 = D.forward(x, w, b)
    return (x, w, b, dy), y64, D.grads(x, w, dy, y64)


def assert_exact(r, y64, want, names=("g", "dw", "db", "dx")):
    assert torch.equal(r["y"] > 0, y64 > 0)
    for name in names:
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ"


@pytest.mark.parametrize("index", range(len(D.CASES)), ids=lambda i: D.case_id(D.CASES[i]))
def test_exact(index):
    """Integer operands: dW and db have ONE right value and dx is that integer rounded once to bf16 - torch.equal.  Run under both
    poisons with NaN-filled outputs and on plain zero-filled allocations: the same bits; the NaN channels beside a dx view stay."""
    case = D.CASES[index]
    (x, w, b, dy), y64, want = exact_reference(index)
    runs = [run_guarded(case, x, w, b, dy, poison) for poison in G.POISONS]
    assert_exact(runs[0], y64, want)
    assert want["dw"].any() and want["db"].any() and want["dx"].any()
    assert same_bits(*runs) and same_bits(runs[0], device_chain(G.Plain(DEV), case, x, w, b, dy, fill=0.0))


@pytest.mark.parametrize("index", range(len(D.CASES)), ids=lambda i: D.case_id(D.CASES[i]))
def test_random_within_bounds(index):
    """Random operands against the restatement, once per poison; the two runs are bit-equal (no atomics, nothing read before it is
    written)."""
    case = D.CASES[index]
    x, w, b, dy = D.random_operands(case)
    runs = [run_guarded(case, x, w, b, dy, poison) for poison in G.POISONS]
    assert same_bits(*runs)
    r = runs[0]
    want = D.grads(x, w, dy, r["y"])
    assert torch.equal(r["g"], want["g"])                                                        # one fp32 multiply, one RNE: exact
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  dx=B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    same = float((r["dx"] == want["dx"]).double().mean())
    print(f"conv_down_bwd {D.case_id(case)}: largest error / bound  dW {ratios['dw']:.4f}  db {ratios['db']:.4f}  dx {ratios['dx']:.4f}"
          f"  (dx == bf16_rne(S) on {100 * same:.2f} % of the elements)")
    assert 0.15 < float((r["y"] <= 0).double().mean()) < 0.85 and want["dw"].any()
    for name, v in ratios.items():
        assert v <= 1.0, f"{name}: error / bound = {v}"


def test_split_case_without_bias_and_under_other_cu_shares():
    """The 1024-output-pixel case: with dbias == NULL dW has the bits of the run with a bias gradient - and the exact value - and the
    workspace behind the splits' partial dW matrices keeps its NaN fill; under 8 and 64 compute units the integer sums are what they are
    under 256, and the old share comes back."""
    index = D.SPLIT_CASE
    case = D.CASES[index]
    n, h, wd, cin, cout, view = case
    (x, w, b, dy), y64, want = exact_reference(index)
    r = run_guarded(case, x, w, b, dy, G.POISONS[0], want_db=False)
    assert_exact(r, y64, want, ("g", "dw", "dx"))
    with_db = device_chain(G.Plain(DEV), case, x, w, b, dy)
    assert torch.equal(r["raw"][1], with_db["raw"][1]) and torch.equal(with_db["db"], want["db"])
    splits = 2
    assert f"splits {splits};" in K.conv2d_down_bwd_pick(D.fwd_desc(case))
    used = splits * cout * 9 * cin
    assert r["ws"].numel() == used + splits * cout
    nan_bits = torch.full((), NAN, dtype=F32).view(torch.int32)
    assert bool((r["ws"][used:] == nan_bits).all()), "the dbias == NULL launch wrote partial db rows"
    assert not bool((r["ws"][:used] == nan_bits).any()) and not bool((with_db["ws"] == nan_bits).any())
    for cus in D.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            r = run_guarded(case, x, w, b, dy, G.POISONS[0])
        finally:
            K.set_launch_cus(old)
        assert old == 256
        assert_exact(r, y64, want)


def test_exact_under_shares_that_change_the_split():
    """D.CU_CASE (5120 output pixels): ten splits at 256 and 64 compute units, eight at 8 - other grids, other partial sums, the same
    integers; the workspace is re-queried after each change (device_chain does) and the old share comes back."""
    case = D.CU_CASE
    n, h, wd, cin, cout, view = case
    x, w, b, dy = D.exact_operands(case)
    y64 = D.forward(x, w, b)
    want = D.grads(x, w, dy, y64)
    assert_exact(run_guarded(case, x, w, b, dy, G.POISONS[0]), y64, want)
    for cus in D.CU_SHARES:
        old = K.set_launch_cus(cus)
        try:
            assert f"splits {D.CU_CASE_SPLITS[cus]};" in K.conv2d_down_bwd_pick(D.fwd_desc(case))
            r = run_guarded(case, x, w, b, dy, G.POISONS[0])
        finally:
            K.set_launch_cus(old)
        assert old == 256 and r["ws"].numel() == D.CU_CASE_SPLITS[cus] * cout * (9 * cin + 1)
        assert_exact(r, y64, want)


# ---- the ops -------------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def test_down_block_contract():
    """down_block: the forward is the stride-2 launch; under no_grad there is no grad_fn; .backward() gives the kernels' gradients bit for
    bit; a weight-only backward leaves x.grad None and gives the same dW bits; a float32 NCHW x gets a float32 gradient; a second
    derivative raises."""
    index = 1
    case = D.CASES[index]
    n, h, wd, cin, cout, view = case
    x, w, b, dy = D.random_operands(case)
    chain = device_chain(G.Plain(DEV), case, x, w, b, dy)
    xd = _cl(x.to(BF16).to(DEV))
    wd_, bd = w.to(F32).to(DEV), b.to(F32).to(DEV)
    dyd = _cl(dy.to(BF16).to(DEV))
    plain = down_block(xd, wd_, bd)
    assert plain.grad_fn is None and plain.dtype == BF16 and tuple(plain.shape) == (n, cout) + D.out_hw(h, wd)
    assert torch.equal(plain.cpu().to(F64), chain["y"])
    wp = torch.nn.Parameter(wd_.clone())
    with torch.no_grad():
        assert down_block(xd, wp, bd).grad_fn is None
    # everything requires grad
    xr, bp = xd.clone().requires_grad_(), torch.nn.Parameter(bd.clone())
    out = down_block(xr, wp, bp)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    out.backward(dyd)
    torch.cuda.synchronize()
    assert xr.grad.dtype == BF16 and wp.grad.dtype == F32 and bp.grad.dtype == F32 and xr.grad.shape == xr.shape
    assert torch.equal(xr.grad.cpu().to(F64), chain["dx"]) and torch.equal(wp.grad.cpu().to(F64), chain["dw"])
    assert torch.equal(bp.grad.cpu().to(F64), chain["db"]) and chain["dx"].any() and chain["dw"].any()
    # only the weight
    wp2 = torch.nn.Parameter(wd_.clone())
    x2 = xd.clone()
    down_block(x2, wp2, bd).backward(dyd)
    assert x2.grad is None and bd.grad is None and torch.equal(bits(wp2.grad), bits(wp.grad))
    # only x; float32 NCHW-contiguous x: a float32 gradient of its own layout, the bf16 gradient widened
    x32 = x.to(F32).to(DEV).contiguous().requires_grad_()
    down_block(x32, wd_, bd).backward(dyd)
    assert x32.grad.dtype == F32 and x32.grad.is_contiguous() and torch.equal(x32.grad, xr.grad.float())
    # act none, no bias
    xn = xd.clone().requires_grad_()
    on = down_block(xn, wd_, act="none")
    on.backward(dyd)
    want = D.grads(x, w, dy, None, "none")
    assert B.ratio(xn.grad.cpu(), want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])) <= 1.0
    # a double backward raises
    scale = torch.tensor(2.0, device=DEV, requires_grad=True)
    xr2 = xd.clone().requires_grad_()
    g1, = torch.autograd.grad((down_block(xr2, wp, bd).float() * scale).sum(), xr2, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g1.float().sum().backward()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        down_block(xd.cpu(), wd_.cpu())


def test_down_bn_block_contract():
    """down_bn_block: training=False is bit-equal to down_block on torch-folded weights and leaves the running tensors; under no_grad
    there is no grad_fn and the running statistics after two calls are the restatement applied twice; a weight-only backward leaves
    x.grad None and gives the bits of the full backward's dW, which are the strided kernel's on the batch norm's g."""
    gen = torch.Generator().manual_seed(17)
    x = _cl(torch.randn((2, 16, 7, 10), generator=gen).to(BF16).to(DEV))
    w = (torch.randn((24, 16, 3, 3), generator=gen) / 12).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(24, generator=gen)).to(DEV), (0.5 * torch.randn(24, generator=gen)).to(DEV)
    rm0, rv0 = torch.randn(24, generator=gen).to(DEV), (0.5 + torch.rand(24, generator=gen)).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    y = down_bn_block(x, w, gamma, beta, rm, rv, training=False)
    assert y.grad_fn is None and y.dtype == BF16 and y.shape == (2, 24, 4, 5) and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    s = gamma / torch.sqrt(rv + N.EPS)
    assert torch.equal(bits(y), bits(down_block(x, w * s.reshape(-1, 1, 1, 1), beta - rm * s))) and bool(y.any())
    wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (w, gamma, beta))
    with torch.no_grad():
        y1 = down_bn_block(x, wp, gp, bp, rm, rv)
        z = down_block(x, w, act="none").permute(0, 2, 3, 1).float().cpu().reshape(-1, 24).numpy()
        y2 = down_bn_block(x, wp, gp, bp, rm, rv)
    assert y1.grad_fn is None and torch.equal(y1, y2) and z.shape[0] == 2 * 4 * 5
    st = N.stats(z, gamma.cpu().numpy(), beta.cpu().numpy(), rm=rm0.cpu().numpy(), rv=rv0.cpu().numpy())
    assert np.array_equal(y1.permute(0, 2, 3, 1).float().cpu().reshape(-1, 24).numpy(), N.forward(z, st["saved"]))
    st = N.stats(z, gamma.cpu().numpy(), beta.cpu().numpy(), rm=st["rm"], rv=st["rv"])
    assert np.array_equal(rm.cpu().numpy(), st["rm"]) and np.array_equal(rv.cpu().numpy(), st["rv"])
    xg = x.clone().requires_grad_()
    out = down_bn_block(xg, wp, gamma, beta)
    assert out.grad_fn is not None
    out.float().sum().backward(inputs=[wp], retain_graph=True)
    assert xg.grad is None and wp.grad is not None and wp.grad.dtype == F32 and gp.grad is None
    gx_full, gw_full = torch.autograd.grad(out.float().square().sum(), [xg, wp], retain_graph=True)
    wp.grad = None
    out.float().square().sum().backward(inputs=[wp], retain_graph=True)
    assert torch.equal(bits(gw_full), bits(wp.grad)) and bool(gw_full.any()) and bool(gx_full.any()) and gx_full.dtype == BF16
    out2 = down_bn_block(x, w, gp, bp, rm, rv)
    out2.float().square().sum().backward()
    assert gp.grad is not None and bp.grad is not None and bool(gp.grad.any()) and bool(bp.grad.any())
    with pytest.raises(ValueError, match="more than 1 value"):
        down_bn_block(x[:1, :, :2, :2], w, gamma, beta)


# ---- the chain (tests/_conv_down.py) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference():
    ops = D.chain_operands()
    return ops, D.chain_autograd64(ops), D.chain_restated(ops)


def run_chain(ops):
    x0 = _cl(ops["x0"].to(BF16).to(DEV)).requires_grad_()
    par = lambda t: torch.nn.Parameter(t.to(F32).to(DEV))
    W, ga, be = [par(t) for t in ops["W"]], [par(t) for t in ops["gamma"]], [par(t) for t in ops["beta"]]
    wh, bh = par(ops["Wh"]), par(ops["bh"])
    calls = [dict() for _ in D.CHAIN_BN]
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))

    def layer(i, x):
        cin, cout, k, stride = D.CHAIN_BN[i]
        alias = x.view_as(x)
        alias.register_hook(keep(calls[i], "dx"))
        y = (down_bn_block if stride == 2 else conv_bn_block)(alias, W[i], ga[i], be[i])
        y.register_hook(keep(calls[i], "dy"))
        calls[i].update(x=alias.detach(), y=y.detach())
        return y
    u = layer(1, layer(0, x0))
    r = u + layer(3, layer(2, u))
    v = layer(4, r)
    h = conv_block(v, wh, bh, act="none", out_dtype=F32)
    (h * ops["R"].to(F32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = dict(Wh=wh.grad, bh=bh.grad)
    for i in range(5):
        grads[f"W{i + 1}"], grads[f"gamma{i + 1}"], grads[f"beta{i + 1}"] = W[i].grad, ga[i].grad, be[i].grad
    return dict(calls=calls, grads=grads, x0_grad=x0.grad)


@functools.lru_cache(maxsize=None)
def chain_on_device():
    return run_chain(chain_reference()[0])


def test_chain_layer_by_layer():
    """conv_bn_block 3x3 8 -> 16, down_bn_block 16 -> 32, a residual unit (1x1 32 -> 16, 3x3 16 -> 32, torch's add), down_bn_block
    32 -> 64 and an fp32 head on a 2 x 16 x 20 input.  Each call against the restatement fed with the device's own x and dy: z and saved
    are the forward's launches repeated on the same tensors, y and g are bit-equal, dgamma / dbeta and the conv's dW / dx within their
    bounds; u's gradient is torch's bf16 sum of its two consumers'.  A second run of the chain gives the same bits."""
    ops = chain_reference()[0]
    run = chain_on_device()
    for i, (c, (cin, cout, k, stride)) in enumerate(zip(run["calls"], D.CHAIN_BN)):
        with torch.no_grad():
            w_dev = ops["W"][i].to(F32).to(DEV)
            z = (down_block(c["x"], w_dev, act="none") if stride == 2 else conv_block(c["x"], w_dev, act="none")).permute(0, 2, 3, 1).contiguous()
        n, ho, wo, _ = z.shape
        m = n * ho * wo
        t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        gamma, beta = ops["gamma"][i].to(F32).numpy(), ops["beta"][i].to(F32).numpy()
        saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
        ws = torch.full((K.bn_workspace_bytes(m, cout) // 4,), NAN, dtype=F32, device=DEV)
        K.bn_train_stats(z, t32(gamma).to(DEV), t32(beta).to(DEV), N.EPS, N.MOMENTUM, None, None, saved, ws)
        zr, sv = z.float().cpu().reshape(m, cout).numpy(), saved.cpu().numpy()
        assert c["dy"].dtype == BF16 and c["dx"].dtype == BF16 and c["dx"].shape == c["x"].shape
        assert np.array_equal(c["y"].permute(0, 2, 3, 1).float().cpu().reshape(m, cout).numpy(), N.forward(zr, sv)), "y"
        dy = c["dy"].permute(0, 2, 3, 1).contiguous()
        g = torch.full((n, ho, wo, cout), NAN, dtype=BF16, device=DEV)
        K.bn_act_bwd(dy, z, saved, _lib.ACT_LEAKY01, True, g, None, None, ws)
        c12 = ws[:2 * cout].cpu().reshape(2, cout).numpy()
        tr = N.backward_terms(dy.float().cpu().reshape(m, cout).numpy(), zr, sv)
        assert np.array_equal(g.float().cpu().reshape(m, cout).numpy(), N.backward_apply(tr, sv, c12[0], c12[1])), "g"
        assert 0.15 < tr["nonpositive"] < 0.85
        conv = D.conv_grads(i, c["x"].cpu().to(F64), ops["W"][i], g.permute(0, 3, 1, 2).cpu().to(F64))
        gr = run["grads"]
        ratios = dict(dgamma=N.ratio(gr[f"gamma{i + 1}"].cpu().numpy(), tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])),
                      dbeta=N.ratio(gr[f"beta{i + 1}"].cpu().numpy(), tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])),
                      dW=B.ratio(gr[f"W{i + 1}"].cpu(), conv["dw"], B.bound_sum(conv["dw_terms"], conv["dw_abs"])),
                      dx=B.ratio(c["dx"].cpu(), conv["dx_sum"], B.bound_dx(conv["dx_sum"], conv["dx_terms"], conv["dx_abs"])))
        print(f"down chain layer {i + 1} ({cin} -> {cout}, k{k}, stride {stride}): largest error / bound  "
              + "  ".join(f"{k_} {v:.4f}" for k_, v in ratios.items()))
        for name, v in ratios.items():
            assert v <= 1.0, (i, name, v)
    calls = run["calls"]
    assert torch.equal(calls[0]["dy"], calls[1]["dx"]) and torch.equal(run["x0_grad"], calls[0]["dx"])
    assert torch.equal(calls[3]["dy"], calls[4]["dx"]) and torch.equal(calls[2]["dy"], calls[3]["dx"])
    assert torch.equal(calls[1]["dy"], calls[4]["dx"] + calls[2]["dx"]) and not torch.equal(calls[1]["dy"], calls[4]["dx"])
    again = run_chain(ops)
    for name, t in run["grads"].items():
        assert torch.equal(bits(t), bits(again["grads"][name])), name
    assert torch.equal(bits(run["x0_grad"]), bits(again["x0_grad"]))


def test_chain_vs_float64_autograd():
    """The chain's parameter gradients against float64 autograd of the same network without any rounding, by relative L2 error; the
    yardstick is the float64 chain WITH every rounding point (tests/test_conv_down_cpu.py keeps it equal to autograd with the rounding
    off).  The device shares the rounding points and has to stay within 1.5 x the yardstick, the rule of the conv_block and
    conv_bn_block chain tests."""
    ops, want, cpu = chain_reference()
    run = chain_on_device()
    rows = []
    for name in D.CHAIN_PARAMS:
        rows.append((name, B.rel_l2(run["grads"][name].cpu(), want[name]), B.rel_l2(cpu[name], want[name])))
        print("down chain vs float64 autograd, relative L2 of d%s: device %.4e  float64 chain with the rounding points %.4e" % rows[-1]
              + "  device / chain %.5f" % (rows[-1][1] / rows[-1][2]))
    for name, e_dev, e_cpu in rows:
        assert e_cpu > 0 and e_dev <= 1.5 * e_cpu, (name, e_dev, e_cpu)
