"""GPU tests of the conv backward (csrc/conv_bwd.hip through pytorch_yolo_amd.kernels and pytorch_yolo_amd.ops.conv_block) against the
float64 restatement of tests/_conv_bwd.py.

Every case runs the whole chain on the device - device weight pack, the FORWARD (yolo_conv2d_fwd), prepare (g), weight / bias gradient,
transposed pack, data gradient - with every operand, g, the workspace, dW, db and dx between the poisoned bands of tests/_guard.py and
the outputs and the workspace pre-filled with NaN.  The slope of LeakyReLU is taken from the y the device's forward wrote.

Exact cases (integer operands, tests/_conv_bwd.exact_operands): torch.equal.  Random cases: per element
    |dW - S| <= 2 T 2^-24 A,   |db - S| <= 2 T 2^-24 A,   |dx - S| <= 2^-8 |S| + 2 T 2^-24 A
(T in-bounds terms, S the float64 sum, A the float64 sum of |terms|); each test prints its largest error / bound ratio.

Measured on an MI355X, largest error / bound over the eight cases: dW 0.0335 (the one-row map; 0.0000-0.0179 elsewhere), db 0.0003,
dx 0.98 - dx is one RNE away from its fp32 sum and half a bf16 spacing IS 2^-8 |S| right above a power of two, so the dx ratio reaches
~1 by construction of the bound; dx == bf16_rne(S) on 99.98-100 % of the elements.  End to end: dW 0.0586, db 0.0000."""
import pytest
import torch

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


def device_chain(a, case, x, w, b, dy, fill=NAN):
    """The whole chain of one case on allocations of ``a`` (a _guard.Guard or _guard.Plain); float64 NCHW results on the host, the dx
    buffer's channels outside the view as raw bits."""
    n, h, wd, cin, cout, k, act, dt, view = case
    total, off = view or (cin, 0)
    d = B.fwd_desc(case)
    cg, ct = K.roundup(cout, 8), d.out_c_total
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
    db = a.alloc("db", (cout,), F32, fill)
    K.conv2d_bwd_weight(xbuf, g, dw, db, ws, d)
    packed_t = a.alloc("w_packed_t", (K.roundup(cin, 128), K.roundup(k * k * cg, 64)), BF16, fill)
    K.pack_conv_weight_dev(w_dev, cg, transposed=True, out=packed_t)
    dxbuf = a.alloc("dx", (n, h, wd, total), BF16, NAN)
    K.conv2d_bwd_data(g, packed_t, dxbuf, d)
    torch.cuda.synchronize()
    outside = torch.cat([dxbuf[..., :off], dxbuf[..., off + cin:]], -1).cpu().view(torch.int16)
    assert torch.equal(xbuf[..., off:off + cin].cpu(), nhwc(x, BF16))                              # the operands are read-only
    return dict(y=nchw64(ybuf[..., :cout].cpu()), g=nchw64(g[..., :cout].cpu()), g_pad=g[..., cout:].cpu(), dw=dw.cpu().to(F64),
                db=db.cpu().to(F64), dx=nchw64(dxbuf[..., off:off + cin].cpu()), dx_outside=outside,
                raw=[t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32) for t in (g, dw, db, dxbuf[..., off:off + cin])])


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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    n, h, wd, cin, cout, k, act, dt, view = case
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
    # only x requires grad
    xr = xd.clone().requires_grad_()
    gx, = torch.autograd.grad(conv_block(xr, wd_, bd), xr, _cl(dy.to(BF16).to(DEV)))
    assert gx.dtype == BF16 and gx.shape == xr.shape
    # only the bias requires grad
    bp = torch.nn.Parameter(bd.clone())
    gb, = torch.autograd.grad(conv_block(xd, wd_, bp), bp, _cl(dy.to(BF16).to(DEV)))
    assert gb.dtype == F32 and gb.shape == bp.shape
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
    # 12 input channels are zero-padded to 16 by torch: gradients of the 12-channel shapes
    x12 = xd[:, :12].float().contiguous().requires_grad_()
    w12 = torch.nn.Parameter(wd_[:, :12].clone())
    conv_block(x12, w12, bd).backward(_cl(dy.to(BF16).to(DEV)))
    assert x12.grad.shape == x12.shape and w12.grad.shape == w12.shape and bool(w12.grad.any())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv_block(xd.cpu(), wd_.cpu())


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
