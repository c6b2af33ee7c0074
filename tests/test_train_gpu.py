"""GPU tests of the training-mode forward and backward of YOLOv3 / YOLOv3-SPP: the glue kernels of csrc/route.hip and
yolo_bn_act_add_fwd bit for bit against the restatements of tests/_train.py, the three new ops' contracts, shallow chains against float64
autograd, and the whole models - layer by layer from the device's own tensors, and as a training step.

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs are NaN / 0xAA filled; the 0xFF and the 0x7F
run give equal bits, and so does a second run.

Whole models: these deep random-weight, batch-statistics networks are chaotic (rounding only the conv weights to bf16 moves p by 13-29 %
relative L2), so no end-to-end tolerance is asserted.  Correctness rests on (1) the wiring leg of tests/test_train_cpu.py, (2) every op
call of one device step re-run on its restatement from the device's own inputs - the conv / batch-norm ops within the bounds of their own
tests, the glue bit-equal -, (3) the chains, where conditioning is sound: the device's gradient error against float64 autograd within
1.5 x that of the float64 chain with the rounding points.

Measured on an MI355X.  Chains, device / yardstick quotients: (a) 0.99424-1.02435 (errors 1.5e-3 to 1.2e-1; equal to
five digits from the second residual unit on), (b) and (c) 1.00000 throughout.  Layer by layer, largest error / bound over all op calls:
YOLOv3-SPP (79 calls) dW 0.2751, dbeta 0.9984, dgamma 0.9988, dx 0.9950; YOLOv3 (77 calls) dW 0.2558, dbeta 1.0000, dgamma 0.9886, dx
0.9938, plain heads dW 0.0494, db 0.0000, dx 0.9893.  Reported, not gated, relative L2 against the float64 reference: YOLOv3-SPP p 0.267,
0.416, 0.694 (the CPU model with every rounding point: 0.251, 0.423, 0.708), head conv weights 0.556, 0.795, 1.152, head BN weights 0.045,
0.069, 0.029; YOLOv3 p 0.099, 0.289, 0.561, plain-head weights 0.060, 0.075, the ConvBlock head's conv weight 0.947."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bn as N
import _conv_bwd as B
import _conv_down as D
import _guard as G
import _loss as L
import _train as T
import helpers
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
FIVE = np.array([-1.5, -0.25, 0.0, 0.4375, 2.0], dtype=np.float32)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def f32np(t):
    return t.detach().float().cpu().contiguous().numpy()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.uint8)


def tied(shape, seed):
    return FIVE[np.random.default_rng(seed).integers(0, 5, shape)]


def randbf(shape, seed):
    return N.bf16(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def both_poisons(run):
    """run(allocator) -> dict of output tensors: under both poisons, twice under the first; all bit-equal; margins intact.  Returns the
    first run's outputs."""
    outs = []
    for poison in G.POISONS + (G.POISONS[0],):
        a = G.Guard(poison, DEV)
        out = run(a)
        torch.cuda.synchronize()
        a.assert_intact()
        outs.append(out)
    for other in outs[1:]:
        for name, t in outs[0].items():
            assert torch.equal(bits(t), bits(other[name])), name
    return outs[0]


# ---- the kernels, bit for bit -------------------------------------------------------------------------------------------------------------
# 2x3: smaller than every window; 7x5: odd, partly smaller; 20x20: the SPP map of a 640 input; c = 72: nine chunks; 40x40 and 41x40: the
# two sides of the LDS threshold (1600 pixels)
SPP_CASES = [(2, 2, 3, 8), (1, 7, 5, 8), (1, 20, 20, 8), (2, 7, 5, 72), (1, 40, 40, 8), (1, 41, 40, 8)]


@pytest.mark.parametrize("case", SPP_CASES, ids=lambda s: "%dx%dx%d_c%d" % s)
def test_spp_kernels_equal_the_restatement(case):
    n, h, w, c = case
    x, dy = tied(case, 11), randbf((n, h, w, 4 * c), 12)
    dy[..., :c] = tied((n, h, w, c), 13)                                       # tied gradients too in the first slice
    want_y, want_idx = T.spp_forward(x)
    want_dx = T.spp_backward(dy, want_idx)

    def run(a):
        xd, dyd = a.like("x", t32(x).to(BF16)), a.like("dy", t32(dy).to(BF16))
        y, dx = a.alloc("y", (n, h, w, 4 * c), BF16, NAN), a.alloc("dx", (n, h, w, c), BF16, NAN)
        idx = a.alloc("idx", (n, h, w, 3 * c), torch.uint8, 0xAA)
        K.spp_train_fwd(xd, y, idx)
        K.spp_bwd(dyd, idx, dx)
        return dict(y=y, idx=idx, dx=dx)

    out = both_poisons(run)
    assert np.array_equal(f32np(out["y"]), want_y) and np.array_equal(out["idx"].cpu().numpy(), want_idx)
    assert np.array_equal(f32np(out["dx"]), want_dx)
    assert want_dx.any() and len(np.unique(want_idx)) > 3


def test_upsample_concat_kernels_equal_the_restatement():
    n, h, w, ca, cb = 2, 3, 5, 8, 24
    a_, b_, dy = tied((n, h, w, ca), 21), tied((n, 2 * h, 2 * w, cb), 22), randbf((n, 2 * h, 2 * w, ca + cb), 23)
    want_da, want_db = T.upcat_backward(dy, ca)

    def run(a):
        ad, bd, dyd = a.like("a", t32(a_).to(BF16)), a.like("b", t32(b_).to(BF16)), a.like("dy", t32(dy).to(BF16))
        y = a.alloc("y", (n, 2 * h, 2 * w, ca + cb), BF16, NAN)
        da, db = a.alloc("da", (n, h, w, ca), BF16, NAN), a.alloc("db", (n, 2 * h, 2 * w, cb), BF16, NAN)
        da1, db1 = a.alloc("da1", (n, h, w, ca), BF16, NAN), a.alloc("db1", (n, 2 * h, 2 * w, cb), BF16, NAN)
        K.upsample2_concat_fwd(ad, bd, y)
        K.upsample2_concat_bwd(dyd, da, db, n=n, h=h, w=w, ca=ca, cb=cb)
        K.upsample2_concat_bwd(dyd, da1, None, n=n, h=h, w=w, ca=ca, cb=cb)             # each gradient alone
        K.upsample2_concat_bwd(dyd, None, db1, n=n, h=h, w=w, ca=ca, cb=cb)
        return dict(y=y, da=da, db=db, da1=da1, db1=db1)

    out = both_poisons(run)
    assert np.array_equal(f32np(out["y"]), T.upcat_forward(a_, b_))
    assert np.array_equal(f32np(out["da"]), want_da) and np.array_equal(f32np(out["db"]), want_db)
    assert torch.equal(bits(out["da"]), bits(out["da1"])) and torch.equal(bits(out["db"]), bits(out["db1"]))
    assert float(np.mean(N.bf16(want_da) != T.upcat_backward(dy, ca, rounding=False)[0])) > 0.2      # the one rounding is exercised


@pytest.mark.parametrize("preadd", [False, True], ids=["y", "y_and_preadd"])
@pytest.mark.parametrize("c", [8, 72])
def test_bn_act_add_equals_the_restatement(c, preadd):
    case = (1, 5, 7, c)                                                        # 35 pixels: an odd count
    z, _, gamma, beta, rm, rv = N.random_operands(case)
    res = randbf(z.shape, 31)
    saved = N.stats(z, gamma, beta)["saved"]
    want_y, want_pre = T.bn_act_add(z, saved, res)

    def run(a):
        zd, rd = a.like("z", t32(z).to(BF16).reshape(case)), a.like("residual", t32(res).to(BF16).reshape(case))
        sd = a.like("saved", t32(saved))
        y = a.alloc("y", case, BF16, NAN)
        pre = a.alloc("y_preadd", case, BF16, NAN) if preadd else None
        K.bn_act_add_fwd(zd, sd, rd, y, pre, _lib.ACT_LEAKY01)
        return dict(y=y, **(dict(pre=pre) if preadd else {}))

    out = both_poisons(run)
    assert np.array_equal(f32np(out["y"]).reshape(-1, c), want_y)
    if preadd:
        assert np.array_equal(f32np(out["pre"]).reshape(-1, c), want_pre)
        assert np.array_equal(want_pre, N.forward(z, saved))                   # y_preadd is yolo_bn_act_fwd's y
    assert not np.array_equal(want_y, N.bf16(want_pre + res))                  # ... and y is not the rounded y_preadd plus the residual


# ---- op contracts -------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _res_operands(seed=41):
    gen = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn((2, 8, 5, 7), generator=gen).to(BF16).to(DEV))
    res = _cl(torch.randn((2, 16, 5, 7), generator=gen).to(BF16).to(DEV))
    w = (torch.randn((16, 8, 3, 3), generator=gen) / 8.5).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(16, generator=gen)).to(DEV), (0.5 * torch.randn(16, generator=gen)).to(DEV)
    return x, res, w, gamma, beta


def test_res_bn_block_contract():
    """y and y_preadd of res_bn_block are conv_bn_block's y plus the residual, rounded once from fp32, and conv_bn_block's y; both carry
    gradients; the residual's gradient is dy itself; a gradient is computed only where asked; running statistics move; no_grad gives no
    grad_fn; a second derivative raises."""
    x, res, w, gamma, beta = _res_operands()
    rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    with torch.no_grad():
        y0 = Y.conv_bn_block(x, w, gamma, beta)
        y, pre = Y.res_bn_block(x, w, gamma, beta, rm, rv, res, want_preadd=True)
        only_y = Y.res_bn_block(x, w, gamma, beta, None, None, res)
    assert y.grad_fn is None and torch.equal(pre, y0) and torch.equal(only_y, y) and y.dtype == BF16
    assert y.permute(0, 2, 3, 1).is_contiguous() and pre.permute(0, 2, 3, 1).is_contiguous()
    assert bool((rm != 0).all()) and bool((rv != 1).all())
    # both gradient paths
    xg, rg = x.clone().requires_grad_(), res.clone().requires_grad_()
    wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (w, gamma, beta))
    y, pre = Y.res_bn_block(xg, wp, gp, bp, None, None, rg, want_preadd=True)
    r1, r2 = torch.randn_like(y), torch.randn_like(pre)
    (y * r1).float().sum().backward(retain_graph=True)
    assert torch.equal(rg.grad, r1)
    g_y = [t.grad.clone() for t in (xg, wp, gp, bp)]
    for t in (xg, wp, gp, bp, rg):
        t.grad = None
    ((y * r1).float().sum() + (pre * r2).float().sum()).backward(retain_graph=True)
    assert torch.equal(rg.grad, r1)                                            # the pre-add path does not reach the residual
    assert all(not torch.equal(a, t.grad) for a, t in zip(g_y, (xg, wp, gp, bp)))
    # only where asked
    for t in (xg, wp, gp, bp, rg):
        t.grad = None
    (pre * r2).float().sum().backward(inputs=[gp], retain_graph=True)
    assert gp.grad is not None and all(t.grad is None for t in (xg, wp, bp, rg))
    y.float().sum().backward(inputs=[rg], retain_graph=True)
    assert rg.grad is not None and xg.grad is None and wp.grad is None
    with pytest.raises(RuntimeError):
        torch.autograd.grad(torch.autograd.grad(y.float().sum(), xg, create_graph=True)[0].float().sum(), xg)


def test_glue_op_contracts():
    """spp_concat / upsample_concat: shapes, layout, dtype conversion by torch, gradients only where asked, errors before any launch."""
    gen = torch.Generator().manual_seed(43)
    x = torch.randn((2, 8, 7, 5), generator=gen).to(DEV)                       # float32 NCHW: converted by torch
    y = Y.spp_concat(x.requires_grad_())
    assert y.shape == (2, 32, 7, 5) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous() and y.grad_fn is not None
    y.float().sum().backward()
    assert x.grad.dtype == F32 and x.grad.shape == x.shape
    want = torch.cat([torch.nn.functional.max_pool2d(x.detach().to(BF16).float(), k, 1, k // 2) for k in T.SPP_K] + [x.detach().to(BF16).float()], 1)
    assert torch.equal(y.detach().float(), want)
    with torch.no_grad():
        assert Y.spp_concat(x).grad_fn is None
    a = _cl(torch.randn((2, 8, 3, 5), generator=gen).to(BF16).to(DEV)).requires_grad_()
    b = _cl(torch.randn((2, 24, 6, 10), generator=gen).to(BF16).to(DEV)).requires_grad_()
    u = Y.upsample_concat(a, b)
    assert u.shape == (2, 32, 6, 10) and u.dtype == BF16 and u.permute(0, 2, 3, 1).is_contiguous()
    r = torch.randn_like(u)
    (u * r).float().sum().backward(inputs=[b], retain_graph=True)
    assert a.grad is None and torch.equal(b.grad, r[:, 8:])
    (u * r).float().sum().backward(inputs=[a])
    assert a.grad is not None and a.grad.dtype == BF16 and a.grad.shape == a.shape
    for call in (lambda: Y.spp_concat(x[:, :4]), lambda: Y.upsample_concat(a, b[:, :, :5]), lambda: Y.upsample_concat(a[:, :4], b)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Y.spp_concat(x.detach().cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        xc, rc, wc, gc, bc = (t.cpu() for t in _res_operands())
        Y.res_bn_block(xc, wc, gc, bc, None, None, rc)


# ---- shallow chains against float64 autograd ----------------------------------------------------------------------------------------------
def _leaf(gen, *shape, scale=1.0, offset=0.0):
    return (offset + scale * torch.randn(shape, generator=gen)).to(F32).to(F64)


def _bn_params(gen, name, cin, cout, k, out):
    out[f"W{name}"] = _leaf(gen, cout, cin, k, k, scale=(cin * k * k) ** -0.5)
    out[f"gamma{name}"] = _leaf(gen, cout, scale=0.25, offset=1.0)
    out[f"beta{name}"] = _leaf(gen, cout, scale=0.5)


def _bn(ops, fn, x, p, name, *extra, **kw):
    return getattr(ops, fn)(x, p[f"W{name}"], p[f"gamma{name}"], p[f"beta{name}"], None, None, *extra, **kw)


def _head(ops, x, p, name, r):
    return (ops.conv_block(x, p[f"W{name}"], p[f"b{name}"], act="none", out_dtype=F32) * r).sum()


def chain_a():
    """down_bn_block, then two residual units, the second with its pre-add output routed to a head of its own."""
    gen, p = torch.Generator().manual_seed(8100), {}
    x0 = torch.randn((2, 8, 12, 20), generator=gen).to(BF16).to(F64)
    _bn_params(gen, "d", 8, 16, 3, p)
    for u in ("1", "2"):
        _bn_params(gen, u + "s", 16, 8, 1, p), _bn_params(gen, u + "e", 8, 16, 3, p)
    for hname in ("y", "p"):
        p["W" + hname], p["b" + hname] = _leaf(gen, 21, 16, 1, 1, scale=0.25), _leaf(gen, 21, scale=0.5)
    ry, rp = _leaf(gen, 2, 21, 6, 10), _leaf(gen, 2, 21, 6, 10)

    def run(ops, p, cast):
        x = _bn(ops, "down_bn_block", cast(x0), p, "d")
        x = _bn(ops, "res_bn_block", _bn(ops, "conv_bn_block", x, p, "1s"), p, "1e", x)
        y, pre = _bn(ops, "res_bn_block", _bn(ops, "conv_bn_block", x, p, "2s"), p, "2e", x, want_preadd=True)
        return _head(ops, y, p, "y", cast(ry)) + _head(ops, pre, p, "p", cast(rp))
    return p, run


def chain_b():
    """conv_bn_block -> spp_concat -> conv_bn_block -> head, on a 7x5 map (smaller than the 9 and 13 windows)."""
    gen, p = torch.Generator().manual_seed(8200), {}
    x0 = torch.randn((2, 8, 7, 5), generator=gen).to(BF16).to(F64)
    _bn_params(gen, "1", 8, 16, 3, p), _bn_params(gen, "2", 64, 16, 1, p)
    p["Wh"], p["bh"] = _leaf(gen, 21, 16, 1, 1, scale=0.25), _leaf(gen, 21, scale=0.5)
    r = _leaf(gen, 2, 21, 7, 5)

    def run(ops, p, cast):
        x = ops.spp_concat(_bn(ops, "conv_bn_block", cast(x0), p, "1"))
        return _head(ops, _bn(ops, "conv_bn_block", x, p, "2"), p, "h", cast(r))
    return p, run


def chain_c():
    """conv_bn_block -> upsample_concat with a routed tensor (a conv_bn_block of its own) -> conv_bn_block -> head."""
    gen, p = torch.Generator().manual_seed(8300), {}
    a0 = torch.randn((2, 8, 3, 5), generator=gen).to(BF16).to(F64)
    r0 = torch.randn((2, 8, 6, 10), generator=gen).to(BF16).to(F64)
    _bn_params(gen, "a", 8, 16, 1, p), _bn_params(gen, "r", 8, 24, 3, p), _bn_params(gen, "2", 40, 16, 3, p)
    p["Wh"], p["bh"] = _leaf(gen, 21, 16, 1, 1, scale=0.25), _leaf(gen, 21, scale=0.5)
    r = _leaf(gen, 2, 21, 6, 10)

    def run(ops, p, cast):
        x = ops.upsample_concat(_bn(ops, "conv_bn_block", cast(a0), p, "a"), _bn(ops, "conv_bn_block", cast(r0), p, "r"))
        return _head(ops, _bn(ops, "conv_bn_block", x, p, "2"), p, "h", cast(r))
    return p, run


def chain_grads(make, ops, device):
    params, run = make()
    if device:
        p = {k: torch.nn.Parameter(v.to(F32).to(DEV)) for k, v in params.items()}
        cast = lambda t: t.to(F32).to(DEV)
    else:
        p = {k: v.clone().requires_grad_() for k, v in params.items()}
        cast = lambda t: t
    run(ops, p, cast).backward()
    return {k: v.grad.detach().cpu().to(F64) for k, v in p.items()}


@pytest.mark.parametrize("make", [chain_a, chain_b, chain_c], ids=["a_down_two_units_preadd", "b_spp", "c_upsample_concat"])
def test_chain_vs_float64_autograd(make):
    """The parameter gradients of a chain on the device against the same chain in float64 without any rounding, by relative L2 error; the
    yardstick is the float64 chain with every rounding point (tests/_train.cpu_ops(True)).  The device shares the rounding points and has
    to stay within 1.5 x the yardstick, the rule of the conv_block, conv_bn_block and down_bn_block chain tests."""
    want = chain_grads(make, T.cpu_ops(False), False)
    cpu = chain_grads(make, T.cpu_ops(True), False)
    dev = chain_grads(make, MT.DEVICE_OPS, True)
    again = chain_grads(make, MT.DEVICE_OPS, True)
    rows = []
    for name in want:
        rows.append((name, B.rel_l2(dev[name], want[name]), B.rel_l2(cpu[name], want[name])))
        print("train chain %s vs float64, relative L2 of d%s: device %.4e  float64 chain with the rounding points %.4e  device / chain %.5f"
              % (make.__name__, name, rows[-1][1], rows[-1][2], rows[-1][1] / rows[-1][2]))
        assert torch.equal(dev[name], again[name]), name
    for name, e_dev, e_cpu in rows:
        assert e_cpu > 0 and e_dev <= 1.5 * e_cpu, (name, e_dev, e_cpu)


# ---- whole models -------------------------------------------------------------------------------------------------------------------------
def new_model(family):
    model = T.load_synthetic(getattr(Y, {"spp": "YOLOv3SPP", "yolov3": "YOLOv3"}[family])(**T.CTOR))
    model.hyper_params = dict(L.HYPER)
    return model.to(DEV).train()


def recording_ops(calls):
    """DEVICE_OPS with every call recorded: kind, the tensors that went in (activations through an alias, so that a hook sees this call's
    gradient alone), the outputs, and - after the backward - dy of every output, dx of every activation, the gradients of the vectors."""
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))

    def alias(rec, key, t):
        if t is None or not t.requires_grad:
            rec[key] = None if t is None else t.detach()
            return t
        a = t.view_as(t)
        a.register_hook(keep(rec, "d" + key))
        rec[key] = a.detach()
        return a

    def watch(rec, key, t):
        rec[key] = t.detach()
        t.register_hook(keep(rec, "d" + key))
        return t

    def params(rec, **named):
        rec["params"] = named
        for t in named.values():
            if t is not None and not t.is_leaf:
                t.retain_grad()

    def bn(kind, fn):
        def call(x, w, gamma, beta, rm=None, rv=None, residual=None, *, want_preadd=False, momentum=0.1, eps=1e-5):
            rec = dict(kind=kind, momentum=momentum, eps=eps, rm0=rm.detach().clone(), rv0=rv.detach().clone(), rm=rm, rv=rv)
            calls.append(rec)
            params(rec, w=w, gamma=gamma, beta=beta)
            x = alias(rec, "x", x)
            if kind == "res":
                out = fn(x, w, gamma, beta, rm, rv, alias(rec, "res", residual), want_preadd=want_preadd, momentum=momentum, eps=eps)
                if want_preadd:
                    return watch(rec, "y", out[0]), watch(rec, "pre", out[1])
                return watch(rec, "y", out)
            return watch(rec, "y", fn(x, w, gamma, beta, rm, rv, momentum=momentum, eps=eps))
        return call

    def conv_block(x, w, b=None, *, act="none", out_dtype=F32):
        rec = dict(kind="head")
        calls.append(rec)
        params(rec, w=w, b=b)
        return watch(rec, "y", Y.conv_block(alias(rec, "x", x), w, b, act=act, out_dtype=out_dtype))

    def spp_concat(x):
        rec = dict(kind="spp")
        calls.append(rec)
        return watch(rec, "y", Y.spp_concat(alias(rec, "x", x)))

    def upsample_concat(a, b):
        rec = dict(kind="upcat")
        calls.append(rec)
        return watch(rec, "y", Y.upsample_concat(alias(rec, "a", a), alias(rec, "b", b)))

    return SimpleNamespace(conv_block=conv_block, conv_bn_block=bn("bn", Y.conv_bn_block), down_bn_block=bn("down", Y.down_bn_block),
                           res_bn_block=bn("res", Y.res_bn_block), spp_concat=spp_concat, upsample_concat=upsample_concat)


def _rows(t):
    """NCHW-shaped device tensor -> float32 numpy [M, C]."""
    return f32np(t.permute(0, 2, 3, 1)).reshape(-1, t.shape[1])


def _nhwc(t):
    return f32np(t.permute(0, 2, 3, 1))


def check_bn_call(rec, worst):
    """One conv_bn_block / down_bn_block / res_bn_block call against the restatement fed with the device's own tensors: z and saved are
    the forward's launches repeated (two runs give the same bits); y (and y_preadd), g, the running statistics bit-equal; dgamma, dbeta,
    dW, dx within the bounds of tests/test_bn_gpu.py / test_conv_bwd_gpu.py / test_conv_down_gpu.py."""
    x, w, gamma, beta = rec["x"], rec["params"]["w"].detach(), rec["params"]["gamma"].detach(), rec["params"]["beta"].detach()
    stride = 2 if rec["kind"] == "down" else 1
    with torch.no_grad():
        z = (Y.down_block if stride == 2 else Y.conv_block)(x, w, act="none").permute(0, 2, 3, 1).contiguous()
    n, ho, wo, cout = z.shape
    m, k = n * ho * wo, w.shape[2]
    saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
    ws = torch.full((K.bn_workspace_bytes(m, cout) // 4,), NAN, dtype=F32, device=DEV)
    rm, rv = rec["rm0"].clone(), rec["rv0"].clone()
    K.bn_train_stats(z, gamma.contiguous(), beta.contiguous(), rec["eps"], rec["momentum"], rm, rv, saved, ws)
    assert torch.equal(rm, rec["rm"].detach()) and torch.equal(rv, rec["rv"].detach()), "running statistics"
    zr, sv = f32np(z).reshape(m, cout), saved.cpu().numpy()
    st = N.stats(zr, f32np(gamma), f32np(beta), rec["eps"], rec["momentum"], f32np(rec["rm0"]), f32np(rec["rv0"]))
    assert np.abs(st["rm"] - f32np(rm)).max() <= 1e-6 * max(1.0, np.abs(st["rm"]).max())
    assert np.abs(st["rv"] - f32np(rv)).max() <= 1e-6 * max(1.0, np.abs(st["rv"]).max())
    dy = rec["dy"].float()
    if rec["kind"] == "res":
        want_y, want_pre = T.bn_act_add(zr, sv, _rows(rec["res"]))
        assert np.array_equal(_rows(rec["y"]), want_y), "y"
        assert torch.equal(rec["dres"], rec["dy"]), "the residual's gradient is dy"
        if "pre" in rec:
            assert np.array_equal(_rows(rec["pre"]), want_pre), "y_preadd"
            dy = dy + rec["dpre"].float()
    else:
        assert np.array_equal(_rows(rec["y"]), N.forward(zr, sv)), "y"
    dy = dy.permute(0, 2, 3, 1).contiguous()
    g = torch.full((n, ho, wo, cout), NAN, dtype=BF16, device=DEV)
    K.bn_act_bwd(dy, z, saved, _lib.ACT_LEAKY01, True, g, None, None, ws)
    c12 = ws[:2 * cout].cpu().reshape(2, cout).numpy()
    tr = N.backward_terms(f32np(dy).reshape(m, cout), zr, sv)
    assert np.array_equal(f32np(g).reshape(m, cout), N.backward_apply(tr, sv, c12[0], c12[1])), "g"
    g64, x64, w64 = g.permute(0, 3, 1, 2).cpu().to(F64), x.to(BF16).float().cpu().to(F64), w.cpu().to(F64)
    conv = D.grads(x64, w64, None, None, "none", g=g64) if stride == 2 else B.grads(x64, w64, g64, None, k, "none")
    grad = lambda name: rec["params"][name].grad.detach().cpu()
    ratios = dict(dgamma=N.ratio(grad("gamma").numpy(), tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])),
                  dbeta=N.ratio(grad("beta").numpy(), tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])),
                  dW=B.ratio(grad("w"), conv["dw"], B.bound_sum(conv["dw_terms"], conv["dw_abs"])))
    if "dx" in rec:
        ratios["dx"] = B.ratio(rec["dx"].float().cpu()[:, :x64.shape[1]], conv["dx_sum"], B.bound_dx(conv["dx_sum"], conv["dx_terms"], conv["dx_abs"]))
    for name, v in ratios.items():
        assert v <= 1.0, (rec["kind"], tuple(w.shape), name, v)
        worst[name] = max(worst.get(name, 0.0), v)


def check_head_call(rec, worst):
    x64, w64 = rec["x"].float().cpu().to(F64), rec["params"]["w"].detach().cpu().to(F64)
    b = rec["params"]["b"]
    want = B.grads(x64, w64, rec["dy"].cpu(), rec["y"].cpu().to(F64), w64.shape[2], "none")
    ratios = dict(head_dW=B.ratio(rec["params"]["w"].grad.cpu(), want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  head_db=B.ratio(b.grad.cpu(), want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  head_dx=B.ratio(rec["dx"].float().cpu(), want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
        worst[name] = max(worst.get(name, 0.0), v)


def check_glue_call(rec):
    if rec["kind"] == "spp":
        y, idx = T.spp_forward(_nhwc(rec["x"]))
        assert np.array_equal(_nhwc(rec["y"]), y) and np.array_equal(_nhwc(rec["dx"]), T.spp_backward(_nhwc(rec["dy"]), idx))
    else:
        assert np.array_equal(_nhwc(rec["y"]), T.upcat_forward(_nhwc(rec["a"]), _nhwc(rec["b"])))
        da, db = T.upcat_backward(_nhwc(rec["dy"]), rec["a"].shape[1])
        assert np.array_equal(_nhwc(rec["da"]), da) and np.array_equal(_nhwc(rec["db"]), db)


@functools.lru_cache(maxsize=None)
def device_step(family, fresh=0):
    """One training step of a fresh model on the device: (model, p, parameter gradients, loss items)."""
    model = new_model(family)
    x, targets = T.golden_inputs()
    p = model(x.to(DEV))
    loss, items = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    return model, [t.detach() for t in p], {n: t.grad for n, t in model.named_parameters()}, items


@pytest.mark.parametrize("family", list(T.MODELS))
def test_model_layer_by_layer(family):
    """Every op call of one device forward + backward, re-run on its restatement from the device's own inputs: the leg that replaces an
    end-to-end tolerance."""
    model = new_model(family)
    x, targets = T.golden_inputs()
    calls = []
    p = MT.forward_train(model, x.to(DEV), ops=recording_ops(calls))
    loss, _ = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    kinds = [c["kind"] for c in calls]
    assert kinds.count("upcat") == 2 and kinds.count("spp") == (1 if family == "spp" else 0) and kinds.count("down") == 5
    assert kinds.count("res") == 23 and kinds.count("head") == (0 if family == "spp" else 2) and sum("pre" in c for c in calls) == 2
    worst = {}
    for rec in calls:
        if rec["kind"] in ("bn", "down", "res"):
            check_bn_call(rec, worst)
        elif rec["kind"] == "head":
            check_head_call(rec, worst)
        else:
            check_glue_call(rec)
    print(f"train layer by layer, {family}: {len(calls)} op calls, largest error / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("family", list(T.MODELS))
def test_model_training_step_contract(family):
    """p as the reference returns it; compute_loss(p, targets, model)[0].backward() gives every parameter a finite gradient of its own
    shape; two fresh runs give the same bits; the running statistics moved and every BN layer counted one batch; a following eval forward
    equals that of a fresh model loaded from state_dict() (no stale plan).  Reported, not gated: p and the head gradients against the
    float64 reference."""
    gold = helpers.load_golden(T.MODELS[family])
    # an eval forward first, so that a plan with the initial running statistics is cached
    model, x = new_model(family), T.golden_inputs()[0].to(DEV)
    fresh_sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        io_before, _ = model.eval()(x)
    model.train()
    targets = T.golden_inputs()[1].to(DEV)
    p = model(x)
    for i, t in enumerate(p):
        assert t.dtype == F32 and t.is_contiguous() and t.grad_fn is not None and tuple(t.shape) == gold[f"p{i}"].shape
    loss, items = Y.compute_loss(p, targets, model)
    loss.backward()
    grads = {n: t.grad for n, t in model.named_parameters()}
    for n, t in model.named_parameters():
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and bool(t.grad.any()), n
    # two fresh runs: the same bits
    model2, p2, grads2, items2 = device_step(family)
    for a, b in zip(p, p2):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(items, items2)
    for n in grads:
        assert torch.equal(bits(grads[n]), bits(grads2[n])), n
    sd, sd2 = model.state_dict(), model2.state_dict()
    for k_ in sd:
        assert torch.equal(sd[k_], sd2[k_]), k_
        if k_.endswith("running_mean") or k_.endswith("running_var"):
            assert not torch.equal(sd[k_], fresh_sd[k_]), k_
        if k_.endswith("num_batches_tracked"):
            assert int(sd[k_]) == 1, k_
    # the stale-plan check
    clone = getattr(Y, type(model).__name__)(**T.CTOR)
    clone.load_state_dict({k: v.cpu() for k, v in sd.items()})
    with torch.no_grad():
        io_after, _ = model.eval()(x)
        io_clone, _ = clone.to(DEV).eval()(x)
    assert torch.equal(io_after, io_clone) and not torch.equal(io_after, io_before)
    # reported: the device against the float64 reference (the rounding-point model's own distance: tests/test_train_cpu.py)
    for i, t in enumerate(p):
        print(f"train step, {family}: p{i} relative L2 vs the float64 reference {B.rel_l2(t.detach().cpu(), torch.from_numpy(gold[f'p{i}'])):.3f}")
    for n in T.stored_gradients(family, list(grads)):
        if n.startswith(T.HEADS[family]):
            print(f"train step, {family}: d {n} relative L2 vs the float64 reference {B.rel_l2(grads[n].cpu(), torch.from_numpy(gold['grad/' + n])):.3f}")
    print(f"train step, {family}: loss items device {items.cpu().numpy()}  reference {gold['items']}")
