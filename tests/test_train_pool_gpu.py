"""GPU tests of the max-pool ops and of the training step of YOLOv3-tiny / LiteYOLOv3: the kernels of csrc/pool_train.hip,
yolo_bn_act_pool_fwd and yolo_concat_upsample2_* bit for bit against the restatements of tests/_train_pool.py, the ops against their
restatement from the device's own inputs, a shallow chain against float64 autograd, and the whole models through
``pytorch_yolo_amd.forward_train`` - layer by layer from the device's own tensors, and as a training step.

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs are NaN / 0xAA filled; the 0xFF and the 0x7F
run give equal bits, and so does a second run.  The whole models follow tests/test_train_gpu.py: no end-to-end tolerance against the
reference (DESIGN.md 3.6f says why); the relative L2 figures are printed.

Measured on an MI355X: DESIGN.md 3.6g."""
import numpy as np
import pytest
import torch

import _bn as N
import _conv_bwd as B
import _loss as L
import _train as T
import _train_pool as TP
import helpers
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT
from test_train_gpu import (BF16, DEV, F32, F64, NAN, _bn, _bn_params, _cl, _head, _leaf, _nhwc, bits, both_poisons, chain_grads, check_bn_call,
                            check_glue_call, check_head_call, f32np, randbf, recording_ops, t32, tied)

pytestmark = pytest.mark.gpu

U8 = torch.uint8
# (n, h, w, c, stride): 2x3 one window row (stride 2) / the smallest map (stride 1); 6x4 even; 7x5 odd: a row and a column are dropped;
# c = 72: nine chunks, more than one block at 7x5
POOL_CASES = [(2, h, w, c, s) for c in (8, 72) for (h, w, s) in ((2, 3, 2), (6, 4, 2), (7, 5, 2), (2, 3, 1), (7, 5, 1))]


def pooled(n, h, w, c, stride):
    return (n, h // 2, w // 2, c) if stride == 2 else (n, h, w, c)


# ---- the kernels, bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POOL_CASES, ids=lambda s: "%dx%dx%d_c%d_s%d" % s)
def test_pool_kernels_equal_the_restatement(case):
    n, h, w, c, stride = case
    shape, out = (n, h, w, c), pooled(*case)
    x, dy = tied(shape, 51), randbf(out, 52)
    dy[..., :4] = tied(out[:3] + (4,), 53)                                     # tied gradients too in the first channels
    want_y, want_idx = TP.pool_forward(x, stride)
    want_dx = TP.pool_backward(dy, want_idx, shape, stride)

    def run(a):
        xd, dyd = a.like("x", t32(x).to(BF16)), a.like("dy", t32(dy).to(BF16))
        y, idx = a.alloc("y", out, BF16, NAN), a.alloc("idx", out, U8, 0xAA)
        dx = a.alloc("dx", shape, BF16, NAN)
        K.maxpool_train_fwd(xd, y, idx, stride)
        K.maxpool_bwd(dyd, idx, dx, stride)
        return dict(y=y, idx=idx, dx=dx)

    got = both_poisons(run)
    assert np.array_equal(f32np(got["y"]), want_y) and np.array_equal(got["idx"].cpu().numpy(), want_idx)
    assert np.array_equal(f32np(got["dx"]), want_dx)
    assert want_dx.any() and len(np.unique(want_idx)) == 4
    if stride == 2 and h % 2:
        assert not f32np(got["dx"])[:, h - 1].any() and not f32np(got["dx"])[:, :, w - 1].any()


def test_stride2_backward_copies_the_gradient_bits():
    """The 2/2 windows do not overlap, so the backward is a copy, not a sum: dx takes dy's bits - a -0.0 stays -0.0, which ``0.f + d`` would
    turn into +0.0 - at the pixel idx names and is +0 everywhere else, the dropped odd row and column included."""
    shape, out = (1, 3, 5, 8), (1, 1, 2, 8)
    gen = torch.Generator().manual_seed(54)
    x = torch.randn(shape, generator=gen).to(BF16).to(DEV)
    dy = -(1.0 + torch.rand(out, generator=gen)).to(BF16)                      # negative normal values ...
    dy[..., ::2] = -0.0                                                        # ... and -0.0 in every other channel
    dy = dy.to(DEV)
    y, idx = torch.empty(out, dtype=BF16, device=DEV), torch.empty(out, dtype=U8, device=DEV)
    dx = torch.full(shape, NAN, dtype=BF16, device=DEV)
    K.maxpool_train_fwd(x, y, idx, 2)
    K.maxpool_bwd(dy, idx, dx, 2)
    torch.cuda.synchronize()
    dy_bits, tap = dy.view(torch.int16).cpu().numpy(), idx.cpu().numpy()
    want = np.zeros(shape, dtype=np.int16)
    for ox in range(out[2]):
        for ch in range(out[3]):
            want[0, tap[0, 0, ox, ch] // 2, 2 * ox + tap[0, 0, ox, ch] % 2, ch] = dy_bits[0, 0, ox, ch]
    assert np.array_equal(dx.view(torch.int16).cpu().numpy(), want)
    assert (want == np.int16(-0x8000)).sum() == 8 and (want != 0).sum() == 16    # the eight -0.0 arrived as -0.0
    assert not want[:, 2].any() and not want[:, :, 4].any()


@pytest.mark.parametrize("c", [8, 72])
@pytest.mark.parametrize("hw", [(6, 4), (7, 5)], ids=["6x4", "7x5"])
def test_bn_act_pool_equals_the_two_launches(hw, c):
    case = (2, hw[0], hw[1], c)
    out = pooled(*case, 2)
    z, _, gamma, beta, rm, rv = N.random_operands(case)
    gamma = gamma.copy()
    gamma[::3] *= -1.0                                                         # some negative gamma: the activation reverses z's order there
    saved = N.stats(z, gamma, beta)["saved"]
    want_y, want_idx = TP.bn_act_pool(z.reshape(case), saved)

    def run(a):
        zd, sd = a.like("z", t32(z).to(BF16).reshape(case)), a.like("saved", t32(saved))
        y, idx = a.alloc("y", out, BF16, NAN), a.alloc("idx", out, U8, 0xAA)
        full = a.alloc("full", case, BF16, NAN)
        y2, idx2 = a.alloc("y2", out, BF16, NAN), a.alloc("idx2", out, U8, 0xAA)
        K.bn_act_pool_fwd(zd, sd, y, idx, _lib.ACT_LEAKY01)
        K.bn_act_fwd(zd, sd, full, _lib.ACT_LEAKY01)
        K.maxpool_train_fwd(full, y2, idx2, 2)
        return dict(y=y, idx=idx, y2=y2, idx2=idx2)

    got = both_poisons(run)
    assert torch.equal(bits(got["y"]), bits(got["y2"])) and torch.equal(got["idx"].cpu(), got["idx2"].cpu())
    assert np.array_equal(f32np(got["y"]), want_y) and np.array_equal(got["idx"].cpu().numpy(), want_idx)
    _, idx_z = TP.bn_act_pool(z.reshape(case), saved, pool_on_z=True)
    assert not np.array_equal(want_idx, idx_z) and len(np.unique(want_idx)) == 4          # pooling z instead would show


def test_concat_upsample_kernels_equal_the_restatement():
    n, h, w, ca, cb = 2, 3, 5, 8, 24
    a_, b_, dy = tied((n, h, w, ca), 61), tied((n, 2 * h, 2 * w, cb), 62), randbf((n, 2 * h, 2 * w, ca + cb), 63)
    want_db, want_da = TP.catup_backward(dy, cb)

    def run(a):
        ad, bd, dyd = a.like("a", t32(a_).to(BF16)), a.like("b", t32(b_).to(BF16)), a.like("dy", t32(dy).to(BF16))
        y = a.alloc("y", (n, 2 * h, 2 * w, ca + cb), BF16, NAN)
        da, db = a.alloc("da", (n, h, w, ca), BF16, NAN), a.alloc("db", (n, 2 * h, 2 * w, cb), BF16, NAN)
        da1, db1 = a.alloc("da1", (n, h, w, ca), BF16, NAN), a.alloc("db1", (n, 2 * h, 2 * w, cb), BF16, NAN)
        K.concat_upsample2_fwd(bd, ad, y)
        K.concat_upsample2_bwd(dyd, db, da, n=n, h=h, w=w, cb=cb, ca=ca)
        K.concat_upsample2_bwd(dyd, None, da1, n=n, h=h, w=w, cb=cb, ca=ca)             # each gradient alone
        K.concat_upsample2_bwd(dyd, db1, None, n=n, h=h, w=w, cb=cb, ca=ca)
        return dict(y=y, da=da, db=db, da1=da1, db1=db1)

    got = both_poisons(run)
    assert np.array_equal(f32np(got["y"]), TP.catup_forward(b_, a_))
    assert np.array_equal(f32np(got["da"]), want_da) and np.array_equal(f32np(got["db"]), want_db)
    assert torch.equal(bits(got["da"]), bits(got["da1"])) and torch.equal(bits(got["db"]), bits(got["db1"]))
    assert float(np.mean(N.bf16(want_da) != TP.catup_backward(dy, cb, rounding=False)[1])) > 0.2      # the one rounding is exercised


# ---- the recording table: tests/test_train_gpu.py's, with the two pool ops and the up_first keyword ---------------------------------------
def recording_pool_ops(calls):
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))

    def alias(rec, key, t):
        if not t.requires_grad:
            rec[key] = t.detach()
            return t
        a = t.view_as(t)
        a.register_hook(keep(rec, "d" + key))
        rec[key] = a.detach()
        return a

    def watch(rec, key, t):
        rec[key] = t.detach()
        if t.requires_grad:
            t.register_hook(keep(rec, "d" + key))
        return t

    def pool_bn_block(x, w, gamma, beta, rm=None, rv=None, *, pool_stride=2, momentum=0.1, eps=1e-5):
        rec = dict(kind="poolbn", stride=pool_stride, momentum=momentum, eps=eps, rm0=rm.detach().clone(), rv0=rv.detach().clone(), rm=rm, rv=rv,
                   params=dict(w=w, gamma=gamma, beta=beta))
        calls.append(rec)
        for t in (w, gamma, beta):
            if not t.is_leaf:
                t.retain_grad()
        y = Y.pool_bn_block(alias(rec, "x", x), w, gamma, beta, rm, rv, pool_stride=pool_stride, momentum=momentum, eps=eps)
        rec["idx"] = y.grad_fn.saved_tensors[4]                                   # (x, weight, z, saved, idx)
        return watch(rec, "y", y)

    def max_pool(x, *, stride=2):
        rec = dict(kind="pool", stride=stride)
        calls.append(rec)
        return watch(rec, "y", Y.max_pool(alias(rec, "x", x), stride=stride))

    base = recording_ops(calls)

    def upsample_concat(a, b, *, up_first=True):
        if up_first:
            return base.upsample_concat(a, b)
        rec = dict(kind="catup")
        calls.append(rec)
        return watch(rec, "y", Y.upsample_concat(alias(rec, "a", a), alias(rec, "b", b), up_first=False))

    table = dict(vars(base))
    table.update(pool_bn_block=pool_bn_block, max_pool=max_pool, upsample_concat=upsample_concat)
    return type(base)(**table)


def check_pool_bn_call(rec, worst):
    """One pool_bn_block call from the device's own tensors: the forward's launches repeated; the pooled y and idx bit-equal to the
    restatement's pool of the device's full-resolution activation; yolo_maxpool_bwd's expansion of dy bit-equal; from there on
    tests/test_train_gpu.check_bn_call on the full-resolution pair (running statistics, g bit-equal; dgamma, dbeta, dW, dx in bounds)."""
    x, w, stride = rec["x"], rec["params"]["w"].detach(), rec["stride"]
    gamma, beta = rec["params"]["gamma"].detach().contiguous(), rec["params"]["beta"].detach().contiguous()
    with torch.no_grad():
        z = Y.conv_block(x, w, act="none").permute(0, 2, 3, 1).contiguous()
    n, h, wd, cout = z.shape
    saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
    ws = torch.full((K.bn_workspace_bytes(n * h * wd, cout) // 4,), NAN, dtype=F32, device=DEV)
    K.bn_train_stats(z, gamma, beta, rec["eps"], rec["momentum"], rec["rm0"].clone(), rec["rv0"].clone(), saved, ws)
    full = torch.full(z.shape, NAN, dtype=BF16, device=DEV)
    K.bn_act_fwd(z, saved, full, _lib.ACT_LEAKY01)
    want_y, want_idx = TP.pool_forward(f32np(full), stride)
    assert np.array_equal(_nhwc(rec["y"]), want_y), "y"
    assert np.array_equal(rec["idx"].cpu().numpy(), want_idx), "idx"
    dy = rec["dy"].permute(0, 2, 3, 1).contiguous()
    assert dy.dtype == BF16
    dfull = torch.full(z.shape, NAN, dtype=BF16, device=DEV)
    K.maxpool_bwd(dy, rec["idx"], dfull, stride)
    assert np.array_equal(f32np(dfull), TP.pool_backward(f32np(dy), want_idx, tuple(z.shape), stride)), "the expanded dy"
    check_bn_call(dict(rec, kind="bn", y=full.permute(0, 3, 1, 2), dy=dfull.permute(0, 3, 1, 2)), worst)


def check_pool_glue_call(rec):
    if rec["kind"] == "pool":
        x = _nhwc(rec["x"])
        y, idx = TP.pool_forward(x, rec["stride"])
        assert np.array_equal(_nhwc(rec["y"]), y)
        assert np.array_equal(_nhwc(rec["dx"]), TP.pool_backward(_nhwc(rec["dy"]), idx, x.shape, rec["stride"]))
    else:
        assert np.array_equal(_nhwc(rec["y"]), TP.catup_forward(_nhwc(rec["b"]), _nhwc(rec["a"])))
        db, da = TP.catup_backward(_nhwc(rec["dy"]), rec["b"].shape[1])
        assert np.array_equal(_nhwc(rec["da"]), da) and np.array_equal(_nhwc(rec["db"]), db)


def check_calls(calls):
    worst = {}
    for rec in calls:
        if rec["kind"] == "poolbn":
            check_pool_bn_call(rec, worst)
        elif rec["kind"] in ("pool", "catup"):
            check_pool_glue_call(rec)
        elif rec["kind"] in ("bn", "down", "res"):
            check_bn_call(rec, worst)
        elif rec["kind"] == "head":
            check_head_call(rec, worst)
        else:
            check_glue_call(rec)
    return worst


# ---- the ops ------------------------------------------------------------------------------------------------------------------------------
def _pool_bn_operands(h, w, seed=71):
    gen = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn((2, 8, h, w), generator=gen).to(BF16).to(DEV))
    wt = (torch.randn((16, 8, 3, 3), generator=gen) / 8.5).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(16, generator=gen)).to(DEV), (0.5 * torch.randn(16, generator=gen)).to(DEV)
    with torch.no_grad():
        gamma[::3] *= -1.0
    return x, wt, gamma, beta


@pytest.mark.parametrize("case", [(6, 4, 2), (7, 5, 2), (7, 5, 1), (2, 3, 1)], ids=lambda s: "%dx%d_s%d" % s)
def test_pool_bn_block_and_max_pool_against_the_restatement(case):
    """pool_bn_block and max_pool as ops, re-run on their restatement from the device's own inputs: y, idx and the running statistics
    bit-equal; dgamma, dbeta, dW and dx within the bounds of tests/test_bn_gpu.py / test_conv_bwd_gpu.py; two runs give the same bits."""
    h, w, stride = case
    x, wt, gamma, beta = _pool_bn_operands(h, w)
    runs = []
    for _ in range(2):
        calls = []
        ops = recording_pool_ops(calls)
        xg = x.clone().requires_grad_()
        wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (wt, gamma, beta))
        rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
        y = ops.pool_bn_block(xg, wp, gp, bp, rm, rv, pool_stride=stride)
        y2 = ops.max_pool(y, stride=stride) if min(y.shape[2:]) >= 2 else y
        r = torch.randn(y2.shape, generator=torch.Generator().manual_seed(72)).to(DEV)
        (y2.float() * r).sum().backward()
        torch.cuda.synchronize()
        assert y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous() and tuple(y.shape) == (2, 16) + pooled(2, h, w, 16, stride)[1:3]
        assert bool((rm != 0).all()) and bool((rv != 1).all())
        runs.append((calls, [y.detach(), y2.detach(), xg.grad, wp.grad, gp.grad, bp.grad, rm, rv]))
    worst = check_calls(runs[0][0])
    print(f"pool_bn_block {h}x{w} stride {stride}: largest error / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(bits(a), bits(b))


def test_pool_op_contracts():
    """pool_bn_block is max_pool(conv_bn_block) bit for bit at both strides; no_grad gives no grad_fn; dtype conversion by torch; a gradient
    only where asked; the concat in tiny's order; a second derivative raises."""
    x, wt, gamma, beta = _pool_bn_operands(6, 4)
    with torch.no_grad():
        full = Y.conv_bn_block(x, wt, gamma, beta)
        for stride in (2, 1):
            y = Y.pool_bn_block(x, wt, gamma, beta, pool_stride=stride)
            assert y.grad_fn is None and torch.equal(y, Y.max_pool(full, stride=stride))
        want = torch.nn.functional.max_pool2d(full.float(), 2, 1, padding=1, dilation=2)
        assert torch.equal(Y.max_pool(full, stride=1).float(), want)
    xf = torch.randn((2, 8, 7, 5), generator=torch.Generator().manual_seed(73)).to(DEV).requires_grad_()      # float32 NCHW: converted by torch
    y = Y.max_pool(xf)
    assert y.shape == (2, 8, 3, 2) and y.dtype == BF16 and y.grad_fn is not None
    assert torch.equal(y.detach().float(), torch.nn.functional.max_pool2d(xf.detach().to(BF16).float(), 2, 2))
    y.float().sum().backward()
    assert xf.grad.dtype == F32 and xf.grad.shape == xf.shape and float(xf.grad.sum()) == y.numel()
    xg = x.clone().requires_grad_()
    wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (wt, gamma, beta))
    y = Y.pool_bn_block(xg, wp, gp, bp)
    y.float().sum().backward(inputs=[gp], retain_graph=True)
    assert gp.grad is not None and all(t.grad is None for t in (xg, wp, bp))
    with pytest.raises(RuntimeError):
        torch.autograd.grad(torch.autograd.grad(y.float().sum(), xg, create_graph=True)[0].float().sum(), xg)
    a = _cl(torch.randn((2, 8, 3, 5)).to(BF16).to(DEV)).requires_grad_()
    b = _cl(torch.randn((2, 24, 6, 10)).to(BF16).to(DEV)).requires_grad_()
    u = Y.upsample_concat(a, b, up_first=False)
    assert torch.equal(u[:, :24], b) and torch.equal(u[:, 24:], a.detach().repeat_interleave(2, 2).repeat_interleave(2, 3))
    assert torch.equal(Y.upsample_concat(a, b), Y.upsample_concat(a, b, up_first=True))
    r = torch.randn_like(u)
    (u * r).float().sum().backward(inputs=[b], retain_graph=True)
    assert a.grad is None and torch.equal(b.grad, r[:, :24])
    (u * r).float().sum().backward(inputs=[a])
    assert a.grad is not None and a.grad.dtype == BF16 and a.grad.shape == a.shape


# ---- a shallow chain against float64 autograd -----------------------------------------------------------------------------------------------
def chain_pool():
    """pool_bn_block -> max_pool -> pool_bn_block(pool_stride=1) -> upsample_concat(up_first=False) with the routed first output ->
    conv_bn_block -> an fp32 head, on a 12x8 map."""
    gen, p = torch.Generator().manual_seed(8400), {}
    x0 = torch.randn((2, 8, 12, 8), generator=gen).to(BF16).to(F64)
    _bn_params(gen, "1", 8, 16, 3, p), _bn_params(gen, "2", 16, 16, 3, p), _bn_params(gen, "3", 32, 16, 3, p)
    p["Wh"], p["bh"] = _leaf(gen, 21, 16, 1, 1, scale=0.25), _leaf(gen, 21, scale=0.5)
    r = _leaf(gen, 2, 21, 6, 4)

    def run(ops, p, cast):
        x1 = _bn(ops, "pool_bn_block", cast(x0), p, "1")
        x3 = _bn(ops, "pool_bn_block", ops.max_pool(x1, stride=2), p, "2", pool_stride=1)
        x4 = ops.upsample_concat(x3, x1, up_first=False)
        return _head(ops, _bn(ops, "conv_bn_block", x4, p, "3"), p, "h", cast(r))
    return p, run


def test_chain_vs_float64_autograd():
    """The parameter gradients of the chain on the device against the same chain in float64 without any rounding, by relative L2; the
    yardstick is the float64 chain with every rounding point (tests/_train_pool.cpu_ops(True)); the allowed quotient is 1.5, the rule of
    the chain tests of 3.6c-f."""
    want = chain_grads(chain_pool, TP.cpu_ops(False), False)
    cpu = chain_grads(chain_pool, TP.cpu_ops(True), False)
    dev = chain_grads(chain_pool, MT.DEVICE_OPS_POOL, True)
    again = chain_grads(chain_pool, MT.DEVICE_OPS_POOL, True)
    rows = []
    for name in want:
        rows.append((name, B.rel_l2(dev[name], want[name]), B.rel_l2(cpu[name], want[name])))
        print("train chain pool vs float64, relative L2 of d%s: device %.4e  float64 chain with the rounding points %.4e  device / chain %.5f"
              % (name, rows[-1][1], rows[-1][2], rows[-1][1] / rows[-1][2]))
        assert torch.equal(dev[name], again[name]), name
    for name, e_dev, e_cpu in rows:
        assert e_cpu > 0 and e_dev <= 1.5 * e_cpu, (name, e_dev, e_cpu)


# ---- whole models -------------------------------------------------------------------------------------------------------------------------
def new_model(family):
    model = T.load_synthetic(getattr(Y, TP.CLASSES[family])(**TP.CTORS[family]))
    model.hyper_params = dict(L.HYPER)
    return model.to(DEV).train()


def device_step(family, ops=None):
    model = new_model(family)
    x, targets = TP.golden_inputs(family)
    p = Y.forward_train(model, x.to(DEV), **({} if ops is None else dict(ops=ops)))
    loss, items = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    return model, p, {n: t.grad for n, t in model.named_parameters()}, items


@pytest.mark.parametrize("family", list(TP.MODELS))
def test_model_layer_by_layer(family):
    """Every op call of one device forward + backward, re-run on its restatement from the device's own inputs."""
    calls = []
    device_step(family, recording_pool_ops(calls))
    kinds = [c["kind"] for c in calls]
    if family == "tiny":
        assert kinds.count("poolbn") == 5 and kinds.count("pool") == 1 and kinds.count("catup") == 1 and kinds.count("upcat") == 0
        assert kinds.count("head") == 2 and kinds.count("bn") == 6 and [c["stride"] for c in calls if c["kind"] == "poolbn"] == [2, 2, 2, 2, 1]
    else:
        assert kinds.count("poolbn") == 5 and kinds.count("pool") == 0 and kinds.count("catup") == 0 and kinds.count("upcat") == 2
        assert kinds.count("head") == 2 and kinds.count("bn") == 13
    worst = check_calls(calls)
    print(f"train layer by layer, {family}: {len(calls)} op calls, largest error / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("family", list(TP.MODELS))
def test_model_training_step_contract(family):
    """p as the reference returns it; compute_loss(p, targets, model)[0].backward() gives every parameter a finite non-zero gradient; two
    fresh runs give the same bits; the running statistics moved and every BN layer counted one batch; a following eval forward equals that
    of a fresh model loaded from state_dict() (no stale plan).  Reported, not gated: p and the head gradients against the float64
    reference."""
    gold = helpers.load_golden(TP.MODELS[family])
    model, x = new_model(family), TP.golden_inputs(family)[0].to(DEV)
    fresh_sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        io_before, _ = model.eval()(x)                                            # a plan with the initial running statistics is cached
    model.train()
    targets = TP.golden_inputs(family)[1].to(DEV)
    p = Y.forward_train(model, x)
    assert len(p) == len(model.yolo_layers)
    for i, t in enumerate(p):
        assert t.dtype == F32 and t.is_contiguous() and t.grad_fn is not None and tuple(t.shape) == gold[f"p{i}"].shape
    loss, items = Y.compute_loss(p, targets, model)
    loss.backward()
    grads = {n: t.grad for n, t in model.named_parameters()}
    for n, t in model.named_parameters():
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and bool(t.grad.any()), n
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
    clone = getattr(Y, type(model).__name__)(**TP.CTORS[family])
    clone.load_state_dict({k: v.cpu() for k, v in sd.items()})
    with torch.no_grad():
        io_after, _ = model.eval()(x)
        io_clone, _ = clone.to(DEV).eval()(x)
    assert torch.equal(io_after, io_clone) and not torch.equal(io_after, io_before)
    for i, t in enumerate(p):
        print(f"train step, {family}: p{i} relative L2 vs the float64 reference {B.rel_l2(t.detach().cpu(), torch.from_numpy(gold[f'p{i}'])):.3f}")
    for n in TP.stored_gradients(family, list(grads)):
        if n.startswith(TP.HEADS[family]):
            print(f"train step, {family}: d {n} relative L2 vs the float64 reference {B.rel_l2(grads[n].cpu(), torch.from_numpy(gold['grad/' + n])):.3f}")
    print(f"train step, {family}: loss items device {items.cpu().numpy()}  reference {gold['items']}")


def test_module_call_in_training_mode():
    """model.train()(x) on the device still raises for YOLOv3-tiny and LiteYOLOv3 and still works for YOLOv3-SPP."""
    x = TP.golden_inputs("tiny")[0].to(DEV)
    for family in TP.MODELS:
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            new_model(family)(x)
    spp = T.load_synthetic(Y.YOLOv3SPP(**T.CTOR)).to(DEV).train()
    p = spp(x)
    assert len(p) == 3 and all(t.grad_fn is not None and t.dtype == F32 for t in p)
