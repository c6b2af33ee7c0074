"""GPU tests of the training-mode forward and backward of YOLOv3-tiny/ShuffleNetV2: the three entries of
csrc/shuffle_train.hip, the four ops on them and forward_train(model, x, ops=DEVICE_OPS_SHUFFLE).

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs are NaN-filled; the 0xFF and the 0x7F run give
equal bits, and so does a second run.  Every test is a plain parity run.
  the pool entries on tests/_train_shuffle.POOL_CASES: integer maps in [-3, 3] (ties everywhere), an all-negative map (a pool that pads
    with 0 cannot pass) and random bf16: y and idx equal the restatement (and torch's values); dx on integer dy in [-7, 7] is exact and
    equals torch's autograd.
  yolo_channel_shuffle2_bwd on SHUFFLE_CASES: dy read as a view of a wider buffer whose pad channels hold NaN, da written into a view of a
    wider buffer whose other channels keep their fill; equal to torch's autograd of the view / transpose shuffle, pad channels zero.
  conv_bn_relu_block (1x1 at stride 1, 3x3 at stride 2 with cin 3) against the restatement with hi = +inf from the device's own tensors.
  max_pool_321 and channel_shuffle2 as ops; shuffle_unit_block against the composed form: bits, launches by need, bytes held.
  the model: one step of YOLOv3TinyShuffle(n_class=2) at 64 x 96 with every op call recorded and held to its restatement; a fused call
    bit-equal to the composed form re-run on its inputs; a second step and a step on the composed table give the same bits.
The conv families: tests/_train_shuffle_families.SHUFFLE_FAMILY_CASES through the runner of tests/test_train_fire_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

import _bn as N
import _conv_bwd as B
import _dw_train as D
import _guard as G
import _loss as L
import _train_families as TF
import _train_shuffle as S
import _train_shuffle_families as SF
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd import ops as O
from pytorch_yolo_amd.models import train as MT
from test_train_dw_gpu import BF16, DEV, F32, NAN, _np, bits, run_guarded, t32
from test_train_pool_gpu import check_calls, recording_pool_ops

pytestmark = pytest.mark.gpu
INF = float("inf")


# ---- the pool entries -----------------------------------------------------------------------------------------------------------------------
def device_pool(a, case, x, dy):
    n, h, w, c = case
    ho, wo = S.pool_out(h, w)
    xd, dyd = a.like("x", t32(x).to(BF16)), a.like("dy", t32(dy).to(BF16))
    y, idx = a.alloc("y", (n, ho, wo, c), BF16, NAN), a.alloc("idx", (n, ho, wo, c), torch.uint8, 0xEE)
    K.maxpool3s2p1_train_fwd(xd, y, idx)
    dx = a.alloc("dx", case, BF16, NAN)
    K.maxpool3s2p1_bwd(dyd, idx, dx)
    torch.cuda.synchronize()
    assert torch.equal(bits(xd), bits(t32(x).to(BF16))) and torch.equal(bits(dyd), bits(t32(dy).to(BF16)))       # operands are read-only
    return dict(y=y.float().cpu().numpy(), idx=idx.cpu().numpy(), dx=dx.float().cpu().numpy(), raw=[bits(y), bits(idx), bits(dx)])


@pytest.mark.parametrize("kind", ["integer", "negative", "random"])
@pytest.mark.parametrize("case", S.POOL_CASES, ids=S.case_id)
def test_pool_entries(case, kind):
    x = dict(integer=S.pool_integer_map, negative=S.pool_negative_map, random=S.pool_random_map)[kind](case)
    dy = S.pool_integer_dy(case)
    r = run_guarded(device_pool, case, x, dy)
    y, idx = S.pool_forward(x)
    assert np.array_equal(r["y"], y) and np.array_equal(r["idx"], idx) and idx.max() <= 8
    y64, dx64 = S.torch_pool(x, dy)
    assert np.array_equal(r["y"], y64), "y against torch"
    assert np.array_equal(r["dx"], S.pool_backward(dy, idx, case)) and np.array_equal(r["dx"], dx64), "dx against the restatement / torch"
    if kind == "negative":
        assert (r["y"] < 0).all()


# ---- the shuffle's inverse --------------------------------------------------------------------------------------------------------------------
def device_shuffle_bwd(a, half, slot, dy, fill=7.0):
    """dy [2, 3, 5, 2 slot] (NaN in its pad channels) as the view at channel 8 of a [.., 2 slot + 16] buffer of NaN; da into the view at
    channel 8 of a [.., slot + 16] buffer filled with ``fill``; db dense."""
    nhw = S.SHUFFLE_MAP
    dyb = a.alloc("dy", nhw + (2 * slot + 16,), BF16, NAN)
    dyb[..., 8:8 + 2 * slot] = t32(dy).to(BF16)
    before = bits(dyb)
    dab, db = a.alloc("da", nhw + (slot + 16,), BF16, fill), a.alloc("db", nhw + (slot,), BF16, NAN)
    K.channel_shuffle2_bwd(dyb, dab, db, half, slot, dy_offset=8, da_offset=8)
    only_b = a.alloc("db_alone", nhw + (slot,), BF16, NAN)
    K.channel_shuffle2_bwd(dyb, None, only_b, half, slot, dy_offset=8)
    torch.cuda.synchronize()
    assert torch.equal(bits(dyb), before) and torch.equal(bits(db), bits(only_b))
    return dict(da=dab.float().cpu().numpy(), db=db.float().cpu().numpy(), raw=[bits(dab), bits(db)])


@pytest.mark.parametrize("half,slot", S.SHUFFLE_CASES, ids=lambda v: str(v))
def test_shuffle_backward_entry(half, slot):
    rng = np.random.default_rng(5100 + half)
    dy = D.bf16(rng.standard_normal(S.SHUFFLE_MAP + (2 * slot,)).astype(np.float32))
    dy[..., half:slot], dy[..., slot + half:] = np.nan, np.nan                # the pad channels of both slots: never read
    r = run_guarded(device_shuffle_bwd, half, slot, dy)
    a_, b_ = (D.bf16(rng.standard_normal(S.SHUFFLE_MAP + (slot,)).astype(np.float32)) for _ in range(2))
    _, da64, db64 = S.torch_shuffle(a_, b_, np.nan_to_num(dy), half)
    da, db = S.shuffle_backward(np.nan_to_num(dy), half)
    assert np.array_equal(da, da64) and np.array_equal(db, db64)
    assert np.array_equal(r["da"][..., 8:8 + slot], da64) and np.array_equal(r["db"], db64)
    assert (r["da"][..., :8] == 7.0).all() and (r["da"][..., 8 + slot:] == 7.0).all()        # nothing outside the view is written
    assert not np.isnan(r["da"]).any() and not np.isnan(r["db"]).any()
    assert (r["da"][..., 8 + half:8 + slot] == 0).all() and (r["db"][..., half:] == 0).all()
    # the forward binding on the same layout: the inverse of the inverse
    y = torch.full(S.SHUFFLE_MAP + (2 * slot,), NAN, dtype=BF16, device=DEV)
    K.channel_shuffle2_fwd(t32(da64).to(BF16).to(DEV), t32(db64).to(BF16).to(DEV), y, half, slot)
    assert np.array_equal(y.float().cpu().numpy(), np.nan_to_num(dy))


# ---- the recording table -----------------------------------------------------------------------------------------------------------------------
def recording_shuffle_ops(calls, fused=True):
    """tests/test_train_pool_gpu.recording_pool_ops with the five functions of DEVICE_OPS_SHUFFLE recorded the same way."""
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
        if t.requires_grad:
            t.register_hook(keep(rec, "d" + key))
        return t

    def retain(*tensors):
        for t in tensors:
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()

    def bn_state(rm, rv):
        return dict(rm0=rm.detach().clone(), rv0=rv.detach().clone(), rm=rm, rv=rv)

    def conv_bn_relu_block(x, w, gamma, beta, rm, rv, *, stride=1, momentum=0.1, eps=1e-5):
        rec = dict(kind="relu", stride=stride, momentum=momentum, eps=eps, params=dict(w=w, gamma=gamma, beta=beta), **bn_state(rm, rv))
        calls.append(rec)
        retain(w, gamma, beta)
        return watch(rec, "y", Y.conv_bn_relu_block(alias(rec, "x", x), w, gamma, beta, rm, rv, stride=stride, momentum=momentum, eps=eps))

    def dw_bn_block(x, w, gamma, beta, rm, rv, *, stride=1, act="relu6", momentum=0.1, eps=1e-5):
        assert act == "none"
        rec = dict(kind="dw", stride=stride, momentum=momentum, eps=eps, params=dict(w=w, gamma=gamma, beta=beta), **bn_state(rm, rv))
        calls.append(rec)
        retain(w, gamma, beta)
        return watch(rec, "y", Y.dw_bn_block(alias(rec, "x", x), w, gamma, beta, rm, rv, stride=stride, act="none", momentum=momentum, eps=eps))

    def max_pool_321(x):
        rec = dict(kind="pool321")
        calls.append(rec)
        return watch(rec, "y", Y.max_pool_321(alias(rec, "x", x)))

    def channel_shuffle2(a, b, half):
        rec = dict(kind="shuffle", half=half)
        calls.append(rec)
        return watch(rec, "y", Y.channel_shuffle2(alias(rec, "a", a), alias(rec, "b", b), half))

    def shuffle_unit_block(x, half, *args, momentum=0.1, eps=1e-5):
        params = tuple(args[i] for i in (0, 1, 2, 5, 6, 7, 10, 11, 12))
        running = tuple(args[i] for i in (3, 4, 8, 9, 13, 14))
        rec = dict(kind="unit", half=half, momentum=momentum, eps=eps, params=params, running0=[t.detach().clone() for t in running], running=running)
        calls.append(rec)
        retain(*params)
        fn = Y.shuffle_unit_block if fused else MT.shuffle_ops(fused=False).shuffle_unit_block
        return watch(rec, "y", fn(alias(rec, "x", x), half, *args, momentum=momentum, eps=eps))

    base = recording_pool_ops(calls)
    table = dict(vars(base))
    table.update(conv_bn_relu_block=conv_bn_relu_block, dw_bn_block=dw_bn_block, max_pool_321=max_pool_321, channel_shuffle2=channel_shuffle2,
                 shuffle_unit_block=shuffle_unit_block)
    return type(base)(**table)


def check_layer_call(rec, worst):
    """One conv_bn_relu_block / dw_bn_block(act="none") call against the restatement fed with the device's own tensors, held the way
    tests/test_train_mobile_gpu.check_layer_call holds ReLU6, with hi = +inf: z and saved are the forward's launches repeated; y, g, the
    running statistics and the depthwise dx bit-equal; dgamma, dbeta, dW and the dense dx within their bounds."""
    kind, stride, x = rec["kind"], rec["stride"], rec["x"]
    w, gamma, beta = (rec["params"][k_].detach().contiguous() for k_ in ("w", "gamma", "beta"))
    xb = x.to(BF16)
    with torch.no_grad():
        if kind == "dw":
            xn = xb.permute(0, 2, 3, 1).contiguous()
            n, h, wd, ch = xn.shape
            ho, wo = D.out_hw(h, wd, stride)
            wq = D.bf16(w.cpu().numpy()[:, 0])
            z = torch.full((n, ho, wo, ch), NAN, dtype=BF16, device=DEV)
            K.dwconv3x3(xn, t32(wq).reshape(ch, 9).t().contiguous().to(DEV), torch.zeros(ch, device=DEV), z, n=n, h=h, w=wd, c=ch,
                        in_view=(ch, 0), out_view=(ch, 0), stride=stride, act=_lib.ACT_NONE)
            assert np.array_equal(z.float().cpu().numpy(), D.dw_forward(_np(xb), wq, stride)), (kind, "z")
        else:
            z = (Y.down_block(x, w, act="none") if stride == 2 else Y.conv_block(x, w, act="none")).permute(0, 2, 3, 1).contiguous()
    n, ho, wo, cout = z.shape
    m = n * ho * wo
    saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
    ws = torch.full((K.bn_workspace_bytes(m, cout) // 4,), NAN, dtype=F32, device=DEV)
    rm, rv = rec["rm0"].clone(), rec["rv0"].clone()
    K.bn_train_stats(z, gamma, beta, rec["eps"], rec["momentum"], rm, rv, saved, ws)
    assert torch.equal(rm, rec["rm"].detach()) and torch.equal(rv, rec["rv"].detach()), (kind, "running statistics")
    zr, sv = z.float().cpu().reshape(m, cout).numpy(), saved.cpu().numpy()
    dy = rec["dy"].permute(0, 2, 3, 1).contiguous()
    assert dy.dtype == BF16
    dyr = dy.float().cpu().reshape(m, cout).numpy()
    g = torch.full((n, ho, wo, cout), NAN, dtype=BF16, device=DEV)
    if kind == "dw":
        K.bn_act_bwd(dy, z, saved, _lib.ACT_NONE, True, g, None, None, ws)
        tr, y = N.backward_terms(dyr, zr, sv, "none"), N.forward(zr, sv, "none")
    else:
        K.bn_clamp_bwd(dy, z, saved, 0.0, INF, True, g, None, None, ws)
        tr, y = D.clamp_terms(dyr, zr, sv, 0.0, INF), D.clamp_forward(zr, sv, 0.0, INF)
    c12 = ws[:2 * cout].cpu().reshape(2, cout).numpy()
    assert np.array_equal(_np(rec["y"]).reshape(m, cout), y), (kind, "y")
    gr = g.float().cpu().reshape(m, cout).numpy()
    assert np.array_equal(gr, N.backward_apply(tr, sv, c12[0], c12[1])), (kind, "g")
    gr = gr.reshape(n, ho, wo, cout)
    grad = lambda name: rec["params"][name].grad.detach().cpu()
    ratios = dict(dgamma=N.ratio(grad("gamma").numpy(), tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])),
                  dbeta=N.ratio(grad("beta").numpy(), tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])))
    if kind == "dw":
        assert np.array_equal(_np(rec["dx"]), D.dw_bwd_data(gr, wq, _np(xb).shape, stride)), (kind, "dx")
        want = D.dw_bwd_weight(_np(xb), gr, stride)
        ratios["dw_dW"] = N.ratio(grad("w").numpy()[:, 0], want["S"], D.dw_weight_bound(want))
    else:
        _, _, q = D.dense_backward(_np(xb), w.cpu().numpy(), gr, stride)
        tq = lambda key: torch.from_numpy(q[key])
        ratios["dW"] = B.ratio(grad("w"), tq("dw"), B.bound_sum(tq("dw_terms"), tq("dw_abs")))
        if "dx" in rec:
            ratios["dx"] = B.ratio(torch.from_numpy(_np(rec["dx"])), tq("dx"), B.bound_dx(tq("dx"), tq("dx_terms"), tq("dx_abs")))
    for name, v in ratios.items():
        assert v <= 1.0, (kind, tuple(w.shape), name, v)
        worst[name] = max(worst.get(name, 0.0), v)


def check_glue_call(rec):
    """max_pool_321 / channel_shuffle2 from the device's own tensors: the restatements, bit for bit."""
    if rec["kind"] == "pool321":
        x = _np(rec["x"])
        y, idx = S.pool_forward(x)
        assert np.array_equal(_np(rec["y"]), y)
        assert np.array_equal(_np(rec["dx"]), S.pool_backward(_np(rec["dy"]), idx, x.shape))
    else:
        assert np.array_equal(_np(rec["y"]), S.shuffle_forward(_np(rec["a"]), _np(rec["b"]), rec["half"]))
        da, db = S.shuffle_backward(_np(rec["dy"]), rec["half"])
        assert np.array_equal(_np(rec["da"]), da) and np.array_equal(_np(rec["db"]), db)


def check_unit_call(rec, worst):
    """A fused call against the composed form re-run on its own inputs: bit-equal output, gradients and running tensors; the calls of the
    composed form are held to their restatements."""
    inner = []
    ops = recording_shuffle_ops(inner)
    leaves = [t.detach().clone().requires_grad_() for t in rec["params"]]
    running = [t.clone() for t in rec["running0"]]
    (m1, m2, m3), (e1, e2, e3) = rec["momentum"], rec["eps"]
    xg = rec["x"].clone().requires_grad_()
    slot = xg.shape[1] // 2
    y = ops.conv_bn_relu_block(xg[:, slot:], *leaves[0:3], *running[0:2], momentum=m1, eps=e1)
    y = ops.dw_bn_block(y, *leaves[3:6], *running[2:4], act="none", momentum=m2, eps=e2)
    y = ops.conv_bn_relu_block(y, *leaves[6:9], *running[4:6], momentum=m3, eps=e3)
    y = ops.channel_shuffle2(xg[:, :slot], y, rec["half"])
    y.backward(rec["dy"])
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(rec["y"])) and torch.equal(bits(xg.grad), bits(rec["dx"])), "unit: y / dx"
    for got, want in zip(rec["params"], leaves):
        assert torch.equal(bits(got.grad), bits(want.grad)), ("unit", tuple(got.shape))
    for got, want in zip(rec["running"], running):
        assert torch.equal(bits(got), bits(want)), "unit: running statistics"
    for c in inner:
        check_layer_call(c, worst) if c["kind"] in ("relu", "dw") else check_glue_call(c)


OURS = ("relu", "dw", "pool321", "shuffle", "unit")


def check_shuffle_calls(calls):
    worst = {}
    for rec in calls:
        if rec["kind"] == "unit":
            check_unit_call(rec, worst)
        elif rec["kind"] in ("relu", "dw"):
            check_layer_call(rec, worst)
        elif rec["kind"] in ("pool321", "shuffle"):
            check_glue_call(rec)
    worst.update(check_calls([c for c in calls if c["kind"] not in OURS]))
    return worst


# ---- conv_bn_relu_block -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wshape,stride", [((2, 24, 5, 7), (32, 24, 1, 1), 1), ((2, 3, 12, 20), (32, 3, 3, 3), 2)], ids=["1x1_s1", "3x3_s2_cin3"])
def test_conv_bn_relu_block_against_the_restatement(shape, wshape, stride):
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=gen).to(DEV)
    w = (torch.randn(wshape, generator=gen) / (wshape[1] * wshape[2] * wshape[3]) ** 0.5).to(DEV)
    cout = wshape[0]
    gamma, beta = (1.5 + 0.25 * torch.randn(cout, generator=gen)).to(DEV), (2.5 + torch.randn(cout, generator=gen)).to(DEV)
    runs = []
    for _ in range(2):
        calls = []
        ops = recording_shuffle_ops(calls)
        xg = x.to(BF16).contiguous(memory_format=torch.channels_last).requires_grad_(stride == 1)
        wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (w, gamma, beta))
        rm, rv = torch.full((cout,), 0.25, device=DEV), torch.full((cout,), 1.5, device=DEV)
        y = ops.conv_bn_relu_block(xg, wp, gp, bp, rm, rv, stride=stride, momentum=0.3, eps=1e-3)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(22)).to(BF16).to(DEV)
        y.backward(dy)
        torch.cuda.synchronize()
        ho, wo = D.out_hw(shape[2], shape[3], stride)
        assert y.dtype == BF16 and tuple(y.shape) == (2, cout, ho, wo) and y.permute(0, 2, 3, 1).is_contiguous()
        assert bool((y == 0).any()) and bool((y > 6).any()) and not bool((y < 0).any())          # ReLU: zeros, and no upper bound
        runs.append((calls, [y.detach(), xg.grad, wp.grad, gp.grad, bp.grad, rm, rv]))
    worst = {}
    check_layer_call(runs[0][0][0], worst)
    print(f"conv_bn_relu_block {shape} stride {stride}: largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    # a 1x1 weight has no stride 2; conv_bn_block / down_bn_block keep refusing act="relu"
    with pytest.raises(ValueError, match="conv_bn_relu_block"):
        Y.conv_bn_relu_block(x, w[:, :, :1, :1] if stride == 2 else w, gamma, beta, stride=2)
    with pytest.raises(ValueError, match="act"):
        Y.conv_bn_block(x, w, gamma, beta, act="relu") if stride == 1 else Y.down_bn_block(x, w, gamma, beta, act="relu")


# ---- max_pool_321 and channel_shuffle2 as ops -----------------------------------------------------------------------------------------------------
def test_glue_op_contracts():
    gen = torch.Generator().manual_seed(31)
    x = torch.randn((2, 16, 7, 9), generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    assert Y.max_pool_321(x).grad_fn is None
    with torch.no_grad():
        assert Y.max_pool_321(x.clone().requires_grad_()).grad_fn is None
    xg = x.clone().requires_grad_()
    y = Y.max_pool_321(xg)
    assert y.dtype == BF16 and tuple(y.shape) == (2, 16, 4, 5) and y.permute(0, 2, 3, 1).is_contiguous() and y.grad_fn is not None
    assert [tuple(t.shape) for t in y.grad_fn.saved_tensors] == [(2, 4, 5, 16)] and y.grad_fn.saved_tensors[0].dtype == torch.uint8     # idx, not x
    dy = torch.randn(y.shape, generator=gen).to(BF16).to(DEV)
    y.backward(dy)
    want_y, idx = S.pool_forward(_np(x))
    assert np.array_equal(_np(y), want_y) and np.array_equal(_np(xg.grad), S.pool_backward(_np(dy), idx, _np(x).shape))
    # a float32 NCHW-contiguous x is converted by torch, and gets a gradient of its own dtype and layout
    xf = x.float().contiguous().requires_grad_()
    yf = Y.max_pool_321(xf)
    yf.backward(dy)
    assert torch.equal(bits(yf), bits(y)) and xf.grad.dtype == F32 and torch.equal(xf.grad, xg.grad.float())
    (gx,) = torch.autograd.grad(Y.max_pool_321(xg).float().square().sum(), [xg], create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()
    # channel_shuffle2
    half, slot = 5, 8
    a, b = (torch.randn((2, slot, 3, 5), generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(2))
    with torch.no_grad():
        a[:, half:], b[:, half:] = 0, 0
    assert Y.channel_shuffle2(a, b, half).grad_fn is None
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        ag, bg = a.clone().requires_grad_(need_a), b.clone().requires_grad_(need_b)
        y = Y.channel_shuffle2(ag, bg, half)
        assert y.dtype == BF16 and tuple(y.shape) == (2, 2 * slot, 3, 5) and np.array_equal(_np(y), S.shuffle_forward(_np(a), _np(b), half))
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(32)).to(BF16).to(DEV)
        y.backward(dy)
        da, db = S.shuffle_backward(_np(dy), half)
        assert (ag.grad is not None) == need_a and (bg.grad is not None) == need_b
        assert (not need_a or np.array_equal(_np(ag.grad), da)) and (not need_b or np.array_equal(_np(bg.grad), db))
    af = a.float().contiguous().requires_grad_()
    yf = Y.channel_shuffle2(af, b, half)
    yf.backward(dy)
    assert torch.equal(bits(yf), bits(y)) and af.grad.dtype == F32 and np.array_equal(_np(af.grad), da)
    ag = a.clone().requires_grad_()
    (ga,) = torch.autograd.grad(Y.channel_shuffle2(ag, b, half).float().square().sum(), [ag], create_graph=True)
    with pytest.raises(RuntimeError):
        ga.float().sum().backward()
    with pytest.raises(ValueError, match="channel_shuffle2"):
        Y.channel_shuffle2(a, b, slot + 1)


# ---- the unit as one op -------------------------------------------------------------------------------------------------------------------------
NAMES = ("x", "w1", "gamma1", "beta1", "w_dw", "gamma2", "beta2", "w3", "gamma3", "beta3")
UNIT_CASES = [((2, 128, 6, 8), 58), ((2, 16, 5, 7), 8)]
STARTS = (0.25, 1.5, -0.5, 0.75, 0.125, 1.25)


def unit_operands(shape, half, seed=41):
    """x in the two-slot layout (zero pad channels), the weights with zero pad rows and columns, gamma 1 and beta 0 in the pad channels:
    what ShuffleTracer hands to the op."""
    gen = torch.Generator().manual_seed(seed)
    n, c2, h, w = shape
    slot = c2 // 2
    live = torch.zeros(slot)
    live[:half] = 1.0
    x = torch.randn(shape, generator=gen) * torch.cat([live, live]).reshape(1, -1, 1, 1)
    x = x.to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    pw = lambda: (torch.randn((slot, slot, 1, 1), generator=gen) / half ** 0.5 * live.reshape(-1, 1, 1, 1) * live.reshape(1, -1, 1, 1)).to(DEV)
    vec = lambda mean, std: ((mean + std * torch.randn(slot, generator=gen)) * live).to(DEV)
    gam = lambda: (vec(1.5, 0.25) + (1 - live).to(DEV))
    wd = (torch.randn((slot, 1, 3, 3), generator=gen) / 3 * live.reshape(-1, 1, 1, 1)).to(DEV)
    return [x, pw(), gam(), vec(0.5, 1.0), wd, gam(), vec(0.0, 0.5), pw(), gam(), vec(0.5, 1.0)]


def run_unit(fn, operands, half, dy, needs=(True,) * 10):
    leaves = [t.clone().requires_grad_(need) for t, need in zip(operands, needs)]
    slot = operands[1].shape[0]
    running = [torch.full((slot,), v, device=DEV) for v in STARTS]
    x, w1, g1, b1, wd, g2, b2, w3, g3, b3 = leaves
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    y = fn(x, half, w1, g1, b1, running[0], running[1], wd, g2, b2, running[2], running[3], w3, g3, b3, running[4], running[5],
           momentum=(0.1, 0.3, 0.2), eps=(1e-5, 1e-3, 1e-4))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    if any(needs):
        y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), [t.grad for t in leaves], running, held


@pytest.mark.parametrize("shape,half", UNIT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_unit_equals_the_composition(shape, half):
    operands = unit_operands(shape, half)
    n, c2, h, w = shape
    slot = c2 // 2
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(42)).to(BF16).to(DEV)
    composed = MT.shuffle_ops(fused=False).shuffle_unit_block
    assert MT.shuffle_ops().shuffle_unit_block is Y.shuffle_unit_block and composed is not Y.shuffle_unit_block
    # a view changes addresses only: the view and the dense descriptor of the first 1x1 conv name the same kernels
    dense = TF.forward_desc(n, h, w, slot, slot, 1)
    view = O._desc(operands[0], operands[1], _lib.ACT_NONE, False, in_offset=slot)
    assert (view.cin, view.in_c_total, view.in_c_offset) == (slot, c2, slot)
    assert K.conv2d_pick(view) == K.conv2d_pick(dense) and K.conv2d_bwd_pick(view) == K.conv2d_bwd_pick(dense)
    assert K.conv2d_pick(TF.dgrad_desc(view)) == K.conv2d_pick(TF.dgrad_desc(dense))
    y, grads, running, held = run_unit(Y.shuffle_unit_block, operands, half, dy)
    y_c, grads_c, running_c, held_c = run_unit(composed, operands, half, dy)
    assert y.dtype == BF16 and tuple(y.shape) == shape and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(bits(y), bits(y_c)) and bool((y == 0).any()) and bool(y.any())
    for name, a, b in zip(NAMES, grads, grads_c):
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)) and bool(a.any()), name
    assert grads[0].permute(0, 2, 3, 1).is_contiguous() and not bool(torch.isnan(grads[0].float()).any())
    for a, b, start in zip(running, running_c, STARTS):
        assert torch.equal(bits(a), bits(b)) and bool((a[:half] != start).all())
    slot_bytes = n * h * w * slot * 2
    print(f"shuffle_unit_block {shape} half {half}: bytes held after the forward {held} (composed {held_c}, slot map {slot_bytes})")
    assert held <= held_c - slot_bytes
    again = run_unit(Y.shuffle_unit_block, operands, half, dy)
    assert torch.equal(bits(y), bits(again[0])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, again[1]))
    # the pad channels stay exactly zero, forward and backward
    if half < slot:
        for t in (y, grads[0]):
            assert not bool(t[:, half:slot].any()) and not bool(t[:, slot + half:].any())


def test_unit_gradients_only_where_asked():
    """Every single gradient alone: what is not asked for is None and the launches that serve only it do not run; what is asked for is
    bit-equal to the composed form's; under no_grad nothing is recorded; a second derivative raises."""
    shape, half = UNIT_CASES[1]
    operands = unit_operands(shape, half)
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(43)).to(BF16).to(DEV)
    composed = MT.shuffle_ops(fused=False).shuffle_unit_block
    launches = []
    names = ("channel_shuffle2_bwd", "bn_clamp_bwd", "bn_act_bwd", "conv2d_bwd_weight", "conv2d_bwd_data", "dwconv3x3_bwd_data", "dwconv3x3_bwd_weight")
    real = {n: getattr(K, n) for n in names}
    try:
        for n in names:
            setattr(K, n, (lambda n: lambda *a, **kw: (launches.append(n), real[n](*a, **kw))[1])(n))
        for i in range(10):
            needs = tuple(j == i for j in range(10))
            del launches[:]
            _, grads, _, _ = run_unit(Y.shuffle_unit_block, operands, half, dy, needs)
            count = {n: launches.count(n) for n in names}
            _, grads_c, _, _ = run_unit(composed, operands, half, dy, needs)
            assert [g is not None for g in grads] == list(needs), NAMES[i]
            assert torch.equal(bits(grads[i]), bits(grads_c[i])), NAMES[i]
            up1, up2 = i < 4, i < 7                       # through y1 (x and the first 1x1 conv), through y2 (the depthwise stage too)
            want = dict(channel_shuffle2_bwd=1, bn_clamp_bwd=1 + int(up1), bn_act_bwd=int(up2), conv2d_bwd_weight=int(i in (1, 7)),
                        conv2d_bwd_data=int(up2) + int(i == 0), dwconv3x3_bwd_data=int(up1), dwconv3x3_bwd_weight=int(i == 4))
            assert count == want, (NAMES[i], count, want)
    finally:
        for n in names:
            setattr(K, n, real[n])
    rest = [t for i, t in enumerate(operands[1:]) for t in ((t, None, None) if i % 3 == 2 else (t,))]
    with torch.no_grad():
        y = Y.shuffle_unit_block(operands[0], half, *rest)
    assert y.grad_fn is None
    y2, _, _, _ = run_unit(Y.shuffle_unit_block, operands, half, dy, (False,) * 10)
    assert y2.grad_fn is None
    xg = operands[0].clone().requires_grad_()
    (gx,) = torch.autograd.grad(Y.shuffle_unit_block(xg, half, *rest).float().square().sum(), [xg], create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()
    with pytest.raises(ValueError, match="shuffle_unit_block"):
        Y.shuffle_unit_block(operands[0], half, operands[1][:4], *rest[1:])
    # a float32 NCHW-contiguous x is converted by torch
    xf = operands[0].float().contiguous().requires_grad_()
    yf = Y.shuffle_unit_block(xf, half, *rest)
    yf.float().sum().backward()
    assert torch.equal(bits(yf), bits(y)) and xf.grad.dtype == F32 and tuple(xf.grad.shape) == shape


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
H, W, BS = 64, 96, 2


def new_model():
    model = S.training_model(custom_bn=False)
    model.hyper_params = dict(L.HYPER)
    return model.to(DEV).train()


def model_inputs(model):
    return S.step_inputs(BS, H, W, model.n_class)


def test_model_layer_by_layer():
    """Every op call of one device forward + backward, re-run on its restatement from the device's own inputs."""
    model = new_model()
    x, targets = model_inputs(model)
    calls = []
    table = recording_shuffle_ops(calls)
    assert set(vars(table)) == set(vars(Y.DEVICE_OPS_SHUFFLE))
    p = Y.forward_train(model, x.to(DEV), ops=table)
    loss, _ = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    kinds = [c["kind"] for c in calls]
    assert kinds.count("unit") == 13 and kinds.count("shuffle") == 3 and kinds.count("pool321") == 1 and kinds.count("dw") == 6
    assert kinds.count("relu") == 2 + 3 * 3 and kinds.count("bn") == 3 and kinds.count("head") == 2 and kinds.count("catup") == 1
    assert len(calls) == 13 + 3 + 1 + 6 + 11 + 3 + 2 + 1
    assert [tuple(c["x"].shape[1:]) for c in calls if c["kind"] == "unit"] == [(128, 8, 12)] * 3 + [(256, 4, 6)] * 7 + [(512, 2, 3)] * 3
    worst = check_shuffle_calls(calls)
    print(f"train layer by layer, shuffle: {len(calls)} op calls, largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))


@functools.lru_cache(maxsize=None)
def device_step(fused=True):
    model = new_model()
    x, targets = model_inputs(model)
    p = Y.forward_train(model, x.to(DEV), ops=Y.DEVICE_OPS_SHUFFLE if fused else MT.shuffle_ops(fused=False))
    loss, items = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    return model, [t.detach() for t in p], {n: t.grad for n, t in model.named_parameters()}, items


def test_model_training_step_contract():
    """p as the reference returns it; every parameter gets a finite, non-zero gradient of its own shape; two steps from the same state give
    the same bits, and so does a step on the composed table; the running statistics moved and every BN layer counted one batch; a
    following eval forward equals that of a fresh model loaded from state_dict() (no stale plan); model.train()(x) and
    forward_train(model, x) keep raising, and the named table checks its input as the default path does."""
    model = new_model()
    x, targets = (t.to(DEV) for t in model_inputs(model))
    fresh_sd = {k_: v.clone() for k_, v in model.state_dict().items()}
    with torch.no_grad():
        io_before, _ = model.eval()(x)
    model.train()
    for call in (lambda: model(x), lambda: Y.forward_train(model, x)):
        with pytest.raises(NotImplementedError, match="training-mode forward"):
            call()
    with pytest.raises(ValueError, match="float32"):
        Y.forward_train(model, x.double(), ops=Y.DEVICE_OPS_SHUFFLE)
    with pytest.raises(ValueError, match="multiples of 32"):
        Y.forward_train(model, x[:, :, :, :80], ops=Y.DEVICE_OPS_SHUFFLE)
    assert all(int(m.num_batches_tracked) == 0 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    p = Y.forward_train(model, x, ops=Y.DEVICE_OPS_SHUFFLE)
    for t, grid in zip(p, ((4, 6), (2, 3))):
        assert t.dtype == F32 and t.is_contiguous() and t.grad_fn is not None and tuple(t.shape) == (BS, 3) + grid + (7,)
    loss, items = Y.compute_loss(p, targets, model)
    loss.backward()
    grads = {n: t.grad for n, t in model.named_parameters()}
    for n, t in model.named_parameters():
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and bool(t.grad.any()), n
    for other in (device_step(True), device_step(False)):
        model2, p2, grads2, items2 = other
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(p, p2)) and torch.equal(items, items2) and bool(torch.isfinite(items).all())
        for n in grads:
            assert torch.equal(bits(grads[n]), bits(grads2[n])), n
        sd, sd2 = model.state_dict(), model2.state_dict()
        for k_ in sd:
            assert torch.equal(sd[k_], sd2[k_]), k_
    for k_ in sd:
        if k_.endswith("running_mean") or k_.endswith("running_var"):
            assert not torch.equal(sd[k_], fresh_sd[k_]), k_
        if k_.endswith("num_batches_tracked"):
            assert int(sd[k_]) == 1, k_
    clone = Y.YOLOv3TinyShuffle(**S.CTOR)
    clone.load_state_dict({k_: v.cpu() for k_, v in sd.items()})
    with torch.no_grad():
        io_after, _ = model.eval()(x)
        io_clone, _ = clone.to(DEV).eval()(x)
    assert torch.equal(io_after, io_clone) and not torch.equal(io_after, io_before)


# ---- the conv families of a full-size step that the sibling tables do not hold ------------------------------------------------------------------
def test_family_cases():
    """tests/_train_shuffle_families.SHUFFLE_FAMILY_CASES through tests/test_train_fire_gpu.py's runner, on integer and on random operands."""
    import test_train_fire_gpu as FG
    for c in SF.CASES:
        for operands in (B.exact_operands, B.random_operands):
            x, w, b, dy = operands(c["case"])
            with FG.tuning(*c["knobs"]):
                d = B.fwd_desc(c["case"])
                got = {"forward": TF.family(K.conv2d_pick(d)), "dgrad": TF.family(K.conv2d_pick(TF.dgrad_desc(d)))}
                want = {role: fam for (role, fam), case in SF.SHUFFLE_FAMILY_CASES.items() if case is c}
                assert want and all(got[role] == fam for role, fam in want.items()), (want, got)
                runs = []
                for poison in G.POISONS:
                    a = G.Guard(poison, DEV)
                    runs.append(FG.device_chain(a, c["case"], x, w, b, dy))
                    a.assert_intact()
                assert FG.same_bits(*runs)
            r = runs[0]
            want = B.grads(x, w, dy, r["y"], c["case"][5], c["case"][6])
            assert torch.equal(r["g"], want["g"])
            assert B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])) <= 1.0
            assert B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])) <= 1.0
    assert len(SF.CASES) == 1 and len(SF.SHUFFLE_FAMILY_CASES) == 2
