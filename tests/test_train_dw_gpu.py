"""GPU tests of the training ops of MobileNetV2's inverted residual: the clamp entries of csrc/batchnorm.hip and
csrc/dw_train.hip through pytorch_yolo_amd.kernels, and conv_bn_relu6_block, dw_bn_block, project_bn_block, against the numpy
restatement of tests/_dw_train.py.

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs and the workspace are NaN-filled; the 0xFF
and the 0x7F run give equal bits, and so does a second run.
  clamp, integer operands with a hand-written saved (mean 0, invstd 1, scale 1, integer shifts): a hits exactly lo, hi and the values
    beside them; y, g, dgamma and dbeta are bit-equal to the restatement; lo = 0, hi = +inf is torch's ReLU rule at a == 0.
  clamp, random operands after yolo_bn_train_stats: y and g torch.equal to the restatement fed with the device's saved (and c1, c2);
    |dgamma - S|, |dbeta - S| <= 2^-24 |S| + T 2^-53 A.
  depthwise, integer operands (x, g in [-7, 7], w in [-2, 2]): dx and dw bit-equal to float64 autograd of F.conv2d(groups=c).
  depthwise, random operands: z (the forward the op runs) and dx torch.equal to the restatement - the fp32 chain in tap order, one RNE -;
    |dw - S| <= 2^-24 |S| + T 2^-53 A against the float64 sum of the exact products; the split cases also under two other
    compute-unit shares.
Op tests: a chain (first layer 3 -> 32 at stride 2, two inverted residuals - stride 2 without and stride 1 with the residual - and a
float32 conv_block head), layer by layer against the restatement fed with the device's own tensors, and as a whole against float64
autograd next to the same chain run through the rounding restatement (reported, no tolerance: the pass conditions are the layer
checks); gradients only where asked; project_bn_block with a residual against conv_bn_block(act="none") followed by an add.

Measured on an MI355X: every bit-equality holds; largest error / bound - clamp dbeta 0.991, dgamma 0.991 over the six
shapes and both dy types; depthwise dw 0.998 over the eight shapes; the chain: dgamma 0.946, dbeta 0.146, depthwise dW 0.992, dense dW
0.023, dx 0.988 (the float64 sums contribute ~1e-9 of a bound, the rest is the one rounding to fp32 or bf16, so the ratios reach ~1 by
construction).  Chain against float64 autograd, relative L2: the device equals the rounding restatement to the five digits printed, 3.8e-3
to 1.1e-1 for the batch-norm layers (dbeta of the second expand 0.11308 on both sides), 1.0e-2 for the head's weight.
project_bn_block with a residual equals conv_bn_block(act="none") followed by a bf16 add in all 1680 elements."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn as N
import _conv_bwd as B
import _dw_train as D
import _guard as G
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.uint8)


def same_bits(r1, r2):
    return len(r1["raw"]) == len(r2["raw"]) and all(torch.equal(p, q) for p, q in zip(r1["raw"], r2["raw"]))


def run_guarded(fn, *args, **kw):
    """One run per poison plus a second run of the first; the bits agree and the margins are intact.  Returns the first run."""
    runs = []
    for poison in G.POISONS + G.POISONS[:1]:
        a = G.Guard(poison, DEV)
        runs.append(fn(a, *args, **kw))
        torch.cuda.synchronize()
        a.assert_intact()
    assert same_bits(runs[0], runs[1]), "the 0xFF and the 0x7F run differ"
    assert same_bits(runs[0], runs[2]), "two runs differ"
    return runs[0]


# ---- the clamp entries -------------------------------------------------------------------------------------------------------------------
def device_clamp(a, case, z, dy, saved=None, vectors=None, lo=0.0, hi=6.0, dy_dtype=BF16, batch_stats=True):
    """Forward and backward of one case on allocations of ``a``; ``saved`` as given, or from yolo_bn_train_stats on ``vectors`` =
    (gamma, beta).  float32 numpy arrays: saved, y, g, dgamma, dbeta, c12; ``raw``: the bits of every output."""
    m, c = z.shape
    n, h, w, _ = case
    zd = a.like("z", t32(z).to(BF16).reshape(n, h, w, c))
    nws = K.bn_workspace_bytes(m, c)
    if saved is None:
        sv = a.alloc("saved", (4, c), F32, NAN)
        ws0 = a.alloc("workspace_stats", (nws // 4,), F32, NAN)
        K.bn_train_stats(zd, a.like("gamma", t32(vectors[0])), a.like("beta", t32(vectors[1])), N.EPS, N.MOMENTUM, None, None, sv, ws0)
    else:
        sv = a.like("saved", t32(saved))
    y = a.alloc("y", (n, h, w, c), BF16, NAN)
    K.bn_clamp_fwd(zd, sv, y, lo, hi)
    dyd = a.like("dy", t32(dy).to(dy_dtype).reshape(n, h, w, c))
    ws = a.alloc("workspace", (nws // 4,), F32, NAN)
    g = a.alloc("g", (n, h, w, c), BF16, NAN)
    dgamma, dbeta = a.alloc("dgamma", (c,), F32, NAN), a.alloc("dbeta", (c,), F32, NAN)
    K.bn_clamp_bwd(dyd, zd, sv, lo, hi, batch_stats, g, dgamma, dbeta, ws)
    torch.cuda.synchronize()
    assert torch.equal(bits(zd), bits(t32(z).to(BF16).reshape(n, h, w, c))) and torch.equal(bits(dyd), bits(t32(dy).to(dy_dtype).reshape(n, h, w, c)))
    return dict(saved=sv.cpu().numpy(), y=y.float().cpu().reshape(m, c).numpy(), g=g.float().cpu().reshape(m, c).numpy(),
                dgamma=dgamma.cpu().numpy(), dbeta=dbeta.cpu().numpy(), c12=ws[:2 * c].cpu().reshape(2, c).numpy(),
                raw=[bits(t) for t in (sv, y, g, dgamma, dbeta, ws)])


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_clamp_at_the_bounds_is_exact(case):
    z, dy, saved = D.clamp_edge_operands(case)
    m = z.shape[0]
    r = run_guarded(device_clamp, case, z, dy, saved=saved)
    a = z + saved[3]
    assert (a == 0).any() and (a == 6).any() and (a == 1).any() and (a == 5).any() and (a == 7).any() and (a == -1).any()
    tr = D.clamp_terms(dy, z, saved)
    assert np.array_equal(r["y"], D.clamp_forward(z, saved)), "y"
    assert np.array_equal(r["dbeta"], tr["B"].astype(np.float32)) and np.array_equal(r["dgamma"], tr["G"].astype(np.float32)), "dgamma / dbeta"
    c1, c2 = N.centre(tr, m, True)
    assert np.array_equal(r["c12"][0], c1) and np.array_equal(r["c12"][1], c2)
    assert np.array_equal(r["g"], N.backward_apply(tr, saved, c1, c2)), "g"
    bad = D.clamp_terms(dy, z, saved, inject="hi")
    assert not np.array_equal(r["dbeta"], bad["B"].astype(np.float32))                     # the slope at a == 6 is 0
    # ReLU (hi = +inf) with running statistics (c1 = c2 = 0, scale 1): g is torch's relu backward, zero at a == 0
    relu = run_guarded(device_clamp, case, z, dy, saved=saved, hi=float("inf"), batch_stats=False)
    at = torch.from_numpy(a.astype(np.float64)).requires_grad_()
    F.relu(at).backward(torch.from_numpy(dy.astype(np.float64)))
    assert np.array_equal(relu["g"], at.grad.numpy()) and np.array_equal(relu["y"], F.relu(at).detach().numpy()) and not relu["c12"].any()


@pytest.mark.parametrize("dy_dtype", [BF16, F32], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_clamp_random_within_bounds(case, dy_dtype):
    z, dy, gamma, beta, rm, rv = N.random_operands(case, dy_dtype)
    gamma, beta = gamma * np.float32(2.0), beta + np.float32(3.0)                          # a ~ N(3, 1..9): both bounds are met
    m, c = z.shape
    r = run_guarded(device_clamp, case, z, dy, vectors=(gamma, beta), dy_dtype=dy_dtype)
    tr = D.clamp_terms(dy, z, r["saved"])
    assert np.array_equal(r["y"], D.clamp_forward(z, r["saved"])), "y"
    ratios = dict(dbeta=N.ratio(r["dbeta"], tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])),
                  dgamma=N.ratio(r["dgamma"], tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])))
    print(f"bn clamp {N.case_id(case)} dy {'bf16' if dy_dtype == BF16 else 'f32'}: clamped {tr['clamped']:.3f}; largest error / bound  "
          + "  ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
    assert np.array_equal(r["g"], N.backward_apply(tr, r["saved"], r["c12"][0], r["c12"][1])), "g"
    assert 0.02 < tr["clamped"] < 0.98 and r["g"].any() and (r["y"] == 0).any() and (r["y"] == 6).any()


# ---- the depthwise entries ----------------------------------------------------------------------------------------------------------------
def device_dw(a, case, x, w, g):
    """Forward (as the op runs it), data gradient and weight gradient of one case on allocations of ``a``: float32 numpy z, dx, dw."""
    n, h, wd, c, stride = case
    ho, wo = D.out_hw(h, wd, stride)
    xd, gd = a.like("x", t32(x).to(BF16)), a.like("g", t32(g).to(BF16))
    w9c = a.like("w9c", t32(w).reshape(c, 9).t().contiguous())
    zero = a.like("bias", torch.zeros(c))
    z = a.alloc("z", (n, ho, wo, c), BF16, NAN)
    K.dwconv3x3(xd, w9c, zero, z, n=n, h=h, w=wd, c=c, in_view=(c, 0), out_view=(c, 0), stride=stride, act=_lib.ACT_NONE)
    dx = a.alloc("dx", (n, h, wd, c), BF16, NAN)
    K.dwconv3x3_bwd_data(gd, w9c, dx, stride)
    ws = a.alloc("workspace", (K.dwconv3x3_bwd_weight_workspace_bytes(*case) // 8,), F64, NAN)
    dw = a.alloc("dw", (c, 1, 3, 3), F32, NAN)
    K.dwconv3x3_bwd_weight(xd, gd, dw, ws, stride)
    torch.cuda.synchronize()
    assert torch.equal(bits(xd), bits(t32(x).to(BF16))) and torch.equal(bits(gd), bits(t32(g).to(BF16)))      # operands are read-only
    return dict(z=z.float().cpu().numpy(), dx=dx.float().cpu().numpy(), dw=dw.cpu().numpy()[:, 0], raw=[bits(t) for t in (z, dx, dw, ws)])


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_depthwise_integer_operands_are_exact(case):
    x, w, g = D.integer_operands(case)
    r = run_guarded(device_dw, case, x, w, g)
    z, dx, dw = D.torch_dw_reference(x, w, g, case[4])
    assert np.array_equal(r["dx"], dx), "dx"
    assert np.array_equal(r["dw"], dw), "dw"
    assert np.array_equal(r["z"], D.bf16(z.astype(np.float32))), "z"
    assert np.abs(dw).max() > 0 and np.abs(dx).max() > 0


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_depthwise_random_operands(case):
    x, w, g = D.random_operands(case)
    r = run_guarded(device_dw, case, x, w, g)
    assert np.array_equal(r["z"], D.dw_forward(x, w, case[4])), "z"
    assert np.array_equal(r["dx"], D.dw_bwd_data(g, w, x.shape, case[4])), "dx"
    want = D.dw_bwd_weight(x, g, case[4])
    ratio = N.ratio(r["dw"], want["S"], D.dw_weight_bound(want))
    print(f"dw {D.case_id(case)}: largest |dw - S| / bound {ratio:.4f}")
    assert ratio <= 1.0 and r["dw"].any()


@pytest.mark.parametrize("i", D.SPLIT_CASES)
def test_depthwise_split_order_under_other_cu_shares(i):
    """The split cases under two other compute-unit shares: another pick, the same bits on integer operands (the float64 sums are exact
    in any order), within the bound on random ones."""
    case = D.CASES[i]
    xi, wi, gi = D.integer_operands(case)
    xr, wr, gr = D.random_operands(case)
    _, dxi, dwi = D.torch_dw_reference(xi, wi, gi, case[4])
    want = D.dw_bwd_weight(xr, gr, case[4])
    try:
        for share in D.CU_SHARES:
            K.set_launch_cus(share)
            assert K.dwconv3x3_bwd_weight_pick(*case) == D.SPLIT_PICKS[(i, share)]
            a = G.Guard(G.POISONS[0], DEV)
            r = device_dw(a, case, xi, wi, gi)
            a.assert_intact()
            assert np.array_equal(r["dw"], dwi) and np.array_equal(r["dx"], dxi)
            a = G.Guard(G.POISONS[1], DEV)
            rr = device_dw(a, case, xr, wr, gr)
            a.assert_intact()
            assert N.ratio(rr["dw"], want["S"], D.dw_weight_bound(want)) <= 1.0
    finally:
        K.set_launch_cus(256)


# ---- the ops ------------------------------------------------------------------------------------------------------------------------------
def _dev_nchw(a, dtype=BF16):
    """NHWC numpy -> NCHW-shaped channels-last tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).permute(0, 3, 1, 2)


def _np(t):
    """NCHW-shaped device tensor -> float32 NHWC numpy."""
    return t.detach().permute(0, 2, 3, 1).float().cpu().contiguous().numpy()


@functools.lru_cache(maxsize=None)
def chain_reference():
    ops = D.chain_operands()
    return ops, D.chain_autograd64(ops), D.chain_restated(ops)


def run_chain(ops):
    par = lambda a, shape=None: torch.nn.Parameter(torch.from_numpy(np.asarray(a, dtype=np.float32)).reshape(shape or a.shape).to(DEV))
    P = {}
    for name, kind, cin, cout, k, stride in D.CHAIN:
        P["W_" + name] = par(ops["W"][name], (cout, 1, 3, 3) if kind == "dw" else None)
        P["gamma_" + name], P["beta_" + name] = par(ops["gamma"][name]), par(ops["beta"][name])
    P["Wh"], P["bh"] = par(ops["Wh"]), par(ops["bh"])
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))
    calls, x, res = {}, _dev_nchw(ops["x0"].astype(np.float32)), None
    for name, kind, cin, cout, k, stride in D.CHAIN:
        c = calls[name] = dict()
        alias = x.view_as(x)
        if alias.requires_grad:
            alias.register_hook(keep(c, "dx"))
        args = (alias, P["W_" + name], P["gamma_" + name], P["beta_" + name])
        if kind == "dense":
            y = Y.conv_bn_relu6_block(*args, stride=stride)
        elif kind == "dw":
            y = Y.dw_bn_block(*args, stride=stride)
        else:
            r_alias = None if res is None else res.view_as(res)
            if r_alias is not None:
                r_alias.register_hook(keep(c, "dres"))
                c["res"] = r_alias.detach()
            y = Y.project_bn_block(*args, None, None, r_alias)
            res = y
        y.register_hook(keep(c, "dy"))
        c.update(x=alias.detach(), y=y.detach())
        x = y
    h = Y.conv_block(x, P["Wh"], P["bh"], act="none", out_dtype=F32)
    (h * _dev_nchw(ops["R"], F32)).sum().backward()
    torch.cuda.synchronize()
    return dict(calls=calls, grads={k_: v.grad for k_, v in P.items()})


@functools.lru_cache(maxsize=None)
def chain_on_device():
    return run_chain(chain_reference()[0])


def _bn_layer(c, z, gamma, beta, act):
    """The BN part of one op call from the device's own z and dy: checks y and g bit for bit, returns (g as NHWC float32, terms)."""
    n, h, w, cout = z.shape
    m = n * h * w
    saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
    ws = torch.full((K.bn_workspace_bytes(m, cout) // 4,), NAN, dtype=F32, device=DEV)
    K.bn_train_stats(z, t32(gamma).to(DEV), t32(beta).to(DEV), N.EPS, N.MOMENTUM, None, None, saved, ws)
    zr, sv = z.float().cpu().reshape(m, cout).numpy(), saved.cpu().numpy()
    dy = c["dy"].permute(0, 2, 3, 1).contiguous()
    dyr = dy.float().cpu().reshape(m, cout).numpy()
    g = torch.full((n, h, w, cout), NAN, dtype=BF16, device=DEV)
    if act == "relu6":
        K.bn_clamp_bwd(dy, z, saved, 0.0, 6.0, True, g, None, None, ws)
        tr, y = D.clamp_terms(dyr, zr, sv), D.clamp_forward(zr, sv)
    else:
        K.bn_act_bwd(dy, z, saved, _lib.ACT_NONE, True, g, None, None, ws)
        tr, y = N.backward_terms(dyr, zr, sv, "none"), N.forward(zr, sv, "none")
        if "res" in c:
            y = D.bf16(y + _np(c["res"]).reshape(m, cout))                   # bf16(a), then the add, rounded once
    c12 = ws[:2 * cout].cpu().reshape(2, cout).numpy()
    assert np.array_equal(_np(c["y"]).reshape(m, cout), y), "y"
    gr = g.float().cpu().reshape(m, cout).numpy()
    assert np.array_equal(gr, N.backward_apply(tr, sv, c12[0], c12[1])), "g"
    return gr.reshape(n, h, w, cout), tr, m


def test_chain_layer_by_layer():
    """Each op call against the restatement fed with the device's own x and dy: z and saved are the forward's launches repeated on the same
    tensors, y and g are bit-equal, the depthwise dx is bit-equal, dgamma / dbeta, the depthwise dW and the dense convs' dW / dx are
    within their bounds; the residual's gradient is the incoming one; a second run of the chain gives the same bits."""
    ops = chain_reference()[0]
    run = chain_on_device()
    gr = run["grads"]
    for name, kind, cin, cout, k, stride in D.CHAIN:
        c = run["calls"][name]
        w = ops["W"][name].astype(np.float32)
        x = c["x"]
        assert c["dy"].dtype == BF16 and c["y"].dtype == BF16
        with torch.no_grad():
            if kind == "dw":
                xn = x.permute(0, 2, 3, 1)
                n, h, wd, ch = xn.shape
                ho, wo = D.out_hw(h, wd, stride)
                wq = D.bf16(w)
                z = torch.full((n, ho, wo, ch), NAN, dtype=BF16, device=DEV)
                K.dwconv3x3(xn, t32(wq).reshape(ch, 9).t().contiguous().to(DEV), torch.zeros(ch, device=DEV), z, n=n, h=h, w=wd, c=ch,
                            in_view=(ch, 0), out_view=(ch, 0), stride=stride, act=_lib.ACT_NONE)
                assert np.array_equal(z.float().cpu().numpy(), D.dw_forward(_np(x), wq, stride)), (name, "z")
            else:
                wt = t32(w).to(DEV)
                z = (Y.down_block(x, wt, act="none") if stride == 2 else Y.conv_block(x, wt, act="none")).permute(0, 2, 3, 1).contiguous()
        g, tr, m = _bn_layer(c, z, ops["gamma"][name].astype(np.float32), ops["beta"][name].astype(np.float32), "none" if kind == "project" else "relu6")
        ratios = dict(dgamma=N.ratio(gr["gamma_" + name].cpu().numpy(), tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])),
                      dbeta=N.ratio(gr["beta_" + name].cpu().numpy(), tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])))
        if kind == "dw":
            assert np.array_equal(_np(c["dx"]), D.dw_bwd_data(g, wq, _np(x).shape, stride)), (name, "dx")
            want = D.dw_bwd_weight(_np(x), g, stride)
            ratios["dW"] = N.ratio(gr["W_" + name].cpu().numpy()[:, 0], want["S"], D.dw_weight_bound(want))
        else:
            _, _, q = D.dense_backward(_np(x), w, g, stride)
            tq = lambda key: torch.from_numpy(q[key])
            ratios["dW"] = B.ratio(gr["W_" + name].cpu(), tq("dw"), B.bound_sum(tq("dw_terms"), tq("dw_abs")))
            if "dx" in c:
                ratios["dx"] = B.ratio(torch.from_numpy(_np(c["dx"])), tq("dx"), B.bound_dx(tq("dx"), tq("dx_terms"), tq("dx_abs")))
        if "res" in c:
            assert torch.equal(c["dres"], c["dy"]), "the residual's gradient is dy"
        print(f"dw chain {name} ({kind} {cin} -> {cout}, k{k} s{stride}): clamped {tr.get('clamped', 0.0):.3f}; largest error / bound  "
              + "  ".join(f"{k_} {v:.4f}" for k_, v in ratios.items()))
        for key, v in ratios.items():
            assert v <= 1.0, (name, key, v)
    assert "dx" not in run["calls"]["stem"] and "dres" in run["calls"]["p2"] and "res" not in run["calls"]["p1"]
    again = run_chain(ops)
    for key, t in gr.items():
        assert torch.equal(bits(t), bits(again["grads"][key])), key


def test_chain_vs_float64_autograd():
    """The parameter gradients against float64 autograd of the same chain without any rounding, by relative L2 error, next to those of
    the float64 chain with every rounding point restated.  Reported, not bounded: a clamp decision that one bf16 rounding flips moves a
    gradient by all of dy, on either side; the pass conditions are test_chain_layer_by_layer's.  (Rounding off, the restated chain equals
    autograd to 1e-14: tests/test_train_dw_cpu.py.)"""
    ops, want, cpu = chain_reference()
    run = chain_on_device()
    for name in D.chain_param_names():
        got = run["grads"][name].double().cpu().numpy().reshape(want[name].shape)
        e_dev, e_cpu = D.rel_l2(got, want[name]), D.rel_l2(cpu[name].reshape(want[name].shape), want[name])
        print(f"dw chain vs float64 autograd, relative L2 of d{name}: device {e_dev:.4e}  float64 chain with the rounding points {e_cpu:.4e}")
        assert np.isfinite(got).all() and got.any() and e_dev < 1.0, name


def _dw_operands(seed=5, c=16, h=5, w=7):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((2, c, h, w), generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    wd = (torch.randn((c, 1, 3, 3), generator=gen) / 3).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(c, generator=gen)).to(DEV), (2 + 0.5 * torch.randn(c, generator=gen)).to(DEV)
    return x, wd, gamma, beta


def test_gradients_only_where_asked():
    """A frozen depthwise weight launches no depthwise weight gradient, an x that needs no gradient launches no data gradient; under
    no_grad nothing is recorded; the running statistics move; a second derivative raises."""
    x, wd, gamma, beta = _dw_operands()
    launches = []
    names = ("dwconv3x3_bwd_weight", "dwconv3x3_bwd_data", "bn_clamp_bwd", "bn_act_bwd")
    real = {n: getattr(K, n) for n in names}
    try:
        for n in names:
            setattr(K, n, (lambda n: lambda *a, **kw: (launches.append(n), real[n](*a, **kw))[1])(n))
        for need_x, need_w, need_g, act in ((True, False, False, "relu6"), (False, True, False, "relu6"), (False, False, True, "relu6"),
                                            (True, True, True, "none")):
            xg, wp = x.clone().requires_grad_(need_x), wd.clone().requires_grad_(need_w)
            gp, bp = gamma.clone().requires_grad_(need_g), beta.clone().requires_grad_(need_g)
            del launches[:]
            y = Y.dw_bn_block(xg, wp, gp, bp, stride=2, act=act)
            assert y.shape == (2, 16, 3, 4) and y.dtype == BF16 and y.permute(0, 2, 3, 1).is_contiguous()
            y.float().square().sum().backward()
            assert launches.count("dwconv3x3_bwd_weight") == int(need_w) and launches.count("dwconv3x3_bwd_data") == int(need_x)
            assert launches.count("bn_clamp_bwd") == int(act == "relu6") and launches.count("bn_act_bwd") == int(act == "none")
            assert (xg.grad is not None) == need_x and (wp.grad is not None) == need_w and (gp.grad is not None) == need_g
            if need_x:
                assert xg.grad.dtype == BF16 and xg.grad.shape == x.shape and bool(xg.grad.any())
            if need_w:
                assert wp.grad.dtype == F32 and wp.grad.shape == wd.shape and bool(wp.grad.any())
    finally:
        for n in names:
            setattr(K, n, real[n])
    rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    with torch.no_grad():
        y = Y.dw_bn_block(x, torch.nn.Parameter(wd), gamma, beta, rm, rv)
    assert y.grad_fn is None and bool((rm != 0).all()) and bool((rv != 1).all())
    xg = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(Y.dw_bn_block(xg, wd, gamma, beta).float().square().sum(), [xg], create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()


def _project_operands():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((2, 48, 5, 7), generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    res = torch.randn((2, 24, 5, 7), generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn((24, 48, 1, 1), generator=gen) / 7).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(24, generator=gen)).to(DEV), (0.5 * torch.randn(24, generator=gen)).to(DEV)
    return x, res, w, gamma, beta


def test_project_bn_block_contract():
    """Without a residual the op is conv_bn_block(act="none"), bit for bit, outputs and gradients.  With one, y = bf16(f32(bf16(a)) +
    f32(residual)) with a the normalised fp32 value (the restatement fed with the device's z and saved; guarded operands for the launch
    itself), the gradients of x, the weight, gamma and beta are conv_bn_block(act="none")'s for the same dy, and the residual's is dy."""
    x, res, w, gamma, beta = _project_operands()
    dy = torch.randn((2, 24, 5, 7), generator=torch.Generator().manual_seed(10)).to(BF16).to(DEV)
    outs = []
    for r in (None, res, "conv_bn_block"):
        xg, wp, gp, bp = (t.clone().requires_grad_() for t in (x, w, gamma, beta))
        rg = None if not isinstance(r, torch.Tensor) else r.clone().requires_grad_()
        y = Y.conv_bn_block(xg, wp, gp, bp, act="none") if isinstance(r, str) else Y.project_bn_block(xg, wp, gp, bp, residual=rg)
        y.backward(dy)
        outs.append((y.detach(), [t.grad for t in (xg, wp, gp, bp)], rg))
    plain, fused, ref = outs
    assert torch.equal(bits(plain[0]), bits(ref[0])) and all(torch.equal(bits(p), bits(q)) for p, q in zip(plain[1], ref[1]))
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(fused[1], ref[1])) and torch.equal(fused[2].grad, dy)
    with torch.no_grad():
        z = Y.conv_block(x, w, act="none").permute(0, 2, 3, 1).contiguous()
    saved = torch.empty((4, 24), dtype=F32, device=DEV)
    ws = torch.empty((K.bn_workspace_bytes(70, 24),), dtype=torch.uint8, device=DEV)
    K.bn_train_stats(z, gamma, beta, N.EPS, N.MOMENTUM, None, None, saved, ws)
    a = N.pre_act(z.float().cpu().reshape(70, 24).numpy(), saved.cpu().numpy())
    want = D.bf16(D.bf16(a) + _np(res).reshape(70, 24))
    assert np.array_equal(_np(fused[0]).reshape(70, 24), want)
    assert not np.array_equal(want, D.bf16(a + _np(res).reshape(70, 24)))                 # the operands tell the two rounding orders apart
    raws = []
    for poison in G.POISONS + G.POISONS[:1]:                                               # the launch itself between the guard bands
        g = G.Guard(poison, DEV)
        zd, sd, rd = g.like("z", z), g.like("saved", saved), g.like("residual", res.permute(0, 2, 3, 1).contiguous())
        yd = g.alloc("y", z.shape, BF16, NAN)
        K.bn_add_rounded_fwd(zd, sd, rd, yd)
        torch.cuda.synchronize()
        g.assert_intact()
        raws.append(bits(yd))
        assert np.array_equal(yd.float().cpu().reshape(70, 24).numpy(), want)
    assert torch.equal(raws[0], raws[1]) and torch.equal(raws[0], raws[2])


def test_project_bn_block_equals_conv_bn_block_then_add():
    """project_bn_block with a residual against conv_bn_block(act="none") followed by a bf16 add done as one fp32 add and one rounding,
    bit for bit.  (The pass rounds the normalised value to bf16 before the add for this reason: yolo_bn_add_rounded_fwd.  Adding to the
    fp32 value and rounding once, as yolo_bn_act_add_fwd does for res_bn_block, differed in 510 of these 1680 elements.)"""
    x, res, w, gamma, beta = _project_operands()
    with torch.no_grad():
        fused = Y.project_bn_block(x, w, gamma, beta, residual=res)
        two_step = (Y.conv_bn_block(x, w, gamma, beta, act="none").float() + res.float()).to(BF16)
        bf16_add = Y.conv_bn_block(x, w, gamma, beta, act="none") + res
    differ = int((bits(fused) != bits(two_step)).sum())
    print(f"project_bn_block vs conv_bn_block(act none) + add: {differ} of {fused.numel()} elements differ")
    assert differ == 0 and torch.equal(bits(fused), bits(bf16_add)) and bool(fused.any())
