"""GPU tests of the training-mode batch norm (csrc/batchnorm.hip through pytorch_yolo_amd.kernels, and pytorch_yolo_amd.conv_bn_block)
against the numpy restatement of tests/_bn.py.

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs and the workspace are NaN-filled; the 0xFF
and the 0x7F run give equal bits, and so does a second run.
  exact operands (odd integers in [-7, 7]): mean, running_mean and running_var are bit-equal to the restatement (the float64 sums are
    exact, the rest is IEEE + x / and roundings), invstd is within one fp32 ulp (the device's double sqrt and divide are not assumed to
    be correctly rounded), scale and shift are bit-equal given the device's invstd.
  random operands (per-channel offsets up to 4 standard deviations):  |mean - S| <= 2^-24 |S| + T 2^-53 A / M, the same form for the
    variance - read as running_var after a call with momentum 1 on zeros, i.e. f32(var64 M / (M - 1)), with the bound scaled by
    M / (M - 1) -; y, and g of the backward, torch.equal to the restatement fed with the device's saved (and c1, c2);
    |dgamma - S|, |dbeta - S| <= 2^-24 |S| + T 2^-53 A against float64 sums of the fp32 terms restated from the device's saved.
Op tests: a chain of two conv_bn_block layers and a conv_block head, layer by layer against the restatement fed with the device's
tensors and as a whole against float64 autograd of conv -> batch_norm(training=True) -> leaky_relu; the op's contract; training=False
against conv_block on folded weights and against float64 torch.

Measured on an MI355X, largest error / bound over the six shapes: mean 0.98, variance 0.97, dbeta 0.998, dgamma 0.996,
c1 0.986, c2 0.980 - the float64 sums contribute ~1e-9 of a bound, the rest is the one rounding to fp32, whose half ulp IS 2^-24 |S|
right above a power of two, so the ratios reach ~1 by construction; invstd is bit-equal on 100 % of the channels of the exact cases.
Chain: dgamma 0.815 / 0.819, dbeta 0.910 / 0.843, dW 0.0093 / 0.0085, dx 0.943 / 0.982 of their bounds; against float64 autograd the
device's relative L2 errors equal the yardstick's to five digits (1.0e-2 - 3.7e-2 for the batch-norm layers, 1.7e-3 - 4.7e-3 for the
head).  training=False (the folded layer): bit-equal to conv_block on torch-folded weights; against float64 batch_norm |y - ref| is 0.63 of
its bound and the gradients differ by a relative L2 of 2.7e-3 (x), 1.6e-3 (W), 8.6e-4 (gamma), 6.7e-4 (beta)."""
import functools

import numpy as np
import pytest
import torch

import _bn as N
import _conv_bwd as B
import _guard as G
from pytorch_yolo_amd import _lib, conv_block, conv_bn_block
from pytorch_yolo_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
ACTS = {"leaky": _lib.ACT_LEAKY01, "none": _lib.ACT_NONE}


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.uint8)


def device_bn(a, case, z, gamma, beta, rm, rv, dy=None, dy_dtype=BF16, act="leaky", training=True, momentum=N.MOMENTUM, fill=NAN):
    """Statistics, forward and (with dy) backward of one case on allocations of ``a``.  Returns float32 numpy arrays: saved, rm, rv, y,
    and g, dgamma, dbeta, c12; ``raw``: the bits of every output."""
    m, c = z.shape
    n, h, w, _ = case
    zd = a.like("z", t32(z).to(BF16).reshape(n, h, w, c))
    gd, bd, rmd, rvd = (a.like(name, t32(v)) for name, v in (("gamma", gamma), ("beta", beta), ("running_mean", rm), ("running_var", rv)))
    saved = a.alloc("saved", (4, c), F32, fill)
    nws = K.bn_workspace_bytes(m, c)
    ws = a.alloc("workspace", (nws // 4,), F32, fill)
    if training:
        K.bn_train_stats(zd, gd, bd, N.EPS, momentum, rmd, rvd, saved, ws)
    else:
        K.bn_eval_stats(gd, bd, rmd, rvd, N.EPS, saved)
    y = a.alloc("y", (n, h, w, c), BF16, fill)
    K.bn_act_fwd(zd, saved, y, ACTS[act])
    outs = [saved, rmd, rvd, y]
    r = dict()
    if dy is not None:
        dyd = a.like("dy", t32(dy).to(dy_dtype).reshape(n, h, w, c))
        ws2 = a.alloc("workspace_bwd", (nws // 4,), F32, fill)
        g = a.alloc("g", (n, h, w, c), BF16, fill)
        dgamma, dbeta = a.alloc("dgamma", (c,), F32, fill), a.alloc("dbeta", (c,), F32, fill)
        K.bn_act_bwd(dyd, zd, saved, ACTS[act], training, g, dgamma, dbeta, ws2)
        outs += [g, dgamma, dbeta, ws2]
        r.update(g=g.float().cpu().reshape(m, c).numpy(), dgamma=dgamma.cpu().numpy(), dbeta=dbeta.cpu().numpy(),
                 c12=ws2[:2 * c].cpu().reshape(2, c).numpy())
        assert torch.equal(bits(dyd), bits(t32(dy).to(dy_dtype).reshape(n, h, w, c)))
    torch.cuda.synchronize()
    assert torch.equal(bits(zd), bits(t32(z).to(BF16).reshape(n, h, w, c))) and torch.equal(gd.cpu(), t32(gamma))      # operands are read-only
    if training:
        outs.append(ws)
    r.update(saved=saved.cpu().numpy(), rm=rmd.cpu().numpy(), rv=rvd.cpu().numpy(), y=y.float().cpu().reshape(m, c).numpy(),
             raw=[bits(t) for t in outs])
    return r


def same_bits(r1, r2):
    return len(r1["raw"]) == len(r2["raw"]) and all(torch.equal(p, q) for p, q in zip(r1["raw"], r2["raw"]))


def run_guarded(*args, **kw):
    """One run per poison plus a second run of the first; the bits agree and the margins are intact.  Returns the first run."""
    runs = []
    for poison in G.POISONS + G.POISONS[:1]:
        a = G.Guard(poison, DEV)
        runs.append(device_bn(a, *args, **kw))
        a.assert_intact()
    assert same_bits(runs[0], runs[1]), "the 0xFF and the 0x7F run differ"
    assert same_bits(runs[0], runs[2]), "two runs differ"
    return runs[0]


def check_exact_stats(r, z, gamma, beta, rm, rv):
    """Returns the share of invstd elements that are bit-equal."""
    want = N.stats(z, gamma, beta, rm=rm, rv=rv)
    assert np.array_equal(r["saved"][0], want["mean"]), "mean"
    assert np.array_equal(r["rm"], want["rm"]) and np.array_equal(r["rv"], want["rv"]), "running statistics"
    assert not np.array_equal(r["rm"], rm) and not np.array_equal(r["rv"], rv)
    ulps = N.ulps32(r["saved"][1], want["invstd"])
    assert int(ulps.max()) <= 1, "invstd"
    scale = gamma * r["saved"][1]
    assert np.array_equal(r["saved"][2], scale) and np.array_equal(r["saved"][3], beta - want["mean"] * scale), "scale / shift"
    return float((ulps == 0).mean())


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_exact_statistics(case):
    z, gamma, beta, rm, rv = N.exact_operands(case)
    r = run_guarded(case, z, gamma, beta, rm, rv)
    same = check_exact_stats(r, z, gamma, beta, rm, rv)
    print(f"bn {N.case_id(case)}: invstd bit-equal on {100 * same:.2f} % of the channels")
    assert np.array_equal(r["y"], N.forward(z, r["saved"]))
    plain = device_bn(G.Plain(DEV), case, z, gamma, beta, rm, rv, fill=0.0)              # zero-filled plain allocations: the same outputs
    assert all(torch.equal(p, q) for p, q in zip(r["raw"][:4], plain["raw"][:4]))


@pytest.mark.parametrize("act", ["leaky", "none"])
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_random_forward_within_bounds(case, act):
    z, dy, gamma, beta, rm, rv = N.random_operands(case)
    m, c = z.shape
    zero = np.zeros_like(rv)
    r = run_guarded(case, z, gamma, beta, zero, zero, act=act, momentum=1.0)          # rm <- mean, rv <- f32(var64 M / (M - 1))
    want = N.stats(z, gamma, beta)
    assert np.array_equal(r["rm"], r["saved"][0])
    unbiased = want["var64"] * m / (m - 1)
    ratios = dict(mean=N.ratio(r["saved"][0], want["mean64"], N.bound_mean(want["mean64"], m, want["a1"], m)),
                  var=N.ratio(r["rv"], unbiased, N.bound_mean(unbiased, m, want["s2"], m - 1)))
    print(f"bn {N.case_id(case)} {act}: largest error / bound  mean {ratios['mean']:.4f}  var {ratios['var']:.4f}")
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
    assert int(N.ulps32(r["saved"][1], want["invstd"]).max()) <= 2               # var64 itself differs by its summation order
    assert np.array_equal(r["y"], N.forward(z, r["saved"], act)), "y"
    assert act == "none" or float((N.pre_act(z, r["saved"]) <= 0).mean()) >= 0.15


@pytest.mark.parametrize("training", [True, False], ids=["batch", "running"])
@pytest.mark.parametrize("act", ["leaky", "none"])
@pytest.mark.parametrize("dy_dtype", [BF16, F32], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_backward(case, dy_dtype, act, training):
    z, dy, gamma, beta, rm, rv = N.random_operands(case, dy_dtype)
    m, c = z.shape
    r = run_guarded(case, z, gamma, beta, rm, rv, dy=dy, dy_dtype=dy_dtype, act=act, training=training)
    if not training:
        want = N.eval_saved(gamma, beta, rm, rv)
        assert np.array_equal(r["saved"][0], rm) and int(N.ulps32(r["saved"][1], want[1]).max()) <= 1
        assert np.array_equal(r["saved"][2], gamma * r["saved"][1]) and np.array_equal(r["saved"][3], beta - rm * r["saved"][2])
        assert np.array_equal(r["rm"], rm) and np.array_equal(r["rv"], rv)
    tr = N.backward_terms(dy, z, r["saved"], act)
    assert act == "none" or tr["nonpositive"] >= 0.15
    ratios = dict(dbeta=N.ratio(r["dbeta"], tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])),
                  dgamma=N.ratio(r["dgamma"], tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])))
    if training:
        ratios.update(c1=N.ratio(r["c12"][0], tr["B"] / m, N.bound_mean(tr["B"] / m, m, tr["Ba"], m)),
                      c2=N.ratio(r["c12"][1], tr["G"] / m, N.bound_mean(tr["G"] / m, m, tr["Ga"], m)))
    else:
        assert not r["c12"].any()
    print(f"bn backward {N.case_id(case)} {act} {'batch' if training else 'running'} dy {'bf16' if dy_dtype == BF16 else 'f32'}: largest error / bound  "
          + "  ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
    assert np.array_equal(r["g"], N.backward_apply(tr, r["saved"], r["c12"][0], r["c12"][1])), "g"
    assert r["g"].any() and r["dgamma"].any() and r["dbeta"].any()


def test_split_order_under_other_cu_shares():
    """The split case under two other compute-unit shares: another pick, the same bits on exact operands (the float64 sums are exact in
    any order), within the bounds on random ones."""
    case = N.CASES[N.SPLIT_CASE]
    z, gamma, beta, rm, rv = N.exact_operands(case)
    zr, dyr, gr, br, rmr, rvr = N.random_operands(case)
    m, c = z.shape
    base = device_bn(G.Plain(DEV), case, z, gamma, beta, rm, rv, fill=0.0)
    picks = [K.bn_pick(m, c)]
    try:
        for share in N.CU_SHARES:
            K.set_launch_cus(share)
            picks.append(K.bn_pick(m, c))
            a = G.Guard(G.POISONS[0], DEV)
            r = device_bn(a, case, z, gamma, beta, rm, rv)
            a.assert_intact()
            check_exact_stats(r, z, gamma, beta, rm, rv)
            assert all(torch.equal(p, q) for p, q in zip(r["raw"][:4], base["raw"][:4]))          # saved, rm, rv, y
            a = G.Guard(G.POISONS[0], DEV)
            rr = device_bn(a, case, zr, gr, br, rmr, rvr, dy=dyr)
            a.assert_intact()
            want = N.stats(zr, gr, br)
            tr = N.backward_terms(dyr, zr, rr["saved"])
            assert N.ratio(rr["saved"][0], want["mean64"], N.bound_mean(want["mean64"], m, want["a1"], m)) <= 1.0
            assert N.ratio(rr["dbeta"], tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])) <= 1.0
            assert N.ratio(rr["dgamma"], tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])) <= 1.0
            assert np.array_equal(rr["g"], N.backward_apply(tr, rr["saved"], rr["c12"][0], rr["c12"][1]))
    finally:
        K.set_launch_cus(256)
    assert picks[1] == N.SPLIT_PICKS[8] and picks[2] == N.SPLIT_PICKS[64] and picks[1] != picks[2] and picks[1] != picks[0]


# ---- conv_bn_block ------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def chain_reference():
    ops = N.chain_operands()
    return ops, N.chain_autograd64(ops), N.chain_restated(ops)


def run_chain(ops):
    x0 = _cl(ops["x0"].to(BF16).to(DEV)).requires_grad_()
    par = lambda t: torch.nn.Parameter(t.to(F32).to(DEV))
    W, ga, be = [par(t) for t in ops["W"]], [par(t) for t in ops["gamma"]], [par(t) for t in ops["beta"]]
    wh, bh = par(ops["Wh"]), par(ops["bh"])
    calls = [dict(), dict()]
    keep = lambda store, key: (lambda grad: store.__setitem__(key, grad.detach().clone()))
    x = x0
    for i in range(2):
        alias = x.view_as(x)
        alias.register_hook(keep(calls[i], "dx"))
        y = conv_bn_block(alias, W[i], ga[i], be[i])
        y.register_hook(keep(calls[i], "dy"))
        calls[i].update(x=alias.detach(), y=y.detach())
        x = y
    h = conv_block(x, wh, bh, act="none", out_dtype=F32)
    (h * ops["R"].to(F32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = dict(W1=W[0].grad, gamma1=ga[0].grad, beta1=be[0].grad, W2=W[1].grad, gamma2=ga[1].grad, beta2=be[1].grad, Wh=wh.grad, bh=bh.grad)
    return dict(calls=calls, grads=grads, x0_grad=x0.grad)


@functools.lru_cache(maxsize=None)
def chain_on_device():
    return run_chain(chain_reference()[0])


def test_chain_layer_by_layer():
    """Each conv_bn_block call against the restatement fed with the device's own x, dy: z and saved are the forward's launches repeated
    on the same tensors (two runs give the same bits), y and g are bit-equal, dgamma / dbeta and the conv's dW / dx within their
    bounds.  A second run of the chain gives the same bits."""
    ops = chain_reference()[0]
    run = chain_on_device()
    for i, (c, (cin, cout, k)) in enumerate(zip(run["calls"], N.CHAIN_BN)):
        n, _, h, w = c["x"].shape
        m = n * h * w
        with torch.no_grad():
            z = conv_block(c["x"], ops["W"][i].to(F32).to(DEV), act="none").permute(0, 2, 3, 1).contiguous()
        gamma, beta = ops["gamma"][i].to(F32).numpy(), ops["beta"][i].to(F32).numpy()
        saved = torch.full((4, cout), NAN, dtype=F32, device=DEV)
        ws = torch.full((K.bn_workspace_bytes(m, cout) // 4,), NAN, dtype=F32, device=DEV)
        K.bn_train_stats(z, t32(gamma).to(DEV), t32(beta).to(DEV), N.EPS, N.MOMENTUM, None, None, saved, ws)
        zr, sv = z.float().cpu().reshape(m, cout).numpy(), saved.cpu().numpy()
        assert c["dy"].dtype == BF16 and c["dx"].dtype == BF16 and c["dx"].shape == c["x"].shape
        assert np.array_equal(c["y"].permute(0, 2, 3, 1).float().cpu().reshape(m, cout).numpy(), N.forward(zr, sv)), "y"
        dy = c["dy"].permute(0, 2, 3, 1).contiguous()
        g = torch.full((n, h, w, cout), NAN, dtype=BF16, device=DEV)
        K.bn_act_bwd(dy, z, saved, _lib.ACT_LEAKY01, True, g, None, None, ws)
        c12 = ws[:2 * cout].cpu().reshape(2, cout).numpy()
        tr = N.backward_terms(dy.float().cpu().reshape(m, cout).numpy(), zr, sv)
        assert np.array_equal(g.float().cpu().reshape(m, cout).numpy(), N.backward_apply(tr, sv, c12[0], c12[1])), "g"
        assert 0.15 < tr["nonpositive"] < 0.85
        g64 = g.permute(0, 3, 1, 2).cpu().to(F64)
        conv = B.grads(c["x"].cpu().to(F64), ops["W"][i], g64, None, k, "none")
        gr = run["grads"]
        ratios = dict(dgamma=N.ratio(gr["gamma%d" % (i + 1)].cpu().numpy(), tr["G"], N.bound_sum(tr["G"], m, tr["Ga"])),
                      dbeta=N.ratio(gr["beta%d" % (i + 1)].cpu().numpy(), tr["B"], N.bound_sum(tr["B"], m, tr["Ba"])),
                      dW=B.ratio(gr["W%d" % (i + 1)].cpu(), conv["dw"], B.bound_sum(conv["dw_terms"], conv["dw_abs"])),
                      dx=B.ratio(c["dx"].cpu(), conv["dx_sum"], B.bound_dx(conv["dx_sum"], conv["dx_terms"], conv["dx_abs"])))
        print(f"bn chain layer {i + 1} ({cin} -> {cout}, k{k}): largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in ratios.items()))
        for name, v in ratios.items():
            assert v <= 1.0, (i, name, v)
    assert torch.equal(run["calls"][0]["dy"], run["calls"][1]["dx"]) and torch.equal(run["x0_grad"], run["calls"][0]["dx"])
    again = run_chain(ops)
    for name, t in run["grads"].items():
        assert torch.equal(bits(t), bits(again["grads"][name])), name
    assert torch.equal(bits(run["x0_grad"]), bits(again["x0_grad"]))


def test_chain_vs_float64_autograd():
    """The parameter gradients against float64 autograd of conv -> batch_norm(training=True) -> leaky_relu without any rounding, by
    relative L2 error; the yardstick is the float64 chain with every rounding point restated (tests/test_bn_cpu.py keeps it equal to
    autograd with the rounding off).  The device shares the rounding points - and the LeakyReLU slopes that bf16 rounding flips - and
    has to stay within 1.5 x the yardstick, the rule of the conv_block chain test."""
    ops, want, cpu = chain_reference()
    run = chain_on_device()
    rows = []
    for name in N.CHAIN_PARAMS:
        rows.append((name, B.rel_l2(run["grads"][name].cpu(), want[name]), B.rel_l2(cpu[name], want[name])))
        print("bn chain vs float64 autograd, relative L2 of d%s: device %.4e  float64 chain with the rounding points %.4e" % rows[-1]
              + "  device / chain %.5f" % (rows[-1][1] / rows[-1][2]))
    for name, e_dev, e_cpu in rows:
        assert e_cpu > 0 and e_dev <= 1.5 * e_cpu, (name, e_dev, e_cpu)


def test_conv_bn_block_contract():
    """The op's contract: training=False leaves the running tensors untouched; under no_grad the result has no grad_fn; the running
    statistics after two training calls are the restatement applied twice; a weight-only backward leaves x.grad None and gives the bits
    of the full backward's dW; a second derivative raises; gamma and beta alone get their gradients; one value per channel raises."""
    gen = torch.Generator().manual_seed(7)
    x = _cl(torch.randn((2, 16, 5, 7), generator=gen).to(BF16).to(DEV))
    w = (torch.randn((24, 16, 3, 3), generator=gen) / 12).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(24, generator=gen)).to(DEV), (0.5 * torch.randn(24, generator=gen)).to(DEV)
    rm0, rv0 = torch.randn(24, generator=gen).to(DEV), (0.5 + torch.rand(24, generator=gen)).to(DEV)
    # eval: the running tensors stay
    rm, rv = rm0.clone(), rv0.clone()
    y = conv_bn_block(x, w, gamma, beta, rm, rv, training=False)
    assert y.grad_fn is None and y.dtype == BF16 and y.shape == (2, 24, 5, 7) and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    # training under no_grad: no grad_fn, the running statistics after two calls are the restatement applied twice
    wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (w, gamma, beta))
    with torch.no_grad():
        y1 = conv_bn_block(x, wp, gp, bp, rm, rv)
        z = conv_block(x, w, act="none").permute(0, 2, 3, 1).float().cpu().reshape(-1, 24).numpy()
        y2 = conv_bn_block(x, wp, gp, bp, rm, rv)
    assert y1.grad_fn is None and torch.equal(y1, y2)
    st = N.stats(z, gamma.cpu().numpy(), beta.cpu().numpy(), rm=rm0.cpu().numpy(), rv=rv0.cpu().numpy())
    st = N.stats(z, gamma.cpu().numpy(), beta.cpu().numpy(), rm=st["rm"], rv=st["rv"])
    assert np.array_equal(rm.cpu().numpy(), st["rm"]) and np.array_equal(rv.cpu().numpy(), st["rv"])
    # a weight-only backward leaves x.grad None; a second backward raises
    xg = x.clone().requires_grad_()
    out = conv_bn_block(xg, wp, gamma, beta)
    assert out.grad_fn is not None
    out.float().sum().backward(inputs=[wp], retain_graph=True)
    assert xg.grad is None and wp.grad is not None and wp.grad.dtype == F32 and gp.grad is None
    gx_full, gw_full = torch.autograd.grad(out.float().sum(), [xg, wp], retain_graph=True)
    assert torch.equal(gw_full, wp.grad) and bool(gw_full.any()) and bool(gx_full.any())
    (gx,) = torch.autograd.grad(out.float().square().sum(), [xg], create_graph=True)
    assert gx.dtype == BF16 and gx.shape == x.shape
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()
    # gamma / beta only: the conv's gradients are not computed
    out = conv_bn_block(x, w, gp, bp, rm, rv)
    out.float().square().sum().backward()
    assert gp.grad is not None and bp.grad is not None and gp.grad.dtype == F32 and bool(gp.grad.any()) and bool(bp.grad.any())
    with pytest.raises(ValueError, match="more than 1 value"):
        conv_bn_block(x[:1, :, :1, :1], w, gamma, beta)


def _eval_operands(seed=8):
    gen = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn((2, 16, 5, 7), generator=gen).to(BF16).to(DEV))
    w = (torch.randn((24, 16, 3, 3), generator=gen) / 12).to(DEV)
    gamma, beta = (1 + 0.25 * torch.randn(24, generator=gen)).to(DEV), (0.5 * torch.randn(24, generator=gen)).to(DEV)
    rm, rv = torch.randn(24, generator=gen).to(DEV), (0.5 + torch.rand(24, generator=gen)).to(DEV)
    r = torch.randn((2, 24, 5, 7), generator=gen).to(DEV)
    return x, w, gamma, beta, rm, rv, r


def test_eval_equals_conv_block_on_folded_weights():
    """training=False against conv_block on torch-folded weights (W gamma / sqrt(rv + eps), beta - rm gamma / sqrt(rv + eps)): within
    one bf16 ulp of y, elementwise.  The folded call IS the eval path of the op (normalising the stored bf16 z instead
    differs by up to 3,299 ulp of y where shift cancels z scale - measured - because z's own rounding and the folded weights' do not
    shrink with |y|), so the two agree to the bit; what the fold computes is checked against torch's batch_norm in
    test_eval_against_float64_batch_norm."""
    x, w, gamma, beta, rm, rv, _ = _eval_operands()
    y = conv_bn_block(x, w, gamma, beta, rm, rv, training=False).float()
    s = gamma / torch.sqrt(rv + N.EPS)
    folded = conv_block(x, w * s.reshape(-1, 1, 1, 1), beta - rm * s).float()
    ulp = 2.0 ** (torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126))) - 7)
    err = (y - folded).abs() / ulp
    print(f"bn eval vs folded conv_block: largest |difference| {float(err.max()):.2f} bf16 ulp of y; within one ulp on "
          f"{100 * float((err <= 1).double().mean()):.2f} % of the elements")
    assert bool((err <= 1).all()) and bool(y.any())


def test_eval_against_float64_batch_norm():
    """training=False against float64 torch: conv2d -> batch_norm(training=False) -> leaky_relu on the fp32 master weights.
    Forward, with A = sum |x| |W| |s| and T = 144 terms: the fold rounds W s once to fp32 and once to bf16 (2^-9 + 2^-23), the
    conv accumulates in fp32 ((T + 2) 2^-24 A), s and the folded bias are a handful of fp32 operations (8 2^-24 (A + |shift| + |rm s|)),
    LeakyReLU does not stretch a difference, y is rounded once to bf16:
        |y - ref| <= 2^-9 |ref| + (2^-9 + 2^-23 + (T + 10) 2^-24) A + 8 2^-24 (|beta| + |rm s|)
    Backward of sum(y R): the gradients of x, W, gamma and beta by relative L2 error against float64 autograd.  They pass the bf16
    roundings of W s, y's slope decision, g and dx (2^-9 each, <= 2^-6 even if they added up) and the LeakyReLU slopes that rounding
    flips (a share p of the elements changes g by 0.9 dy: 1.27 sqrt(p) of its norm; p is below 0.4 % as in tests/test_conv_bwd_cpu.py):
    2^-6 + 1.27 sqrt(0.004) <= 0.1 is the ceiling; a dropped term of the fold's chain rule is off by order one."""
    import torch.nn.functional as F
    x, w, gamma, beta, rm, rv, r = _eval_operands()
    xg = x.clone().requires_grad_()
    wp, gp, bp = (torch.nn.Parameter(t.clone()) for t in (w, gamma, beta))
    rm0, rv0 = rm.clone(), rv.clone()
    y = conv_bn_block(xg, wp, gp, bp, rm, rv, training=False)
    (y.float() * r).sum().backward()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    x64, r64 = x.cpu().to(F64).requires_grad_(), r.cpu().to(F64)
    w64, g64, b64 = (t.detach().cpu().to(F64).requires_grad_() for t in (w, gamma, beta))
    rm64, rv64 = rm.cpu().to(F64), rv.cpu().to(F64)
    ref = F.leaky_relu(F.batch_norm(F.conv2d(x64, w64, padding=1), rm64, rv64, g64, b64, False, N.MOMENTUM, N.EPS), 0.1)
    (ref * r64).sum().backward()
    sc = (g64 / torch.sqrt(rv64 + N.EPS)).detach().reshape(1, -1, 1, 1)
    a = F.conv2d(x64.detach().abs(), w64.detach().abs(), padding=1) * sc.abs()
    bound = 2.0 ** -9 * ref.detach().abs() + (2.0 ** -9 + 2.0 ** -23 + 154 * 2.0 ** -24) * a + \
        8 * 2.0 ** -24 * (b64.detach().abs().reshape(1, -1, 1, 1) + (rm64.reshape(1, -1, 1, 1) * sc).abs())
    ratio = float(((y.detach().cpu().to(F64) - ref.detach()).abs() / bound).max())
    print(f"bn eval vs float64 batch_norm: largest |y - ref| / bound {ratio:.4f}")
    assert ratio <= 1.0 and 0.15 < float((ref <= 0).double().mean()) < 0.85
    assert xg.grad.dtype == BF16 and wp.grad.dtype == F32 and gp.grad.dtype == F32 and bp.grad.dtype == F32
    for name, got, want in (("x", xg.grad, x64.grad), ("W", wp.grad, w64.grad), ("gamma", gp.grad, g64.grad), ("beta", bp.grad, b64.grad)):
        e = B.rel_l2(got.cpu(), want)
        print(f"bn eval vs float64 autograd, relative L2 of d{name}: {e:.3e}")
        assert want.any() and e <= 0.1, (name, e)
