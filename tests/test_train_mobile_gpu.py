"""GPU tests of the training-mode forward and backward of YOLOv3-tiny/MobileNetV2: the two entries of csrc/dw_train.hip
that take a batch-normed operand, expand_dw_bn_block, and forward_train(model, x, ops=DEVICE_OPS_MOBILE).

Kernel tests: every operand sits between the poisoned bands of tests/_guard.py, the outputs and the workspace are NaN-filled; the 0xFF
and the 0x7F run give equal bits, and so does a second run.  Every test is a plain parity run.
  the two entries against the materialised form - yolo_bn_clamp_fwd into a y buffer, then yolo_dwconv3x3_fwd / yolo_dwconv3x3_bwd_weight
    on it: z and dw bit-equal on integer and on random operands, on tests/_dw_train.CASES (the split shapes also under 8 and 64 compute
    units) and on four more shapes (windows that are mostly padding, a partial second strip at either stride).  On the integer operands
    (scale 1, shifts in [1, 4] that differ from channel to channel) every value is exact: z equals tests/_dw_train.dw_forward of the
    restated y and dw the float64 autograd value; with every shift >= 1 a kernel that pads with clamp(shift) cannot pass, and the
    restatement with that fault injected differs.  One case with hi = +inf.
  the op against dw_bn_block(conv_bn_relu6_block(..)) on the same operands at both strides: the output, the seven gradients and the four
    running tensors bit-equal; gradients only where asked; the forward holds at least one hidden map less.
  the model: one step of YOLOv3TinyMobile(n_class=2) at 64 x 96 with every op call recorded and held to its restatement fed with the
    device's own inputs (bit-equal y, g, running statistics and depthwise dx; the float64-sum gradients within the bounds of
    tests/_bn.py / tests/_dw_train.py / tests/_conv_bwd.py; a fused call bit-equal to the composed form re-run on its inputs, whose two
    calls are held to the restatement in turn); a second step gives the same bits; no stale plan; what keeps raising.
The conv families: tests/_train_mobile_families.MOBILE_FAMILY_CASES through the runner of tests/test_train_fire_gpu.py.
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
import _train_mobile as M
import _train_mobile_families as MF
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.models import train as MT
from test_train_dw_gpu import BF16, DEV, F32, F64, NAN, _np, bits, run_guarded, t32
from test_train_pool_gpu import check_calls, recording_pool_ops

pytestmark = pytest.mark.gpu
INF = float("inf")


# ---- the two entries against the materialised form ------------------------------------------------------------------------------------------
def device_bnin(a, case, zin, saved, w, g, lo=0.0, hi=6.0):
    """The fused forward and weight gradient and the materialised form of one case on allocations of ``a``: float32 numpy y, z, dw (fused)
    and z_m, dw_m (materialised)."""
    n, h, wd, c, stride = case
    ho, wo = D.out_hw(h, wd, stride)
    zd, gd, sv = a.like("zin", t32(zin).to(BF16)), a.like("g", t32(g).to(BF16)), a.like("saved", t32(saved))
    w9c = a.like("w9c", t32(w).reshape(c, 9).t().contiguous())
    nws = K.dwconv3x3_bwd_weight_workspace_bytes(*case) // 8
    z = a.alloc("z", (n, ho, wo, c), BF16, NAN)
    K.dwconv3x3_bnin_fwd(zd, sv, lo, hi, w9c, z, stride)
    ws, dw = a.alloc("workspace", (nws,), F64, NAN), a.alloc("dw", (c, 1, 3, 3), F32, NAN)
    K.dwconv3x3_bnin_bwd_weight(zd, sv, lo, hi, gd, dw, ws, stride)
    y = a.alloc("y", (n, h, wd, c), BF16, NAN)
    K.bn_clamp_fwd(zd, sv, y, lo, hi)
    z_m = a.alloc("z_m", (n, ho, wo, c), BF16, NAN)
    K.dwconv3x3(y, w9c, a.like("bias", torch.zeros(c)), z_m, n=n, h=h, w=wd, c=c, in_view=(c, 0), out_view=(c, 0), stride=stride, act=_lib.ACT_NONE)
    ws_m, dw_m = a.alloc("workspace_m", (nws,), F64, NAN), a.alloc("dw_m", (c, 1, 3, 3), F32, NAN)
    K.dwconv3x3_bwd_weight(y, gd, dw_m, ws_m, stride)
    torch.cuda.synchronize()
    assert torch.equal(bits(zd), bits(t32(zin).to(BF16))) and torch.equal(bits(gd), bits(t32(g).to(BF16)))      # operands are read-only
    assert torch.equal(bits(z), bits(z_m)), f"z: {int((bits(z) != bits(z_m)).sum())} of {z.numel()} elements differ from the materialised form"
    assert torch.equal(bits(dw), bits(dw_m)), "dw differs from the materialised form"
    assert torch.equal(bits(ws), bits(ws_m)), "the partials differ from the materialised form"
    return dict(y=y.float().cpu().numpy(), z=z.float().cpu().numpy(), dw=dw.cpu().numpy()[:, 0], raw=[bits(t) for t in (z, dw, ws, y, z_m, dw_m)])


def check_integer(case, r, zin, saved, w, g, lo=0.0, hi=6.0):
    y = M.bnin_operand(zin, saved, lo, hi)
    assert np.array_equal(r["y"], y)
    if y.size >= 256:                                                         # (a 1 x 1 map of 8 channels need not hold both bounds)
        assert (y == lo).any() and (hi == INF or (y == hi).any())
    assert np.array_equal(r["z"], D.dw_forward(y, w, case[4])), "z"
    z64, _, dw64 = D.torch_dw_reference(y, w, g, case[4])
    assert np.array_equal(r["z"], z64) and np.array_equal(r["dw"], dw64), "z / dw against float64 autograd"
    # the fault the operands are built to show: the padding taken as clamp(shift) (every shift is >= 1)
    assert not np.array_equal(r["z"], M.fused_forward(zin, saved, w, case[4], lo, hi, inject="pad"))
    assert not np.array_equal(r["dw"], M.fused_bwd_weight(zin, saved, g, case[4], lo, hi, inject="pad")["dw"])


@pytest.mark.parametrize("case", M.KERNEL_CASES, ids=D.case_id)
def test_entries_equal_the_materialised_form_on_integer_operands(case):
    zin, saved, w, g = M.integer_operands(case)
    r = run_guarded(device_bnin, case, zin, saved, w, g)
    check_integer(case, r, zin, saved, w, g)
    assert len(set(saved[3][:8])) == 4 and (case[3] == 8 or not np.array_equal(saved[3][:8], saved[3][8:16]))


@pytest.mark.parametrize("case", M.KERNEL_CASES, ids=D.case_id)
def test_entries_equal_the_materialised_form_on_random_operands(case):
    zin, saved, w, g = M.random_operands(case)
    r = run_guarded(device_bnin, case, zin, saved, w, g)
    y = M.bnin_operand(zin, saved)
    assert np.array_equal(r["y"], y) and np.array_equal(r["z"], D.dw_forward(y, w, case[4])), "z against the restatement"
    want = D.dw_bwd_weight(y, g, case[4])
    ratio = N.ratio(r["dw"], want["S"], D.dw_weight_bound(want))
    print(f"dw bnin {D.case_id(case)}: largest |dw - S| / bound {ratio:.4f}")
    assert ratio <= 1.0 and r["dw"].any() and (y.size < 256 or ((y == 0).any() and (y == 6).any()))


def test_entries_with_an_open_upper_bound():
    """hi = +inf (ReLU): the same parity on an odd map at stride 2."""
    case = D.CASES[2]
    zin, saved, w, g = M.integer_operands(case)
    r = run_guarded(device_bnin, case, zin, saved, w, g, hi=INF)
    check_integer(case, r, zin, saved, w, g, hi=INF)
    assert r["y"].max() == 8.0


@pytest.mark.parametrize("i", D.SPLIT_CASES)
def test_weight_gradient_split_under_other_cu_shares(i):
    case = D.CASES[i]
    zi, si, wi, gi = M.integer_operands(case)
    zr, sr, wr, gr = M.random_operands(case)
    try:
        for share in D.CU_SHARES:
            K.set_launch_cus(share)
            assert K.dwconv3x3_bwd_weight_pick(*case) == D.SPLIT_PICKS[(i, share)]
            a = G.Guard(G.POISONS[0], DEV)
            r = device_bnin(a, case, zi, si, wi, gi)
            a.assert_intact()
            check_integer(case, r, zi, si, wi, gi)
            a = G.Guard(G.POISONS[1], DEV)
            device_bnin(a, case, zr, sr, wr, gr)
            a.assert_intact()
    finally:
        K.set_launch_cus(256)


# ---- the op -------------------------------------------------------------------------------------------------------------------------------
NAMES = ("x", "w_expand", "gamma1", "beta1", "w_dw", "gamma2", "beta2")
OP_CASES = [((2, 24, 6, 8), 144, 1), ((2, 24, 6, 8), 144, 2), ((2, 16, 5, 7), 96, 1), ((2, 16, 5, 7), 96, 2)]


def op_operands(shape, hidden, seed=11):
    gen = torch.Generator().manual_seed(seed)
    n, cin, h, w = shape
    x = torch.randn(shape, generator=gen).to(BF16).to(DEV).contiguous(memory_format=torch.channels_last)
    we = (torch.randn((hidden, cin, 1, 1), generator=gen) / cin ** 0.5).to(DEV)
    wd = (torch.randn((hidden, 1, 3, 3), generator=gen) / 3).to(DEV)
    vec = lambda mean, std: (mean + std * torch.randn(hidden, generator=gen)).to(DEV)
    return [x, we, vec(1.5, 0.25), vec(2.5, 1.0), wd, vec(1.5, 0.25), vec(2.5, 1.0)]


def run_op(fn, operands, stride, dy, needs=(True,) * 7):
    leaves = [t.clone().requires_grad_(need) for t, need in zip(operands, needs)]
    hidden = operands[1].shape[0]
    running = [torch.full((hidden,), v, device=DEV) for v in (0.25, 1.5, -0.5, 0.75)]
    x, we, g1, b1, wd, g2, b2 = leaves
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    y = fn(x, we, g1, b1, running[0], running[1], wd, g2, b2, running[2], running[3], stride=stride, momentum=(0.1, 0.3), eps=(1e-5, 1e-3))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    if any(needs):
        y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), [t.grad for t in leaves], running, held


@pytest.mark.parametrize("shape,hidden,stride", OP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_op_equals_the_composition(shape, hidden, stride):
    operands = op_operands(shape, hidden)
    ho, wo = D.out_hw(shape[2], shape[3], stride)
    dy = torch.randn((shape[0], hidden, ho, wo), generator=torch.Generator().manual_seed(12)).to(BF16).to(DEV)
    composed = MT.mobile_ops(fused=False).expand_dw_bn_block
    assert MT.mobile_ops().expand_dw_bn_block is Y.expand_dw_bn_block and composed is not Y.expand_dw_bn_block
    y, grads, running, held = run_op(Y.expand_dw_bn_block, operands, stride, dy)
    y_c, grads_c, running_c, held_c = run_op(composed, operands, stride, dy)
    assert y.dtype == BF16 and tuple(y.shape) == (shape[0], hidden, ho, wo) and y.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(bits(y), bits(y_c)) and bool((y == 0).any()) and bool((y == 6).any())
    for name, a, b in zip(NAMES, grads, grads_c):
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)) and bool(a.any()), name
    for a, b, start in zip(running, running_c, (0.25, 1.5, -0.5, 0.75)):
        assert torch.equal(bits(a), bits(b)) and bool((a != start).all())
    y1_bytes = shape[0] * hidden * shape[2] * shape[3] * 2
    print(f"expand_dw_bn_block {shape} hidden {hidden} stride {stride}: bytes held after the forward {held} (composed {held_c}, y1 {y1_bytes})")
    assert held <= held_c - y1_bytes
    again = run_op(Y.expand_dw_bn_block, operands, stride, dy)
    assert torch.equal(bits(y), bits(again[0])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, again[1]))


def test_op_gradients_only_where_asked():
    """Every single gradient alone, and none: what is not asked for is None and the launches that serve only it do not run; what is asked
    for is bit-equal to the composed form's; under no_grad nothing is recorded; a second derivative raises."""
    shape, hidden, stride = OP_CASES[1]
    operands = op_operands(shape, hidden)
    dy = torch.randn((2, hidden, 3, 4), generator=torch.Generator().manual_seed(13)).to(BF16).to(DEV)
    composed = MT.mobile_ops(fused=False).expand_dw_bn_block
    launches = []
    names = ("dwconv3x3_bnin_bwd_weight", "dwconv3x3_bwd_data", "bn_clamp_bwd", "conv2d_bwd_weight", "conv2d_bwd_data", "dwconv3x3_bwd_weight")
    real = {n: getattr(K, n) for n in names}
    try:
        for n in names:
            setattr(K, n, (lambda n: lambda *a, **kw: (launches.append(n), real[n](*a, **kw))[1])(n))
        for i in range(7):
            needs = tuple(j == i for j in range(7))
            del launches[:]
            _, grads, _, _ = run_op(Y.expand_dw_bn_block, operands, stride, dy, needs)
            count = {n: launches.count(n) for n in names}
            _, grads_c, _, _ = run_op(composed, operands, stride, dy, needs)
            assert [g is not None for g in grads] == list(needs), NAMES[i]
            assert torch.equal(bits(grads[i]), bits(grads_c[i])), NAMES[i]
            upstream = i < 4                                                                 # x, w_expand, gamma1, beta1: through y1
            assert count["dwconv3x3_bnin_bwd_weight"] == int(i == 4) and count["dwconv3x3_bwd_weight"] == 0, (NAMES[i], count)
            assert count["dwconv3x3_bwd_data"] == int(upstream) and count["bn_clamp_bwd"] == 1 + int(upstream), (NAMES[i], count)
            assert count["conv2d_bwd_weight"] == int(i == 1) and count["conv2d_bwd_data"] == int(i == 0), (NAMES[i], count)
    finally:
        for n in names:
            setattr(K, n, real[n])
    with torch.no_grad():
        y = Y.expand_dw_bn_block(*operands[:4], None, None, *operands[4:], None, None, stride=stride)
    assert y.grad_fn is None
    y2, _, _, _ = run_op(Y.expand_dw_bn_block, operands, stride, dy, (False,) * 7)
    assert y2.grad_fn is None
    xg = operands[0].clone().requires_grad_()
    out = Y.expand_dw_bn_block(xg, *operands[1:4], None, None, *operands[4:], None, None)
    (gx,) = torch.autograd.grad(out.float().square().sum(), [xg], create_graph=True)
    with pytest.raises(RuntimeError):
        gx.float().sum().backward()
    with pytest.raises(ValueError, match="expand_dw_bn_block"):
        Y.expand_dw_bn_block(*operands[:4], None, None, operands[4][:8], *operands[5:], None, None)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
H, W, BS = 64, 96, 2


def new_model():
    model = M.training_model(custom_bn=False)
    model.hyper_params = dict(L.HYPER)
    return model.to(DEV).train()


def model_inputs(model):
    return M.step_inputs(BS, H, W, model.n_class)


def recording_mobile_ops(calls):
    """tests/test_train_pool_gpu.recording_pool_ops with the four functions of DEVICE_OPS_MOBILE recorded the same way."""
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

    def bn_state(rm, rv):
        return dict(rm0=rm.detach().clone(), rv0=rv.detach().clone(), rm=rm, rv=rv)

    def conv_bn_relu6_block(x, w, gamma, beta, rm, rv, *, stride=1, momentum=0.1, eps=1e-5):
        rec = dict(kind="relu6", stride=stride, momentum=momentum, eps=eps, params=dict(w=w, gamma=gamma, beta=beta), **bn_state(rm, rv))
        calls.append(rec)
        return watch(rec, "y", Y.conv_bn_relu6_block(alias(rec, "x", x), w, gamma, beta, rm, rv, stride=stride, momentum=momentum, eps=eps))

    def dw_bn_block(x, w, gamma, beta, rm, rv, *, stride=1, momentum=0.1, eps=1e-5):
        rec = dict(kind="dw", stride=stride, momentum=momentum, eps=eps, params=dict(w=w, gamma=gamma, beta=beta), **bn_state(rm, rv))
        calls.append(rec)
        return watch(rec, "y", Y.dw_bn_block(alias(rec, "x", x), w, gamma, beta, rm, rv, stride=stride, momentum=momentum, eps=eps))

    def project_bn_block(x, w, gamma, beta, rm, rv, residual=None, *, momentum=0.1, eps=1e-5):
        rec = dict(kind="project", stride=1, momentum=momentum, eps=eps, params=dict(w=w, gamma=gamma, beta=beta), **bn_state(rm, rv))
        calls.append(rec)
        return watch(rec, "y", Y.project_bn_block(alias(rec, "x", x), w, gamma, beta, rm, rv, alias(rec, "res", residual), momentum=momentum, eps=eps))

    def expand_dw_bn_block(x, we, g1, b1, rm1, rv1, wd, g2, b2, rm2, rv2, *, stride=1, momentum=0.1, eps=1e-5):
        rec = dict(kind="expand", stride=stride, momentum=momentum, eps=eps, params=(we, g1, b1, wd, g2, b2),
                   running0=[t.detach().clone() for t in (rm1, rv1, rm2, rv2)], running=(rm1, rv1, rm2, rv2))
        calls.append(rec)
        return watch(rec, "y", Y.expand_dw_bn_block(alias(rec, "x", x), we, g1, b1, rm1, rv1, wd, g2, b2, rm2, rv2, stride=stride,
                                                   momentum=momentum, eps=eps))

    base = recording_pool_ops(calls)
    table = dict(vars(base))
    table.update(conv_bn_relu6_block=conv_bn_relu6_block, dw_bn_block=dw_bn_block, project_bn_block=project_bn_block,
                 expand_dw_bn_block=expand_dw_bn_block)
    return type(base)(**table)


def check_layer_call(rec, worst):
    """One conv_bn_relu6_block / dw_bn_block / project_bn_block call against the restatement fed with the device's own tensors: z and
    saved are the forward's launches repeated; y, g, the running statistics and the depthwise dx bit-equal; dgamma, dbeta, dW and the dense
    dx within their bounds."""
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
    if kind == "project":
        K.bn_act_bwd(dy, z, saved, _lib.ACT_NONE, True, g, None, None, ws)
        tr, y = N.backward_terms(dyr, zr, sv, "none"), N.forward(zr, sv, "none")
        if rec.get("res") is not None:
            y = D.bf16(y + _np(rec["res"]).reshape(m, cout))
            assert torch.equal(rec["dres"], rec["dy"]), "the residual's gradient is dy"
    else:
        K.bn_clamp_bwd(dy, z, saved, 0.0, 6.0, True, g, None, None, ws)
        tr, y = D.clamp_terms(dyr, zr, sv), D.clamp_forward(zr, sv)
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


def check_expand_call(rec, worst):
    """A fused call against the composed form re-run on its own inputs: bit-equal output, gradients and running tensors; the two calls
    of the composed form are held to the restatement."""
    inner = []
    ops = recording_mobile_ops(inner)
    leaves = [t.detach().clone().requires_grad_() for t in rec["params"]]
    running = [t.clone() for t in rec["running0"]]
    (m1, m2), (e1, e2) = rec["momentum"], rec["eps"]
    xg = rec["x"].clone().requires_grad_()
    y1 = ops.conv_bn_relu6_block(xg, leaves[0], leaves[1], leaves[2], running[0], running[1], momentum=m1, eps=e1)
    y = ops.dw_bn_block(y1, leaves[3], leaves[4], leaves[5], running[2], running[3], stride=rec["stride"], momentum=m2, eps=e2)
    y.backward(rec["dy"])
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(rec["y"])) and torch.equal(bits(xg.grad), bits(rec["dx"])), "expand: y / dx"
    for got, want in zip(rec["params"], leaves):
        assert torch.equal(bits(got.grad), bits(want.grad)), ("expand", tuple(got.shape))
    for got, want in zip(rec["running"], running):
        assert torch.equal(bits(got), bits(want)), "expand: running statistics"
    for c in inner:
        check_layer_call(c, worst)


def check_mobile_calls(calls):
    worst = {}
    for rec in calls:
        if rec["kind"] == "expand":
            check_expand_call(rec, worst)
        elif rec["kind"] in ("relu6", "dw", "project"):
            check_layer_call(rec, worst)
    worst.update(check_calls([c for c in calls if c["kind"] not in ("expand", "relu6", "dw", "project")]))
    return worst


def test_model_layer_by_layer():
    """Every op call of one device forward + backward, re-run on its restatement from the device's own inputs."""
    model = new_model()
    x, targets = model_inputs(model)
    calls = []
    table = recording_mobile_ops(calls)
    assert set(vars(table)) == set(vars(Y.DEVICE_OPS_MOBILE))
    p = Y.forward_train(model, x.to(DEV), ops=table)
    loss, _ = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    kinds = [c["kind"] for c in calls]
    assert kinds.count("expand") == 16 and kinds.count("relu6") == 2 and kinds.count("dw") == 1 and kinds.count("project") == 17
    assert kinds.count("bn") == 3 and kinds.count("head") == 2 and kinds.count("catup") == 1 and len(calls) == 42
    assert sum(c.get("res") is not None for c in calls if c["kind"] == "project") == 10
    assert [c["stride"] for c in calls if c["kind"] == "expand"].count(2) == 4
    worst = check_mobile_calls(calls)
    print(f"train layer by layer, mobile: {len(calls)} op calls, largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))


@functools.lru_cache(maxsize=None)
def device_step(fused=True):
    model = new_model()
    x, targets = model_inputs(model)
    p = Y.forward_train(model, x.to(DEV), ops=Y.DEVICE_OPS_MOBILE if fused else MT.mobile_ops(fused=False))
    loss, items = Y.compute_loss(p, targets.to(DEV), model)
    loss.backward()
    torch.cuda.synchronize()
    return model, [t.detach() for t in p], {n: t.grad for n, t in model.named_parameters()}, items


def test_model_training_step_contract():
    """p as the reference returns it; every parameter gets a finite gradient of its own shape; two steps from the same state give the same
    bits, and so does a step on the composed table; the running statistics moved and every BN layer counted one batch; a following eval
    forward equals that of a fresh model loaded from state_dict() (no stale plan); model.train()(x) and forward_train(model, x) keep
    raising, and the named table checks its input as the default path does."""
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
        Y.forward_train(model, x.double(), ops=Y.DEVICE_OPS_MOBILE)
    with pytest.raises(ValueError, match="multiples of 32"):
        Y.forward_train(model, x[:, :, :, :80], ops=Y.DEVICE_OPS_MOBILE)
    assert all(int(m.num_batches_tracked) == 0 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    p = Y.forward_train(model, x, ops=Y.DEVICE_OPS_MOBILE)
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
    clone = Y.YOLOv3TinyMobile(**M.CTOR)
    clone.load_state_dict({k_: v.cpu() for k_, v in sd.items()})
    with torch.no_grad():
        io_after, _ = model.eval()(x)
        io_clone, _ = clone.to(DEV).eval()(x)
    assert torch.equal(io_after, io_clone) and not torch.equal(io_after, io_before)


# ---- the conv families of a full-size step that the sibling tables do not hold --------------------------------------------------------------
def test_family_cases():
    """tests/_train_mobile_families.MOBILE_FAMILY_CASES through tests/test_train_fire_gpu.py's runner, on integer and on random operands.
    (The full-size step selects no (role, family) beyond the two sibling tables, whose cases tests/test_train_families_gpu.py and
    tests/test_train_fire_gpu.py launch: the table is empty and the loop has nothing to run.  tests/test_train_mobile_cpu.py keeps that
    statement true.)"""
    import test_train_fire_gpu as FG
    for c in MF.CASES:
        for operands in (B.exact_operands, B.random_operands):
            x, w, b, dy = operands(c["case"])
            with FG.tuning(*c["knobs"]):
                d = B.fwd_desc(c["case"])
                got = {"forward": TF.family(K.conv2d_pick(d)), "dgrad": TF.family(K.conv2d_pick(TF.dgrad_desc(d)))}
                want = {role: fam for (role, fam), case in MF.MOBILE_FAMILY_CASES.items() if case is c}
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
    assert len(MF.CASES) == len(MF.MOBILE_FAMILY_CASES)
