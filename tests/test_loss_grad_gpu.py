"""GPU tests of the gradient of compute_loss (yolo_loss_bwd of csrc/loss.hip through loss_grad_raw and through autograd): against the
reference's own ``loss.backward()`` (tests/golden/loss_grad.npz) and against the float64 restatement of tests/_loss_grad.py.

The measure and the bar (tests/_loss_grad.py): per layer and word group (xy, wh, conf, class) max |g - g64| / max |g64|
<= 5e-6, a group that is all zero on the other side all zero; every element outside word 4 and the assigned cells +0.0 bit for bit.
Each comparison prints the kernel's error beside the reference's own fp32 error against the same restatement.

Every device operand of the kernels - the p layers, the targets, the class weights, the workspace, grad_loss and the gradient
tensors - sits between the poisoned bands of tests/_guard.py (0xFF and 0x7F), the gradient tensors are pre-filled with NaN, and the
bands are checked after each test.

Measured on an MI355X, the largest over all tests and layers, kernel vs restatement: xy 4.53e-7 (case D layer 1, where the reference's
own fp32 autograd has 4.50e-7), wh 1.21e-7, conf 1.35e-7, class 1.67e-7; kernel vs reference 2.61e-7."""
import functools

import numpy as np
import pytest
import torch

import _cases as C
import _guard as G
import _loss as L
import _loss_grad as LG
from helpers import build_case, load_golden
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.utils import utils as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32


class Operands:
    """The device operands of one gradient call, allocated through ``a`` (a _guard.Guard); ``grad_fill``: what the gradient tensors
    hold before the call."""

    def __init__(self, a, layers, p, targets, cw, nc, bs, ws_fill=0xCD, hyper=L.HYPER, upstream=1.0, grad_fill=float("nan")):
        self.layers, self.nc, self.bs, self.nt = layers, nc, bs, len(targets)
        self.model = L.namespace_model(layers, nc, hyper=hyper, device=DEV)
        self.p = [a.like(f"p{i}", torch.from_numpy(t)) for i, t in enumerate(p)]
        self.targets = a.like("targets", torch.from_numpy(np.ascontiguousarray(targets)))
        self.cw = None if cw is None else a.like("class_weight", torch.from_numpy(cw))
        geom = [(Ly["na"], Ly["ny"], Ly["nx"]) for Ly in layers]
        self.ws = a.alloc("workspace", (K.loss_workspace_bytes(geom, bs, self.nt),), torch.uint8, ws_fill)
        self.grad_loss = a.alloc("grad_loss", (1,), F32, upstream)
        self.grads = [a.alloc(f"grad_p{i}", t.shape, F32, grad_fill) for i, t in enumerate(p)]

    def grad(self):
        """One launch; the gradient tensors (on the device)."""
        out = U.loss_grad_raw(self.p, self.targets, self.model, self.cw, grad_loss=self.grad_loss, workspace=self.ws, out=self.grads)
        assert [t.data_ptr() for t in out] == [t.data_ptr() for t in self.grads]
        torch.cuda.synchronize()
        return out

    def grad_numpy(self):
        return [t.cpu().numpy() for t in self.grad()]


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(inputs, restatement float64 per layer, assignment, golden float32 per layer, the reference's own error [layers, 4]) of a case;
    computed once, never modified."""
    inputs = L.case_inputs(name)
    layers, p, targets, cw, nc, bs = inputs
    want, asg = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw)
    gold = load_golden("loss_grad")
    return inputs, want, asg, LG.golden_grads(gold, name, [t.shape for t in p], asg), LG.golden_ref_err(gold, name, len(layers))


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(L.CASES))
def test_grad_vs_golden_and_restatement(name):
    """A: rows << one workgroup, a non-square grid.  B: nc == 1, 24-byte rows.  C: nc = 80 > 64 lanes, weighted CE, 340-byte rows,
    an 864-row tail.  D: many workgroups.  E: no targets.  A-D hold the duplicate cell of make_targets."""
    inputs, want, asg, gold, ref_err = _expected(name)
    runs = []
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, *inputs)
        got = op.grad_numpy()
        assert all(g.dtype == np.float32 and g.shape == t.shape for g, t in zip(got, inputs[1]))
        LG.assert_grads(got, gold, f"case {name} (poison 0x{poison:02X}): kernel vs reference", ref_err)
        LG.assert_grads(got, want, f"case {name} (poison 0x{poison:02X}): kernel vs restatement", ref_err)
        for i, (g, w, A) in enumerate(zip(got, want, asg)):
            LG.assert_structure(g, A, f"case {name} layer {i}")
            assert np.array_equal(g != 0, w != 0), f"case {name} layer {i}: the zero pattern differs from the restatement's"
        if name == "E":
            assert all(not g[..., :4].any() and not g[..., 5:].any() for g in got)
        a.assert_intact()
        runs.append(got)
    # whatever the buffers held before - NaN between 0xFF bands, NaN between 0x7F bands, zeros - the same bits come out
    a = G.Guard(G.POISONS[0], DEV)
    runs.append(Operands(a, *inputs, ws_fill=0x00, grad_fill=0.0).grad_numpy())
    a.assert_intact()
    for other in runs[1:]:
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(runs[0], other))


@pytest.mark.parametrize("upstream", [0.5, -3.0])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_upstream_gradient(name, upstream):
    """G is read from a device tensor and multiplied into the gain first: a call with G equals, bit for bit, the call with G = 1 and
    the four gains scaled by G (k * h * G is exact for these hyper-parameters and these G); and it is within the bar of the
    restatement at that G."""
    inputs = L.case_inputs(name)
    layers, p, targets, cw, nc, bs = inputs
    a = G.Guard(G.POISONS[0] if upstream > 0 else G.POISONS[1], DEV)
    got = Operands(a, *inputs, upstream=upstream).grad()
    scaled = {k: (v if k == "iou_thresh" else v * upstream) for k, v in L.HYPER.items()}
    for k in scaled:
        assert k == "iou_thresh" or float(np.float32(bs * scaled[k])) == bs * scaled[k]
    folded = Operands(a, *inputs, hyper=scaled, upstream=1.0).grad()
    assert _same_bits(got, folded)
    want, _ = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw, G=upstream)
    LG.assert_grads([t.cpu().numpy() for t in got], want, f"case {name}, upstream {upstream}: kernel vs restatement", _expected(name)[4])
    unit = Operands(a, *inputs).grad()
    assert not _same_bits(got, unit)
    a.assert_intact()


def test_determinism_and_dirty_workspace():
    """Case D twice, the second time with the workspace pre-filled with 0xFF bytes: the same bits - the call re-initialises what it
    reads, and nothing depends on how the workgroups were scheduled."""
    inputs = _expected("D")[0]
    a = G.Guard(0x7F, DEV)
    first = Operands(a, *inputs, ws_fill=0x00)
    g1 = [t.clone() for t in first.grad()]
    second = Operands(a, *inputs, ws_fill=0xFF)
    g2 = second.grad()
    assert all(torch.equal(x, y) for x, y in zip(g1, g2)) and _same_bits(g1, g2)
    for t in second.grads:
        t.fill_(float("nan"))
    g3 = second.grad()                                                  # ... and again on the workspace the call itself left behind
    assert _same_bits(g1, g3)
    a.assert_intact()


def test_cell_shared_by_many_targets():
    """Case A with five more targets copied onto target 0's cell, each with another class: seven records share the cell on every
    layer that keeps target 0.  Two runs give the same bits, and the sum is within the bar of the restatement's."""
    layers, p, targets, cw, nc, bs = L.case_inputs("A")
    extra = np.repeat(targets[:1], 5, 0)
    extra[:, 1] = (targets[0, 1] + 1 + np.arange(5)) % nc
    targets = np.concatenate([targets[:7], extra[:2], targets[7:], extra[2:]], 0)         # not next to each other in slot order
    want, asg = LG.loss_grad(p, targets, layers, L.HYPER, nc, cw)
    sharers = [int(((A["b"] == A["b"][0]) & (A["a"] == A["a"][0]) & (A["gj"] == A["gj"][0]) & (A["gi"] == A["gi"][0])).sum()) for A in asg]
    assert max(sharers) >= 7 and len(set(targets[[0, 1, 7, 8, -3, -2, -1], 1].tolist())) == nc, sharers
    a = G.Guard(0xFF, DEV)
    g1 = [t.clone() for t in Operands(a, layers, p, targets, cw, nc, bs).grad()]
    g2 = Operands(a, layers, p, targets, cw, nc, bs, ws_fill=0xFF).grad()
    assert _same_bits(g1, g2)
    got = [t.cpu().numpy() for t in g1]
    LG.assert_grads(got, want, "case A + 5 sharers: kernel vs restatement", _expected("A")[4])
    for i, (g, A) in enumerate(zip(got, asg)):
        LG.assert_structure(g, A, f"case A + 5 sharers, layer {i}")
    a.assert_intact()


def test_flagged_targets_contribute_nothing():
    """Case A with one target at x = 1.0 (gi == nx on every layer) and one with image == bs (test_loss_gpu.test_bad_targets): the
    gradient is, bit for bit, that of the call without them; with check=True compute_loss raises before any backward can be called,
    with check=False the loss back-propagates the same gradient."""
    layers, p, targets, cw, nc, bs = L.case_inputs("A")
    targets = targets.copy()
    wh = layers[0]["anchor_vec"][1] / np.asarray([layers[0]["nx"], layers[0]["ny"]], dtype=np.float32)
    targets[5, 2], targets[5, 4:6] = 1.0, wh
    targets[6, 0], targets[6, 4:6] = bs, wh
    rest = np.delete(targets, [5, 6], 0)
    assert L.compute_loss(p, targets, layers, L.HYPER, nc, cw)[2] == 2 and L.compute_loss(p, rest, layers, L.HYPER, nc, cw)[2] == 0
    want, _ = LG.loss_grad(p, rest, layers, L.HYPER, nc, cw)
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, layers, p, targets, cw, nc, bs)
        got = [t.clone() for t in op.grad()]
        assert _same_bits(got, Operands(a, layers, p, rest, cw, nc, bs).grad())
        LG.assert_grads([t.cpu().numpy() for t in got], want, f"flagged targets (poison 0x{poison:02X}): kernel vs the restatement without them")
        leaves = [t.detach().requires_grad_() for t in op.p]
        with pytest.raises(RuntimeError, match="2 targets outside the batch / grid / class range"):
            U.compute_loss(leaves, op.targets, op.model, op.cw)
        assert all(t.grad is None for t in leaves)
        loss, _ = U.compute_loss(leaves, op.targets, op.model, op.cw, check=False)
        loss.backward()
        assert _same_bits([t.grad for t in leaves], got)
        a.assert_intact()


def _live_layers(model):
    out = []
    for y in model.yolo_layers:
        nx, ny = (int(v) for v in y.n_grids.cpu().tolist())
        out.append(dict(anchor_vec=y.anchor_vec.cpu().numpy().astype(np.float32), nx=nx, ny=ny, na=int(y.anchor_vec.shape[0])))
    return out


@functools.lru_cache(maxsize=None)
def _live():
    """tiny_small after one forward: (model, p of that forward - no grad_fn -, targets, restatement of the gradient on p.cpu(),
    loss_grad_raw on p)."""
    case = C.MODEL_CASES["tiny_small"]
    model, _, x = build_case(case)
    model.hyper_params = dict(L.HYPER)
    model = model.to(DEV)
    nc, bs = case[1]["n_class"], case[2]
    with torch.no_grad():
        _, p = model(x.to(DEV))
    assert all(t.grad_fn is None and not t.requires_grad for t in p)
    layers = _live_layers(model)
    targets, seed = L.good_targets(301, layers, bs, nc, 40)
    L.assert_conditions(L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc), f"tiny_small targets (seed {seed})")
    want, _ = LG.loss_grad([t.cpu().numpy() for t in p], targets, layers, L.HYPER, nc)
    tt = torch.from_numpy(targets)
    raw = U.loss_grad_raw(p, tt, model)
    return model, p, tt, want, raw


def _leaves(p):
    return [t.detach().requires_grad_() for t in p]


def test_autograd_through_a_model():
    model, p0, tt, want, raw = _live()
    LG.assert_grads([t.cpu().numpy() for t in raw], want, "tiny_small: loss_grad_raw vs restatement on the live p")
    plain_loss, plain_items = U.compute_loss(p0, tt, model)                       # no p requires grad: today's path
    assert plain_loss.grad_fn is None and not plain_loss.requires_grad and plain_items.grad_fn is None
    p = _leaves(p0)
    loss, items = U.compute_loss(p, tt, model)
    assert loss.grad_fn is not None and loss.requires_grad and tuple(loss.shape) == (1,) and loss.dtype == F32
    assert items.requires_grad is False and items.grad_fn is None and tuple(items.shape) == (5,)
    assert torch.equal(items, plain_items) and torch.equal(loss.detach(), plain_loss)          # the same bits either way
    loss.backward()
    assert all(t.grad is not None and t.grad.dtype == F32 and t.grad.shape == t.shape for t in p)
    assert _same_bits([t.grad for t in p], raw)
    with torch.no_grad():                                                          # grad mode off: today's path although p requires grad
        loss_ng, items_ng = U.compute_loss(p, tt, model)
    assert loss_ng.grad_fn is None and not loss_ng.requires_grad and torch.equal(items_ng, items)
    p = _leaves(p0)
    (2 * U.compute_loss(p, tt, model)[0]).backward()
    LG.assert_grads([t.grad.cpu().numpy() for t in p], [2.0 * t.double().cpu().numpy() for t in raw], "tiny_small: (2 * loss).backward() vs 2 x loss_grad_raw")
    p = [p0[0].detach().requires_grad_(), p0[1]]                                   # a p[i] that does not require grad gets none
    U.compute_loss(p, tt, model)[0].backward()
    assert p[1].grad is None and _same_bits([p[0].grad], raw[:1])


def test_autograd_converts_outside_the_function():
    """A float64 p[0] and a non-contiguous p[1]: the conversions are torch operations outside the Function, so each leaf gets a
    gradient of its own dtype and layout."""
    model, p0, tt, want, raw = _live()
    lf64 = p0[0].double().requires_grad_()
    lnc = p0[1].permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4).detach().requires_grad_()
    assert not lnc.is_contiguous() and torch.equal(lnc, p0[1]) and lnc.is_leaf
    loss, items = U.compute_loss([lf64, lnc], tt, model)
    assert torch.equal(items, U.compute_loss(p0, tt, model)[1])
    loss.backward()
    assert lf64.grad.dtype == torch.float64 and lf64.grad.shape == lf64.shape and torch.equal(lf64.grad, raw[0].double())
    assert lnc.grad.dtype == F32 and lnc.grad.shape == lnc.shape and lnc.grad.stride() == lnc.stride() and torch.equal(lnc.grad, raw[1])


def test_double_backward_raises():
    model, p0, tt, _, raw = _live()
    p = _leaves(p0)
    loss, _ = U.compute_loss(p, tt, model)
    # an upstream gradient that does not require grad: the first derivative comes back detached, nothing to differentiate again
    first = torch.autograd.grad(loss, p, create_graph=True)
    assert _same_bits(first, raw) and not any(g.requires_grad for g in first)
    with pytest.raises(RuntimeError, match="does not require grad"):
        sum(g.sum() for g in first).backward()
    # an upstream gradient that does: the first derivative is attached to a node that refuses to be differentiated
    scale = torch.tensor([2.0], device=DEV, requires_grad=True)
    loss, _ = U.compute_loss(p, tt, model)
    first = torch.autograd.grad(loss * scale, p, create_graph=True)
    assert all(g.requires_grad for g in first)
    LG.assert_grads([g.detach().cpu().numpy() for g in first], [2.0 * t.double().cpu().numpy() for t in raw], "tiny_small: create_graph, upstream 2")
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        sum(g.sum() for g in first).backward()
