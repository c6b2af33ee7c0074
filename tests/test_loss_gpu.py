"""GPU tests of the validation loss (csrc/loss.hip through compute_loss / build_targets / loss_raw): against the reference's own answers
(tests/golden/loss.npz) and against the numpy restatement of tests/_loss.py.

Bars (tests/_loss.py): b, a, gj, gi, tcls equal; txy bit-equal; twh rtol 1e-6 / atol 1e-7; each of the five loss items
within 5e-6 relative, and exactly 0.0 where the other side is exactly 0.0.  Two GPU runs of the same call are compared with torch.equal.

Every device operand of the kernels - the p layers, the targets, the class weights, the workspace, out and the status array - sits
between the poisoned bands of tests/_guard.py (0xFF and 0x7F), and the bands are checked after each test."""
import numpy as np
import pytest
import torch

import _cases as C
import _guard as G
import _loss as L
from helpers import build_case, load_golden
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd.utils import utils as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32


class Operands:
    """The device operands of one loss call, allocated through ``a`` (a _guard.Guard or _guard.Plain)."""

    def __init__(self, a, layers, p, targets, cw, nc, bs, ws_fill=0xCD, hyper=L.HYPER):
        self.layers, self.nc, self.bs, self.nt = layers, nc, bs, len(targets)
        self.model = L.namespace_model(layers, nc, hyper=hyper, device=DEV)
        self.p = [a.like(f"p{i}", torch.from_numpy(t)) for i, t in enumerate(p)]
        self.targets = a.like("targets", torch.from_numpy(np.ascontiguousarray(targets)))
        self.cw = None if cw is None else a.like("class_weight", torch.from_numpy(cw))
        geom = [(Ly["na"], Ly["ny"], Ly["nx"]) for Ly in layers]
        self.ws = a.alloc("workspace", (K.loss_workspace_bytes(geom, bs, self.nt),), torch.uint8, ws_fill)
        self.out = a.alloc("out", (5,), F32, float("nan"))
        self.status = a.alloc("status", (1 + len(layers),), torch.int32, -3)

    def loss(self):
        out, status, _ = U.loss_raw(self.p, self.targets, self.model, self.cw, workspace=self.ws, out=self.out, status=self.status)
        assert out.data_ptr() == self.out.data_ptr() and status.data_ptr() == self.status.data_ptr()
        torch.cuda.synchronize()
        return out.cpu().numpy(), status.cpu().tolist()

    def assignment(self):
        txy, twh, tcls, indices = U.build_targets(self.model, self.targets, bs=self.bs, workspace=self.ws)
        return txy, twh, tcls, indices

    def records(self):
        return U._records(self.ws, len(self.layers), self.nt).clone()


def _as_numpy(txy, twh, tcls, indices):
    return [dict(b=ix[0].cpu().numpy(), a=ix[1].cpu().numpy(), gj=ix[2].cpu().numpy(), gi=ix[3].cpu().numpy(), tcls=c.cpu().numpy(),
                 txy=xy.cpu().numpy(), twh=wh.cpu().numpy()) for xy, wh, c, ix in zip(txy, twh, tcls, indices)]


def _golden_assignment(g, name, nl):
    return [{k: g[f"{name}_L{i}_{k}"] for k in ("b", "a", "gj", "gi", "tcls", "txy", "twh")} for i in range(nl)]


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_assignment_vs_golden(name):
    g = load_golden("loss")
    inputs = L.case_inputs(name)
    nl = len(inputs[0])
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, *inputs)
        txy, twh, tcls, indices = op.assignment()
        for i in range(nl):                                            # dtypes and shapes as the reference's
            n = len(g[f"{name}_L{i}_b"])
            assert len(indices[i]) == 4 and all(t.dtype == torch.int64 and tuple(t.shape) == (n,) and t.is_cuda for t in indices[i])
            assert tcls[i].dtype == torch.int64 and tuple(tcls[i].shape) == (n,)
            assert txy[i].dtype == twh[i].dtype == F32 and tuple(txy[i].shape) == tuple(twh[i].shape) == (n, 2)
        worst = L.assert_assignment(_as_numpy(txy, twh, tcls, indices), _golden_assignment(g, name, nl), f"case {name}: kernel vs reference")
        print(f"[loss] case {name} (poison 0x{poison:02X}): kernel vs reference, largest relative twh difference {worst:.3e}")
        a.assert_intact()


@pytest.mark.parametrize("name", list(L.CASES))
def test_loss_vs_golden(name):
    g = load_golden("loss")
    inputs = L.case_inputs(name)
    want_r, asg, _ = L.compute_loss(inputs[1], inputs[2], inputs[0], L.HYPER, inputs[4], inputs[3])
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, *inputs)
        items, status = op.loss()
        L.assert_items(items, g[f"{name}_items"], f"case {name} (poison 0x{poison:02X}): kernel vs reference")
        L.assert_items(items, want_r, f"case {name} (poison 0x{poison:02X}): kernel vs restatement")
        assert status == [0] + [len(A["b"]) for A in asg]
        if name == "E":
            assert items[0] == items[1] == items[3] == 0.0 and items[2] == items[4] > 0
        a.assert_intact()
    # the public entry point: the reference's return pair, on the device, without a grad_fn, and the same bits
    loss, items2 = U.compute_loss(op.p, op.targets, op.model, op.cw)
    assert tuple(loss.shape) == (1,) and tuple(items2.shape) == (5,) and loss.dtype == items2.dtype == F32 and loss.is_cuda and items2.is_cuda
    assert loss.grad_fn is None and items2.grad_fn is None and not loss.requires_grad
    assert np.array_equal(items2.cpu().numpy(), items) and float(loss) == float(items[4])
    loss3, items3 = U.compute_loss(op.p, op.targets.cpu(), op.model, None if op.cw is None else op.cw.cpu(), check=False)    # host targets
    assert torch.equal(items3, items2) and torch.equal(loss3, loss)


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("geometry", list(L.SWEEP_SEEDS))
def test_restatement_sweep(geometry, k):
    *inputs, seed = L.sweep_inputs(geometry, k)
    layers, p, targets, cw, nc, bs = inputs
    L.assert_conditions(L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc), f"sweep {geometry}{k} (seed {seed})")
    want, asg, n_bad = L.compute_loss(p, targets, layers, L.HYPER, nc, cw)
    assert n_bad == 0
    a = G.Guard(G.POISONS[k % 2], DEV)
    op = Operands(a, *inputs)
    items, status = op.loss()
    L.assert_items(items, want, f"sweep {geometry}{k} (seed {seed}): kernel vs restatement")
    assert status == [0] + [len(A["b"]) for A in asg]
    L.assert_assignment(_as_numpy(*op.assignment()), asg, f"sweep {geometry}{k} (seed {seed})")
    a.assert_intact()


def test_determinism_and_dirty_workspace():
    """Case D twice, the second time with the workspace pre-filled with 0xFF bytes: the same bits in the items and in the records -
    every call re-initialises what it reads, and no sum depends on how the workgroups were scheduled."""
    inputs = L.case_inputs("D")
    a = G.Guard(0x7F, DEV)
    first = Operands(a, *inputs, ws_fill=0x00)
    items1, status1 = first.loss()
    rec1 = first.records()
    second = Operands(a, *inputs, ws_fill=0xFF)
    items2, status2 = second.loss()
    assert np.array_equal(items1.view(np.int32), items2.view(np.int32)) and status1 == status2
    assert torch.equal(rec1, second.records())
    items3, _ = second.loss()                                           # ... and again on the workspace the call itself left behind
    assert np.array_equal(items1.view(np.int32), items3.view(np.int32)) and torch.equal(rec1, second.records())
    a.assert_intact()


def test_bad_targets():
    """Case A with one target at x = 1.0 (gi == nx on every layer) and one with image == bs, both with the wh of an anchor of layer 0
    (IoU 1 there): the reference raises an IndexError; here check=True raises, the status word says 2, check=False returns the loss
    of the remaining targets, and nothing is written outside the operands."""
    layers, p, targets, cw, nc, bs = L.case_inputs("A")
    targets = targets.copy()
    wh = layers[0]["anchor_vec"][1] / np.asarray([layers[0]["nx"], layers[0]["ny"]], dtype=np.float32)
    targets[5, 2], targets[5, 4:6] = 1.0, wh
    targets[6, 0], targets[6, 4:6] = bs, wh
    rest = np.delete(targets, [5, 6], 0)
    want, asg, n_bad = L.compute_loss(p, rest, layers, L.HYPER, nc, cw)
    assert n_bad == 0 and L.compute_loss(p, targets, layers, L.HYPER, nc, cw)[2] == 2
    for poison in G.POISONS:
        a = G.Guard(poison, DEV)
        op = Operands(a, layers, p, targets, cw, nc, bs)
        items, status = op.loss()
        assert status == [2] + [len(A["b"]) for A in asg]
        L.assert_items(items, want, f"bad targets (poison 0x{poison:02X}): kernel vs the restatement without them")
        with pytest.raises(RuntimeError, match="2 targets outside the batch / grid / class range"):
            U.compute_loss(op.p, op.targets, op.model, op.cw)
        loss, items2 = U.compute_loss(op.p, op.targets, op.model, op.cw, check=False)
        assert np.array_equal(items2.cpu().numpy(), items)
        with pytest.raises(RuntimeError, match="2 targets outside the batch / grid / class range"):
            op.assignment()
        a.assert_intact()


def _live_layers(model):
    out = []
    for y in model.yolo_layers:
        nx, ny = (int(v) for v in y.n_grids.cpu().tolist())
        out.append(dict(anchor_vec=y.anchor_vec.cpu().numpy().astype(np.float32), nx=nx, ny=ny, na=int(y.anchor_vec.shape[0])))
    return out


def test_through_a_model():
    """tiny_small in its default precision: compute_loss(p, targets, model) on the p of a live forward equals the restatement applied
    to p.cpu() and the layers' live anchor_vec / n_grids - the attribute plumbing, not the network's arithmetic."""
    case = C.MODEL_CASES["tiny_small"]
    model, _, x = build_case(case)
    model.hyper_params = dict(L.HYPER)
    model = model.to(DEV)
    nc, bs = case[1]["n_class"], case[2]
    fake_p = [torch.zeros((bs, 3, 2, 3, 5 + nc), device=DEV), torch.zeros((bs, 3, 4, 6, 5 + nc), device=DEV)]
    with pytest.raises(RuntimeError, match="run the model"):             # no forward yet: the layers have no grid
        U.compute_loss(fake_p, torch.zeros((0, 6)), model)
    with torch.no_grad():
        io, p = model(x.to(DEV))
    assert all(t.grad_fn is None for t in p)
    layers = _live_layers(model)
    assert [(Ly["ny"], Ly["nx"]) for Ly in layers] == [tuple(t.shape[2:4]) for t in p]
    targets, seed = L.good_targets(301, layers, bs, nc, 40)
    L.assert_conditions(L.input_conditions(layers, targets, L.HYPER["iou_thresh"], bs, nc), f"tiny_small targets (seed {seed})")
    want, asg, n_bad = L.compute_loss([t.cpu().numpy() for t in p], targets, layers, L.HYPER, nc)
    assert n_bad == 0
    loss, items = U.compute_loss(p, torch.from_numpy(targets), model)
    L.assert_items(items.cpu().numpy(), want, "tiny_small: kernel vs restatement on the live p")
    assert float(loss) == float(items[4]) and loss.grad_fn is None
    L.assert_assignment(_as_numpy(*U.build_targets(model, torch.from_numpy(targets), bs=bs)), asg, "tiny_small")
    # p of another input size than the one the layers last saw
    with pytest.raises(RuntimeError, match="do not match"):
        U.compute_loss([torch.zeros((bs, 3, 4, 4, 5 + nc), device=DEV), torch.zeros((bs, 3, 8, 8, 5 + nc), device=DEV)], torch.from_numpy(targets), model)
    model.train()
    with pytest.raises(NotImplementedError):                             # forward value only: training-mode forward keeps raising
        model(x.to(DEV))


def test_predict_dataset_with_loss():
    from pytorch_yolo_amd.utils.synthetic import synth_images
    case = C.MODEL_CASES["tiny_small"]
    model, _, x = build_case(case)
    model.hyper_params = dict(L.HYPER)
    model = model.to(DEV)
    nc = case[1]["n_class"]
    with torch.no_grad():
        io, _ = model(x.to(DEV))
    conf = float((io[..., 4] * io[..., 5:].max(-1).values).flatten().median())     # a threshold this random-weight model clears
    layers = _live_layers(model)
    batches = []
    for k, bs in enumerate((2, 1)):
        imgs = synth_images(bs, 64, 96, 40 + k)
        targets, _ = L.good_targets(400 + k, layers, bs, nc, 24)
        batches.append((imgs, torch.from_numpy(targets), [f"img{k}_{i}" for i in range(bs)], [(128, 192)] * bs))
    plain = U.predict_dataset(model, batches, conf, 0.5)
    data, items = U.predict_dataset(model, batches, conf, 0.5, loss=True)
    assert isinstance(plain, dict) and sum(len(v) for v in plain.values()) >= 5, "the comparison is vacuous"
    assert data == plain
    want = torch.zeros(5, dtype=torch.float64)
    for imgs, targets, _, _ in batches:
        with torch.no_grad():
            _, p = model(imgs.to(DEV))
        want += U.compute_loss(p, targets, model)[1].double().cpu() * imgs.shape[0]
    want = (want / 3).tolist()
    assert isinstance(items, list) and len(items) == 5 and all(isinstance(v, float) for v in items)
    assert items == pytest.approx(want, rel=1e-12) and all(v > 0 for v in items)
