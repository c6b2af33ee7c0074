"""GPU tests of the training path on every conv kernel family a full-size training step selects (the table and its
enumeration: tests/_train_families.py, kept complete by tests/test_train_families_cpu.py).

The training forward (ops._forward) and the stride-1 data gradient (yolo_conv2d_bwd_data) run the FORWARD's dispatcher, so on full-size
maps they reach the halo, streaming and 20x20-tile kernels and the large GEMM tiles, which the small maps of tests/_conv_bwd.py never
do.  Those kernels are tested bit for bit in their forward role (tests/test_conv_exact_gpu.py); here they run in the training role: fed
by the device-side packs, the transposed one included, with the zero-bias symbol, with the output counts only a data gradient has (384,
768, 2048), and inside the ops.

Every case is the whole chain of tests/test_conv_bwd_gpu.py (stride 2: tests/test_conv_down_gpu.py) - device pack, forward, prepare,
weight / bias gradient, transposed pack, data gradient - between the poisoned bands of tests/_guard.py with NaN-filled outputs, under
both poisons.  Right before the launches the picks of the forward and of the data-gradient descriptor are asserted under the case's
tuning words, which a ``with`` block restores.
    exact operands   y, g, dW, db and dx bit-equal to the float64 restatement (integer sums below 2^24, one bf16 rounding)
    random operands  dW, db, dx within the bounds of tests/_conv_bwd.py, g bit-equal
    op level         one call of the op the models run the family through (conv_bn_block, res_bn_block, down_bn_block), through the
                     recording table and check_bn_call of tests/test_train_gpu.py, z bit-equal to the restatement on integer x and w

Measured on an MI355X: every exact case bit-equal; random operands, largest error / bound over the 24 layers: dW 0.0105, db 0.0011, dx
0.992 (dx is one RNE away from its fp32 sum, so its ratio reaches ~1 by the bound's own bf16 term; dx == bf16_rne(S) on 99.96-100 % of
the elements); the seven op calls: dW 0.0003, dbeta 0.9895, dgamma 0.9726, dx 0.992.  The slowest test takes 1.1 s (the 1.98 GMAC
stream1x1p<K 384> layer with its float64 restatement), the file 13 s.
"""
import pytest
import torch

import _conv_bwd as B
import _conv_down as D
import _guard as G
import _train_families as TF
import pytorch_yolo_amd as Y
import test_conv_down_gpu as TD
from pytorch_yolo_amd import kernels as K
from test_conv_bwd_gpu import check_untouched, device_chain, same_bits
from test_conv_exact_cpu import tuning
from test_train_gpu import _cl, check_bn_call, recording_ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def assert_picks(c):
    """The kernels the coming launches take, from the descriptors the harness launches (call inside the case's tuning block)."""
    want = {role: fam for (role, fam), case in TF.FAMILY_CASES.items() if case is c}
    d = D.fwd_desc(TF.down_case(c)) if c["stride"] == 2 else B.fwd_desc(c["case"])
    got = {"forward": TF.family(K.conv2d_pick(d))}
    if c["stride"] == 1:
        got["dgrad"] = TF.family(K.conv2d_pick(TF.dgrad_desc(d)))
    assert want and all(got[role] == fam for role, fam in want.items()), (want, got)
    return got


def run_both_poisons(c, x, w, b, dy):
    """The chain of a case under its tuning words, once per poison: margins intact, nothing outside the views, equal bits."""
    runs = []
    with tuning(*c["knobs"]):
        picks = assert_picks(c)
        for poison in G.POISONS:
            if c["stride"] == 2:
                runs.append(TD.run_guarded(TF.down_case(c), x, w, b, dy, poison))
            else:
                a = G.Guard(poison, DEV)
                runs.append(device_chain(a, c["case"], x, w, b, dy))
                a.assert_intact()
                check_untouched(runs[-1])
    assert (TD.same_bits if c["stride"] == 2 else same_bits)(*runs)
    return runs[0], picks


def restated(c, x, w, b, dy, y):
    n, h, wd, cin, cout, k, act, dt, view, oview = c["case"]
    return D.grads(x, w, dy, y) if c["stride"] == 2 else B.grads(x, w, dy, y, k, act)


@pytest.mark.parametrize("c", TF.CASES, ids=TF.layer_id)
def test_exact(c):
    """Integer operands: y (act none) is the integer sum rounded once to its storage type, dW and db have ONE right value, dx is that
    integer rounded once to bf16 - torch.equal, under both poisons."""
    n, h, wd, cin, cout, k, act, dt, view, oview = c["case"]
    down = c["stride"] == 2
    x, w, b, dy = D.exact_operands(TF.down_case(c)) if down else B.exact_operands(c["case"])
    r, picks = run_both_poisons(c, x, w, b, dy)
    y64 = D.forward(x, w, b) if down else B.forward(x, w, b, k, act)
    if down:                                  # (LeakyReLU in the stride-2 harness: 0.1f y is no float64 value; test_op_on_its_family has its z bit for bit)
        assert torch.equal(r["y"] > 0, y64 > 0)
    else:
        y_want = B.bf16(y64) if dt == BF16 else y64
        assert torch.equal(r["y"], y_want), f"y: {int((r['y'] != y_want).sum())} of {y64.numel()} elements differ ({picks})"
    want = restated(c, x, w, b, dy, r["y"])
    for name in ("g", "dw", "db", "dx"):
        assert torch.equal(r[name], want[name]), f"{name}: {int((r[name] != want[name]).sum())} of {want[name].numel()} elements differ ({picks})"
    assert want["dw"].any() and want["db"].any() and want["dx"].any()


@pytest.mark.parametrize("c", TF.CASES, ids=TF.layer_id)
def test_random_within_bounds(c):
    """Random operands against the restatement fed with the device's y: g bit-equal, dW, db and dx within the derived bounds."""
    down = c["stride"] == 2
    x, w, b, dy = D.random_operands(TF.down_case(c)) if down else B.random_operands(c["case"])
    r, picks = run_both_poisons(c, x, w, b, dy)
    want = restated(c, x, w, b, dy, r["y"])
    assert torch.equal(r["g"], want["g"])
    ratios = dict(dw=B.ratio(r["dw"], want["dw"], B.bound_sum(want["dw_terms"], want["dw_abs"])),
                  db=B.ratio(r["db"], want["db"], B.bound_sum(want["db_terms"], want["db_abs"])),
                  dx=B.ratio(r["dx"], want["dx_sum"], B.bound_dx(want["dx_sum"], want["dx_terms"], want["dx_abs"])))
    same = float((r["dx"] == want["dx"]).double().mean())
    print(f"train families {TF.layer_id(c)} {picks}: largest error / bound  dW {ratios['dw']:.4f}  db {ratios['db']:.4f}  dx {ratios['dx']:.4f}"
          f"  (dx == bf16_rne(S) on {100 * same:.2f} % of the elements)")
    assert want["dw"].any() and want["dx"].any()
    for name, v in ratios.items():
        assert v <= 1.0, f"{name}: error / bound = {v}"


# ---- op level: the forward families only large maps reach, through the op the models run them in ----------------------------------------
_fwd = lambda fam: TF.FAMILY_CASES[("forward", fam)]
OP_CASES = [("conv_bn_block", "halo<16x16,64 couts,CK32,1 halo buffers>"),                       # a 3x3 ConvBlock (conv1 of the encoder's stages)
            ("res_bn_block", "halo<16x16,128 couts,CK64,1 halo buffers,16x16x32>"),              # the 3x3 of a residual unit
            ("res_bn_block", "t20v2<400px x 128 couts, 4 waves>"),
            ("conv_bn_block", "stream1x1<64 couts,K 128>"),                                    # the 1x1 of a unit / of the FPN
            ("conv_bn_block", "stream1x1p<128 couts,K 256,80 px>"),
            ("conv_bn_block", "stream1x1p<128 couts,K 384,48 px>"),
            ("down_bn_block", "t20s2<400px x 128 couts, 4 waves, parity planes>")]


@pytest.mark.parametrize("op,fam", OP_CASES, ids=[f"{op}-{fam.split('<')[0]}-{TF.layer_id(_fwd(fam))}" for op, fam in OP_CASES])
def test_op_on_its_family(op, fam):
    """One call of the op with its backward, recorded and re-run on the restatement from the device's own tensors (check_bn_call: y, g and
    the running statistics bit-equal; dgamma, dbeta, dW, dx in bounds).  x and w are the integer operands of the exact test, so the z the
    op's conv wrote has one right value: the float64 sum rounded once to bf16."""
    c = _fwd(fam)
    n, h, wd, cin, cout, k, act, dt, view, oview = c["case"]
    down = c["stride"] == 2
    assert down == (op == "down_bn_block")
    x, w, _, _ = D.exact_operands(TF.down_case(c)) if down else B.exact_operands(c["case"])
    gen = torch.Generator().manual_seed(9100)
    xg = _cl(x.to(BF16).to(DEV)).requires_grad_()
    wp = torch.nn.Parameter(w.to(F32).to(DEV))
    gp = torch.nn.Parameter((1 + 0.25 * torch.randn(cout, generator=gen)).to(DEV))
    bp = torch.nn.Parameter((0.5 * torch.randn(cout, generator=gen)).to(DEV))
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    ho, wo = D.out_hw(h, wd) if down else (h, wd)
    res = _cl(torch.randn((n, cout, ho, wo), generator=gen).to(BF16).to(DEV)).requires_grad_() if op == "res_bn_block" else None
    r = torch.randn((n, cout, ho, wo), generator=gen).to(DEV)
    calls, worst = [], {}
    ops = recording_ops(calls)
    with tuning(*c["knobs"]):
        assert TF.family(K.conv2d_pick(TF.case_desc(c))) == fam
        y = getattr(ops, op)(xg, wp, gp, bp, rm, rv, res) if res is not None else getattr(ops, op)(xg, wp, gp, bp, rm, rv)
        (y.float() * r).sum().backward()
        torch.cuda.synchronize()
        with torch.no_grad():
            z = (Y.down_block if down else Y.conv_block)(xg.detach(), wp.detach(), act="none")
        check_bn_call(calls[0], worst)
    z64 = D.forward(x, w, None, "none") if down else B.forward(x, w, None, k, "none")
    assert torch.equal(z.cpu().to(F64), B.bf16(z64)), f"z: {int((z.cpu().to(F64) != B.bf16(z64)).sum())} of {z64.numel()} elements differ"
    assert len(calls) == 1 and bool((rm != 0).all()) and bool((rv != 1).all()) and xg.grad.dtype == BF16 and bool(xg.grad.any())
    print(f"train families op {op} on {fam}, {TF.layer_id(c)}: largest error / bound  " + "  ".join(f"{k_} {v:.4f}" for k_, v in sorted(worst.items())))
