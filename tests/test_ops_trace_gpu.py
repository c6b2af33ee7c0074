"""The launch lists of the training ops (pytorch_yolo_amd/ops.py), pinned: every case below runs one forward - and a backward where a
``grad_fn`` exists - of a public op with the launching bindings of ``pytorch_yolo_amd.kernels`` wrapped, and the recorded calls equal
tests/golden/ops_trace.json record for record.  A record is the binding's name and, per argument, a tensor's dtype, shape and contiguity,
a YoloConvDesc's fields, or the number itself: no pointers, no element values.  tests/golden/make_golden_ops_trace.py writes the file from
this module's case list; it is re-recorded only when an op's launch list changes on purpose.

Beside the golden, the ops' "each gradient computed only where asked" contract is asserted on the recorded names themselves.

The file uses the public ops and ``pytorch_yolo_amd.kernels`` only, so it runs unchanged on any revision of ops.py."""
import json
import os
import zlib

import pytest
import torch

import pytorch_yolo_amd as Y
from pytorch_yolo_amd import _lib
from pytorch_yolo_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_trace.json")

# every launching binding ops.py reaches (it looks them up as K.<name> at call time)
BINDINGS = ("pack_conv_weight_dev", "pack_conv_weight_down_dev", "conv2d", "conv2d_bwd_prepare", "conv2d_bwd_weight", "conv2d_bwd_data",
            "conv2d_down_bwd_weight", "conv2d_down_bwd_data", "bn_train_stats", "bn_act_fwd", "bn_act_add_fwd", "bn_act_pool_fwd", "bn_act_bwd",
            "spp_train_fwd", "spp_bwd", "upsample2_concat_fwd", "upsample2_concat_bwd", "concat_upsample2_fwd", "concat_upsample2_bwd",
            "maxpool_train_fwd", "maxpool_bwd")
WEIGHT_GRADS = ("conv2d_bwd_weight", "conv2d_down_bwd_weight")
DATA_GRADS = ("conv2d_bwd_data", "conv2d_down_bwd_data")
BN_OPS = ("conv_bn_block", "down_bn_block", "res_bn_block", "pool_bn_block")


# ---- the recorder -------------------------------------------------------------------------------------------------------------------------
def describe(v):
    if isinstance(v, torch.Tensor):
        return dict(dtype=str(v.dtype), shape=list(v.shape), contiguous=v.is_contiguous())
    if isinstance(v, _lib.YoloConvDesc):
        return {"desc": {name: int(getattr(v, name)) for name, _ in v._fields_}}
    if v is None or isinstance(v, (bool, int, float)):
        return v
    raise TypeError(f"ops trace: an argument of type {type(v).__name__} has no record form")


def install(monkeypatch):
    """Wrap every binding of BINDINGS; returns the list the wrappers append their records to."""
    sink = []

    def wrap(name, real):
        def recorded(*args, **kwargs):
            sink.append(dict(name=name, args=[describe(a) for a in args], kwargs={k: describe(v) for k, v in kwargs.items()}))
            return real(*args, **kwargs)
        return recorded

    for name in BINDINGS:
        monkeypatch.setattr(K, name, wrap(name, getattr(K, name)))
    return sink


# ---- the cases: n = 2, 5 x 7 maps (4 x 6 where a pool needs an even map), 8 / 16 / 24 channels -------------------------------------------------
def _map(gen, c, hw=(5, 7)):
    t = torch.randn((2, c) + tuple(hw), generator=gen).to(BF16).to(DEV)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # bf16, dense channels-last: the zero-copy form


def _vec(gen, c, scale=0.5, shift=0.0):
    return (shift + scale * torch.randn(c, generator=gen)).to(DEV)


def _leaves(req, **tensors):
    """The tensors as leaves, those named in ``req`` requiring grad; None stays None."""
    unknown = set(req) - set(tensors)
    assert not unknown, unknown
    return {k: (None if t is None else t.requires_grad_(k in req)) for k, t in tensors.items()}


def _conv(gen, op, *, cin=8, cout=16, k=3, act="leaky", bias=True, out_dtype=None, req=("x", "weight", "bias"), no_grad=False):
    lv = _leaves([r for r in req if bias or r != "bias"], x=_map(gen, cin), weight=(torch.randn((cout, cin, k, k), generator=gen) / 8).to(DEV),
                 bias=_vec(gen, cout) if bias else None)
    kw = dict(act=act) if out_dtype is None else dict(act=act, out_dtype=out_dtype)
    with torch.set_grad_enabled(not no_grad):
        y = getattr(Y, op)(lv["x"], lv["weight"], lv["bias"], **kw)
    return dict(outs=dict(y=y), leaves=lv)


def _bn(gen, op, *, cin=8, cout=16, k=3, hw=(5, 7), req=("x", "weight", "gamma", "beta"), running=True, residual=False, through=None, **kw):
    tensors = dict(x=_map(gen, cin, hw), weight=(torch.randn((cout, cin, k, k), generator=gen) / 8).to(DEV), gamma=_vec(gen, cout, 0.25, 1.0),
                   beta=_vec(gen, cout))
    state = dict(running_mean=_vec(gen, cout), running_var=(0.5 + torch.rand(cout, generator=gen)).to(DEV)) if running else {}
    if residual:
        tensors["residual"] = _map(gen, cout, hw)
    lv = _leaves(req, **tensors)
    args = (lv["x"], lv["weight"], lv["gamma"], lv["beta"], state.get("running_mean"), state.get("running_var"))
    out = getattr(Y, op)(*args, *((lv["residual"],) if residual else ()), **kw)
    outs = dict(y=out[0], y_preadd=out[1]) if isinstance(out, tuple) else dict(y=out)
    return dict(outs=outs, leaves=lv, state=state, through=through)


def _spp(gen):
    lv = _leaves(("x",), x=_map(gen, 8))
    return dict(outs=dict(y=Y.spp_concat(lv["x"])), leaves=lv)


def _upcat(gen, *, up_first, req):
    lv = _leaves(req, a=_map(gen, 8), b=_map(gen, 16, (10, 14)))
    return dict(outs=dict(y=Y.upsample_concat(lv["a"], lv["b"], up_first=up_first)), leaves=lv)


def _pool(gen, *, stride, hw):
    lv = _leaves(("x",), x=_map(gen, 8, hw))
    return dict(outs=dict(y=Y.max_pool(lv["x"], stride=stride)), leaves=lv)


def _cases():
    c = {}
    for op in ("conv_block", "down_block"):
        ks = (1, 3) if op == "conv_block" else (3,)
        for k in ks:                                                            # the forms: kernel, act, bias
            for act in ("leaky", "none"):
                for bias in (True, False):
                    c[f"{op}/k{k}_{act}_{'bias' if bias else 'nobias'}"] = (_conv, dict(op=op, k=k, act=act, bias=bias))
        for name, req in (("x", ("x",)), ("weight", ("weight",)), ("bias", ("bias",)), ("all", ("x", "weight", "bias")), ("none", ())):
            c[f"{op}/req_{name}"] = (_conv, dict(op=op, req=req))
        c[f"{op}/req_all_no_grad"] = (_conv, dict(op=op, no_grad=True))
    c["conv_block/head_f32_cout21"] = (_conv, dict(op="conv_block", cin=16, cout=21, k=1, act="none", out_dtype=F32))       # g: roundup(cout, 8)
    c["conv_block/cin3"] = (_conv, dict(op="conv_block", cin=3))                                                            # zero-padded to 8
    subsets = (("x", ("x",)), ("weight", ("weight",)), ("gamma", ("gamma",)), ("beta", ("beta",)), ("gamma_beta", ("gamma", "beta")),
               ("all", ("x", "weight", "gamma", "beta")))
    for op in ("conv_bn_block", "down_bn_block"):
        for name, req in subsets:
            c[f"{op}/{name}"] = (_bn, dict(op=op, req=req))
        c[f"{op}/all_no_running"] = (_bn, dict(op=op, running=False))
        c[f"{op}/all_act_none"] = (_bn, dict(op=op, act="none"))
        c[f"{op}/all_eval"] = (_bn, dict(op=op, training=False))                # the folded conv_block / down_block launch list
    c["conv_bn_block/all_k1"] = (_bn, dict(op="conv_bn_block", k=1))
    res = dict(op="res_bn_block", cin=16, cout=16, residual=True)
    every = ("x", "weight", "gamma", "beta", "residual")
    c["res_bn_block/all"] = (_bn, dict(res, req=every))
    for name, through in (("y", ("y",)), ("preadd", ("y_preadd",)), ("both", ("y", "y_preadd"))):
        c[f"res_bn_block/want_preadd_through_{name}"] = (_bn, dict(res, req=every, want_preadd=True, through=through))
    c["res_bn_block/residual_only"] = (_bn, dict(res, req=("residual",)))                    # no batch-norm or conv launch in the backward
    c["res_bn_block/residual_only_want_preadd"] = (_bn, dict(res, req=("residual",), want_preadd=True))
    for name, req in subsets[:2] + subsets[4:5]:
        c[f"res_bn_block/{name}"] = (_bn, dict(res, req=req))
    for stride, hw in ((2, (4, 6)), (1, (5, 7))):
        for name, req in subsets[:2] + subsets[4:]:
            c[f"pool_bn_block/s{stride}_{name}"] = (_bn, dict(op="pool_bn_block", req=req, pool_stride=stride, hw=hw))
        c[f"max_pool/s{stride}"] = (_pool, dict(stride=stride, hw=hw))
    c["spp_concat"] = (_spp, {})
    for up_first in (True, False):
        for name, req in (("a", ("a",)), ("b", ("b",)), ("both", ("a", "b"))):
            c[f"upsample_concat/{'up_first' if up_first else 'up_last'}_{name}"] = (_upcat, dict(up_first=up_first, req=req))
    return c


CASES = _cases()


def run_case(name, sink=None):
    """One forward, and a backward where a grad_fn exists, on inputs seeded by the case's name.  Returns every output, gradient and running
    tensor by name, and the number of records the forward left in ``sink``."""
    fn, kw = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    r = fn(gen, **kw)
    n_forward = 0 if sink is None else len(sink)
    tensors = dict(r["outs"], **r.get("state", {}))
    through = [r["outs"][k] for k in (r.get("through") or r["outs"])]
    if any(t.grad_fn is not None for t in through):
        sum((t.float() * torch.randn(t.shape, generator=gen).to(DEV)).sum() for t in through).backward()
        for k, t in r["leaves"].items():
            if t is not None and t.grad is not None:
                tensors["d" + k] = t.grad
    torch.cuda.synchronize()
    return tensors, n_forward


def trace_case(name, sink):
    """The records of the case's forward and of its backward, in JSON's types."""
    del sink[:]
    _, n_forward = run_case(name, sink)
    records = json.loads(json.dumps(sink))
    return records[:n_forward], records[n_forward:]


@pytest.fixture
def sink(monkeypatch):
    return install(monkeypatch)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------
def test_golden_holds_the_case_list(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_list_equals_the_golden(name, sink, golden):
    forward, backward = trace_case(name, sink)
    got, want = forward + backward, golden[name]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: record {i} differs\n  got  {json.dumps(a, sort_keys=True)}\n  want {json.dumps(b, sort_keys=True)}"
    assert len(got) == len(want), f"{name}: {len(got)} records, the golden has {len(want)}: {[r['name'] for r in got]} / {[r['name'] for r in want]}"
    if name.endswith(("/req_none", "/req_all_no_grad")):
        assert not backward, name                                               # no grad_fn: the forward alone


# the four batch-norm ops (pool_bn_block at both pool strides) x the three subsets
CONTRACT = [f"{op}{subset}" for op in ("conv_bn_block/", "down_bn_block/", "res_bn_block/", "pool_bn_block/s2_", "pool_bn_block/s1_")
            for subset in ("x", "weight", "gamma_beta")]


def test_contract_cases_are_cases():
    assert set(CONTRACT) <= set(CASES) and {n.split("/")[0] for n in CONTRACT} == set(BN_OPS)


@pytest.mark.parametrize("name", CONTRACT)
def test_each_gradient_only_where_asked(name, sink):
    """What the docstrings promise, on the names of the backward's launches: gamma / beta alone run neither conv gradient nor a pack; the
    weight alone runs no data gradient and no pack; x alone runs no weight gradient."""
    forward, backward = trace_case(name, sink)
    names = [r["name"] for r in backward]
    assert "bn_train_stats" in [r["name"] for r in forward] and names.count("bn_act_bwd") == 1, names
    if name.endswith("gamma_beta"):
        assert not [n for n in names if n.startswith(("conv2d_bwd_", "conv2d_down_bwd_", "pack_"))], names
    elif name.endswith("weight"):
        assert not [n for n in names if n in DATA_GRADS or n.startswith("pack_")], names
        assert sum(n in WEIGHT_GRADS for n in names) == 1, names
    else:
        assert not [n for n in names if n in WEIGHT_GRADS], names
        assert sum(n in DATA_GRADS for n in names) == 1 and sum(n.startswith("pack_") for n in names) == 1, names


@pytest.mark.parametrize("name", ["res_bn_block/residual_only", "res_bn_block/residual_only_want_preadd"])
def test_residual_only_backward_launches_nothing(name, sink):
    forward, backward = trace_case(name, sink)
    assert forward and not backward, [r["name"] for r in backward]
