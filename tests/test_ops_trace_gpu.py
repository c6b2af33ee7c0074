"""The launch lists of the training ops (pytorch_yolo_amd/ops.py), pinned: every case below runs one forward - and a backward where a
``grad_fn`` exists - of a public op with the launching bindings of ``pytorch_yolo_amd.kernels`` wrapped, and the recorded calls equal
tests/golden/ops_trace.json record for record.  A record is the binding's name and, per argument, a tensor's dtype, shape and contiguity,
a YoloConvDesc's fields, the number itself, or a tuple of numbers (a channel view) as a list: no pointers, no element values.
tests/golden/make_golden_ops_trace.py writes the file from this module's case list; it is re-recorded only when an op's launch list changes
on purpose.

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
            "maxpool_train_fwd", "maxpool_bwd",
            # the SqueezeNet, MobileNetV2 and ShuffleNetV2 families
            "conv2d_stem_bwd_weight", "maxpool3s2_train_fwd", "maxpool3s2_bwd", "fire_bwd_split", "fire_bwd_join", "bn_clamp_fwd", "bn_clamp_bwd",
            "bn_add_rounded_fwd", "dwconv3x3", "dwconv3x3_bwd_data", "dwconv3x3_bwd_weight", "dwconv3x3_bnin_fwd", "dwconv3x3_bnin_bwd_weight",
            "maxpool3s2p1_train_fwd", "maxpool3s2p1_bwd", "channel_shuffle2_fwd", "channel_shuffle2_bwd")
WEIGHT_GRADS = ("conv2d_bwd_weight", "conv2d_down_bwd_weight")
DATA_GRADS = ("conv2d_bwd_data", "conv2d_down_bwd_data")
DW_GRADS = ("dwconv3x3_bwd_data", "dwconv3x3_bwd_weight", "dwconv3x3_bnin_bwd_weight")
BN_OPS = ("conv_bn_block", "down_bn_block", "res_bn_block", "pool_bn_block")


# ---- the recorder -------------------------------------------------------------------------------------------------------------------------
def describe(v):
    if isinstance(v, torch.Tensor):
        return dict(dtype=str(v.dtype), shape=list(v.shape), contiguous=v.is_contiguous())
    if isinstance(v, _lib.YoloConvDesc):
        return {"desc": {name: int(getattr(v, name)) for name, _ in v._fields_}}
    if isinstance(v, float) and v in (float("inf"), float("-inf")):
        return repr(v)                                                          # (strict JSON has no infinity: "inf", a ReLU clamp's hi)
    if v is None or isinstance(v, (bool, int, float)):
        return v
    if isinstance(v, tuple) and all(isinstance(e, (bool, int, float)) for e in v):
        return list(v)                                                          # a channel view (c_total, c_offset)
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


# ---- the cases: n = 2, 5 x 7 maps (4 x 6 where a pool needs an even map, 7 x 9 for the unpadded first layer), 8 / 16 / 24 channels, slot 8
# with half 5 for the shuffle ops --------------------------------------------------------------------------------------------------------
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


def _conv(gen, op, *, cin=8, cout=16, k=3, hw=(5, 7), act="leaky", bias=True, out_dtype=None, req=("x", "weight", "bias"), no_grad=False):
    lv = _leaves([r for r in req if bias or r != "bias"], x=_map(gen, cin, hw), weight=(torch.randn((cout, cin, k, k), generator=gen) / 8).to(DEV),
                 bias=_vec(gen, cout) if bias else None)
    kw = dict(act=act) if out_dtype is None else dict(act=act, out_dtype=out_dtype)
    with torch.set_grad_enabled(not no_grad):
        y = getattr(Y, op)(lv["x"], lv["weight"], lv["bias"], **kw)
    return dict(outs=dict(y=y), leaves=lv)


def _bn(gen, op, *, cin=8, cout=16, k=3, hw=(5, 7), req=("x", "weight", "gamma", "beta"), running=True, residual=False, through=None, dw=False,
        **kw):
    """``dw``: a depthwise layer - x has cout channels and the weight is [cout, 1, 3, 3]."""
    wshape = (cout, 1, 3, 3) if dw else (cout, cin, k, k)
    tensors = dict(x=_map(gen, cout if dw else cin, hw), weight=(torch.randn(wshape, generator=gen) / 8).to(DEV), gamma=_vec(gen, cout, 0.25, 1.0),
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


def _w(gen, *shape):
    return (torch.randn(shape, generator=gen) / 8).to(DEV)


def _bn_set(gen, c, tag):
    """The four batch-norm tensors of one layer, named with ``tag``: (leaves gamma / beta, state running_mean / running_var)."""
    leaves = {f"gamma{tag}": _vec(gen, c, 0.25, 1.0), f"beta{tag}": _vec(gen, c)}
    return leaves, {f"running_mean{tag}": _vec(gen, c), f"running_var{tag}": (0.5 + torch.rand(c, generator=gen)).to(DEV)}


def _fire(gen, *, req, no_grad=False):
    names = ("x", "squeeze_w", "squeeze_b", "e1_w", "e1_b", "e3_w", "e3_b")
    lv = _leaves(req, x=_map(gen, 8), squeeze_w=_w(gen, 8, 8, 1, 1), squeeze_b=_vec(gen, 8), e1_w=_w(gen, 16, 8, 1, 1), e1_b=_vec(gen, 16),
                 e3_w=_w(gen, 24, 8, 3, 3), e3_b=_vec(gen, 24))
    with torch.set_grad_enabled(not no_grad):
        y = Y.fire_block(*(lv[k] for k in names))
    return dict(outs=dict(y=y), leaves=lv)


def _pool_op(gen, op, *, hw, req=("x",)):
    lv = _leaves(req, x=_map(gen, 8, hw))
    return dict(outs=dict(y=getattr(Y, op)(lv["x"])), leaves=lv)


def _expand_dw(gen, *, req, stride=1, cin=8, hidden=24):
    bn1, state1 = _bn_set(gen, hidden, "1")
    bn2, state2 = _bn_set(gen, hidden, "2")
    lv = _leaves(req, x=_map(gen, cin), w_expand=_w(gen, hidden, cin, 1, 1), w_dw=_w(gen, hidden, 1, 3, 3), **bn1, **bn2)
    y = Y.expand_dw_bn_block(lv["x"], lv["w_expand"], lv["gamma1"], lv["beta1"], state1["running_mean1"], state1["running_var1"], lv["w_dw"],
                             lv["gamma2"], lv["beta2"], state2["running_mean2"], state2["running_var2"], stride=stride)
    return dict(outs=dict(y=y), leaves=lv, state=dict(state1, **state2))


def _slot_map(gen, slot, half):
    t = _map(gen, slot)
    t[:, half:] = 0                                                             # the pad channels of a slot hold zero
    return t


def _shuffle(gen, *, req, slot=8, half=5):
    lv = _leaves(req, a=_slot_map(gen, slot, half), b=_slot_map(gen, slot, half))
    return dict(outs=dict(y=Y.channel_shuffle2(lv["a"], lv["b"], half)), leaves=lv)


def _shuffle_unit(gen, *, req, slot=8, half=5, no_grad=False):
    x = torch.cat([_slot_map(gen, slot, half), _slot_map(gen, slot, half)], 1).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    sets = [_bn_set(gen, slot, tag) for tag in "123"]
    lv = _leaves(req, x=x, w1=_w(gen, slot, slot, 1, 1), w_dw=_w(gen, slot, 1, 3, 3), w3=_w(gen, slot, slot, 1, 1),
                 **{k: t for leaves, _ in sets for k, t in leaves.items()})
    state = {k: t for _, st in sets for k, t in st.items()}
    args = [lv["x"], half]
    for tag, wname in zip("123", ("w1", "w_dw", "w3")):
        args += [lv[wname], lv["gamma" + tag], lv["beta" + tag], state["running_mean" + tag], state["running_var" + tag]]
    with torch.set_grad_enabled(not no_grad):
        y = Y.shuffle_unit_block(*args)
    return dict(outs=dict(y=y), leaves=lv, state=state)


def _family_cases(c):
    """The ops of the SqueezeNet, MobileNetV2 and ShuffleNetV2 families: per op one all-gradients case and the subsets that switch a launch
    on or off."""
    stem = dict(op="stem_block", cin=3, hw=(7, 9), act="relu")
    c["stem_block/weight_bias"] = (_conv, dict(stem, req=("weight", "bias")))
    c["stem_block/weight"] = (_conv, dict(stem, req=("weight",)))
    c["stem_block/no_grad"] = (_conv, dict(stem, req=("weight", "bias"), no_grad=True))
    fire_all = ("x", "squeeze_w", "squeeze_b", "e1_w", "e1_b", "e3_w", "e3_b")
    c["fire_block/all"] = (_fire, dict(req=fire_all))
    c["fire_block/x"] = (_fire, dict(req=("x",)))
    c["fire_block/e3_w"] = (_fire, dict(req=("e3_w",)))                           # no expand data gradient, no join
    c["fire_block/no_grad"] = (_fire, dict(req=fire_all, no_grad=True))
    for hw in ((4, 6), (5, 7)):
        c["max_pool_ceil/%dx%d" % hw] = (_pool_op, dict(op="max_pool_ceil", hw=hw))
        c["max_pool_321/%dx%d" % hw] = (_pool_op, dict(op="max_pool_321", hw=hw))
    c["max_pool_321/no_grad"] = (_pool_op, dict(op="max_pool_321", hw=(5, 7), req=()))
    c["conv_bn_relu6_block/k1_all"] = (_bn, dict(op="conv_bn_relu6_block", k=1))
    c["conv_bn_relu6_block/k3_s2_all"] = (_bn, dict(op="conv_bn_relu6_block", stride=2))
    c["conv_bn_relu6_block/gamma_beta"] = (_bn, dict(op="conv_bn_relu6_block", req=("gamma", "beta")))
    c["conv_bn_relu_block/k1_all"] = (_bn, dict(op="conv_bn_relu_block", k=1))
    dw = dict(op="dw_bn_block", cout=16, dw=True)
    c["dw_bn_block/s1_all"] = (_bn, dict(dw))
    c["dw_bn_block/s2_all"] = (_bn, dict(dw, stride=2))
    for name, req in (("x", ("x",)), ("weight", ("weight",)), ("gamma_beta", ("gamma", "beta"))):
        c[f"dw_bn_block/{name}"] = (_bn, dict(dw, req=req))
    c["dw_bn_block/all_act_none"] = (_bn, dict(dw, act="none"))
    proj = dict(op="project_bn_block", cin=24, cout=16, k=1)
    every = ("x", "weight", "gamma", "beta", "residual")
    c["project_bn_block/all"] = (_bn, dict(proj))
    c["project_bn_block/residual_all"] = (_bn, dict(proj, residual=True, req=every))
    c["project_bn_block/residual_only"] = (_bn, dict(proj, residual=True, req=("residual",)))
    pair_all = ("x", "w_expand", "gamma1", "beta1", "w_dw", "gamma2", "beta2")
    c["expand_dw_bn_block/s1_all"] = (_expand_dw, dict(req=pair_all))
    c["expand_dw_bn_block/s2_all"] = (_expand_dw, dict(req=pair_all, stride=2))
    for name, req in (("x", ("x",)), ("w_dw", ("w_dw",)), ("gamma2_beta2", ("gamma2", "beta2"))):
        c[f"expand_dw_bn_block/{name}"] = (_expand_dw, dict(req=req))
    for name, req in (("a", ("a",)), ("b", ("b",)), ("both", ("a", "b"))):
        c[f"channel_shuffle2/{name}"] = (_shuffle, dict(req=req))
    unit_all = ("x", "w1", "gamma1", "beta1", "w_dw", "gamma2", "beta2", "w3", "gamma3", "beta3")
    c["shuffle_unit_block/all"] = (_shuffle_unit, dict(req=unit_all))
    for name in ("x", "w1", "w_dw", "w3"):
        c[f"shuffle_unit_block/{name}"] = (_shuffle_unit, dict(req=(name,)))
    c["shuffle_unit_block/no_grad"] = (_shuffle_unit, dict(req=unit_all, no_grad=True))


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
    _family_cases(c)
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
    if name.endswith(("/req_none", "/req_all_no_grad", "/no_grad")):
        assert not backward, name                                               # no grad_fn: the forward alone


# the four batch-norm ops (pool_bn_block at both pool strides) x the three subsets
CONTRACT = [f"{op}{subset}" for op in ("conv_bn_block/", "down_bn_block/", "res_bn_block/", "pool_bn_block/s2_", "pool_bn_block/s1_")
            for subset in ("x", "weight", "gamma_beta")]


# the batch-norm ops of the newer families: per subset case, how often the backward runs a batch-norm backward ("bn": bn_act_bwd or
# bn_clamp_bwd), a weight pack ("pack") and each conv / depthwise gradient - every gradient launch not named runs zero times.  A weight
# alone runs no data gradient of its own layer (the data gradients below it are those of the layers after it, which lead to it).
FAMILY_CONTRACT = {
    "conv_bn_relu6_block/gamma_beta": dict(bn=1),
    "dw_bn_block/x": dict(bn=1, dwconv3x3_bwd_data=1),
    "dw_bn_block/weight": dict(bn=1, dwconv3x3_bwd_weight=1),
    "dw_bn_block/gamma_beta": dict(bn=1),
    "expand_dw_bn_block/x": dict(bn=2, dwconv3x3_bwd_data=1, conv2d_bwd_data=1, pack=1),
    "expand_dw_bn_block/w_dw": dict(bn=1, dwconv3x3_bnin_bwd_weight=1),
    "expand_dw_bn_block/gamma2_beta2": dict(bn=1),
    "shuffle_unit_block/x": dict(bn=3, dwconv3x3_bwd_data=1, conv2d_bwd_data=2, pack=2),
    "shuffle_unit_block/w1": dict(bn=3, dwconv3x3_bwd_data=1, conv2d_bwd_data=1, pack=1, conv2d_bwd_weight=1),
    "shuffle_unit_block/w_dw": dict(bn=2, dwconv3x3_bwd_weight=1, conv2d_bwd_data=1, pack=1),
    "shuffle_unit_block/w3": dict(bn=1, conv2d_bwd_weight=1),
}


def test_contract_cases_are_cases():
    assert set(CONTRACT) <= set(CASES) and {n.split("/")[0] for n in CONTRACT} == set(BN_OPS)
    assert set(FAMILY_CONTRACT) <= set(CASES)


@pytest.mark.parametrize("name", CONTRACT + list(FAMILY_CONTRACT))
def test_each_gradient_only_where_asked(name, sink):
    """What the docstrings promise, on the names of the backward's launches: gamma / beta alone run neither conv gradient nor a pack; the
    weight alone runs no data gradient and no pack; x alone runs no weight gradient.  The newer families: FAMILY_CONTRACT's counts."""
    forward, backward = trace_case(name, sink)
    names = [r["name"] for r in backward]
    assert "bn_train_stats" in [r["name"] for r in forward], names
    if name in FAMILY_CONTRACT:
        got = {g: names.count(g) for g in WEIGHT_GRADS + DATA_GRADS + DW_GRADS}
        got.update(bn=names.count("bn_act_bwd") + names.count("bn_clamp_bwd"), pack=sum(n.startswith("pack_") for n in names))
        assert {k: v for k, v in got.items() if v} == FAMILY_CONTRACT[name], names
        return
    assert names.count("bn_act_bwd") == 1, names
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
