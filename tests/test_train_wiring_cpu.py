"""One wiring per model: training runs the model's ``_trace`` through models/train.TrainTracer.

  the fixture leg    tests/golden/train_wiring.json was recorded (make_golden_train_wiring.py) on the commit that still had a hand-written
                     ``_train_wiring`` per model: every op call of one ``forward_train`` on ``meta`` tensors, for the four full-size
                     configurations of tests/_train_families.py and the four golden-size ones of tests/_train.py / tests/_train_pool.py.  A
                     call is its op name and every argument in order; a tensor argument is named by what it IS - a parameter or buffer by
                     its state_dict key, an activation by (the call that returned it, output slot), the image "x", anything else (the
                     padded head weights) by shape and dtype - so the record pins the dataflow (which ``sub`` feeds which concat), not only
                     the shapes.  The same recording on this tree has to equal it.
  the tracer leg     the tracer refuses what it cannot run: a max-pool that is not 2/2, a head out of order.
  the recorder leg   Recorder.conv_block / plain_conv / upsample_concat record the nodes that conv / maxpool / upsample2 / concat called
                     directly record (what every ``_trace`` did before the three methods existed).
"""
import functools
import hashlib
import json
import os

import pytest
import torch

import _cases as C
import _train as T
import _train_families as TF
import _train_pool as TP
import pytorch_yolo_amd as Y
from pytorch_yolo_amd import graph
from pytorch_yolo_amd.models import train as MT
from pytorch_yolo_amd.models.yolo_base import ConvPoolBlock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_wiring.json")

# name -> (class, constructor keywords, (bs, H, W))
CONFIGS = {name: (cls, dict(n_class=80, anchors=getattr(C, anchors)), (bs, size, size)) for name, (cls, size, bs, anchors) in TF.CONFIGS.items()}
CONFIGS.update({"spp_golden": ("YOLOv3SPP", T.CTOR, (T.BS, T.H, T.W)), "yolov3_golden": ("YOLOv3", T.CTOR, (T.BS, T.H, T.W)),
                "tiny_golden": (TP.CLASSES["tiny"], TP.CTORS["tiny"], (T.BS, T.H, T.W)),
                "lite_golden": (TP.CLASSES["lite"], TP.CTORS["lite"], (T.BS, T.H, T.W))})


def _shape(t):
    return [list(t.shape), str(t.dtype).replace("torch.", "")]


def record(config):
    """{"calls": [...], "branches": [...]} of one forward_train of ``config`` on meta tensors."""
    cls, ctor, (bs, h, w) = CONFIGS[config]
    model = getattr(Y, cls)(**ctor).to("meta").train()
    x = torch.empty((bs, 3, h, w), dtype=torch.float32, device="meta")
    params = {id(t): name for name, t in model.state_dict(keep_vars=True).items()}
    acts, calls, alive = {id(x): "x"}, [], [x]                   # (alive: no id is handed out twice)

    def enc(v):
        if not isinstance(v, torch.Tensor):
            return v if v is None or isinstance(v, (bool, int, float, str)) else str(v).replace("torch.", "")
        alive.append(v)
        if id(v) in params:
            return {"param": params[id(v)]}
        if id(v) in acts:
            return {"act": acts[id(v)]}
        return {"tensor": _shape(v)}

    def wrap(name, fn):
        def op(*args, **kw):
            rec = {"op": name, "args": [enc(a) for a in args], "kwargs": [[k, enc(v)] for k, v in kw.items()]}
            out = fn(*args, **kw)
            outs = out if isinstance(out, tuple) else (out,)
            for slot, t in enumerate(outs):
                acts[id(t)] = [len(calls), slot]
                alive.append(t)
            rec["out"] = [_shape(t) for t in outs]
            calls.append(rec)
            return out
        return op

    table = TF.recording_meta_ops([])
    for name, fn in vars(table).items():
        setattr(table, name, wrap(name, fn))
    p = MT.forward_train(model, x, ops=table)
    return {"calls": calls, "branches": [_shape(t) for t in p]}


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_has_the_eight_configurations():
    assert sorted(golden()) == sorted(CONFIGS)
    assert [len(golden()[c]["calls"]) for c in TF.CONFIGS] == [79, 77, 15, 22]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_training_runs_the_recorded_op_calls(config):
    got, want = json.loads(json.dumps(record(config))), golden()[config]
    assert len(got["calls"]) == len(want["calls"])
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"
    assert got["branches"] == want["branches"]


# ---- the tracer refuses what it cannot run -------------------------------------------------------------------------------------------
def _tiny():
    return Y.YOLOv3Tiny(**TP.CTORS["tiny"])


@pytest.mark.parametrize("size,stride", [(2, 1), (3, 2), (5, 1)])
def test_tracer_runs_the_2x2_stride_2_pool_only(size, stride):
    g = MT.TrainTracer(TF.recording_meta_ops([]), _tiny().yolo_layers)
    x = torch.empty((1, 8, 8, 8), dtype=torch.bfloat16, device="meta")
    assert g.maxpool(x, 2, 2).shape == (1, 8, 4, 4)
    with pytest.raises(NotImplementedError, match=f"{size}.*{stride}"):
        g.maxpool(x, size, stride)


def test_tracer_takes_the_heads_in_the_order_of_yolo_layers():
    model = _tiny()
    x = torch.empty((1, 21, 2, 2), device="meta")
    g = MT.TrainTracer(TF.recording_meta_ops([]), model.yolo_layers)
    with pytest.raises(RuntimeError, match="order"):
        g.head(x, model.yolo2)
    g = MT.TrainTracer(TF.recording_meta_ops([]), model.yolo_layers)
    g.head(x, model.yolo1), g.head(x, model.yolo2)
    assert len(g.branches) == 2
    with pytest.raises(RuntimeError, match="order"):
        g.head(x, model.yolo1)


def test_tracer_has_the_trainable_vocabulary_only():
    names = {n for n in vars(MT.TrainTracer) if not n.startswith("_")}
    assert names == {"conv_block", "plain_conv", "maxpool", "spp_concat", "upsample_concat", "head"}
    assert all(hasattr(graph.Recorder, n) for n in names)


# ---- the recorder side did not move ----------------------------------------------------------------------------------------------------
class DirectRecorder(graph.Recorder):
    """The three composite methods written out as the direct calls every ``_trace`` made before they existed."""

    def conv_block(self, block, x, **kw):
        y = self.conv(x, block.folded(), stride=block.stride, act="leaky", name=getattr(block, "_trace_name", None), **kw)
        return self.maxpool(y, block.pool.size, block.pool.stride) if isinstance(block, ConvPoolBlock) else y

    def plain_conv(self, conv, x):
        return self.conv(x, (conv.weight.detach().float().cpu(), conv.bias.detach().float().cpu()), stride=1, act="none", f32_out=True,
                         name=getattr(conv, "_trace_name", None))

    def upsample_concat(self, a, b, up_first=True):
        up = self.upsample2(a)
        return self.concat([up, b]) if up_first else self.concat([b, up])


def node_list(rec):
    """Every node as plain data: kind, sources and outputs as (producer node, slot), output shapes, attrs with tensors hashed."""
    where = {id(o): (i, o.slot) for i, n in enumerate(rec.nodes) for o in n.outs}

    def plain(v):
        if isinstance(v, torch.Tensor):
            return (tuple(v.shape), str(v.dtype), hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest())
        return tuple(plain(e) for e in v) if isinstance(v, (tuple, list)) else v
    return [(n.kind, [where[id(s)] for s in n.srcs], [(where[id(o)], o.n, o.h, o.w, o.c, o.f32) for o in n.outs],
             sorted((k, plain(v)) for k, v in n.attrs.items())) for n in rec.nodes] + [[where[id(s)] for s, _ in rec.heads]]


@pytest.mark.parametrize("config", ["spp_golden", "yolov3_golden", "tiny_golden", "lite_golden"])
def test_recorder_composites_record_the_direct_nodes(config):
    cls, ctor, (bs, h, w) = CONFIGS[config]
    torch.manual_seed(0)
    model = getattr(Y, cls)(**ctor).eval()
    for name, m in model.named_modules():
        m._trace_name = name
    lists = []
    for kind in (graph.Recorder, DirectRecorder):
        rec = kind(bs, 3, h, w)
        model._trace(rec, rec.input)
        lists.append(node_list(rec))
    assert len(lists[0]) > 10 and any(n[0] == "cat" for n in lists[0][:-1])
    assert lists[0] == lists[1]
    assert [layer for _, layer in rec.heads] == list(model.yolo_layers)
