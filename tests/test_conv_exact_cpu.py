"""Host-side half of the bit-exact conv tests (no GPU): every instance of the bf16 gather kernel has a recipe - a shape and tuning
words - that yolo_conv2d_pick answers with that instance, the test tables name exactly the instances csrc/conv_igemm.hip builds, and
every exact case's reference determines every bit and exercises the rounding (tests/helpers.py::exact_conv_reference rejects it
otherwise).  tests/test_conv_exact_gpu.py launches the same tables."""
import contextlib

import pytest
import torch

import _exact_cases as E
from _exact_cases import BF16_INSTANCES
from helpers import exact_conv
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import ACT_LEAKY01, ACT_NONE, ACT_RELU6, DT_BF16, DT_F16, DT_F32, load

ACT = {"leaky": ACT_LEAKY01, "none": ACT_NONE, "relu6": ACT_RELU6}
NON_DECODE = [n for n, r in BF16_INSTANCES.items() if "head" not in r]
RECIPES = [(n, BF16_INSTANCES[n]) for n in NON_DECODE] + [(k, dict(r, pick=BF16_INSTANCES[inst]["pick"])) for k, (inst, r) in E.BF16_EXTRA.items()]


def exact_desc(shape, view="v8", dtype=torch.bfloat16, in_place_res=False):
    """The descriptor of an exact case: every view at an 8-channel offset inside a buffer 8 (input: 16) channels wider ("v4": the
    output at a 4-channel offset).  in_place_res: the residual view is the output view (tests/test_fp16_t20_gpu.py)."""
    n, h, w, cin, cout, k, stride, act, use_res, use_aux, up, f32 = shape
    ct = K.roundup(cout, 8) + (16 if in_place_res else 8)
    wide = {torch.bfloat16: DT_BF16, torch.float16: DT_F16}[dtype]
    return K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 16, in_c_offset=8, cout=cout, out_c_total=ct, out_c_offset=8 if view == "v8" else 4,
                       ksize=k, stride=stride, act=ACT[act], kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128), upsample2x=int(up),
                       out_dtype=DT_F32 if f32 else wide, res=(ct, 8) if use_res else (0, 0),
                       aux=(K.roundup(cout, 8) + 8, 8) if use_aux else (0, 0))


@contextlib.contextmanager
def knob(i, value):
    """with knob(i, value): yolo_set_tuning(i, value), and the previous value on the way out."""
    old = load().yolo_set_tuning(i, value)
    try:
        yield
    finally:
        load().yolo_set_tuning(i, old)


def tuning(knob0=-1, knob1=0, knob2=0):
    """with tuning(knob0, knob1, knob2): the three conv tuning words set, and restored on the way out."""
    stack = contextlib.ExitStack()
    for i, v in enumerate((knob0, knob1, knob2)):
        stack.enter_context(knob(i, v))
    return stack


def epilogue_of(name):
    """"direct" / "epi": which epilogue the instance runs - the pick string does not say it for the 32x32x16 tiles."""
    return "direct" if name.split("/")[0].endswith("_direct") else "epi"


def assert_recipe_pick(name, r, splits_ok=False):
    shape = r["shape"]
    d = exact_desc(shape, r["view"])
    with tuning(r["knob0"], r["knob1"]):
        pick = K.conv2d_pick(d, shape[8], shape[9])
    inst = name.split("/")[0]
    want = BF16_INSTANCES[E.SPLITK_PLAIN.get(inst, inst)]["pick"]
    assert pick.startswith("igemm" + want + " grid "), f"{name}: picked {pick}"
    # the views and the dtype that decide between the LDS-staged and the direct epilogue (lds_epilogue_views, kCdNoLdsEpilogue)
    lds_ok = not shape[11] and shape[4] % 32 == 0 and r["view"] == "v8" and not (r["knob1"] & E.NO_LDS_EPI)
    assert lds_ok == (epilogue_of(name) == "epi"), name
    return d


def test_bf16_table_is_the_librarys_table():
    """Adding an instance to YOLO_IGEMM_INSTANCES without a recipe here fails; so does a pick string that is not what launch_cfg
    prints for the instance's template arguments."""
    parsed = E.parse_instances("YOLO_IGEMM_INSTANCES")
    assert set(parsed) == set(BF16_INSTANCES)
    assert {n: r["pick"] for n, r in BF16_INSTANCES.items()} == parsed
    assert all(inst in BF16_INSTANCES for inst, _ in E.BF16_EXTRA.values())
    assert len(NON_DECODE) == len(parsed) - 3


def test_fp16_table_is_the_librarys_table():
    from test_fp16_gpu import CONV_F16_CASES, F16_INSTANCES, HEAD_F16_CASES
    parsed = E.parse_instances("YOLO_IGEMM_F16_INSTANCES")
    assert set(parsed) == set(F16_INSTANCES)
    assert {n: s.split("|")[0] for n, s in F16_INSTANCES.items()} == parsed
    assert {c[-1] for c in CONV_F16_CASES} | {c[-1] for c in HEAD_F16_CASES} == set(parsed)


@pytest.mark.parametrize("name,r", RECIPES, ids=[n for n, _ in RECIPES])
def test_bf16_recipe_picks_its_instance(name, r):
    assert load().yolo_set_tuning(0, -1) == -1 and load().yolo_set_tuning(1, 0) == 0       # the defaults are in force outside a recipe
    shape = r["shape"]
    d = assert_recipe_pick(name, r)
    n, h, w, cin, cout, k, stride = shape[:7]
    m = n * d.ho * d.wo
    bm, bk = int(r["pick"][1:].split("x")[0]), int(r["pick"].split(",BK")[1].split(",")[0])
    assert m % bm != 0 and -(-k * k * cin // bk) >= 2, "every case has a partial last pixel tile and at least two K steps"
    assert n <= 8 and max(h, w) <= 64
    if r["knob0"] >= 0:
        bn = int(r["pick"][1:].split("x")[1].split(",")[0])
        assert cin % 64 == 0 and cout > 64 and cout % max(bn, 128) == 0


@pytest.mark.parametrize("name", sorted(E.SPLITK_PLAIN))
def test_split_k_recipes(name):
    r = BF16_INSTANCES[name]
    d = exact_desc(r["shape"])
    splits, ws_bytes, n_cnt = K.conv2d_splitk_plan(d, r["shape"][8], r["shape"][9])
    assert splits >= 2 and ws_bytes > 0 and n_cnt > 0
    if name == "k128x256_loaders_3st_splitk":        # ... the smallest: one pixel tile, and half the K no longer splits
        n, h, w, cin = r["shape"][:4]
        half = exact_desc(r["shape"][:3] + (cin // 2,) + r["shape"][4:])
        assert n * h * w <= 128 and K.conv2d_splitk_plan(half, r["shape"][8], r["shape"][9])[0] == 1


def test_decode_instances_are_picked_by_the_head_shapes():
    for name, r in BF16_INSTANCES.items():
        if "head" not in r:
            continue
        n, h, w, cin, k, nc = r["head"]
        cout = 3 * (nc + 5)
        d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin + 8, in_c_offset=8, cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                        ksize=k, stride=1, act=ACT_NONE, kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128), out_dtype=DT_F32)
        for filt in (False, True):
            assert K.head_decode_pick(d, 3, nc, filt).startswith("igemm" + r["pick"] + " grid "), name


def test_the_tables_cover_the_epilogue_features():
    shapes = [r["shape"] for _, r in RECIPES]
    assert {s[7] for s in shapes} == {"leaky", "none", "relu6"} and {s[6] for s in shapes} == {1, 2}
    assert {(s[8], s[9]) for s in shapes} == {(False, False), (True, False), (False, True), (True, True)}
    assert any(s[10] for s in shapes) and any(s[11] for s in shapes)
    for direct in (False, True):       # both epilogues store a rounded residual sum, a pre-add copy and an upsampled map
        mine = [r["shape"] for n, r in RECIPES if (epilogue_of(n) == "direct") == direct and not r["shape"][11]]
        assert any(s[8] for s in mine) and any(s[9] for s in mine) and any(s[10] for s in mine)


def _family_pick(fam, knob1, knob2, shape):
    with tuning(-1, knob1, knob2):
        return K.conv2d_pick(exact_desc(shape), shape[8], shape[9])


@pytest.mark.parametrize("fam,knob1,knob2,shape", E.FAMILY_CASES, ids=[f"{c[0]}_{c[1]}_{E.case_id(c[3])}" for c in E.FAMILY_CASES])
def test_family_cases_pick_their_family(fam, knob1, knob2, shape):
    pick = _family_pick(fam, knob1, knob2, shape)
    assert pick.startswith(fam), pick
    if fam == "stream1x1":           # cout 128 with K 128 / 256 / 384 runs the pipelined form unless the first form is asked for
        assert pick.startswith("stream1x1p<") == (shape[4] == 128 and not knob1), pick


def all_exact_cases():
    """(shape, seed, dtype) of every 16-bit exact case of the GPU file."""
    from test_fp16_gpu import CONV_F16_CASES
    from test_fp16_t20_gpu import T20_F16_CASES
    out = [(r["shape"], 1, torch.bfloat16) for _, r in RECIPES]
    out += [(c[3], 2, torch.bfloat16) for c in E.FAMILY_CASES]
    out += [(c[:12], 3, torch.float16) for c in CONV_F16_CASES]
    out += [(c[:5] + (3, c[5], c[6], c[7], c[8], False, False), 4, torch.float16) for c in T20_F16_CASES]
    return sorted(set(out), key=str)


@pytest.mark.parametrize("shape,seed,dtype", all_exact_cases(), ids=lambda v: E.case_id(v) if isinstance(v, tuple) else str(v).split(".")[-1])
def test_exact_reference_conditions(shape, seed, dtype):
    """exact_conv_reference's self-checks pass for every case: fp32 conv == fp64 conv, |values| < 2^24, >= 25 % of what is narrowed
    is not representable, >= 10 % are exact ties.  (CPU only; the GPU tests then take the same tensors from the cache.)"""
    x, wt, bias, res, y, aux = exact_conv(shape[:9], seed, dtype, up=shape[10], f32_out=shape[11])
    assert y.dtype == (torch.float32 if shape[11] else dtype) and aux.dtype == dtype
    assert (res is not None) == shape[8] and bool(torch.isfinite(y.float()).all())


def test_f32_exact_cases():
    from test_gpu_parity import F32_CONV_CASES
    for c in F32_CONV_CASES:
        x, wt, bias, res, y, aux = exact_conv(c[:9], 5, torch.float32, up=c[10])
        assert float(x.abs().max()) >= 2 ** 10 and y.dtype == torch.float32       # eleven significant bits are in use
