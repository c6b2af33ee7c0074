"""Host-side half of the bit-exact tests of the fused multi-conv kernels (no GPU): every chained case of tests/_exact_cases.py has a
reference that determines every bit and exercises the rounding (tests/helpers.py::exact_chain_reference rejects it otherwise - the GPU
file can then never meet a rejected case), the reference alone tells a subtly wrong kernel from a right one (one perturbed reference per
failure class, each must differ from the true one in every case it applies to), and every case takes the kernel it names, with the tile
its row says: the library's pick functions answer that without a GPU.  tests/test_fused_exact_gpu.py launches the same tables and
takes the tensors from the same cache."""
import pytest
import torch

import _exact_cases as E
from helpers import exact_chain, exact_chain_reference, exact_conv
from pytorch_yolo_amd import kernels as K
from test_conv_exact_cpu import knob

UNIT_IDS = [u["kernel"] for u in E.UNIT_CASES]
STEM_IDS = ["%s_n%d_c%d_%dx%d_%s" % ((k,) + s) for k, s, _, _ in E.STEM_CASES]
MB_IDS = ["%s_n%d_%dx%d_c%d-%d-%d_s%d" % ((f,) + s) for f, s, _ in E.MBCONV_CASES]
POOL_IDS = ["n%d_%dx%d_c%d-%d_pool%d" % tuple(int(v) for v in c) for c in E.POOL_CASES]


def chained_cases():
    """(id, kind, shape, seed, output tile of the kernel) of every chained case."""
    out = [(u["kernel"], "unit", u["shape"], u["seed"], u["tile"]) for u in E.UNIT_CASES]
    out += [(i, "stem", s, seed, tile) for i, (_, s, tile, seed) in zip(STEM_IDS, E.STEM_CASES)]
    out += [(i, "mbconv", s, E.MBCONV_SEED, tile) for i, (_, s, tile) in zip(MB_IDS, E.MBCONV_CASES)]
    return out


CHAINED = chained_cases()
CHAINED_IDS = [c[0] for c in CHAINED]


@pytest.mark.parametrize("cid,kind,shape,seed,tile", CHAINED, ids=CHAINED_IDS)
def test_chained_reference_conditions(cid, kind, shape, seed, tile):
    """exact_chain_reference's guards pass: every stage's fp32 conv equals its fp64 conv and stays below 2^24 units, >= 15 % negative
    pre-activations (LeakyReLU) / >= 2 % at each clamp (ReLU6), >= 1 % of every intermediate needs rounding, >= 25 % of the output (and
    of the pre-add copy) needs rounding and >= 2 % are ties."""
    x, stages, res, unit, y, aux, stats = exact_chain(kind, shape, seed)
    assert y.dtype == torch.bfloat16 and aux.dtype == torch.bfloat16 and bool(torch.isfinite(y.float()).all())
    assert stats["out_nonrep"] >= 0.25 and stats["out_ties"] >= 0.02
    if kind == "unit":
        assert res is x and y.shape == x.shape


def _perturbed(kind, shape, seed, **kw):
    x, stages, res, unit, y, aux, _ = exact_chain(kind, shape, seed)
    y2, aux2, _ = exact_chain_reference(x, stages, res, unit=unit, **kw)
    return y, aux, y2, aux2


@pytest.mark.parametrize("cid,kind,shape,seed,tile", CHAINED, ids=CHAINED_IDS)
def test_reference_notices_a_dropped_tap_at_a_tile_edge(cid, kind, shape, seed, tile):
    """The 3x3 loses its tap below / right of the centre on the last row / column of every output tile of the kernel the case names
    (16x16, 20x20, 8x20, 8x16, 8x8, 4x8, 8x26, 13x13, 7x7): the output differs."""
    for fault in ("drop_tap_row", "drop_tap_col"):
        y, aux, y2, aux2 = _perturbed(kind, shape, seed, fault=fault, tile=tile)
        h, w = y.shape[2:]
        size, t = (h, tile[0]) if fault == "drop_tap_row" else (w, tile[1])
        if not [p for p in range(size - 1) if p % t == t - 1]:
            continue                                     # (no tile edge inside the map: at stride 1 the dropped tap reads the zero padding)
        bad = (y.float() != y2.float()).nonzero()
        assert len(bad), fault
        edge = bad[:, 2] % tile[0] == tile[0] - 1 if fault == "drop_tap_row" else bad[:, 3] % tile[1] == tile[1] - 1
        assert bool(edge.all())                          # (behind the depthwise 3x3 the 1x1 projection keeps the pixel: there too)


@pytest.mark.parametrize("cid,kind,shape,seed,tile", CHAINED, ids=CHAINED_IDS)
def test_reference_notices_a_wrongly_narrowed_intermediate(cid, kind, shape, seed, tile):
    """Truncation instead of round-to-nearest-even, and no narrowing at all, of EACH intermediate (the inverted residual has two)."""
    x, stages, res, unit, y, aux, _ = exact_chain(kind, shape, seed)
    for st in range(1, len(stages)):
        for fault in ("trunc_mid", "wide_mid"):
            y2, _, _ = exact_chain_reference(x, stages, res, unit=unit, fault=fault, fault_stage=st)
            assert not torch.equal(y, y2), (fault, st)


@pytest.mark.parametrize("u", E.UNIT_CASES, ids=UNIT_IDS)
def test_reference_notices_a_pre_add_copy_taken_after_the_add(u):
    y, aux, y2, aux2 = _perturbed("unit", u["shape"], u["seed"], fault="aux_after_add")
    assert torch.equal(y, y2) and not torch.equal(aux, aux2)
    assert float((aux.float() != aux2.float()).float().mean()) > 0.25


@pytest.mark.parametrize("cid,kind,shape,seed,tile", [c for c in CHAINED if c[2][0] >= 2], ids=[c[0] for c in CHAINED if c[2][0] >= 2])
def test_reference_notices_halo_rows_of_the_neighbouring_image(cid, kind, shape, seed, tile):
    """Every case with n >= 2: the rows above / below an image are zeros, not the neighbouring image's last / first row - around the
    map the last 3x3 reads and, in the stem, around x as well: its first 3x3 reads the NCHW batch itself."""
    for st in (None, 0) if kind == "stem" else (None,):
        y, aux, y2, aux2 = _perturbed(kind, shape, seed, fault="halo_neighbour", fault_stage=st)
        bad = (y.float() != y2.float()).nonzero()
        assert len(bad) and set(bad[:, 2].tolist()) <= {0, y.shape[2] - 1}, st


@pytest.mark.parametrize("cid,kind,shape,seed,tile", [c for c in CHAINED if not (c[1] == "mbconv" and c[2][3] == c[2][4])],
                         ids=[c[0] for c in CHAINED if not (c[1] == "mbconv" and c[2][3] == c[2][4])])
def test_reference_notices_an_intermediate_padded_with_the_activated_bias(cid, kind, shape, seed, tile):
    """What a kernel computes that runs the first conv on zero-padded x at the border: act(b1) instead of 0 around the intermediate.
    (A block without expand conv has no intermediate in front of its 3x3.)"""
    y, aux, y2, aux2 = _perturbed(kind, shape, seed, fault="pad_act_bias")
    bad = (y.float() != y2.float()).nonzero()
    assert len(bad)
    h, w = y.shape[2:]
    assert bool(((bad[:, 2] == 0) | (bad[:, 2] == h - 1) | (bad[:, 3] == 0) | (bad[:, 3] == w - 1)).all())


# ---- the forms the cases name: the library's own answer (yolo_resunit_pick / yolo_stem_pick / yolo_mbconv_pick), no GPU ----------------
def test_unit_cases_reach_their_forms():
    for u in E.UNIT_CASES:
        n, h, w, c, act = u["shape"]
        assert K.resunit_supported(c, h, w), u["kernel"]
        th, tw = u["tile"]
        assert h % 16 and w % 16 and h % th and (w % tw or w == 100), u["kernel"]
        # the shipped rule keeps the 20-pixel-wide kernels away from these small maps: the knob decides
        assert K.resunit_form(c, n, h, w) == (2 if c == 64 else 1), u["kernel"]
        if u["knob3"] == 0:
            assert u["kernel"] == "resunit64_persistent" and n * -(-h // 16) * -(-w // 16) > 256
        assert ("t20" in u["kernel"]) == bool(u["knob3"] & E.RU_T20_ALWAYS)
        assert ("generic16" in u["kernel"]) == bool(u["knob3"] & (E.RU_T20_NEVER | E.RU_GENERIC64))
        with knob(3, u["knob3"]):                        # the kernel the name says, with the tile the row says
            for use_aux in (False, True):
                assert K.resunit_pick(E.unit_desc(u, use_aux), use_aux).startswith(E.unit_pick_wanted(u)), u["kernel"]
    kernels = {(u["kernel"].split("_w101")[0].split("_relu6")[0]) for u in E.UNIT_CASES}
    assert kernels == {"resunit64_persistent", "resunit_generic16_c64", "resunit64_t20", "resunit_generic16_c128", "resunit_t20w_c128",
                       "resunit_generic16_c256", "resunit_t20w_c256"}
    assert any(u["shape"][2] % 20 for u in E.UNIT_CASES if "t20" in u["kernel"])
    assert {u["shape"][4] for u in E.UNIT_CASES if "t20" in u["kernel"]} == {"leaky", "relu6"} == \
        {u["shape"][4] for u in E.UNIT_CASES if "generic16" in u["kernel"]}


def test_stem_cases_cover_both_kernels_and_partial_tiles():
    assert [s for _, s, _, _ in E.STEM_CASES if s[4] == "leaky"] == [(1, 3, 2, 2, "leaky"), (1, 3, 33, 17, "leaky"), (2, 3, 70, 106, "leaky"),
                                                                    (2, 1, 37, 50, "leaky")]
    for kernel, (n, cin, h, w, act), tile, _ in E.STEM_CASES:
        assert kernel == ("stem2" if cin == 3 else "stem_one_role")
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        assert ho % tile[0] and wo % tile[1]
        d = E.stem_desc((n, cin, h, w, act))
        assert K.stem_pick(cin, d).startswith(E.stem_pick_wanted(kernel, (n, cin, h, w, act), tile))
        with knob(6, 1):                                 # YOLO_STEM_ONE_ROLE: stem_kernel for three channels too
            assert K.stem_pick(cin, d).startswith("stem<") and ",16x16 outputs>" in K.stem_pick(cin, d)
    assert any(s[4] == "relu6" for _, s, _, _ in E.STEM_CASES)


def test_mbconv_cases_reach_their_forms():
    rows = {"tile": set(), "strip": set()}
    for form, shape, tile in E.MBCONV_CASES:
        n, h, w, cin, hidden, cout, stride = shape
        assert K.mbconv_supported(cin, hidden, cout, stride)
        assert K.mbconv_form(cin, hidden, cout, stride) == (1 if form in ("tile", "strip") else 2)
        with knob(4, E.MB_STRIP if form == "strip" else 0):          # the kernel the form says, with the tile the row says
            assert E.mbconv_pick(shape).startswith(E.mbconv_pick_wanted(form, shape, tile)), (form, shape, E.mbconv_pick(shape))
        if form in ("tile", "strip"):
            rows[form] |= {name for name, hit in (("no expand", hidden == cin), ("stride 2", stride == 2), ("residual", stride == 1 and cin == cout),
                                                  ("hidden % 32", hidden % 32 != 0), ("cout % 16", cout % 16 != 0)) if hit}
        assert form.startswith("wide") or h * w * cin <= 100000
    assert rows["tile"] == rows["strip"] == {"no expand", "stride 2", "residual", "hidden % 32", "cout % 16"}
    assert {f for f, _, _ in E.MBCONV_CASES} == {"tile", "strip", "wide13", "wide7"}
    with knob(4, E.MB_STRIP):        # the 144- / 192-hidden blocks of the tolerance test take the tile form then too (hence 24-80-24)
        for shape in ((1, 23, 19, 24, 144, 24, 1), (3, 33, 41, 24, 144, 32, 2), (2, 16, 24, 32, 192, 32, 1)):
            assert E.mbconv_pick(shape).startswith("mbconv<"), shape
    # the tile form's persistent loop: min(tiles, slots) workgroups, slots = 1024 / 512 / 256 for <= 40 / <= 80 / more KB of LDS.
    # 24-144-24 at stride 1 takes 8x8 tiles (10x10 inputs, 112 padded; 160 padded hidden channels, 352-byte rows) and
    # 112 * 96 + 112 * 328 + 64 * 352 + 160 * 96 + 32 * 352 + 352 * 4 = 98 048 bytes: 256 slots, one workgroup of 1024 threads per CU
    shape, = [s for f, s, _ in E.MBCONV_CASES if f == "tile" and s[3:] == (24, 144, 24, 1) and s[0] > 1]
    assert shape[0] * -(-shape[1] // 8) * -(-shape[2] // 8) == 320 > 256 and E.mbconv_pick(shape) == "mbconv<S 1,8x8,expand,1024 threads> grid 256"


@pytest.mark.parametrize("case", E.POOL_CASES, ids=POOL_IDS)
def test_pool_cases(case):
    n, h, w, cin, cout, pool = case
    assert K.conv3x3_pool_supported(cin, cout) and (h % 2 or w % 2 or h % 16 and w % 16)
    x, wt, bias, res, y, aux = exact_conv((n, h, w, cin, cout, 3, 1, "leaky", False), E.POOL_SEED, torch.bfloat16)
    assert res is None and y.shape == (n, cout, h, w)


def test_pool_cases_cover_every_pair():
    """Each (cin, cout, pool) is its own instantiation of conv3x3_small_kernel: all four pairs with the pool and all four without, an
    odd x odd map on either side."""
    for pool in (True, False):
        assert {(c[3], c[4]) for c in E.POOL_CASES if c[5] == pool} == {(ci, co) for ci in (16, 32) for co in (32, 64)}
        assert any(c[1] % 2 and c[2] % 2 for c in E.POOL_CASES if c[5] == pool)
