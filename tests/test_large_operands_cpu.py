"""Host-side half of the large-operand tests (no GPU; tables and geometry in tests/_large_cases.py): every row of the tables returns its
pinned pick and has the operand sizes the header states, every source that addresses an activation operand with 32-bit offsets has a
row on that operand, and the host bounds sit where include/yolo_hip.h says - an x view of 0xF0000000 bytes is refused with the
"3.75 GiB" message and one plane less is accepted; the same pair on y, the residual or the pre-add copy makes each 32-bit form give
way to a named other kernel, never to an error; the wide MBConv form flips at 2^31 bytes; M stops below 2^31 / 4 pixels.
tests/test_large_operands_gpu.py launches the tables."""
import pytest

import _large_cases as L
from _exact_cases import RU_T20_NEVER, STREAM_ALWAYS, STREAM_FIRST_FORM, T20_ALWAYS
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import ACT_LEAKY01, load
from test_conv_exact_cpu import knob, tuning

ids = lambda rows: [r["id"] for r in rows]


def _defaults_in_force():
    assert load().yolo_set_tuning(0, -1) == -1 and load().yolo_set_tuning(1, 0) == 0 and load().yolo_set_tuning(2, 0) == 0 and load().yolo_set_tuning(3, 0) == 0


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", L.CONV_ROWS, ids=ids(L.CONV_ROWS))
def test_conv_row_picks_its_kernel(r):
    _defaults_in_force()
    d = L.conv_desc_of(r)
    assert L.conv_pick(r, d) == r["pick"]
    if r["api"] == "t20_f16":          # no pick function: the shipped rule takes the layer, and with force the entry launches the tile kernel or fails
        assert r["pick"] is None and K.conv3x3_t20_f16_supported(d, r["shape"][8], r["shape"][9])
    k, cin = r["shape"][5], r["shape"][3]
    bk = 32 if r["pick"] is None or ",BK" not in r["pick"] else int(r["pick"].split(",BK")[1].split(",")[0])
    assert -(-k * k * cin // bk) >= 2, "at least two K steps"


def test_head_row_picks_its_instance():
    r = L.HEAD_ROW
    for filt in (False, True):
        assert K.head_decode_pick(L.head_desc_of(r), 3, r["head"][5], filt) == r["pick"]


@pytest.mark.parametrize("r", L.FUSED_ROWS, ids=ids(L.FUSED_ROWS))
def test_fused_row_picks_its_kernel(r):
    _defaults_in_force()
    pick = L.fused_pick(r)
    assert pick.startswith(r["pick"]) and (r["pick"].endswith("grid ") or pick == r["pick"]), pick
    if r["kind"] == "unit":
        assert K.resunit_supported(r["shape"][3], L.H, L.W)


@pytest.mark.parametrize("r", L.ALL_ROWS, ids=ids(L.ALL_ROWS))
def test_operand_sizes_and_slots(r):
    """A band row's wide operands lie in [2^31 + one plane, 0xF0000000), less than one plane below the limit; a table-D row's y lies
    beyond 2^32; the slots are the first image, the one that contains byte 2^31 (2^32) and the last one, which lies wholly above."""
    sizes = L.operand_bytes(r)
    assert set(sizes) == set(r["wide"]) and sizes
    lo, mid, hi = r["slots"]
    assert lo == 0 and hi == r["n"] - 1
    for nbytes in sizes.values():
        assert nbytes == r["n"] * L.PLANE
        if r["n"] == L.N_BAND:
            assert nbytes == 0xEECC8000 and 2 ** 31 + L.PLANE <= nbytes < L.LIMIT and L.LIMIT - nbytes < L.PLANE
            assert mid * L.PLANE < 2 ** 31 < (mid + 1) * L.PLANE and (mid + 1) * L.PLANE <= hi * L.PLANE
            assert L.LIMIT - (hi + 1) * L.PLANE < 21 * 10 ** 6
        else:
            assert r["n"] == L.N_BEYOND and nbytes == 0x113898000 and nbytes > 2 ** 32 and set(r["wide"]) == {"y"}
            assert mid * L.PLANE < 2 ** 32 < (mid + 1) * L.PLANE and (mid + 1) * L.PLANE <= hi * L.PLANE
    assert L.H % 16 and L.W % 16 and L.H % 20 and L.W % 20 and min(L.H, L.W) >= 80, "partial 16x16 and 20x20 tiles in both directions"


def test_row_ids_are_unique_and_tables_complete():
    assert len({r["id"] for r in L.ALL_ROWS}) == len(L.ALL_ROWS)
    assert len(L.TABLE_A) == 14 and len(L.TABLE_B) == 6 and len(L.TABLE_D) + 1 == 4 and len(L.FUSED_ROWS) == 6 + 2 + 1


# ---- completeness ---------------------------------------------------------------------------------------------------------------------------
def test_every_32_bit_addressed_operand_has_a_row():
    """The keys of COVERAGE / NO_BAND_ROW are what a text search of csrc/ finds: a buffer descriptor over a.x / a.y / a.res / a.aux, or
    a file that names kOobOffset.  A new family that addresses an activation operand this way fails here until it has a row."""
    found = L.addressed_by_text_search()
    rows = {r["id"]: r for r in L.ALL_ROWS}
    files_with_rows = {f for f, _ in L.COVERAGE}
    for f, o in sorted(found, key=str):
        if (f, o) in L.NO_BAND_ROW:
            continue
        assert (f in files_with_rows) if o is None else ((f, o) in L.COVERAGE), f"{f} addresses {o or 'an operand'} with 32-bit offsets and has no row"
    named_only = {f for f, o in found if o is None}
    for (f, o), why in L.NO_BAND_ROW.items():
        assert (f, o) in found and why
    for (f, o), ids_ in L.COVERAGE.items():
        assert ((f, o) in found or f in named_only) and ids_, (f, o)
        for rid in ids_:
            r = rows[rid]
            # the fused units read the residual from x: their "res" descriptor lies over the wide x
            assert (o in r["wide"]) or (o == "res" and r.get("kind") == "unit" and "x" in r["wide"]), (f, o, rid)
            assert (None in L.KERNELS_OF[f]) if r["pick"] is None else any(r["pick"].startswith(p) for p in L.KERNELS_OF[f] if p), (f, rid)
    # and every row stands in the table at least once, the fallback rows of table D and the 64-bit-pointer kernels aside
    listed = {rid for ids_ in L.COVERAGE.values() for rid in ids_}
    assert set(rows) - listed == {"b_halo", "c_mbconv_tile", "d_halo_for_t20v2", "d_igemm_for_stream1x1p", "d_igemm_for_t20s2", "d_stem_one_role"}


def test_the_stem_input_cannot_reach_the_band():
    """2^31 bytes of float32 NCHW input are 2^31 / 12 pixels; the output has a quarter as many of >= 72 channels (64 + an 8-channel
    offset) x 2 bytes: 2^31 / 12 / 4 * 144 = 6.4e9 bytes, past the limit - stem_plan hands that batch to the one-role kernel."""
    assert 2 ** 31 // 12 // 4 * 72 * 2 > L.LIMIT


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
AT, BELOW = (15, 256, 256), (15, 256, 255)           # n, h, w of a 2048-wide operand: exactly 0xF0000000 bytes / one image row less


def test_the_boundary_shapes():
    assert AT[0] * AT[1] * AT[2] * L.CT * 2 == L.LIMIT and BELOW[0] * BELOW[1] * BELOW[2] * L.CT * 2 == L.LIMIT - 15 * 256 * L.CT * 2


def _conv_desc(nhw, cin, cout, k, stride, wide, res=False, aux=False, dtype="bf16", in_hw_scale=1):
    n, h, w = nhw
    r = L._c("boundary", (3, h * in_hw_scale, w * in_hw_scale, cin, cout, k, stride, L.L, res, aux, False, False), None, wide, dtype=dtype)
    return L.conv_desc_of(r, n=n)


def test_an_x_view_of_the_limit_is_refused():
    """yolo_conv2d_pick, yolo_conv2d_f16_pick, yolo_head_decode_pick, yolo_resunit_pick and yolo_conv3x3_t20_f16_supported."""
    _defaults_in_force()
    for pick, args, desc in (
            (K.conv2d_pick, (), lambda nhw: _conv_desc(nhw, 32, 128, 3, 1, "x")),
            (K.conv2d_pick, (), lambda nhw: _conv_desc(nhw, 256, 128, 1, 1, "x")),
            (K.conv2d_f16_pick, (), lambda nhw: _conv_desc(nhw, 256, 128, 1, 1, "x", dtype="f16")),
            (K.head_decode_pick, (3, 80), lambda nhw: L.head_desc_of(L.HEAD_ROW | dict(head=(3,) + nhw[1:] + (256, 1, 80)), n=nhw[0])),
            (K.resunit_pick, (True,), lambda nhw: L.fused_desc_of(dict(kind="unit", shape=(2,) + nhw[1:] + (128, L.L)), n=nhw[0]))):
        assert pick(desc(BELOW), *args)
        with pytest.raises(RuntimeError, match="tensor larger than 3.75 GiB not supported"):
            pick(desc(AT), *args)
    f16 = lambda nhw: _conv_desc(nhw, 32, 128, 3, 1, "x", dtype="f16")
    assert K.conv3x3_t20_f16_supported(f16(BELOW)) and not K.conv3x3_t20_f16_supported(f16(AT))


@pytest.mark.parametrize("form,cin,cout,k,stride,knob1,knob2,gives_way_to", [
    ("t20v2<", 32, 128, 3, 1, 0, T20_ALWAYS, "halo<"), ("t20s2<", 32, 128, 3, 2, 0, T20_ALWAYS, "igemm<"),
    ("stream1x1p<", 256, 128, 1, 1, 0, 0, "igemm<"), ("stream1x1<", 128, 64, 1, 1, 0, 0, "igemm<"),
    ("stream1x1<", 256, 128, 1, 1, STREAM_FIRST_FORM, STREAM_ALWAYS, "igemm<")])
def test_a_y_of_the_limit_gives_way_to_another_kernel(form, cin, cout, k, stride, knob1, knob2, gives_way_to):
    _defaults_in_force()
    with tuning(-1, knob1, knob2):
        assert K.conv2d_pick(_conv_desc(BELOW, cin, cout, k, stride, "y", in_hw_scale=stride)).startswith(form)
        assert K.conv2d_pick(_conv_desc(AT, cin, cout, k, stride, "y", in_hw_scale=stride)).startswith(gives_way_to)


@pytest.mark.parametrize("operand", ["res", "aux"])
def test_a_residual_or_pre_add_copy_of_the_limit_gives_way(operand):
    """t20v2 with a narrow y: the residual / the pre-add copy alone decides."""
    _defaults_in_force()
    with tuning(-1, 0, T20_ALWAYS):
        pick = lambda nhw: K.conv2d_pick(_conv_desc(nhw, 32, 128, 3, 1, operand, res=True, aux=True), True, True)
        assert pick(BELOW).startswith("t20v2<") and pick(AT).startswith("halo<")


@pytest.mark.parametrize("c,form,gives_way_to", [(64, "resunit64_t20<", "resunit64<"), (128, "resunit_t20w<", "resunit<"), (256, "resunit_t20w<", "resunit<")])
@pytest.mark.parametrize("operand", ["y", "aux"])
def test_a_fused_unit_of_the_limit_gives_way(c, form, gives_way_to, operand):
    """x stays narrow (an x of the limit is an error, above); y or the pre-add copy of the limit hands the unit to a 16x16-tile kernel."""
    _defaults_in_force()

    def pick(nhw):
        d = L.fused_desc_of(dict(kind="unit", shape=(2,) + nhw[1:] + (c, L.L)), n=nhw[0], ct=c + 16)
        if operand == "y":
            d.out_c_total, d.out_c_offset = L.CT, L.CT - c - 8
        else:
            d.aux_c_total, d.aux_c_offset = L.CT, L.CT - c - 8
        return K.resunit_pick(d, True)
    assert pick(BELOW).startswith(form) and pick(AT).startswith(gives_way_to)
    with knob(3, RU_T20_NEVER):
        assert pick(AT).startswith(gives_way_to)


def test_a_stem_output_of_the_limit_gives_way():
    stem = lambda nhw: K.stem_pick(3, L.fused_desc_of(dict(kind="stem", shape=(2, 3, 2 * nhw[1], 2 * nhw[2], L.L)), n=nhw[0]))
    assert stem(BELOW).startswith("stem2<leaky,8x16 outputs> grid ") and stem(AT).startswith("stem<leaky,CIN 3,16x16 outputs> grid ")


def test_wide_mbconv_flips_at_2_gib():
    """The wide form (csrc/conv_mbwide.hip) addresses x with a signed 32-bit count: 8 x 256 x 256 x 2048 x 2 bytes = 2^31 is refused,
    one image row less is accepted.  The wording is pinned: a caller sees it."""
    args = dict(cin=96, hidden=192, cout=96, stride=1, in_view=(L.CT, L.CT - 96 - 8), out_view=(96 + 8, 4))
    assert K.mbconv_form(96, 192, 96, 1) == 2 and 8 * 256 * 256 * L.CT * 2 == 2 ** 31
    assert K.mbconv_pick(n=8, h=256, w=255, **args).startswith("mbwide<S 1,")
    with pytest.raises(RuntimeError, match=r"mbconv \(wide\): cin 96 cout 96 does not fit the \d+x\d+ tile form \(\d+ bytes of LDS\), or a tensor of 2 GB"):
        K.mbconv_pick(n=8, h=256, w=256, **args)


def test_the_pixel_count_bound():
    """conv2d_launch_ex: M = n * ho * wo < 0x7fffffff / 4 = 536 870 911.  Only a padded one-row image reaches that many OUTPUT pixels
    below the byte limit of x: 233 * 1103 * 2089 = 536 870 911 is refused, 30 * 1247 * 14351 = 536 870 910 is accepted."""
    def pick(n, w, pad):
        d = K.conv_desc(n=n, h=1, w=w, cin=8, in_c_total=8, in_c_offset=0, cout=32, out_c_total=32, out_c_offset=0, ksize=3, stride=1,
                        act=ACT_LEAKY01, kpad=128, cout_pad=128, pad=pad)
        return d, K.conv2d_pick
    d, f = pick(30, 13105, 624)
    assert d.n * d.ho * d.wo == 0x7fffffff // 4 - 1 and f(d).startswith("igemm<")
    d, f = pick(233, 987, 552)
    assert d.n * d.ho * d.wo == 0x7fffffff // 4
    with pytest.raises(RuntimeError, match="conv: M out of range"):
        f(d)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------
def _conv_cases():
    import torch
    return sorted({(r["shape"], r["seed"], {"bf16": torch.bfloat16, "f16": torch.float16}[r["dtype"]]) for r in L.CONV_ROWS}, key=str)


@pytest.mark.parametrize("shape,seed,dtype", _conv_cases(), ids=lambda v: "x".join(str(int(e) if not isinstance(e, str) else e) for e in v) if isinstance(v, tuple) else str(v).split(".")[-1])
def test_conv_reference_conditions(shape, seed, dtype):
    """exact_conv's guards (fp32 conv == fp64 conv, rounding and tie shares) pass for every shape of the tables with the seed of the row."""
    from helpers import exact_conv
    x, wt, bias, res, y, aux = exact_conv(shape[:9], seed, dtype, up=shape[10], f32_out=shape[11])
    assert y.shape[0] == 3 and (res is not None) == shape[8]


@pytest.mark.parametrize("kind,shape,seed", sorted({(r["kind"], r["shape"], r["seed"]) for r in L.FUSED_ROWS}, key=str), ids=lambda v: str(v))
def test_fused_reference_conditions(kind, shape, seed):
    from helpers import exact_chain
    assert exact_chain(kind, shape, seed)[4].shape[0] == 2


def test_head_reference_conditions():
    from test_large_operands_gpu import head_reference
    p_ref = head_reference()[3]
    assert p_ref.shape == (3, 3, L.H, L.W, 85)
