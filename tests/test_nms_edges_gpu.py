"""GPU half of the NMS edge tests: csrc/nms.hip on inputs that sit ON its branch points (tests/_nms_edges.py; the CPU half,
tests/test_nms_edges_cpu.py, proves that every table row sits where it claims): the four register key sorts and the global one, the
final order's three forms, ties of conf, max_per_class 1 .. 128 against the two-candidates-per-lane masks, a caller cap below the
kept count, more than 8192 kept rows, rows of up to 256 floats, images off a 16-byte boundary, a batch that mixes all of it, and the
compact form on crafted logits.

Comparison: tests/_nms_styles.assert_same against the restatements (oracle/nms.py for 'MERGE', tests/_nms_styles.py for the others):
kept indices and all seven columns bit-equal; 'SOFT': kept-index sets, conf within its documented rtol 4e-5.  The tie cases ask for
the kept indices IN ORDER in all four styles.  Two GPU runs of one input are compared for bit-equality.  Output buffers are pre-filled
with -3 (no valid row holds a -3: corners and scores are positive here, classes and rows >= 0)."""
import numpy as np
import pytest
import torch

import _guard as G
import _nms_edges as E
import _nms_styles as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
FILL = -3


def _launch(pred_t, style, max_per_class=100, cap=None, alloc=None):
    """K.nms_styled on a device tensor; outputs pre-filled with -3, the workspace with 0xCD.  Returns (dets, idx, count) tensors."""
    from pytorch_yolo_amd import _lib
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd.utils.utils import MIN_WH
    a = alloc or G.Plain(DEV)
    bs, rows, no = pred_t.shape
    nc = no - 5
    cap = cap or max(1, min(rows, nc * max_per_class))           # include/yolo_hip.h: nothing is dropped from this cap on
    ws = a.alloc("workspace", (K.nms_workspace_bytes(bs, rows, nc),), torch.uint8, 0xCD)
    dets = a.alloc("dets", (bs, cap, 7), F32, float(FILL), plane=cap * 7)
    idx = a.alloc("idx", (bs, cap), torch.int32, FILL, plane=cap)
    cnt = a.alloc("count", (bs,), torch.int32, FILL)
    K.nms_styled(pred_t, E.CONF_THRES, E.NMS_THRES, dets, idx, cnt, ws, style=_lib.NMS_STYLES[style], min_wh=MIN_WH,
                 max_per_class=max_per_class)
    torch.cuda.synchronize()
    return dets, idx, cnt


def _images(out):
    """(dets, idx, count) -> per image (dets [n,7], idx [n]) numpy or (None, None); the rows past the count must hold the pre-fill."""
    dets, idx, cnt = (t.cpu().numpy() for t in out)
    cap = dets.shape[1]
    res = []
    for b, n in enumerate(cnt.tolist()):
        assert 0 <= n <= cap, f"image {b}: count {n} outside [0, {cap}]"
        assert not (dets[b, :n] == FILL).any() and not (idx[b, :n] == FILL).any(), f"image {b}: unwritten rows inside [0, count)"
        assert (dets[b, n:] == FILL).all() and (idx[b, n:] == FILL).all(), f"image {b}: rows past the count were written"
        res.append((dets[b, :n].copy(), idx[b, :n].copy()) if n else (None, None))
    return res


def _check(style, got, want, tag, ordered=False):
    """Every image of ``got`` (from _images) against the restatement's (dets list, kept list)."""
    assert len(got) == len(want[0])
    worst = 0.0
    for b, (d, k) in enumerate(got):
        worst = max(worst, S.assert_same(style, d, k, want[0][b], want[1][b], f"{style} {tag} image {b}"))
        if ordered and k is not None:
            assert np.array_equal(k.astype(np.int64), want[1][b]), f"{style} {tag} image {b}: kept indices differ in order"
    if style == "SOFT":
        print(f"[nms edges] SOFT {tag}: largest relative conf difference {worst:.3e} (bound {S.SOFT_RTOL:.1e})")


def _case(kind, *args, style, max_per_class=100, ordered=False):
    pred = E.case_pred(kind, *args)
    pred_t = torch.from_numpy(pred.copy()).to(DEV)
    got = _images(_launch(pred_t, style, max_per_class))
    assert np.array_equal(pred_t.cpu().numpy(), pred), "pred is read-only without mutate_conf"
    _check(style, got, E.case_want(style, max_per_class, kind, *args), f"{kind} {args} cap/class {max_per_class}", ordered)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.KEY_SORT_N)
def test_key_sort_boundaries(n):
    """n survivors in one image of n + 37 rows, nc = 4: 1 .. 1024 / .. 2048 / .. 4096 / .. 8192 keys take block_sort_regs<1 | 2 | 4 | 8>
    in LDS, 8193 and 16385 the bitonic network in the workspace; both sides of every boundary."""
    for style in E.ALL_STYLES:
        _case("key_sort", n, style=style)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["SOFT", "OR"])
@pytest.mark.parametrize("n_out", E.FINAL_SORT_N_OUT)
def test_final_sort_boundaries(n_out, style):
    """Exactly n_out kept rows ('SOFT' removes nothing; 'OR' on disjoint boxes): the wave-local network up to 512, block_sort_regs
    beyond, both sides of 512 / 1024 / 2048 / 4096 and the 8000 rows of 80 full classes."""
    got = _case("final_sort", n_out, style, style=style)
    assert len(got[0][1]) == n_out


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", E.ALL_STYLES)
def test_mixed_batch(style):
    """An empty image, a one-row image, an LDS-sorted one, a globally sorted one and a small one in ONE launch: every image equals the
    restatement and its own single-image run."""
    pred = E.case_pred("mixed")
    got = _case("mixed", style=style)
    assert got[0] == (None, None) and [0 if k is None else 1 for _, k in got] == [0, 1, 1, 1, 1]
    for b in range(pred.shape[0]):
        (d1, k1), = _images(_launch(torch.from_numpy(pred[b:b + 1].copy()).to(DEV), style))
        assert (d1 is None) == (got[b][0] is None)
        if d1 is not None:
            assert np.array_equal(d1.view(np.uint32), got[b][0].view(np.uint32)) and np.array_equal(k1, got[b][1]), \
                f"{style} image {b}: the batched run differs from the single-image run"


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", E.UNALIGNED_NC)
def test_unaligned_images(nc):
    """Rows of 6, 7 and 9 floats, 65 rows: later images start off a 16-byte boundary (the filter's scalar load loop) and the last tile
    is the single row 64, which survives."""
    for style in E.ALL_STYLES:
        got = _case("unaligned", nc, style=style)
        assert all(k is not None for _, k in got)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.TIE_CASES))
def test_conf_ties(name):
    """Equal conf inside a class, across classes, on duplicate rows and over a whole class of 130 rows: the library's total order
    (conf descending, class ascending, input row ascending; pivot order inside a class) decides which rows are heads and where they
    land - kept indices equal IN ORDER in all four styles."""
    for style in E.ALL_STYLES:
        _case("tie", name, style=style, ordered=True)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mpc", list(E.MAX_PER_CLASS_TABLE))
def test_max_per_class(mpc):
    """max_per_class against class segments below, at and above it (E.MAX_PER_CLASS_TABLE): the alive masks of the two candidates per
    lane at 1, 2, 63, 64, 65, 100, 127 and 128."""
    for style in E.ALL_STYLES:
        _case("max_per_class", mpc, style=style, max_per_class=mpc)


def test_max_per_class_and_shortcut_and_refusals():
    """'AND' with max_per_class 1 on a class of 5 rows emits nothing (n == 1 looks at the length before the cap); 0 and 129 are refused."""
    got = _case("and_cap1", style="AND", max_per_class=1)
    assert got == [(None, None)]
    for style in ("MERGE", "OR", "SOFT"):
        got = _case("and_cap1", style=style, max_per_class=1)
        assert len(got[0][1]) == 1
    pred_t = torch.from_numpy(E.case_pred("and_cap1").copy()).to(DEV)
    for bad in E.MAX_PER_CLASS_REFUSED:
        with pytest.raises(RuntimeError, match=rf"max_per_class {bad} not in \[1,128\]"):
            _launch(pred_t, "OR", max_per_class=bad, cap=4)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", E.ALL_STYLES)
def test_small_cap(style):
    """The caller's buffers hold cap = 10 rows per image; image 0 keeps 57, image 1 keeps 3.  out_count is the true count, rows 0..9
    of image 0 are the restatement's first ten, image 1 (whose rows follow image 0's in the buffer) holds its three rows and the
    pre-fill behind them, nothing outside the operands is touched under either poison, and split_detections refuses the buffers."""
    from pytorch_yolo_amd.utils.utils import split_detections
    pred = E.case_pred("small_cap", style)
    want = E.case_want(style, 100, "small_cap", style)
    cap = E.SMALL_CAP
    first = None
    for poison in (None,) + G.POISONS:
        a = G.Plain(DEV) if poison is None else G.Guard(poison, DEV)
        p = a.like("pred", torch.from_numpy(pred.copy()), plane=pred.shape[1] * pred.shape[2])
        dets, idx, cnt = _launch(p, style, cap=cap, alloc=a)
        a.assert_intact()
        assert cnt.cpu().tolist() == list(E.SMALL_CAP_KEPT) == [57, 3]
        d, k = dets.cpu().numpy(), idx.cpu().numpy()
        # (with disjoint boxes 'SOFT' conf is bit-defined: every factor is exp(0) = 1)
        S.assert_same(style, d[0], k[0], want[0][0][:cap], want[1][0][:cap], f"{style} small cap image 0")
        assert np.array_equal(k[0].astype(np.int64), want[1][0][:cap])
        S.assert_same(style, d[1, :3], k[1, :3], want[0][1], want[1][1], f"{style} small cap image 1")
        assert (d[1, 3:] == FILL).all() and (k[1, 3:] == FILL).all(), "rows beyond the count of image 1 lost their pre-fill"
        assert np.array_equal(p.cpu().numpy(), pred)
        if first is None:
            first = (d, k)
        else:
            assert np.array_equal(d.view(np.uint32), first[0].view(np.uint32)) and np.array_equal(k, first[1]), \
                f"poison 0x{poison:02X}: the guarded run differs from the plain run: a read outside an operand"
        with pytest.raises(RuntimeError, match="image 0: 57 detections exceed the output capacity 10"):
            split_detections(dets, idx, cnt)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["many", "many_batch"])
@pytest.mark.parametrize("style", E.MANY_KEPT_STYLES)
def test_more_kept_rows_than_lds_keys(style, kind):
    """90 classes x 95 surviving rows on disjoint boxes: 'SOFT' and 'OR' keep all 8550 > 8192, with rows = 9000 and the library's own
    cap nms_capacity(9000, 90) = 9000.  All 8550 rows equal the restatement, through K.nms_styled and through non_max_suppression(),
    two runs are bit-equal and no row inside [0, count) is left unwritten; also as image 1 of a batch whose image 0 keeps 225."""
    from pytorch_yolo_amd.utils.utils import nms_capacity, non_max_suppression
    pred = E.case_pred(kind)
    want = E.case_want(style, 100, kind)
    bs, rows, no = pred.shape
    cap = nms_capacity(rows, no - 5)
    assert cap == 9000 and len(want[1][-1]) == E.MANY_KEPT
    pred_t = torch.from_numpy(pred.copy()).to(DEV)
    runs = []
    for _ in range(2):
        out = _launch(pred_t, style, cap=cap)
        assert out[2].cpu().tolist() == [len(k) for k in want[1]]
        got = _images(out)
        _check(style, got, want, f"{kind} via nms_styled")
        runs.append(got)
    for (d0, k0), (d1, k1) in zip(*runs):
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(k0, k1), "two runs of one input differ"
    dets, idx = non_max_suppression(pred_t, E.CONF_THRES, E.NMS_THRES, with_indices=True, nms_style=style)
    got = [(d.cpu().numpy(), i.cpu().numpy()) for d, i in zip(dets, idx)]
    _check(style, got, want, f"{kind} via non_max_suppression")
    for (d0, k0), (d1, k1) in zip(runs[0], got):
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(k0, k1)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", E.WIDE_NC)
def test_wide_rows(nc):
    """Rows of 86, 133, 255 and 256 floats; the four lanes of a row split the classes unevenly, with ties of the class maximum between
    the first and the last class and across the first quarter boundary.  At nc = 251 the filter tile is exactly 64 KiB of dynamic LDS
    beside the kernel's two static ints: the launch goes through as it is (no hipFuncSetAttribute; a gfx950 workgroup has 160 KiB),
    so the host bound of 64 KiB stands - pinned here from below and by test_too_wide_is_refused from above."""
    for style in E.ALL_STYLES:
        got = _case("wide", nc, style=style)
        assert all(k is not None for _, k in got)


def test_too_wide_is_refused():
    pred_t = torch.zeros((1, 8, 5 + E.TOO_WIDE_NC), device=DEV)
    with pytest.raises(RuntimeError, match="row of 257 floats too wide"):
        _launch(pred_t, "OR")


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def _compact_vs_plain(spec, styles, want_counts):
    """Crafted logits through an identity head conv: head_decode -> io -> nms_styled against head_decode_filter -> nms_styled_compact:
    counts, kept rows and all seven columns bit-equal."""
    from pytorch_yolo_amd import _lib
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_NONE, DT_F32
    from pytorch_yolo_amd.utils.utils import MIN_WH, nms_capacity
    nc, na, h, w = spec["nc"], spec["na"], spec["h"], spec["w"]
    no = nc + 5
    cout = na * no
    cin = K.roundup(cout, 32)
    anchors, stride = E.COMPACT_ANCHORS[na], 16.0
    lg = torch.from_numpy(E.edge_logits(spec))
    n = lg.shape[0]
    assert torch.equal(lg.to(torch.bfloat16).float(), lg), "the crafted logits must be bf16-exact"
    x = torch.zeros(n, cin, h, w)
    x[:, :cout] = lg.permute(0, 1, 4, 2, 3).reshape(n, cout, h, w)
    wt = torch.zeros(cout, cin, 1, 1)
    wt[torch.arange(cout), torch.arange(cout), 0, 0] = 1.0
    xin = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    wp, bp, kpad, cout_pad = K.pack_conv_weight(wt, torch.zeros(cout), cin)
    wp, bp = wp.to(DEV), bp.to(DEV)
    rows = na * h * w
    d = K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=K.roundup(cout, 8), out_c_offset=0,
                    ksize=1, stride=1, act=ACT_NONE, kpad=kpad, cout_pad=cout_pad, out_dtype=DT_F32)
    cap = nms_capacity(rows, nc)
    io = torch.zeros((n, rows, no), device=DEV)
    p = torch.zeros((n, na, h, w, no), device=DEV)
    K.head_decode(xin, wp, bp, d, anchors, nc, stride, io, 0, p)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), lg), "the identity head does not pass the crafted logits through"
    ws_b = torch.full((K.nms_compact_workspace_bytes(n, rows, nc),), 0xCD, dtype=torch.uint8, device=DEV)
    for style in styles:
        plain = _images(_launch(io, style, cap=cap))
        out = (torch.full((n, cap, 7), float(FILL), device=DEV), torch.full((n, cap), FILL, dtype=torch.int32, device=DEV),
               torch.full((n,), FILL, dtype=torch.int32, device=DEV))
        K.head_decode_filter(xin, wp, bp, d, anchors, nc, stride, rows, 0, E.COMPACT_CONF_THRES, ws_b, min_wh=MIN_WH)
        K.nms_styled_compact(ws_b, n, rows, nc, E.NMS_THRES, *out, style=_lib.NMS_STYLES[style], max_per_class=100)
        torch.cuda.synchronize()
        compact = _images(out)
        if want_counts.get(style) is not None:
            assert [0 if k is None else len(k) for _, k in plain] == want_counts[style], f"{style}: kept counts of the plain form"
        for b, ((d0, k0), (d1, k1)) in enumerate(zip(plain, compact)):
            assert (d0 is None) == (d1 is None), f"{style} image {b}: one form is empty"
            if d0 is not None:
                assert np.array_equal(k0, k1), f"{style} image {b}: kept rows differ between the plain and the compact form"
                assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), f"{style} image {b}: detections differ"
        # the plain form on this io is the restatement's, too (io holds decoded fp32 values; conf may repeat, the order is total)
        io_np = io.cpu().numpy()
        want = E.onms.non_max_suppression(io_np, E.COMPACT_CONF_THRES, E.NMS_THRES, mutate=False) if style == "MERGE" else \
            S.non_max_suppression(io_np, E.COMPACT_CONF_THRES, E.NMS_THRES, style)
        _check(style, plain, want, f"compact case nc {nc} {na}x{h}x{w}, plain form")
    return io


@pytest.mark.parametrize("n", E.COMPACT_KEY_SORT_N)
def test_compact_key_sort_boundaries(n):
    spec = E.compact_key_sort_spec(n)
    io = _compact_vs_plain(spec, E.ALL_STYLES, {})
    assert [len(E.survivors(v)[0]) for v in io.cpu().numpy()] == [n], "the crafted logits miss their survivor count"


def test_compact_conf_ties():
    """Equal conf inside a class and across three classes (equal logits decode to equal scores), rows of a cell overlapping."""
    io = _compact_vs_plain(E.COMPACT_TIE_SPEC, E.ALL_STYLES, {"SOFT": [110, 51]})
    for b, v in enumerate(io.cpu().numpy()):
        rows, conf, cls = E.survivors(v)
        assert E.segments(v) == E.COMPACT_TIE_SPEC["images"][b]
        assert len(np.unique(conf[np.isin(cls, (0, 1, 2))])) == 1, "the tied classes do not share one conf value"


def test_compact_more_kept_rows_than_lds_keys():
    """The case of test_more_kept_rows_than_lds_keys through the compact form: 2 anchors x 68 x 68 cells, 90 classes x 95 rows; the two
    rows of a cell have IoU 0.44, every other pair is disjoint: 'SOFT' and 'OR' keep all 8550."""
    io = _compact_vs_plain(E.COMPACT_MANY_SPEC, E.MANY_KEPT_STYLES, {"SOFT": [E.MANY_KEPT], "OR": [E.MANY_KEPT]})
    assert E.segments(io.cpu().numpy()[0]) == {c: 95 for c in range(90)}
