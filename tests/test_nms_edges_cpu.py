"""Host-side half of the NMS edge tests: every row of the case tables of tests/_nms_edges.py really sits where it claims to sit - the
survivor count, the class segment lengths and the kept count come out of the restatements (oracle/nms.py, tests/_nms_styles.py) as
the table says, so a row that misses its boundary fails here and not silently on the GPU -, conf values are pairwise distinct where a
case is tie-free and tied exactly where it has ties, the ``max_per_class`` argument of both restatements at 100 is today's behaviour,
and the library refuses bad arguments before it touches a device.  tests/test_nms_edges_gpu.py runs the same tables through the kernels.

Which branch of csrc/nms.hip a row takes (E.key_sort_branch, E.final_sort_branch) is derived from the kernel's own rules
(n_pad = max(1024, pow2 >= n), f_pad = pow2 >= n_out, LDS up to 8192 keys) and pinned here per row."""
import ctypes

import numpy as np
import pytest

import _cases as C
import _nms_edges as E
import _nms_styles as S
from oracle import nms as onms
from pytorch_yolo_amd import _lib


def _counts(kept):
    return [0 if k is None else len(k) for k in kept]


def _assert_tie_free(pred_image):
    _, conf, _ = E.survivors(pred_image)
    assert len(np.unique(conf)) == len(conf), "conf values repeat in a tie-free case"


KEY_SORT_BRANCH = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 4, 4096: 4, 4097: 8, 8192: 8, 8193: 0, 16385: 0}


@pytest.mark.parametrize("n", E.KEY_SORT_N)
def test_key_sort_rows_sit_on_their_boundary(n):
    pred = E.case_pred("key_sort", n)
    assert pred.shape == (1, n + 37, 9)
    rows, _, _ = E.survivors(pred[0])
    assert len(rows) == n and E.segments(pred[0]) == E.spread(n, 4) and sum(E.spread(n, 4).values()) == n
    _assert_tie_free(pred[0])
    kpt = KEY_SORT_BRANCH[n]
    want = f"LDS, registers KPT {kpt}" if kpt else f"global bitonic ({16384 if n == 8193 else 32768} keys)"
    assert E.key_sort_branch(n) == want
    for style in E.ALL_STYLES:                      # every style has something to do, except AND on a lone row's neighbours
        kept = E.case_want(style, 100, "key_sort", n)[1][0]
        assert kept is not None and 0 < len(kept) <= min(n, 400)
        print(f"[nms edges] key sort n {n}: {E.key_sort_branch(n)}; {style} keeps {len(kept)}: final order {E.final_sort_branch(len(kept))}")


def test_key_sort_table_covers_both_sides_of_every_boundary():
    for edge in (1024, 2048, 4096, 8192):
        assert edge in E.KEY_SORT_N and edge + 1 in E.KEY_SORT_N
        assert E.key_sort_branch(edge) != E.key_sort_branch(edge + 1)
    assert max(E.KEY_SORT_N) + 37 == 16422                                   # the largest input of the GPU file: 16422 x 9 floats


FINAL_SORT_BRANCH = {1: "LDS wave-local network (1 keys)", 511: "LDS wave-local network (512 keys)", 512: "LDS wave-local network (512 keys)",
                     513: "LDS, registers KPT 1", 1024: "LDS, registers KPT 1", 1025: "LDS, registers KPT 2", 2048: "LDS, registers KPT 2",
                     2049: "LDS, registers KPT 4", 4096: "LDS, registers KPT 4", 4097: "LDS, registers KPT 8", 8000: "LDS, registers KPT 8"}


@pytest.mark.parametrize("style", ["SOFT", "OR"])
@pytest.mark.parametrize("n_out", E.FINAL_SORT_N_OUT)
def test_final_sort_rows_keep_exactly_n_out(n_out, style):
    spec = E.case_spec("final_sort", n_out, style)
    pred = E.case_pred("final_sort", n_out, style)
    segs = spec["images"][0]
    assert spec["nc"] <= 80 and E.segments(pred[0]) == segs and E.kept_soft(segs) == n_out
    _assert_tie_free(pred[0])
    assert _counts(E.case_want(style, 100, "final_sort", n_out, style)[1]) == [n_out]
    assert E.final_sort_branch(n_out) == FINAL_SORT_BRANCH[n_out]
    print(f"[nms edges] final sort n_out {n_out} ({style}): survivors {sum(segs.values())}: {E.key_sort_branch(sum(segs.values()))}; "
          f"final order {E.final_sort_branch(n_out)}")


def test_final_sort_beyond_lds_is_the_global_form():
    assert E.final_sort_branch(8192) == "LDS, registers KPT 8" and E.final_sort_branch(8193) == "global bitonic (16384 keys)"
    assert E.final_sort_branch(E.MANY_KEPT) == "global bitonic (16384 keys)"


def test_mixed_batch_counts():
    pred = E.case_pred("mixed")
    assert pred.shape == (5, 8230, 9)
    assert [len(E.survivors(p)[0]) for p in pred] == list(E.MIXED_COUNTS) == [0, 1, 1025, 8193, 300]
    assert [E.key_sort_branch(n) for n in E.MIXED_COUNTS] == ["none (empty image)", "LDS, registers KPT 1", "LDS, registers KPT 2",
                                                              "global bitonic (16384 keys)", "LDS, registers KPT 1"]
    for p in pred:
        _assert_tie_free(p)
    for style in E.ALL_STYLES:
        kept = E.case_want(style, 100, "mixed")[1]
        assert kept[0] is None and len(kept[1]) == 1 and all(k is not None for k in kept[2:])


@pytest.mark.parametrize("nc", E.UNALIGNED_NC)
def test_unaligned_images(nc):
    pred = E.case_pred("unaligned", nc)
    assert pred.shape == (3, 65, 5 + nc)
    image_bytes = 65 * (5 + nc) * 4
    # image 1 starts off a 16-byte boundary, and so does image 2 except at nc = 1 (2 x 1560 bytes is a multiple of 16 again: there the
    # batch has the aligned and the unaligned load loop in one launch)
    assert image_bytes % 16 != 0 and ((2 * image_bytes) % 16 != 0) == (nc != 1), "images 1 and 2 must start off a 16-byte boundary"
    assert [len(E.survivors(p)[0]) for p in pred] == [40, 23, 65]
    for p in pred:
        assert 64 in E.survivors(p)[0], "the single row of the last tile must survive"
        _assert_tie_free(p)


def _final_order_is_total(dets, kept):
    """conf descending, then class ascending, then input row ascending."""
    order = np.lexsort((kept, dets[:, 6], -dets[:, 4].astype(np.float64)))
    return np.array_equal(order, np.arange(len(kept)))


@pytest.mark.parametrize("name", list(E.TIE_CASES))
def test_tie_cases_are_tied_where_they_say(name):
    pred = E.case_pred("tie", name)[0]
    rows, conf, cls = E.survivors(pred)
    values, counts = np.unique(conf, return_counts=True)
    tied = {float(v): int(m) for v, m in zip(values, counts) if m > 1}
    if name == "a_one_class":
        assert tied == {0.75: 5} and set(cls[conf == np.float32(.75)].tolist()) == {0}
    elif name == "b_across_classes":
        assert tied == {0.75: 6, 0.5625: 9}
        assert set(cls[conf == np.float32(.75)].tolist()) == {0, 2} and set(cls[conf == np.float32(.5625)].tolist()) == {0, 1, 3}
    elif name == "c_duplicates":
        assert tied == {0.75: 6}
        dup = pred[rows[(conf == np.float32(.75)) & (pred[rows, 0] == 100)]][:, :5]
        assert len(dup) == 5 and (dup == dup[0]).all()
    else:
        assert int((cls == 0).sum()) == 130 and set(conf[cls == 0].tolist()) == {0.75}
        first100 = set(rows[cls == 0][:100].tolist())
        for style in ("MERGE", "OR", "SOFT"):                # disjoint boxes: the 100 rows that take part are all kept
            dets, kept = (v[0] for v in E.case_want(style, 100, "tie", name))
            assert set(kept[dets[:, 6] == 0].tolist()) == first100, f"{style}: not the first 100 by input row"
        assert E.case_want("AND", 100, "tie", name)[1][0] is None
    for style in ("MERGE", "OR", "AND"):
        dets, kept = (v[0] for v in E.case_want(style, 100, "tie", name))
        if kept is not None:
            assert _final_order_is_total(dets, kept), f"{style}: the restatement's order is not (conf desc, class asc, row asc)"
    # ... and the ties decide something: with the tied rows of a class in the opposite input order, other rows are kept
    if name == "a_one_class":
        assert E.case_want("OR", 100, "tie", name)[1][0].tolist() == [6, 0, 4, 7]
        assert S.nms_image(pred[::-1].copy(), E.CONF_THRES, E.NMS_THRES, "OR")[1].tolist() != [7 - r for r in (6, 0, 4, 7)]


@pytest.mark.parametrize("mpc", list(E.MAX_PER_CLASS_TABLE))
def test_max_per_class_table(mpc):
    table_set = {1, 2, 64, 65, 128, 129, 200}
    segs = E.MAX_PER_CLASS_TABLE[mpc]
    assert 1 <= mpc <= E.MAX_PER_CLASS_CAP
    assert mpc in segs and any(s > mpc for s in segs) and (mpc == 1 or any(s < mpc for s in segs))
    assert set(segs) - {mpc} <= table_set
    pred = E.case_pred("max_per_class", mpc)
    assert E.segments(pred[0]) == dict(enumerate(segs))
    _assert_tie_free(pred[0])
    assert _counts(E.case_want("SOFT", mpc, "max_per_class", mpc)[1]) == [E.kept_soft(dict(enumerate(segs)), mpc)]
    for style in E.ALL_STYLES:
        dets = E.case_want(style, mpc, "max_per_class", mpc)[0][0]
        for c, s in enumerate(segs):
            got = 0 if dets is None else int((dets[:, 6] == c).sum())
            assert got <= min(s, mpc) and (style == "AND" or got >= 1)
        n_out = 0 if dets is None else len(dets)
        print(f"[nms edges] max_per_class {mpc}, segments {segs}: {E.key_sort_branch(sum(segs))}; {style} keeps {n_out}: "
              f"final order {E.final_sort_branch(n_out)}")


def test_max_per_class_values_and_the_and_shortcut():
    assert tuple(E.MAX_PER_CLASS_TABLE) == (1, 2, 63, 64, 65, 100, 127, 128) and E.MAX_PER_CLASS_REFUSED == (0, 129)
    pred = E.case_pred("and_cap1")
    assert E.segments(pred[0]) == {1: 5}
    assert E.case_want("AND", 1, "and_cap1")[1] == [None]       # n == 1 looks at the length before the cap: 5 rows, capped to 1, none emitted
    assert _counts(E.case_want("OR", 1, "and_cap1")[1]) == [1] and _counts(E.case_want("MERGE", 1, "and_cap1")[1]) == [1]


@pytest.mark.parametrize("style", E.ALL_STYLES)
def test_small_cap_case_keeps_57(style):
    pred = E.case_pred("small_cap", style)
    assert _counts(E.case_want(style, 100, "small_cap", style)[1]) == list(E.SMALL_CAP_KEPT) == [57, 3]
    assert E.SMALL_CAP < 57
    for p in pred:
        _assert_tie_free(p)


@pytest.mark.parametrize("style", E.MANY_KEPT_STYLES)
def test_many_kept_case_exceeds_the_lds_keys(style):
    from pytorch_yolo_amd.utils.utils import nms_capacity
    spec = E.MANY_KEPT_SPEC
    assert nms_capacity(spec["rows"], spec["nc"]) == 9000 > E.MANY_KEPT == 8550 > E.LDS_KEYS
    pred = E.case_pred("many")
    assert E.segments(pred[0]) == {c: 95 for c in range(90)}
    _assert_tie_free(pred[0])
    assert _counts(E.case_want(style, 100, "many")[1]) == [8550]
    batch = E.case_pred("many_batch")
    assert [len(E.survivors(p)[0]) for p in batch] == [225, 8550]
    assert _counts(E.case_want(style, 100, "many_batch")[1]) == [225, 8550]
    assert E.key_sort_branch(8550) == E.final_sort_branch(8550) == "global bitonic (16384 keys)"


@pytest.mark.parametrize("nc", E.WIDE_NC)
def test_wide_rows(nc):
    spec = E.case_spec("wide", nc)
    pred = E.case_pred("wide", nc)
    assert pred.shape == (2, 300, 5 + nc) and 64 * (5 + nc) * 4 <= 65536
    cps = (nc + 3) // 4
    for b, segs in enumerate(spec["images"]):
        assert E.segments(pred[b]) == segs                   # the tied rows went to the FIRST of their two classes
        assert {0, cps - 1, cps, 3 * cps, nc - 1} <= set(segs)
        rows, _, cls = E.survivors(pred[b])
        assert bool((pred[b][rows[cls == 0], 5 + nc - 1] == 1.0).all()) and bool((pred[b][rows[cls == cps - 1], 5 + cps] == 1.0).all())
        _assert_tie_free(pred[b])
    assert nc % 4 != 0 or nc == 128                          # 81, 250, 251: the last lane scans fewer classes than the others
    assert 64 * (5 + E.TOO_WIDE_NC) * 4 > 65536 and E.TOO_WIDE_NC == max(E.WIDE_NC) + 1


@pytest.mark.parametrize("name", list(C.NMS_CASES))
def test_max_per_class_100_is_todays_restatement(name):
    pred, conf, iou = C.nms_case_inputs(name)
    same = lambda a, b: all((u is None and v is None) or np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u,
                                                                        v.view(np.uint32) if v.dtype == np.float32 else v) for u, v in zip(a, b))
    d0, k0 = onms.non_max_suppression(pred.copy(), conf, iou, mutate=False)
    d1, k1 = onms.non_max_suppression(pred.copy(), conf, iou, mutate=False, max_per_class=100)
    assert same(d0, d1) and same(k0, k1)
    for style in S.STYLES:
        d0, k0 = S.non_max_suppression(pred, conf, iou, style)
        d1, k1 = S.non_max_suppression(pred, conf, iou, style, 100)
        assert same(d0, d1) and same(k0, k1)
    if name == "nms_dense_nc3":                             # ... and another value is another result
        assert _counts(S.non_max_suppression(pred, conf, iou, "SOFT", 10)[1]) == [30, 30]
        assert _counts(onms.non_max_suppression(pred.copy(), conf, iou, mutate=False, max_per_class=10)[1]) != _counts(k1)


def _styled(nc=2, max_per_class=100, style=_lib.NMS_OR, workspace_bytes=1 << 20, rows=4, cap=4):
    """yolo_nms_styled on HOST buffers: only for calls the argument checks refuse before anything is launched."""
    lib = _lib.load()
    buf = lambda n: (ctypes.c_float * n)()
    pred, dets, idx, cnt, ws = buf(rows * (5 + nc)), buf(cap * 7), buf(cap), buf(1), buf(16)
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    rc = lib.yolo_nms_styled(ptr(pred), 1, rows, nc, 0.5, 0.5, 2.0, max_per_class, 0, ptr(dets), ptr(idx), ptr(cnt), cap, ptr(ws),
                             workspace_bytes, style, None)
    return rc, lib.yolo_last_error().decode()


def test_refusals_come_before_any_device_work():
    """Bad arguments are error returns of the argument checks: no device is needed (this machine may have none)."""
    for mpc in E.MAX_PER_CLASS_REFUSED:
        rc, msg = _styled(max_per_class=mpc)
        assert rc != 0 and f"max_per_class {mpc} not in [1,128]" in msg
    rc, msg = _styled(nc=E.TOO_WIDE_NC)
    assert rc != 0 and "too wide" in msg and "257 floats" in msg
    for style in (-1, 4):
        rc, msg = _styled(style=style)
        assert rc != 0 and "unknown style" in msg
    # the widest accepted row passes the width check: the next check (the workspace size) is the one that refuses
    rc, msg = _styled(nc=max(E.WIDE_NC), workspace_bytes=0)
    assert rc != 0 and "workspace 0 <" in msg
    with pytest.raises(ValueError):
        _lib.nms_style_id("or")


def test_staging_area_is_not_clamped_to_the_lds_keys():
    """yolo_nms_workspace_bytes = counts | keys [pow2 >= rows] u64 | stage [min(rows, nc * 128)] x 8 f32, each part rounded up to
    256 bytes (csrc/nms_common.h carve): for 9000 rows x 90 classes the stage holds all 9000 rows, not 8192."""
    lib = _lib.load()
    al = lambda v: (v + 255) // 256 * 256
    for bs, rows, nc in ((1, 9000, 90), (2, 9000, 90), (1, 25200, 80), (3, 300, 2), (1, 9000, 64)):
        pitch = 1 << (rows - 1).bit_length()
        want = al(bs * 4) + al(bs * pitch * 8) + al(bs * min(rows, nc * 128) * 32)
        assert lib.yolo_nms_workspace_bytes(bs, rows, nc) == want
        assert lib.yolo_nms_compact_workspace_bytes(bs, rows, nc) == want + al(bs * rows * 8) + al(bs * rows * 32)
