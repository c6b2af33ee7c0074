"""The guard-band allocator of tests/_guard.py on the CPU device: that it reports what it must (a one-byte write on either side, with
the side and the offset), keeps what it promises (alignment, margin rule, untouched payload), that the two poison bytes decode to
what its header claims, and - on a torch emulation of a 3x3 window that is one pixel row off - why the kernel tests run with both."""
import pytest
import torch
import torch.nn.functional as F

import _guard as G

TYPES = (torch.bfloat16, torch.float16, torch.float32)


@pytest.mark.parametrize("poison", G.POISONS)
@pytest.mark.parametrize("shape,dtype,fill", [((2, 5, 7, 24), torch.bfloat16, float("nan")), ((1, 3, 3, 8), torch.float32, -77.0),
                                             ((128, 192), torch.float16, 1.5), ((11,), torch.int32, 0), ((3, 200, 200, 48), torch.float32, -77.0)])
def test_payload_margins_and_alignment(shape, dtype, fill, poison):
    g = G.Guard(poison, "cpu")
    t = G.guarded(shape, dtype, fill, poison, "cpu", g, "t")
    name, raw, rz, nbytes = g.items[0]
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 256 == 0
    assert nbytes == t.numel() * t.element_size() and raw.numel() == nbytes + 2 * rz and t.data_ptr() == raw.data_ptr() + rz
    plane = shape[1] * shape[2] * shape[3] * t.element_size() if len(shape) == 4 else 0
    assert rz % 256 == 0 and rz >= 65536 and rz >= plane and rz < max(65536, plane) + 256
    assert bool((raw[:rz] == poison).all()) and bool((raw[rz + nbytes:] == poison).all())
    if fill != fill:
        assert bool(torch.isnan(t).all())
    else:
        assert bool((t == fill).all())
    g.assert_intact()
    assert g.report() == []


def test_margin_rule():
    assert G.margin_bytes((4, 8, 8, 16), torch.bfloat16) == 65536                       # a small plane: the floor
    assert G.margin_bytes((4, 104, 104, 40), torch.bfloat16) == 104 * 104 * 40 * 2      # one image plane (a multiple of 256 already)
    assert G.margin_bytes((2, 51, 103, 9), torch.float32) == (51 * 103 * 9 * 4 + 255) // 256 * 256
    assert G.margin_bytes((2, 3, 201, 203), torch.float32) == (3 * 201 * 203 * 4 + 255) // 256 * 256    # NCHW input: c x h x w
    assert G.margin_bytes((1000,), torch.int32) == 65536 and G.margin_bytes((128, 4608), torch.bfloat16) == 65536
    assert G.margin_bytes((10,), torch.uint8, plane=100000) == 100096


@pytest.mark.parametrize("poison", G.POISONS)
def test_one_byte_writes_are_reported_with_side_and_offset(poison):
    g = G.Guard(poison, "cpu")
    a = g.alloc("x", (1, 4, 4, 8), torch.bfloat16, float("nan"))
    b = g.alloc("y", (2, 3, 5, 16), torch.float32, -77.0)
    _, raw_a, rz_a, nb_a = g.items[0]
    _, raw_b, rz_b, nb_b = g.items[1]
    g.assert_intact()
    raw_b[rz_b - 1] = 0                                           # the last byte below y
    assert g.report() == [("y", "below", 1, -1)]
    with pytest.raises(AssertionError, match=r"y: 1 byte\(s\) below the payload changed, first at offset -1"):
        g.assert_intact()
    raw_b[rz_b - 1] = poison
    raw_a[rz_a + nb_a] = 1                                        # the first byte above x
    raw_a[rz_a + nb_a + 700] = 2
    assert g.report() == [("x", "above", 2, 0)]
    with pytest.raises(AssertionError, match=r"x: 2 byte\(s\) above the payload changed, first at offset 0"):
        g.assert_intact()
    raw_a[rz_a + nb_a] = poison
    raw_a[rz_a + nb_a + 700] = poison
    raw_a[0] = 3                                                  # the far ends of both margins
    raw_b[-1] = 3
    assert g.report() == [("x", "below", 1, -rz_a), ("y", "above", 1, rz_b - 1)]
    assert bool(torch.isnan(a).all()) and bool((b == -77.0).all()), "the payload changed"
    # writing the payload's own first and last byte is no finding
    raw_a[0] = poison
    raw_b[-1] = poison
    raw_b[rz_b] = 0
    raw_b[rz_b + nb_b - 1] = 0
    g.assert_intact()


def test_like_copies_and_plain_has_the_same_interface():
    src = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).view(2, 3, 4, 8)
    for a in (G.Guard(0xFF, "cpu"), G.Plain("cpu")):
        t = a.like("src", src)
        assert torch.equal(t, src) and t.data_ptr() != src.data_ptr()
        z = a.alloc("z", (5,), torch.int32)
        assert z.dtype == torch.int32 and int(z.abs().sum()) == 0
        f = a.alloc("f", (1, 2, 2, 8), torch.bfloat16, -77.0)
        assert bool((f == -77.0).all())
        a.assert_intact()
        assert a.report() == []


def test_poisons_decode_as_documented():
    def decode(byte, dtype):
        return torch.full((8,), byte, dtype=torch.uint8).view(dtype)
    for dt in TYPES:
        assert bool(torch.isnan(decode(0xFF, dt)).all()), dt
    assert bool((decode(0xFF, torch.int32) == -1).all())
    for dt in (torch.bfloat16, torch.float32):
        v = decode(0x7F, dt).double()
        assert bool(torch.isfinite(v).all()) and bool(((v - 3.39e38).abs() < 0.01e38).all()), dt
    assert bool(torch.isnan(decode(0x7F, torch.float16)).all())
    assert bool((decode(0x7F, torch.int32) == 0x7F7F7F7F).all())


def _window_off_by_one_row(poison, dtype, pool):
    """A 3x3 / pad 1 window over the first image of a guarded NHWC map whose padding test is one row off: the row ABOVE row 0 - the
    bytes in front of the payload - takes part instead of being masked.  ``pool``: max pool; otherwise a conv whose taps on that row
    have zero weights (what a weight matrix zero-padded to kpad gives a stray k index)."""
    h, w, c = 5, 6, 8
    g = G.Guard(poison, "cpu")
    x = G.guarded((1, h, w, c), dtype, 0.0, poison, "cpu", g, "x")
    gen = torch.Generator().manual_seed(7)
    x.copy_(torch.randint(-3, 4, (1, h, w, c), generator=gen).to(dtype))
    _, raw, rz, nbytes = g.items[0]
    row = w * c * x.element_size()
    wide = raw[rz - row:rz + nbytes].view(dtype).view(1, h + 1, w, c)          # the map as the faulty kernel addresses it
    a = wide.float().permute(0, 3, 1, 2)                                       # NCHW, rows -1 .. h - 1
    good = x.float().permute(0, 3, 1, 2)
    if pool:
        got = F.max_pool2d(F.pad(a, (1, 1, 0, 1), value=float("-inf")), 3, 1)   # output row i is centred on image row i; row 0 sees row -1
        want = F.max_pool2d(good, 3, 1, 1)
    else:
        wt = torch.randint(-2, 3, (4, c, 3, 3), generator=gen).float()
        wt[:, :, 0, :] = 0.0                                                   # the taps that reach row -1 from output row 0
        got = F.conv2d(F.pad(a, (1, 1, 0, 1)), wt)
        want = F.conv2d(good, wt, padding=1)
    assert got.shape == want.shape == (1, got.shape[1], h, w)
    g.assert_intact()                                                          # a read leaves the margins alone
    return got, want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_why_both_poisons_conv_window_with_zero_weights(dtype):
    """The stray tap meets a zero weight: 0xFF (NaN * 0 = NaN) shows in the output, 0x7F (3.39e38 * 0 = 0) does not."""
    got, want = _window_off_by_one_row(0xFF, dtype, pool=False)
    assert bool(torch.isnan(got[:, :, 0]).all()) and torch.equal(got[:, :, 1:], want[:, :, 1:])
    got, want = _window_off_by_one_row(0x7F, dtype, pool=False)
    assert torch.equal(got, want), "0x7F times a zero weight must vanish"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_why_both_poisons_max_window(dtype):
    """A max keeps 3.39e38 (0x7F); the NaN of 0xFF is dropped by a kernel's compare-and-select max (v > m ? v : m), which the
    emulation below spells out, so there the 0xFF run sees nothing."""
    got, want = _window_off_by_one_row(0x7F, dtype, pool=True)
    assert bool((got[:, :, 0] > 3e38).all()) and torch.equal(got[:, :, 1:], want[:, :, 1:])
    # compare-and-select over the same faulty window with NaN in the stray row
    h, w, c = 5, 6, 8
    g = G.Guard(0xFF, "cpu")
    x = G.guarded((1, h, w, c), dtype, 0.0, 0xFF, "cpu", g, "x")
    x.copy_(torch.randint(-3, 4, (1, h, w, c), generator=torch.Generator().manual_seed(7)).to(dtype))
    _, raw, rz, nbytes = g.items[0]
    row = w * c * x.element_size()
    wide = raw[rz - row:rz + nbytes].view(dtype).view(1, h + 1, w, c).float()
    m = torch.full((w, c), float("-inf"))
    for r in (0, 1, 2):                                                        # rows -1, 0, 1 of the image: output row 0
        for dx in (-1, 0, 1):
            v = torch.full((w, c), float("-inf"))
            lo, hi = max(0, -dx), min(w, w - dx)
            v[lo:hi] = wide[0, r, lo + dx:hi + dx]
            m = torch.where(v > m, v, m)                                       # NaN > m is false: the poison is dropped
    assert torch.equal(m, F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 1, 1)[0, :, 0].t())


# ---- the plan-level audit's case table (tests/_guard_plan_cases.py): what each chosen input size yields, without a GPU ----------------
def _plan_case_ids():
    from _guard_plan_cases import PLAN_CASES
    return list(PLAN_CASES)


@pytest.mark.parametrize("name", _plan_case_ids())
def test_guarded_plan_cases_hold_every_launch_kind(name, monkeypatch):
    """The launch list of every case of the plan-level guard-band audit holds exactly the op kinds its row names - for the fp16 mode
    both 20x20-tile kernels (stride 1 and stride 2) where the family has layers for them, none with YOLO_FP16_T20=0 -, at batch 3 and
    an input of unequal sides that are multiples of 32."""
    from _guard_plan_cases import PLAN_CASES, build_model, plan_kinds
    from pytorch_yolo_amd import engine
    from pytorch_yolo_amd import kernels as K
    family, kw, precision, env, (bs, h, w), kinds, t20_strides = PLAN_CASES[name]
    assert bs == 3 and h % 32 == 0 and w % 32 == 0 and h != w
    monkeypatch.delenv("YOLO_FP16_T20", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert K.set_launch_cus(256) == 256            # (the size of the chip the rules of the table are written for)
    torch.manual_seed(0)
    model = build_model(family, kw)
    rec = engine.Recorder(bs, 3, h, w)
    model._trace(rec, rec.input)
    plan = engine.Plan(rec, torch.device("cpu"), model.n_class, max(h, w), precision)
    got, strides = plan_kinds(plan)
    assert got == set(kinds), sorted(got)
    assert strides == set(t20_strides)


@pytest.mark.parametrize("word,byte", [(None, 0x7F), ("0xFF", 0xFF), ("255", 0xFF), ("0x7f", 0x7F)])
def test_plan_allocator_takes_its_poison_from_the_environment(word, byte, monkeypatch):
    """pytorch_yolo_amd/diag.py::GuardedAlloc: YOLO_REDZONE_BYTE next to YOLO_REDZONE selects the poison of the plan's margins (0x7F
    without it); redzone_report() compares with that byte and counts a changed byte on either side."""
    from pytorch_yolo_amd import YOLOv3Tiny, engine
    monkeypatch.setenv("YOLO_REDZONE", "4096")
    if word is None:
        monkeypatch.delenv("YOLO_REDZONE_BYTE", raising=False)
    else:
        monkeypatch.setenv("YOLO_REDZONE_BYTE", word)
    torch.manual_seed(0)
    model = YOLOv3Tiny(n_class=3, kernels_divider=8).eval()
    rec = engine.Recorder(2, 3, 64, 96)
    model._trace(rec, rec.input)
    plan = engine.Plan(rec, torch.device("cpu"), model.n_class, 96, "bf16")
    assert plan.redzone_byte() == byte and len(plan._redzones) >= plan.n_ops
    for raw, rz, nbytes in plan._redzones:
        assert rz == 4096 and bool((raw[:rz] == byte).all()) and bool((raw[rz + nbytes:] == byte).all())
    assert plan.redzone_report() == []
    monkeypatch.setenv("YOLO_REDZONE_BYTE", "0x00")              # (the plan keeps the byte it was built with)
    assert plan.redzone_report() == []
    raw, rz, nbytes = plan._redzones[3]
    raw[rz - 1] = byte ^ 1
    raw[rz + nbytes] = byte ^ 1
    raw[rz + nbytes + 9] = byte ^ 1
    assert plan.redzone_report() == [(3, nbytes, 1, 2)]
    monkeypatch.setenv("YOLO_REDZONE_BYTE", "300")
    rec = engine.Recorder(2, 3, 64, 96)
    model._trace(rec, rec.input)
    with pytest.raises(RuntimeError, match="not a byte"):
        engine.Plan(rec, torch.device("cpu"), model.n_class, 96, "bf16")
