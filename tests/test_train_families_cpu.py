"""Host-side half of the training-family tests (no GPU): the conv kernels the four full-size training steps select -
forward, stride-1 data gradient, weight gradient, stride-2 data gradient - are enumerated from the models' own wiring, every
(role, family) has a case in tests/_train_families.FAMILY_CASES, every case picks its family under its own tuning words, and every case's
integer operands determine every bit (tests/_conv_bwd.exact_conditions).  tests/test_train_families_gpu.py launches the same table.

A new dispatch rule that sends a training layer to a family without a case fails test_every_family_of_a_full_size_step_has_a_case."""
import functools
import time

import pytest

import _conv_bwd as B
import _conv_down as D
import _train_families as TF
from pytorch_yolo_amd import kernels as K
from pytorch_yolo_amd._lib import load
from test_conv_exact_cpu import tuning

KEYS = list(TF.FAMILY_CASES)
key_id = lambda key: f"{key[0]}-{key[1]}"


@functools.lru_cache(maxsize=None)
def enumeration():
    """{config: Counter of (role, family)} of the four full-size steps at the default 256 compute units (computed once, shared)."""
    assert load().yolo_set_tuning(0, -1) == -1 and load().yolo_set_tuning(1, 0) == 0 and load().yolo_set_tuning(2, 0) == 0
    return {config: TF.enumerate_step(config)[0] for config in TF.CONFIGS}


def test_every_family_of_a_full_size_step_has_a_case():
    counts = enumeration()
    seen = sorted(set().union(*counts.values()))
    print("\nrole      family" + " " * 62 + "  ".join(f"{c:>12s}" for c in TF.CONFIGS) + "   case")
    for role, fam in seen:
        c = TF.FAMILY_CASES.get((role, fam))
        print(f"{role:9s} {fam:67s}" + "  ".join(f"{counts[cfg].get((role, fam), 0):12d}" for cfg in TF.CONFIGS) + "   "
              + (TF.layer_id(c) if c else "(pinned as a set: OTHER_FAMILIES)" if (role, fam) in TF.OTHER_FAMILIES else "NONE"))
    wanted = {key for key in seen if key[0] in ("forward", "dgrad")}
    assert wanted - set(TF.FAMILY_CASES) == set(), "a full-size training layer takes a kernel family that no case launches"
    assert set(TF.FAMILY_CASES) - wanted == set(), "a case for a family no full-size step takes"
    assert {key for key in seen if key[0] in ("wgrad", "dgrad_s2")} == TF.OTHER_FAMILIES
    # the counts the table was built against: 70 stride-1 data gradients in a YOLOv3-SPP step, every conv call has a forward
    spp = counts["spp640x8"]
    assert sum(v for (role, _), v in spp.items() if role == "dgrad") == 70 and sum(v for (role, _), v in spp.items() if role == "forward") == 76
    assert sum(v for (role, _), v in spp.items() if role == "dgrad_s2") == 5 and sum(v for (role, _), v in spp.items() if role == "wgrad") == 76


def test_the_recording_table_follows_the_models():
    """The calls of a step are the models' own: kinds, the padded ConvBlock heads, the fp32 heads, the image layer without a data gradient."""
    for config, (n_calls, kinds) in dict(spp640x8=(76, dict(bn=48, down=5, res=23)), yolov3_416x8=(75, dict(bn=45, down=5, res=23, head=2)),
                                         tiny416x32=(13, dict(bn=6, poolbn=5, head=2)), lite416x16=(20, dict(bn=13, poolbn=5, head=2))).items():
        count, rows = TF.enumerate_step(config)
        got = {}
        for kind, layer, stride, picks in rows:
            got[kind] = got.get(kind, 0) + 1
            assert (stride == 2) == (kind == "down") and ("dgrad" in picks or "dgrad_s2" in picks) == (layer[3] != 3)
        assert len(rows) == n_calls and got == kinds, (config, len(rows), got)
        assert rows[0][1][3] == 3 and sum(layer[3] == 3 for _, layer, _, _ in rows) == 1
        # a plain head keeps its 255 couts (fp32 out), a ConvBlock head arrives padded to 256 (models/train.conv_bn)
        assert all((kind == "head") == (layer[4] == 255) and (kind == "head" or layer[4] % 8 == 0) for kind, layer, _, _ in rows)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_case_picks_its_family(key):
    """Under its own tuning words a case's descriptors - the ones ops._desc / yolo_conv2d_bwd_data build and the ones the test harness
    launches - pick the family; the shape has more than one pixel tile, a partial last one and two K steps; a tuning word is set only
    where the shipped rule does not reach the family, with the reason beside it."""
    role, fam = key
    c = TF.FAMILY_CASES[key]
    n, h, w, cin, cout, k = c["case"][:6]
    assert load().yolo_set_tuning(0, -1) == -1 and load().yolo_set_tuning(1, 0) == 0 and load().yolo_set_tuning(2, 0) == 0
    picks = TF.case_picks(c)
    print(f"\n{role} {fam}: {TF.layer_id(c)} picks {picks}")
    assert picks[role] == fam
    with tuning(*c["knobs"]):
        harness = D.fwd_desc(TF.down_case(c)) if c["stride"] == 2 else B.fwd_desc(c["case"])
        assert TF.family(K.conv2d_pick(harness)) == picks["forward"]
        if c["stride"] == 1:
            assert TF.family(K.conv2d_pick(TF.dgrad_desc(harness))) == picks["dgrad"] and TF.family(K.conv2d_bwd_pick(harness)) == picks["wgrad"]
    d = TF.case_desc(c)
    ho, wo = (d.ho, d.wo) if role == "forward" else (h, w)
    assert TF.partial_and_two_k_steps(fam, n, ho, wo, k * k * (K.roundup(cin, 8) if role == "forward" else K.roundup(cout, 8)))
    if c["knobs"] != (-1, 0, 0):
        assert c["why"] and TF.picks_of(d)[role] != fam, "a tuning word where the shipped rule reaches the family"
    else:
        assert not c["why"]


@pytest.mark.parametrize("c", TF.CASES, ids=TF.layer_id)
def test_case_is_exact_and_inside_the_cost_cap(c):
    """The float64 witnesses of exactness (tests/_conv_bwd.exact_conditions / _conv_down.exact_conditions): every operand and sum an
    integer, every sum of |terms| below 2^24, dx leaves the bf16 integers where it has 128 terms or more; and the restatement stays inside
    the cap the shapes were searched under."""
    n, h, w, cin, cout, k = c["case"][:6]
    assert n * cin * k * k * h * w <= TF.UNFOLD_CAP and n * h * w * cin * cout * k * k // c["stride"] ** 2 <= TF.MAC_CAP
    t0 = time.perf_counter()
    r = D.exact_conditions(TF.down_case(c)) if c["stride"] == 2 else B.exact_conditions(c["case"])
    print(f"\n{TF.layer_id(c)}: {r}  ({time.perf_counter() - t0:.2f} s for the restatement)")
    assert r["integers"] and r["largest_abs_sum"] < 2 ** 24
    if cout * k * k >= B.DX_ROUNDING_FROM_TERMS:
        assert r["dx_rounded"] is not None and r["dx_rounded"] > 0
    if c["stride"] == 2:
        assert 0.15 < r["y_nonpositive"] < 0.85          # (LeakyReLU in the stride-2 harness; the stride-1 cases run act none)


def test_the_other_families_are_launched():
    """The weight-gradient tiles and the parity data-gradient tiles of the full-size steps: each is what a case of this table or of
    tests/_conv_down.py launches."""
    launched = set()
    for c in TF.CASES:
        p = TF.case_picks(c)
        launched |= {(role, p[role]) for role in ("wgrad", "dgrad_s2") if role in p}
    for pick in D.PICKS:
        wgrad, dgrad = TF.family(pick).split("; ")
        launched |= {("wgrad", wgrad), ("dgrad_s2", dgrad)}
    assert TF.OTHER_FAMILIES <= launched, TF.OTHER_FAMILIES - launched


def test_the_widths_only_a_data_gradient_has():
    """384 and 768 (the FPN concats) and 2048 (the SPP) are output counts only in a data gradient: each has a case in the family the
    full-size layer takes."""
    rows = TF.enumerate_step("spp640x8")[1]
    for width in (384, 768, 2048):
        full = [picks["dgrad"] for _, layer, _, picks in rows if layer[3] == width]
        mine = [TF.case_picks(c)["dgrad"] for c in TF.CASES if c["case"][3] == width and c["stride"] == 1]
        assert len(full) == 1 and full[0] in mine, (width, full, mine)
