#!/usr/bin/env python3
"""Canonical text of the conv dispatcher's answers, for "did this refactor change which kernel a layer gets?" checks.

The pick entry points run the real dispatch path without launching (no GPU needed), so two builds whose rules agree print the
same text byte for byte:

    python tools/pick_dump.py > head.txt
    YOLO_HIP_LIB=<libyolo_hip.so of another commit> python tools/pick_dump.py > other.txt && cmp head.txt other.txt

One line per case: the case, then the answer of yolo_conv2d_pick / yolo_head_decode_pick / yolo_conv2d_splitk_plan, or the error
text.  Cases: every combination of batch, map, (cin, cout), kernel size / stride, residual, pre-add copy, output view alignment,
output type, upsample2x and yolo_set_launch_cus; on a thinner set of shapes every named bit of tuning knobs 1 and 2 alone (the
names and values come from csrc/tuning.h of THIS checkout; the numbers mean the same to an older library) and variants 0..13.
The last line on stderr is the line count and the SHA-256 of the text."""
import ctypes as C
import hashlib
import itertools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_yolo_amd import _lib                                        # noqa: E402

BATCHES = (1, 16, 32)
MAPS = (13, 20, 26, 40, 52, 80, 160, 320)
CHANNELS = ((8, 32), (24, 64), (40, 256), (32, 18), (32, 64), (64, 24), (64, 64), (64, 128), (96, 255), (128, 64), (128, 256),
            (256, 128), (256, 255), (256, 512), (384, 128), (512, 256), (512, 1024), (1024, 512), (1024, 255), (1280, 64), (1280, 1024))
KS = ((1, 1), (1, 2), (3, 1), (3, 2))
CUS = (256, 128, 64)
HEADS = ((18, 3, 1), (24, 3, 3), (255, 3, 80))          # cout, na, nc


def up(v, m):
    return (v + m - 1) // m * m


def desc(n, hw, cin, cout, k, s, view4=False, f32=False, upsample=False):
    pad = k // 2
    ho = (hw + 2 * pad - k) // s + 1
    total, off = (up(cout, 4) + 4, 4) if view4 else (up(cout, 8), 0)      # 4-aligned view / 8-aligned view of y, residual, pre-add copy
    return _lib.YoloConvDesc(n=n, h=hw, w=hw, cin=cin, in_c_total=cin, in_c_offset=0, ho=ho, wo=ho, cout=cout, out_c_total=total,
                             out_c_offset=off, ksize=k, stride=s, pad=pad, act=_lib.ACT_LEAKY01, upsample2x=int(upsample),
                             out_dtype=_lib.DT_F32 if f32 else _lib.DT_BF16, kpad=up(k * k * cin, 64), cout_pad=up(cout, 128),
                             res_c_total=total, res_c_offset=off, aux_c_total=total, aux_c_offset=off)


def knob_bits(prefix):
    text = open(os.path.join(ROOT, "pytorch_yolo_amd", "csrc", "tuning.h")).read()
    return [(name, int(value)) for name, value in re.findall(r"^\s*(%s\w+) = (\d+),?" % prefix, text, re.M)]


def main():
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    lines = []

    def answer(rc):
        return buf.value.decode() if rc == 0 else "error: " + lib.yolo_last_error().decode("utf-8", "replace")

    def conv(tag, d, res, aux):
        lines.append(f"{tag} -> {answer(lib.yolo_conv2d_pick(C.byref(d), int(res), int(aux), buf, len(buf)))}")

    def shape(n, hw, cin, cout, k, s):
        return f"n{n} {hw}x{hw} {cin}->{cout} k{k}s{s}"

    for cus in CUS:
        lib.yolo_set_launch_cus(cus)
        for (n, hw, (cin, cout), (k, s)) in itertools.product(BATCHES, MAPS, CHANNELS, KS):
            for res, aux, view4, f32, ups in itertools.product((False, True), repeat=5):
                d = desc(n, hw, cin, cout, k, s, view4, f32, ups)
                tag = f"cus{cus} {shape(n, hw, cin, cout, k, s)} res{int(res)} aux{int(aux)} view{4 if view4 else 8} {'f32' if f32 else 'bf16'} up{int(ups)}"
                conv(tag, d, res, aux)
                if cus == CUS[0]:                                         # the split-K plan does not depend on the CU share
                    sp, ws, cnt = C.c_int(), C.c_size_t(), C.c_int()
                    rc = lib.yolo_conv2d_splitk_plan(C.byref(d), int(res), int(aux), C.byref(sp), C.byref(ws), C.byref(cnt))
                    lines.append(f"splitk {tag} -> " + (f"{sp.value} {ws.value} {cnt.value}" if rc == 0 else answer(rc)))
        for (n, hw, cin, (cout, na, nc), filt) in itertools.product(BATCHES, MAPS, sorted({c for c, _ in CHANNELS}), HEADS, (0, 1)):
            d = desc(n, hw, cin, cout, 1, 1)
            rc = lib.yolo_head_decode_pick(C.byref(d), na, nc, filt, buf, len(buf))
            lines.append(f"head cus{cus} n{n} {hw}x{hw} {cin}->{cout} na{na} nc{nc} filter{filt} -> {answer(rc)}")
    lib.yolo_set_launch_cus(256)

    # every named bit of YOLO_CONV_DEBUG (knob 1) and YOLO_CONV_PP (knob 2) alone, and every variant (knob 0)
    settings = [(1, name, v) for name, v in knob_bits("kCd")] + [(2, name, v) for name, v in knob_bits("kFam")] + \
               [(0, f"variant{v}", v) for v in range(14)]
    for knob, name, value in settings:
        old = lib.yolo_set_tuning(knob, value)
        try:
            for (hw, (cin, cout), (k, s), res) in itertools.product((13, 20, 40, 80, 160), CHANNELS, KS, (False, True)):
                conv(f"{name} {shape(16, hw, cin, cout, k, s)} res{int(res)}", desc(16, hw, cin, cout, k, s), res, False)
            for (hw, (cout, na, nc)) in itertools.product((20, 80), HEADS):
                for cin in (24, 32, 256):
                    d = desc(16, hw, cin, cout, 1, 1)
                    rc = lib.yolo_head_decode_pick(C.byref(d), na, nc, 0, buf, len(buf))
                    lines.append(f"{name} head n16 {hw}x{hw} {cin}->{cout} -> {answer(rc)}")
        finally:
            lib.yolo_set_tuning(knob, old)

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    print(f"{len(lines)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
