#!/usr/bin/env python3
"""Capture tests/golden/nms_styles.npz from the REFERENCE itself: its ``non_max_suppression`` in the styles 'OR', 'AND' and 'SOFT'.

The reference hard-codes ``nms_style = 'MERGE'`` inside the function.  This script holds no reference text: it takes the function's
source at run time (``inspect.getsource``), replaces that single assignment by the wanted style (exactly one occurrence, asserted) and
executes the result in the reference module's own namespace.  Runs only where make_golden.py runs (it imports the reference through
``make_golden.import_reference``):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nms_styles.py

For each style and each image of three inputs - the known-answer rows (_cases.NMS_KAT_ROWS / NMS_KAT_ARGS), ``nms_small_nc2`` and
``nms_none_pass`` - the file holds
    <style>_<input>_count_<b>            number of detections (0: the reference returned None)
    <style>_<input>_dets_<b>   [n, 7]    the reference's rows
    <style>_<input>_kept_<b>   [n]       the input row of each: these styles leave the corners alone, so it is the one input row
                                         whose xywh2xyxy corners equal the output row's four box columns exactly (asserted unique)
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (also puts the repository root and tests/ on sys.path)

STYLES = ("OR", "AND", "SOFT")
NEEDLE = "nms_style = 'MERGE'"


def styled_reference(fn, style):
    src = inspect.getsource(fn)
    assert src.count(NEEDLE) == 1, f"expected exactly one {NEEDLE!r} in the reference's non_max_suppression"
    scope = {}
    exec(compile(src.replace(NEEDLE, f"nms_style = {style!r}"), f"<{fn.__name__}, nms_style {style}>", "exec"),
         sys.modules[fn.__module__].__dict__, scope)
    return scope[fn.__name__]


def kept_indices(pred_before, dets):
    import _nms_styles as S
    xyxy = S.corners(pred_before)
    out = []
    for row in dets:
        hit = np.nonzero((xyxy == row[:4]).all(1))[0]
        assert hit.size == 1, f"{hit.size} input rows have the corners of an output row"
        out.append(hit[0])
    return np.asarray(out, dtype=np.int64)


def main():
    import _cases as C
    torch.set_num_threads(8)
    ref = MG.import_reference()
    inputs = {"kat": (C.NMS_KAT_ROWS[None].copy(), C.NMS_KAT_ARGS["conf_thres"], C.NMS_KAT_ARGS["nms_thres"])}
    for name in ("nms_small_nc2", "nms_none_pass"):
        inputs[name] = C.nms_case_inputs(name)
    arrs = {}
    for style in STYLES:
        fn = styled_reference(ref["nms"], style)
        for name, (pred_np, conf, iou) in inputs.items():
            dets = fn(torch.from_numpy(pred_np.copy()), conf, iou)
            for b, d in enumerate(dets):
                key = f"{style}_{name}"
                n = 0 if d is None else len(d)
                arrs[f"{key}_count_{b}"] = np.int64(n)
                if n:
                    d = d.numpy().astype(np.float32)
                    arrs[f"{key}_dets_{b}"] = d
                    arrs[f"{key}_kept_{b}"] = kept_indices(pred_np[b], d)
                print(f"{key} image {b}: {n} detections")
    path = os.path.join(HERE, "nms_styles.npz")
    np.savez_compressed(path, **arrs)
    print(f"nms_styles.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
