#!/usr/bin/env python3
"""Record tests/golden/ops_trace.json on the GPU: the launch list of every case of tests/test_ops_trace_gpu.py - case name -> list of
records (binding name; per argument a tensor's dtype, shape and contiguity, a YoloConvDesc's fields, the number itself, or a tuple of
numbers as a list), the forward's records followed by the backward's.  Sorted keys, one record per line; a rerun on the same code reproduces the file byte for byte.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ops_trace.py [output path]

Re-record only when an op's launch list changes on purpose, and review the diff: one line is one launch."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def dumps(traces):
    lines = ["{"]
    names = sorted(traces)
    for name in names:
        lines.append(f" {json.dumps(name)}: [")
        lines.extend(f"  {json.dumps(r, sort_keys=True)}," for r in traces[name])
        if traces[name]:
            lines[-1] = lines[-1][:-1]
        lines.append(" ]," if name != names[-1] else " ]")
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    import test_ops_trace_gpu as T
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    traces = {}
    with pytest.MonkeyPatch.context() as mp:
        sink = T.install(mp)
        for name in T.CASES:
            forward, backward = T.trace_case(name, sink)
            traces[name] = forward + backward
    text = dumps(traces)
    assert json.loads(text) == traces
    with open(path, "w") as f:
        f.write(text)
    print(f"{os.path.basename(path)}  {len(text) / 1024:.1f} KiB  ({len(traces)} cases, {sum(len(v) for v in traces.values())} records)")


if __name__ == "__main__":
    main()
