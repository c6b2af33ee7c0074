#!/usr/bin/env python3
"""Record tests/golden/train_wiring.json: the op calls of one ``forward_train`` on ``meta`` tensors for the eight configurations of
tests/test_train_wiring_cpu.py (no GPU needed) - configuration -> {"calls": one record per op call (op name, positional and keyword
arguments in order, output shapes; a tensor argument as the parameter, activation or plain tensor it is), "branches": the shapes of the
returned list}.  Sorted keys, one call per line; a rerun on the same code reproduces the file byte for byte.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_wiring.py [output path]

The committed file was recorded on the commit whose models still had one hand-written ``_train_wiring`` each.  Re-record only when a
model's training wiring changes on purpose, and review the diff: one line is one op call."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def dumps(traces):
    lines = ["{"]
    names = sorted(traces)
    for name in names:
        lines.append(f" {json.dumps(name)}: {{")
        lines.append(f"  \"branches\": {json.dumps(traces[name]['branches'])},")
        lines.append("  \"calls\": [")
        lines.extend(f"   {json.dumps(r, sort_keys=True)}," for r in traces[name]["calls"])
        lines[-1] = lines[-1][:-1]
        lines.append("  ]")
        lines.append(" }," if name != names[-1] else " }")
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    import test_train_wiring_cpu as T
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    traces = {name: T.record(name) for name in T.CONFIGS}
    text = dumps(traces)
    assert json.loads(text) == json.loads(json.dumps(traces))
    with open(path, "w") as f:
        f.write(text)
    print(f"{os.path.basename(path)}  {len(text) / 1024:.1f} KiB  ({len(traces)} configurations, "
          f"{sum(len(v['calls']) for v in traces.values())} calls)")


if __name__ == "__main__":
    main()
