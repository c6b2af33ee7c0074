#!/usr/bin/env python3
"""Record tests/golden/shuffle_trace_nodes.json: the node list of YOLOv3TinyShuffle's eval trace at 416 (tests/_train_shuffle.eval_trace_nodes;
no GPU needed) - one node per line: kind, sources, outputs, attrs with every tensor as (shape, dtype, sha256).  A rerun on the same code
reproduces the file byte for byte.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shuffle_trace.py [output path]

The committed file was recorded on the commit whose InvertedResidual._trace, ShuffleEncoder._trace and the head's mapped conv still called
Recorder.conv / dwconv / slice / shuffle2 themselves, before Recorder.conv_bn_relu / shuffle_unit / conv_block_mapped existed.  Re-record
only when the eval graph of the model changes on purpose."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _train_shuffle as S
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "shuffle_trace_nodes.json")
    nodes = S.eval_trace_nodes()
    text = "[\n" + ",\n".join(" " + json.dumps(n) for n in nodes) + "\n]\n"
    assert json.loads(text) == nodes
    with open(path, "w") as f:
        f.write(text)
    print(f"{os.path.basename(path)}  {len(text) / 1024:.1f} KiB  ({len(nodes) - 1} nodes)")


if __name__ == "__main__":
    main()
