#!/usr/bin/env python3
"""The smallest layers the shipped rules send to each conv kernel family of a full-size training step (tests/_train_families.py).

CPU only: yolo_conv2d_pick is a pure function of the descriptor, the tuning words and the compute-unit count (256 by default).  For every
(role, family) of the four enumerated steps - role "forward" (ops._desc of the training forward) or "dgrad" (the descriptor
yolo_conv2d_bwd_data builds) - the script walks a grid of layers (n, h, w, cin, cout, k) over odd maps and prints the cheapest ones by
multiply-accumulates that
  * pick the family under no tuning word; a family no such layer reaches inside the cost cap is searched again under the word the forward
    exact tests use for it (tests/_exact_cases.py: T20_ALWAYS for the 20x20-tile kernels) and printed with it;
  * have more than one pixel tile, the last one partial (h, w no multiples of the 16- or 20-pixel tile side, n h w no multiple of the GEMM tile's rows or of the
    streaming kernels' pixel block) and at least two K steps (k k cin against the tile's BK / CK);
  * keep the float64 restatement (tests/_conv_bwd.grads: three convs and the unfold for dW) inside the cap: the unfolded input
    n cin k k h w at most UNFOLD_CAP elements (8 bytes each, about four copies live at once) and at most MAC_CAP multiply-accumulates.
Beside each layer stands the family its OTHER role picks: one layer may serve two entries of FAMILY_CASES.

    PYTHONPATH=. python tests/diag/family_shape_search.py [--top N] [--cin C]      (--cin: only layers with that cin, e.g. 768 or 2048)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _exact_cases as E                                 # noqa: E402
import _train_families as TF                             # noqa: E402
from test_conv_exact_cpu import tuning                   # noqa: E402

UNFOLD_CAP, MAC_CAP = TF.UNFOLD_CAP, TF.MAC_CAP
SIDES = (5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 35, 37, 39, 41, 43, 45, 47, 49, 51, 53, 57, 61, 67, 71, 75, 79, 83, 87, 91, 97, 101, 103,
         107, 113, 119, 121, 127, 131, 139, 149, 157, 163)
CHANNELS = (8, 16, 32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048)
BATCHES = (1, 2, 3, 4, 5, 6, 7, 8)


def layers(strides, only_cin):
    for i, h in enumerate(SIDES[:-1]):
        w = SIDES[i + 1]
        for k in (1, 3):
            for stride in strides:
                if stride == 2 and k == 1:
                    continue
                for cin in CHANNELS:
                    if only_cin and cin != only_cin:
                        continue
                    for n in BATCHES:
                        if n * cin * k * k * h * w > UNFOLD_CAP:
                            break
                        for cout in CHANNELS + (255,):
                            ho, wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if stride == 2 else (h, w)
                            macs = n * ho * wo * cin * cout * k * k
                            if macs > MAC_CAP:
                                break
                            yield (n, h, w, cin, cout, k), stride, macs


def search(targets, knobs, strides, only_cin, top):
    """{(role, family): [(macs, layer, stride, other role's family)]} of the ``top`` cheapest layers."""
    from pytorch_yolo_amd import kernels as K
    found = {t: [] for t in targets}
    with tuning(*knobs):
        for (n, h, w, cin, cout, k), stride, macs in layers(strides, only_cin):
            d = TF.forward_desc(n, h, w, cin, cout, k, stride, cout % 8 != 0)       # cout 255: the fp32 head form
            fams = {"forward": TF.family(K.conv2d_pick(d))}
            if stride == 1 and cout % 8 == 0:
                fams["dgrad"] = TF.family(K.conv2d_pick(TF.dgrad_desc(d)))
            for role, fam in fams.items():
                if (role, fam) not in found or (stride == 2 and not fam.startswith("t20s2")):
                    continue           # (a stride-2 layer is a case only for the stride-2 kernel: the other families have stride-1 layers)
                k_terms = k * k * (cin if role == "forward" else cout)
                if not TF.partial_and_two_k_steps(fam, n, d.ho if role == "forward" else h, d.wo if role == "forward" else w, k_terms):
                    continue
                other = fams.get("dgrad" if role == "forward" else "forward", "-")
                found[(role, fam)].append((macs, (n, h, w, cin, cout, k), stride, other))
    return {t: sorted(v)[:top] for t, v in found.items()}


def main():
    top = int(sys.argv[sys.argv.index("--top") + 1]) if "--top" in sys.argv else 3
    only_cin = int(sys.argv[sys.argv.index("--cin") + 1]) if "--cin" in sys.argv else 0
    targets = set()
    for config in TF.CONFIGS:
        targets |= {key for key in TF.enumerate_step(config)[0] if key[0] in ("forward", "dgrad")}
    found = search(targets, (-1, 0, 0), (1, 2), only_cin, top)
    missing = sorted(t for t, v in found.items() if not v)
    forced = search(missing, (-1, 0, E.T20_ALWAYS), (1, 2), only_cin, top) if missing else {}
    for t in sorted(targets):
        rows, word = (found[t], "no tuning word") if found[t] else (forced.get(t, []), "knob 2 = T20_ALWAYS")
        print(f"{t[0]:8s} {t[1]}   [{word if rows else 'NOT REACHED inside the cap'}]")
        for macs, layer, stride, other in rows:
            print(f"           {layer} stride {stride}  {macs / 1e9:.3f} GMAC   other role: {other}")


if __name__ == "__main__":
    main()
