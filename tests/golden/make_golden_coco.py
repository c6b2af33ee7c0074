#!/usr/bin/env python3
"""Golden for the results list of test_model(): the reference's ``results_from_dict``
(/root/reference/pytorch_yolo/utils/coco_helper.py:119-139) run on the prediction dictionaries of CASES below.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_coco.py      # needs /root/reference (build container only)

Writes tests/golden/coco_results.json = {case: {"data", "annotations", "results"}}: the inputs travel with the answers
("data" as a list of (file name, predictions) pairs: the order of the dictionary matters)."""
import json
import os

from make_golden import HERE, import_reference      # sets sys.path, stubs the reference's parent package

IMAGES = {"images": [{"file_name": "a/0001.jpg", "id": 7}, {"file_name": "a/0002.jpg", "id": 3}, {"file_name": "b.png", "id": 11}]}
CASES = {
    "some": {"a/0002.jpg": [{"type": 2, "score": 0.75, "left": 10, "top": 20, "right": 30, "bottom": 50},
                            {"type": 0, "score": 0.125, "left": 0, "top": 0, "right": 0, "bottom": 0}],
             "a/0001.jpg": [{"type": 1, "score": 0.5, "left": 5, "top": 6, "right": 4, "bottom": 5}],
             "b.png": []},
    "none": {},
    "only_empty_lists": {"b.png": [], "a/0001.jpg": []},
}


def main():
    import_reference()
    from pytorch_yolo.utils.coco_helper import results_from_dict
    out = {name: {"data": list(data.items()), "annotations": IMAGES, "results": results_from_dict(data, IMAGES)} for name, data in CASES.items()}
    with open(os.path.join(HERE, "coco_results.json"), "w") as f:
        json.dump(out, f, indent=0)
    print({k: len(v["results"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
