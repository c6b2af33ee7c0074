"""Host mirror of the part of reference utils/coco_helper.py that validation uses."""
from __future__ import annotations


def results_from_dict(data: dict, annotations: dict):
    """The prediction dictionary of ``predict_dataset`` ({file name: [{'type', 'score', 'left', 'top', 'right', 'bottom'}]}) as a
    COCO results list (reference coco_helper.py:119-139): image ids come from ``annotations['images']``, a box is
    [left, top, right - left + 1, bottom - top + 1].  Without a single prediction the list holds one placeholder (image 1,
    category 0, zero box, score 0), as in the reference, so that a results file is never empty."""
    ids = {img["file_name"]: img["id"] for img in annotations["images"]}
    results = []
    for file_name, preds in data.items():
        image_id = ids[file_name]
        for p in preds:
            box = [p["left"], p["top"], p["right"] - p["left"] + 1, p["bottom"] - p["top"] + 1]
            results.append({"image_id": image_id, "category_id": p["type"], "bbox": box, "score": p["score"]})
    if not results:
        results.append({"image_id": 1, "category_id": 0, "bbox": [0, 0, 0, 0], "score": 0})
    return results
