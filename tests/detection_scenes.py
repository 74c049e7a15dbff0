"""Seeded random detection scenes shared by tests/test_detection_eval_cpu.py and tests/test_gpu_detection_eval.py, and the converters between
the three forms a scene is fed in: tests/cocoeval_ref.py's dicts, DetectionEvaluator.process's raw arrays and the device kernel's tensors.

A scene: 1-6 images, 1-5 classes, 0-40 ground-truth boxes and 0-150 detections per image.  Coordinates lie on a 1/4-pixel grid (exact in
fp32) and a large share of the detections are shifted copies of ground-truth boxes, so many IoUs tie or sit exactly on a threshold;
10 % of the ground truth is crowd; scores come from a 1/64 grid, so duplicates are common."""
import numpy as np

from focoos_amd.ports import DetectionDatasetEntry


def _boxes(rs, n, size):
    x0 = rs.randint(0, 4 * size - 8, size=n) / 4.0
    y0 = rs.randint(0, 4 * size - 8, size=n) / 4.0
    w = rs.choice([2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 200], size=n) * rs.choice([0.25, 0.5, 1.0, 1.0, 1.5], size=n)
    h = rs.choice([2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 200], size=n) * rs.choice([0.25, 0.5, 1.0, 1.0, 1.5], size=n)
    return np.stack([x0, y0, np.minimum(x0 + w, size), np.minimum(y0 + h, size)], 1).astype(np.float32)


def make_scene(seed, n_images=None, n_classes=None, max_gt=40, max_det=150, size=256):
    rs = np.random.RandomState(seed)
    K = int(rs.randint(1, 6)) if n_classes is None else n_classes
    images = []
    for i in range(int(rs.randint(1, 7)) if n_images is None else n_images):
        G, D = int(rs.randint(0, max_gt + 1)), int(rs.randint(0, max_det + 1))
        gxyxy = _boxes(rs, G, size)
        gcat = rs.randint(0, K, size=G)
        crowd = rs.rand(G) < 0.10
        dxyxy = _boxes(rs, D, size)
        if G and D:
            cp = rs.rand(D) < 0.6                                  # shifted copies of gt boxes: ties and on-threshold IoUs
            src = rs.randint(0, G, size=D)
            shift = (rs.randint(-8, 9, size=(D, 1)) / 4.0 * (rs.rand(D, 1) < 0.5)).astype(np.float32)
            dxyxy = np.where(cp[:, None], np.clip(gxyxy[src] + shift * np.array([[1, 0, 1, 0]], np.float32), 0, size), dxyxy).astype(np.float32)
            dcat = np.where(cp & (rs.rand(D) < 0.8), gcat[src], rs.randint(0, K, size=D))
        else:
            dcat = rs.randint(0, K, size=D)
        ok = (dxyxy[:, 2] > dxyxy[:, 0]) & (dxyxy[:, 3] > dxyxy[:, 1])
        dxyxy, dcat = dxyxy[ok], dcat[ok]
        score = (rs.randint(1, 64, size=len(dxyxy)) / 64.0).astype(np.float32)
        gts = []
        for b, c, cr in zip(gxyxy.astype(np.float64), gcat, crowd):
            gts.append({"bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], "category_id": int(c), "iscrowd": int(cr)})
        images.append({"image_id": i, "xyxy": dxyxy, "score": score, "cls": dcat.astype(np.int64), "gts": gts})
    return {"class_names": [f"c{k}" for k in range(K)], "images": images}


def ref_images(scene):
    """tests/cocoeval_ref.py's input: XYWH with the subtraction done in fp32 (what the evaluator does to float32 predictions)."""
    out = []
    for im in scene["images"]:
        b = im["xyxy"].astype(np.float32)
        xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float64) if len(b) else np.zeros((0, 4))
        dets = [{"bbox": [float(v) for v in xywh[j]], "score": float(im["score"][j]), "category_id": int(im["cls"][j])} for j in range(len(b))]
        out.append({"image_id": im["image_id"], "dets": dets, "gts": [dict(g) for g in im["gts"]]})
    return out


def entries_and_outputs(scene):
    """(inputs, outputs) of DetectionEvaluator.process in the raw-array form"""
    inputs = [DetectionDatasetEntry(image_id=im["image_id"], height=256, width=256, annotations=[dict(g) for g in im["gts"]]) for im in scene["images"]]
    outputs = [{"boxes": im["xyxy"].copy(), "scores": im["score"].copy(), "classes": im["cls"].copy()} for im in scene["images"]]
    return inputs, outputs


def golden_scene(case):
    """a case of tests/golden/coco_bbox_cases.json in make_scene's form"""
    images = []
    for im in case["images"]:
        d = im["dets"]
        images.append({"image_id": im["image_id"], "xyxy": np.array([x["bbox_xyxy"] for x in d], np.float32).reshape(-1, 4),
                       "score": np.array([x["score"] for x in d], np.float32), "cls": np.array([x["category_id"] for x in d], np.int64),
                       "gts": [dict(g) for g in im["gts"]]})
    return {"class_names": list(case["class_names"]), "images": images}
