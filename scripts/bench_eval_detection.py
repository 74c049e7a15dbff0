"""End-to-end images/s of FocoosModel.eval_detection on synthetic 640 x 640 images with 300 detections each:
the device matcher (fx_detr_eval_boxes_f32 + fx_coco_match_bbox) against the same run with the matching done by the vectorised host path of
DetectionEvaluator.process / evaluate, and the engine alone (forward + top-k, no evaluator) to state the evaluator's share of the wall time.
Ground truth = the model's own best detections, jittered, so that matches exist.

    python scripts/bench_eval_detection.py [--images 512] [--batch 32] [--gt 12] [--device-only]

The kernel's own time comes from a separate run under ``rocprofv3 --kernel-trace --stats -- python scripts/bench_eval_detection.py
--device-only``."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from focoos_amd import detection_eval as D   # noqa: E402
from focoos_amd.evaluation import _batches   # noqa: E402
from focoos_amd.model import ModelManager   # noqa: E402
from focoos_amd.ports import DetectionDatasetEntry, TrainerArgs   # noqa: E402
from focoos_amd.synth import synth_image_structured   # noqa: E402


def make_data(fm, n, n_gt, size=640, distinct=32):
    dev = fm.model.device
    rs = np.random.RandomState(0)
    base = []
    for i in range(min(n, distinct)):
        img = torch.from_numpy(synth_image_structured(900 + i, size, size)).permute(2, 0, 1).contiguous()
        e = DetectionDatasetEntry(image=img, height=size, width=size)
        out = fm.model.forward(img.permute(1, 2, 0)[None].contiguous().to(dev))
        inst = fm.processor.eval_postprocess(out, [e])[0]["instances"]
        base.append((img, inst.boxes.tensor[:n_gt].cpu().numpy().astype(np.float64), inst.classes[:n_gt].cpu().numpy()))
    data = []
    for i in range(n):
        img, bx, cl = base[i % len(base)]
        b = bx + rs.randint(-3, 4, size=bx.shape)
        b = np.stack([np.clip(b[:, 0], 0, size), np.clip(b[:, 1], 0, size), np.clip(b[:, 2], 0, size), np.clip(b[:, 3], 0, size)], 1)
        anns = [{"bbox": [float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1])], "category_id": int(c), "iscrowd": 0}
                for r, c in zip(b, cl) if r[2] - r[0] >= 1 and r[3] - r[1] >= 1]
        data.append(DetectionDatasetEntry(image=img, height=size, width=size, image_id=i, annotations=anns))
    return data


def engine_only(fm, data, bs):
    """forward + batched eval_postprocess on the device, nothing matched"""
    dev = fm.model.device
    for batch in _batches(data, range(len(data)), bs):
        x = torch.stack([img for _, img in batch]).to(dev).contiguous()
        pl = fm.model.engine.forward(x)
        D.eval_boxes(pl.probs, pl.boxes, [(e.height, e.width) for e, _ in batch], fm.processor.top_k)
    torch.cuda.synchronize(dev)


def host_path(fm, data, bs, names):
    """the same run with the matching on the host: detections copied back per batch into DetectionEvaluator.process"""
    dev = fm.model.device
    ev = D.DetectionEvaluator(names)
    for batch in _batches(data, range(len(data)), bs):
        x = torch.stack([img for _, img in batch]).to(dev).contiguous()
        pl = fm.model.engine.forward(x)
        score, label, keep, xyxy, _ = (t.cpu().numpy() for t in D.eval_boxes(pl.probs, pl.boxes, [(e.height, e.width) for e, _ in batch],
                                                                             fm.processor.top_k))
        outs = [{"boxes": xyxy[i][keep[i] != 0], "scores": score[i][keep[i] != 0], "classes": label[i][keep[i] != 0]} for i in range(len(batch))]
        ev.process([e for e, _ in batch], outs)
    return ev.evaluate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--gt", type=int, default=12)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    fm = ModelManager.get("fai-detr-l-coco", device="cuda:0", seed=1)
    names = list(fm.model_info.classes)
    data = make_data(fm, a.images, a.gt)
    tmp = tempfile.mkdtemp()
    args = TrainerArgs(run_name="bench", output_dir=tmp, batch_size=a.batch)
    engine_only(fm, data[:a.batch], a.batch)                      # the batch's plan exists before anything is timed (eval releases only plans it made)
    fm.eval_detection(args, data[:a.batch], save_json=False)      # warm-up: library, allocator
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fm.eval_detection(args, data, save_json=False)
    t_dev = time.perf_counter() - t
    out = {"images": a.images, "batch": a.batch, "gt_per_image": a.gt, "AP": res["bbox"]["AP"], "device_matcher_s": round(t_dev, 4),
           "device_matcher_img_s": round(a.images / t_dev, 1)}
    if not a.device_only:
        t = time.perf_counter()
        engine_only(fm, data, a.batch)
        t_eng = time.perf_counter() - t
        t = time.perf_counter()
        rec = D.collect(fm, data, range(len(data)), a.batch)
        t_collect = time.perf_counter() - t
        t = time.perf_counter()
        D.results_from(rec, names)
        t_acc = time.perf_counter() - t
        t = time.perf_counter()
        res_h = host_path(fm, data, a.batch, names)
        t_host = time.perf_counter() - t
        out.update(engine_only_s=round(t_eng, 4), device_collect_s=round(t_collect, 4), accumulate_summarize_s=round(t_acc, 4),
                   host_matcher_s=round(t_host, 4), host_matcher_img_s=round(a.images / t_host, 1), results_equal=res == res_h,
                   evaluator_share_device=round(max(0.0, t_dev - t_eng) / t_dev, 3), evaluator_share_host=round(max(0.0, t_host - t_eng) / t_host, 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
