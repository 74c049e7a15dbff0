#!/usr/bin/env python
"""Throughput of the device annotator (focoos_amd/annotate.py, csrc/annotate.hip) on a synthetic 1920 x 1080 uint8 frame, next to the numpy
restatement of the same drawing (tests/annotate_ref.py) on 16 threads of the same host.  Two workloads: 50 boxes + labels, and the same frame
with 20 instance masks (boxes + masks + labels).
    python scripts/bench_annotate.py [--frames 50] [--warmup 5] [--host-frames 16] [--no-host] [--no-stream]
Device: frames/s of upload + records + draw + pinned copy back (host wall clock per frame, median) and the draw kernel alone by HIP events.
Host: 16 frames drawn by 16 threads, frames/s of the pool (numpy releases the GIL in its array loops; the restatement is not tuned code, it
is the only host implementation this project has - supervision / cv2 are not dependencies).  Unless --no-stream, also
FocoosModel.infer_stream images/s with and without annotate=True for RT-DETR-L at 640 x 640, batch 32, seeded synthetic weights."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd import annotate as A  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402
from tests import annotate_ref as R  # noqa: E402

H, W = 1080, 1920
CLASSES = ["person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light"]


def workload(n, with_masks, seed):
    """n detections on the H x W frame: boxes of 60..500 pixels a side, an ellipse mask in each box when asked."""
    rs = np.random.RandomState(seed)
    x0, y0 = rs.randint(0, W - 80, n), rs.randint(0, H - 80, n)
    x1, y1 = np.minimum(x0 + rs.randint(60, 500, n), W - 1), np.minimum(y0 + rs.randint(60, 500, n), H - 1)
    boxes = np.stack([x0, y0, x1, y1], -1).astype(np.int32)[None]
    scores = np.sort(rs.rand(1, n).astype(np.float32))[:, ::-1].copy()
    labels = rs.randint(0, len(CLASSES), (1, n)).astype(np.int32)
    masks = area = None
    if with_masks:
        masks = np.zeros((1, n, H, W), bool)
        ys, xs = np.mgrid[0:H, 0:W]
        for j in range(n):
            cx, cy, rx, ry = (x0[j] + x1[j]) / 2, (y0[j] + y1[j]) / 2, (x1[j] - x0[j]) / 2 + 0.5, (y1[j] - y0[j]) / 2 + 0.5
            masks[0, j] = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0
        area = masks.sum((2, 3)).astype(np.int32)
    return SimpleNamespace(scores=scores, labels=labels, boxes=boxes, count=np.array([n], np.int32), masks=masks, area=area, n=n)


def device_results(w, dev):
    res = SimpleNamespace(det_scores=torch.from_numpy(w.scores).to(dev), det_labels=torch.from_numpy(w.labels).to(dev),
                          det_boxes=torch.from_numpy(w.boxes).to(dev), det_count=torch.from_numpy(w.count).to(dev))
    if w.masks is not None:
        res.mask_words = torch.from_numpy(R.pack_words(w.masks, (W + 31) // 32)).to(dev)
        res.det_area = torch.from_numpy(w.area).to(dev)
    return res


def bench_device(ann, frame, res, frames, warmup):
    dev = ann.device
    pinned = torch.from_numpy(frame[None]).pin_memory()

    def one():
        return A.to_host(ann.annotate(pinned.to(dev, non_blocking=True), res))

    ts, kern = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = one()
        if it >= warmup:
            ts.append(time.perf_counter() - t0)
    fr = torch.from_numpy(frame[None]).to(dev)
    out = torch.empty_like(fr)
    rec = ann.records(res, 0, 1, H, W, A.scale_for(H, W))
    for it in range(warmup + frames):           # the draw kernel alone (separate destination: every byte read and written)
        e0.record()
        ann.draw(fr, res, rec, out=out)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            kern.append(e0.elapsed_time(e1))
    return img[0], float(np.median(ts)), float(np.median(kern))


def bench_host(frame, w, flags, nframes, threads):
    atlas, gw, gh = A.glyph_atlas()
    s = A.scale_for(H, W)
    tab, ln = R.name_table(CLASSES)

    def one(_):
        rec = R.records(w.scores, w.labels, w.boxes, w.count, tab, ln, len(CLASSES), H, W, s, gw, gh)
        return R.draw(frame[None], w.count, w.labels, w.boxes, flags, s, area=w.area, masks=w.masks, rec=rec, atlas=atlas, gw=gw, gh=gh)[0]

    ref = one(0)
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        list(pool.map(one, range(nframes)))
        dt = time.perf_counter() - t0
    return ref, nframes / dt


def bench_stream(frames_n, warmup_n):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    out = {}
    for key, ann in (("plain", False), ("annotate", True)):
        for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, annotate=ann):
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dets = 0
        for res in fm.infer_stream([batch] * frames_n, threshold=0.3, annotate=ann):
            dets += sum(len(r.detections) for r in res)
        out[key] = round(32 * frames_n / (time.perf_counter() - t0), 1)
        out["detections_per_image"] = round(dets / (32 * frames_n), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_annotate needs a GPU (no CPU fallback, no figure without one)")
    dev = torch.device("cuda:0")
    frame = synth_image_structured(0, H, W)
    out = {"bench": "annotate", "frame": [H, W], "scale": A.scale_for(H, W), "frames": a.frames}
    for key, task, n, with_masks in (("boxes50_labels", "detection", 50, False), ("masks20_boxes_labels", "instseg", 20, True)):
        w = workload(n, with_masks, 7)
        ann = A.DeviceAnnotator(CLASSES, task, dev)
        img, t_frame, t_kernel = bench_device(ann, frame, device_results(w, dev), a.frames, a.warmup)
        r = {"detections": n, "device_frames_per_s": round(1.0 / t_frame, 1), "device_ms_per_frame": round(t_frame * 1e3, 3),
             "draw_kernel_ms": round(t_kernel, 4), "draw_kernel_GB_per_s": round(2 * H * W * 3 / (t_kernel * 1e-3) / 1e9, 1)}
        if not a.no_host:
            ref, fps = bench_host(frame, w, ann.flags, a.host_frames, a.threads)
            r["host_numpy_frames_per_s"] = round(fps, 2)
            r["host_threads"] = a.threads
            r["equal_to_host"] = bool(np.array_equal(ref, img))
        out[key] = r
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_img_per_s"] = bench_stream(max(4, a.frames // 5), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
