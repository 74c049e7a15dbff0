#!/usr/bin/env python
"""Throughput of FocoosModel.infer_tiled on one synthetic 4000 x 3000 uint8 frame (tile 640, overlap 0.2, the whole frame as one more view),
upload included, next to the host composition of the same work at the same commit: numpy crops -> FocoosModel.infer_batch per chunk ->
origins added and class-aware greedy NMS in numpy.  The two are different code paths (the engine plans are shared); seeded synthetic
weights, so the number of candidates is arbitrary - it is printed, and --threshold moves it.
    python scripts/bench_infer_tiled.py [--model fai-detr-l-coco] [--frames 20] [--warmup 3] [--threshold 0.05] [--no-host]
Per frame: host wall clock around a call that ends in the packed device-to-host copy; the median over the frames is reported.  The per-phase
split (upload, gather, inference, merge) comes from HIP events around the same calls infer_tiled makes, in a loop of its own."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd import _lib, tiled  # noqa: E402
from focoos_amd.model import ModelManager  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402


def host_nms(scores, labels, boxes, thr, max_det):
    """Class-aware greedy IoU NMS in numpy (int64 areas, the decision inter > thr * union in float64), candidates sorted by score."""
    order = np.argsort(-scores, kind="stable")
    scores, labels, b = scores[order], labels[order], boxes[order].astype(np.int64)
    area = np.maximum(b[:, 2] - b[:, 0], 0) * np.maximum(b[:, 3] - b[:, 1], 0)
    removed = np.zeros(len(scores), dtype=bool)
    keep = []
    for i in range(len(scores)):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) == max_det:
            break
        if area[i] <= 0:
            continue
        r = b[i + 1:]
        iw = np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0])
        ih = np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
        union = area[i] + area[i + 1:] - inter
        removed[i + 1:] |= (inter.astype(np.float64) > np.float64(np.float32(thr)) * union) & (labels[i + 1:] == labels[i]) & (area[i + 1:] > 0)
    return scores[keep], labels[keep], b[keep]


def host_path(fm, frame, wins, thr, chunk, merge_thr, max_det):
    """numpy crops -> infer_batch per chunk (its preprocess resizes what is not tile-sized) -> frame coordinates -> numpy NMS."""
    H, W = frame.shape[:2]
    s, l, b = [], [], []
    for c0 in range(0, len(wins), chunk):
        part = wins[c0:c0 + chunk]
        crops = [np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w]) for x0, y0, w, h in part.tolist()]
        for (x0, y0, _, _), res in zip(part.tolist(), fm.infer_batch(crops, threshold=thr)):
            for d in res.detections:
                s.append(d.conf)
                l.append(d.cls_id)
                b.append([min(max(d.bbox[0] + x0, 0), W), min(max(d.bbox[1] + y0, 0), H), min(max(d.bbox[2] + x0, 0), W), min(max(d.bbox[3] + y0, 0), H)])
    if not s:
        return 0, 0
    ks, _, _ = host_nms(np.array(s, np.float32), np.array(l, np.int64), np.array(b, np.int64).reshape(-1, 4), merge_thr, max_det)
    return len(s), len(ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fai-detr-l-coco")
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer_tiled needs a GPU (no CPU fallback, no figure without one)")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get(a.model, seed=0)
    dev = fm.model.device
    frame = synth_image_structured(0, a.height, a.width)
    wins = tiled.views_of(a.height, a.width, a.tile, a.tile, a.overlap, True)
    N, bs = len(wins), min(len(wins), 32)
    kw = dict(tile=a.tile, overlap=a.overlap, threshold=a.threshold)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    res = fm.infer_tiled(frame, **kw)
    med, lo, hi = timed(lambda: fm.infer_tiled(frame, **kw))
    out = {"bench": "infer_tiled", "model": a.model, "frame": [a.height, a.width], "tile": a.tile, "overlap": a.overlap, "views": N, "batch_size": bs,
           "threshold": a.threshold, "frames": a.frames, "detections": len(res.detections), "device_frames_per_s": round(1.0 / med, 2),
           "device_ms_per_frame": {"median": round(med * 1e3, 2), "min": round(lo * 1e3, 2), "max": round(hi * 1e3, 2)}}

    # the per-phase split: HIP events around the calls infer_tiled makes
    lib = _lib.load("bf16")
    Npad = -(-N // bs) * bs
    wins_h = torch.from_numpy(wins)
    sizes_np = np.full((Npad, 2), a.tile, dtype=np.int32)
    sizes_np[:N] = wins[:, [3, 2]]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    phases = []
    cand = 0
    for it in range(a.warmup + a.frames):
        ev[0].record()
        frame_d = torch.from_numpy(frame).to(dev)
        wins_d, sizes_d = wins_h.to(dev), torch.from_numpy(sizes_np).to(dev)
        ev[1].record()
        views = torch.empty(Npad, a.tile, a.tile, 3, dtype=torch.float32, device=dev)
        views[N:].zero_()
        tiled.gather_views(lib, frame_d, wins_h, wins_d, views)
        ev[2].record()
        s, l, b, c = tiled.detect_views(fm.model, views, sizes_d, bs, a.threshold)
        ev[3].record()
        tiled.merge_detections(lib, s, l, b, c, wins_d, N, (a.height, a.width), 0.5, "iou", 300)
        ev[4].record()
        torch.cuda.synchronize()
        cand = int(c[:N].sum())
        if it >= a.warmup:
            phases.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)])
    ph = np.median(np.array(phases), 0)
    out["candidates"] = cand
    out["phase_ms_median"] = {"upload": round(float(ph[0]), 3), "gather": round(float(ph[1]), 3), "inference": round(float(ph[2]), 3),
                              "merge": round(float(ph[3]), 3)}
    out["gather_GB_per_s"] = round(N * a.tile * a.tile * 3 * (4 + 1) / (ph[1] * 1e-3) / 1e9, 1)   # float32 written + at least one byte read per element

    if not a.no_host:
        n_c, n_k = host_path(fm, frame, wins, a.threshold, bs, 0.5, 300)
        hmed, hlo, hhi = timed(lambda: host_path(fm, frame, wins, a.threshold, bs, 0.5, 300))
        out["host_frames_per_s"] = round(1.0 / hmed, 2)
        out["host_ms_per_frame"] = {"median": round(hmed * 1e3, 2), "min": round(hlo * 1e3, 2), "max": round(hhi * 1e3, 2)}
        out["host_candidates"], out["host_detections"] = n_c, n_k
    print(json.dumps(out))


if __name__ == "__main__":
    main()
