#!/usr/bin/env python
"""Throughput of FocoosModel.infer_stream(classify=...) on 32 synthetic 1920 x 1080 NV12 camera frames that are already on the device
(RT-DETR-L, fai-cls-n-coco on the objects, a tracker, K = 16 crops per stream and frame), next to infer_stream without it and to the only
route the project offered before: infer_stream on the same frames, numpy crops from pre-converted RGB host arrays, classifier.infer_batch in
chunks of 512, and a host join.  Seeded synthetic weights, so how many detections there are is arbitrary - it is printed, and --threshold
moves it; the tracker runs with high = new_thresh = --track-high (0.06), because seeded weights score far below the defaults of track=True
(--track-high 0 gives track=True).
    python scripts/bench_cascade.py [--model fai-detr-l-coco] [--classifier fai-cls-n-coco] [--batches 30] [--warmup 2] [--threshold 0.05]
Frames per second: host wall clock around a whole call that ends in a device synchronise, one run each.  The four device steps are timed by
HIP events around the launches alone: median, minimum and maximum over --events repeats."""
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

from focoos_amd import cascade as CS  # noqa: E402
from focoos_amd.frames import Frame, FrameBatch  # noqa: E402
from focoos_amd.model import ModelManager  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402
from focoos_amd.tracking import DeviceTracker, TrackerConfig  # noqa: E402


def nv12_of(rgb: np.ndarray):
    """A full-range BT.601 forward map, chroma averaged over 2 x 2: test material, nothing depends on it being exact."""
    f = rgb.astype(np.float32)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    u, v = (b - y) * 0.564 + 128.0, (r - y) * 0.713 + 128.0
    H, W = y.shape
    half = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean((1, 3))      # noqa: E731
    uv = np.stack([half(u), half(v)], -1)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fai-detr-l-coco")
    ap.add_argument("--classifier", default="fai-cls-n-coco")
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--max-objects", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--track-high", type=float, default=0.06, help="TrackerConfig.high and new_thresh: seeded weights score low; 0 = track=True")
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cascade needs a GPU (no CPU fallback, no figure without one)")
    if a.height % 2 or a.width % 2:
        raise SystemExit("bench_cascade builds its NV12 frames from even sizes")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get(a.model, seed=0)
        cls = ModelManager.get(a.classifier, seed=4)
    dev = fm.model.device
    S, H, W, K = a.streams, a.height, a.width, a.max_objects
    cascade = CS.Cascade(cls, max_objects=K, pad=0.1, threshold=0.01)
    track = True if a.track_high <= 0 else TrackerConfig(high=a.track_high, low=min(0.05, a.track_high), new_thresh=a.track_high, max_tracks=1024)

    # 4 distinct pictures, cycled over the streams; the planes live on the device as a decoder would leave them
    planes = [nv12_of(synth_image_structured(i, H, W)) for i in range(4)]
    dev_planes = [(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)) for y, uv in planes]

    def frame_batch():
        return FrameBatch([Frame("nv12", list(dev_planes[s % 4]), H, W) for s in range(S)])

    def run(n, classify):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = dets = attrs = 0
        for out in fm.infer_stream((frame_batch() for _ in range(n)), threshold=a.threshold, track=track, classify=classify):
            k += len(out)
            dets += sum(len(o.detections) for o in out)
            attrs += sum(d.attr_id is not None for o in out for d in o.detections)
        torch.cuda.synchronize()
        return k / (time.perf_counter() - t0), dets / max(k, 1), attrs / max(k, 1)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # the tracker-slot and crop-budget warnings of arbitrary weights
        run(a.warmup, None)
        run(a.warmup, cascade)
        fps_plain, per_frame, _ = run(a.batches, None)
        fps_cascade, _, attrs = run(a.batches, cascade)
    out = {"bench": "cascade", "model": a.model, "classifier": a.classifier, "streams": S, "frame": [H, W], "format": "nv12 (device)",
           "max_objects": K, "threshold": a.threshold, "track_high": a.track_high, "frame_batches": a.batches, "detections_per_frame": round(per_frame, 1),
           "attributes_per_frame": round(attrs, 1),
           "stream_frames_per_s": {"track": round(fps_plain, 1), "track_classify": round(fps_cascade, 1)},
           "crop_buffer_bytes": S * K * 224 * 224 * 12}

    # HIP events around each of the four steps: the launches alone, on one detector result
    fb = frame_batch()
    trk = DeviceTracker(S, TrackerConfig() if track is True else track, dev)
    dc = CS.DeviceCascade(cascade, S, trk, dev)
    x, _ = fm.processor.preprocess(fb, device=dev, dtype=fm.model.dtype)
    pl = fm.model.detect(x, sizes=torch.tensor(fb.sizes, dtype=torch.int32), threshold=a.threshold)
    ids = trk.update(pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)
    names = fm.model_info.classes
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def events(fn):
        ts = []
        for it in range(3 + a.events):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                ts.append(e0.elapsed_time(e1))
        return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    ms = {"select": events(lambda: dc.select(pl, fb, ids, names))}
    out["crops_filled"] = int(dc.roi_count.sum().item())
    ms["gather"] = events(lambda: dc.gather(fb))
    ms["classifier_forward"] = events(lambda: dc.forward())
    logits = dc.forward()
    ms["attributes"] = events(lambda: dc.attributes(logits, pl, ids))      # the frame counter advances per repeat: the work is the same
    out["event_ms"] = ms
    out["gather_GB_per_s_written"] = round(out["crops_filled"] * 224 * 224 * 12 / (ms["gather"]["median"] * 1e-3) / 1e9, 1)

    if not a.no_host_route:
        # the route without classify=: detections back on the host, numpy crops from RGB arrays converted once outside the timed window,
        # the public classifier in chunks of 512, the answers joined to the detections by hand
        rgbs = [t.cpu().numpy() for t in frame_batch().rgb_frames(dev)]

        def host_route(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            for res in fm.infer_stream((frame_batch() for _ in range(n)), threshold=a.threshold, track=track):
                crops, where = [], []
                for s, r in enumerate(res):
                    for j, d in enumerate(sorted(r.detections, key=lambda d: -d.conf)[:K]):
                        x0, y0, x1, y1 = d.bbox
                        px, py = (x1 - x0) // 10, (y1 - y0) // 10
                        crop = rgbs[s][max(0, y0 - py):min(H, y1 + py), max(0, x0 - px):min(W, x1 + px)]
                        if crop.shape[0] >= 8 and crop.shape[1] >= 8:
                            crops.append(np.ascontiguousarray(crop)), where.append(d)
                for c0 in range(0, len(crops), 512):
                    chunk = crops[c0:c0 + 512]
                    chunk = chunk + [chunk[-1]] * (512 - len(chunk))      # one batch size, so one classifier plan serves every chunk
                    for d, ans in zip(where[c0:c0 + 512], cls.infer_batch(chunk, threshold=0.01)):
                        if ans.detections:
                            best = max(ans.detections, key=lambda t: t.conf)
                            d.attr_id, d.attr_label, d.attr_conf = best.cls_id, best.label, best.conf
                k += len(res)
            torch.cuda.synchronize()
            return k / (time.perf_counter() - t0)

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host_route(a.warmup)
            out["stream_frames_per_s"]["track_then_host_crops_and_classifier"] = round(host_route(a.batches), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
