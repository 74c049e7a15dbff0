#!/usr/bin/env python
"""First measurements of the overlay (focoos_amd/annotate.py Overlay / DeviceTraces, csrc/overlay.hip).
    python scripts/bench_overlay.py [--reps 200] [--warmup 10] [--stream-batches 30] [--stream-reps 2] [--no-stream] [--true-only]
Reports, as one JSON line:
  * on one 1920 x 1080 frame (drawing scale 2) with the 8 regions of scripts/bench_zones.py and 60 tracks of 30 trace points each (60
    boxes moved through the real DeviceTracker and DeviceTraces for 30 frames), by HIP events, median / mean / max over --reps launches:
    the geometry pass (all three flags, in place), fx_annotate_labels_tracked, fx_annotate_zone_records, fx_trace_update, the whole
    annotate_overlay (geometry, records, draw, zone records, zone labels) and, for comparison, the whole annotate() of annotate=True
    (records + draw) on the same frame and detections;
  * unless --no-stream: FocoosModel.infer_stream images/s for RT-DETR-L at 640 x 640, batch 32, seeded synthetic weights, with
    track + zones + annotate=True against annotate=Overlay(traces=30), the two modes alternating --stream-reps times in one process.
--true-only runs the annotate=True mode of the stream alone and imports nothing of the overlay: the same file measures the commit before it.
Nothing gates on these numbers."""
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

from focoos_amd.synth import synth_image_structured  # noqa: E402
from focoos_amd.tracking import DeviceTracker, TrackerConfig  # noqa: E402
from focoos_amd.zones import DeviceZones  # noqa: E402
from scripts.bench_zones import regions  # noqa: E402

H, W, T, TRACKS, POINTS = 1080, 1920, 300, 60, 30


def moving_boxes(frames):
    """``frames`` packed frames of one stream: 60 boxes of 3 labels drifting across the 1920 x 1080 frame, score 0.9."""
    rs = np.random.RandomState(0)
    pos = np.stack([rs.randint(100, W - 400, TRACKS), rs.randint(100, H - 400, TRACKS)], -1)
    size, vel = rs.randint(60, 240, (TRACKS, 2)), rs.randint(-6, 7, (TRACKS, 2))
    out = []
    for f in range(frames):
        s, l, bx = np.zeros((1, T), np.float32), np.zeros((1, T), np.int32), np.zeros((1, T, 4), np.int32)
        p = pos + f * vel
        s[0, :TRACKS], l[0, :TRACKS] = 0.9, np.arange(TRACKS) % 3
        bx[0, :TRACKS] = np.concatenate([p, p + size], -1)
        out.append((s, l, bx, np.array([TRACKS], np.int32)))
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return {"median": round(float(np.median(ms)), 4), "mean": round(float(ms.mean()), 4), "max": round(float(ms.max()), 4)}


def bench_frame(reps, warmup, dev):
    from types import SimpleNamespace

    from focoos_amd.annotate import OVL_FILL, OVL_STROKE, OVL_TRACES, DeviceAnnotator, DeviceTraces, Overlay, OverlayPass, scale_for

    trk = DeviceTracker(1, TrackerConfig(), dev)
    zon, tr = DeviceZones(1, regions(H), trk), DeviceTraces(trk, POINTS)
    for fr in moving_boxes(POINTS):
        d = [torch.from_numpy(a).to(dev) for a in fr]
        ids = trk.update(*d)
        zon.update(d[1], d[2], d[3], ids)
        tr.update(d[1], d[2], d[3], ids)
    res = SimpleNamespace(det_scores=d[0], det_labels=d[1], det_boxes=d[2], det_count=d[3])
    st = tr.state()
    live = int(((st["id"] != 0) & (st["id"] == trk.state()["id"]) & (st["len"] >= 2)).sum())
    ann = DeviceAnnotator([f"class{i}" for i in range(3)], "detection", dev)
    frame = torch.from_numpy(synth_image_structured(0, H, W)[None].copy()).to(dev)
    s = scale_for(H, W)
    ov = OverlayPass(Overlay(traces=tr), ids, zon, tr)
    work = frame.clone()
    out = {"frame": [H, W], "scale": s, "regions": len(zon.regions), "live_traces": live, "trace_points": int(st["len"].max()),
           "detections": TRACKS,
           "geometry_pass_ms": timed(lambda: ann.geometry(work, 0, zon, tr, OVL_FILL | OVL_STROKE | OVL_TRACES), reps, warmup),
           "labels_tracked_ms": timed(lambda: ann.records_tracked(res, ids, 0, 1, H, W, s), reps, warmup),
           "zone_records_ms": timed(lambda: ann.zone_records(zon, H, W, s), reps, warmup),
           "trace_update_ms": timed(lambda: tr.update(d[1], d[2], d[3], ids), reps, warmup),
           "annotate_overlay_ms": timed(lambda: ann.annotate_overlay(work, res, 0, ov), reps, warmup),
           "annotate_true_ms": timed(lambda: ann.annotate(work, res, 0), reps, warmup)}
    drawn = frame.clone()
    ann.geometry(drawn, 0, zon, tr, OVL_FILL | OVL_STROKE | OVL_TRACES)
    out["pixels_touched_by_geometry"] = int((drawn != frame).any(-1).sum())
    return out


def bench_stream(frames_n, warmup_n, reps, true_only):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    modes = [("track_zones_annotate_true", dict(annotate=True))]
    if not true_only:
        from focoos_amd.annotate import Overlay

        modes.append(("track_zones_overlay_traces30", dict(annotate=Overlay(traces=POINTS))))
    out = {}
    for rep in range(reps):                      # the modes alternate in one process
        for key, kw in modes:
            for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, track=True, zones=regions(640), **kw):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in fm.infer_stream([batch] * frames_n, threshold=0.3, track=True, zones=regions(640), **kw):
                pass
            out.setdefault(key, []).append(round(32 * frames_n / (time.perf_counter() - t0), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stream-batches", type=int, default=30)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--true-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlay needs a GPU (no CPU fallback, no figure without one)")
    out = {"bench": "overlay"}
    if not a.true_only:
        out.update(bench_frame(a.reps, a.warmup, torch.device("cuda:0")))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_img_per_s"] = bench_stream(a.stream_batches, 3, a.stream_reps, a.true_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
