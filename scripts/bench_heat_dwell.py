#!/usr/bin/env python
"""First measurements of the device dwell times and heat maps (focoos_amd/zones.py DeviceDwell, focoos_amd/heat.py, csrc/dwell_ops.hip,
csrc/heat_ops.hip) in the setting of scripts/bench_zones.py / bench_overlay.py: 32 streams of synthetic moving boxes
(the generator of scripts/bench_track.py), T = 300 slots per stream, the 8 regions of bench_zones (6 of them zones: 6 dwell rows per
stream), a heat map of 1920 x 1080 frames at cell 8, radius 2.
    python scripts/bench_heat_dwell.py [--frames 200] [--warmup 10] [--objects 60] [--draw-reps 50] [--no-stream]
Reports, as one JSON line:
  * DeviceDwell.update, DeviceHeatmap.update (both launches) and DeviceHeatmap.render on 32 frames of 1920 x 1080 per batch by HIP events
    (median / mean / max over the frames of the sequence, the tracker, zone, dwell and heat state evolving as they would on video), and
    whether dwell and heat equal the restatements (tests/dwell_ref.py, tests/heat_ref.py) after the first --host-frames frames;
  * unless --no-stream: FocoosModel.infer_stream images/s for RT-DETR-L at 640 x 640, batch 32, seeded synthetic weights: track + zones
    against the same plus dwell + heatmap, with and without detections=False, and annotate=Overlay(traces=30) against the same plus
    heat=True; the modes alternate twice in one process, so the new cost can be read against the parent mode's own run-to-run spread.
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

from focoos_amd.heat import DeviceHeatmap, Heatmap  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402
from focoos_amd.tracking import DeviceTracker, TrackerConfig  # noqa: E402
from focoos_amd.zones import DeviceDwell, DeviceZones  # noqa: E402
from scripts.bench_track import B, T, sequence  # noqa: E402
from scripts.bench_zones import regions  # noqa: E402
from tests import dwell_ref as DR  # noqa: E402
from tests import heat_ref as HR  # noqa: E402

H, W, CELL, RADIUS = 1080, 1920, 8, 2


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "mean": round(float(ms.mean()), 4), "max": round(float(ms.max()), 4)}


def bench_device(seq, warmup, host_frames, draw_reps, dev):
    trk = DeviceTracker(B, TrackerConfig(), dev)
    zon = DeviceZones(B, regions(), trk)
    dw, hm = DeviceDwell(zon), DeviceHeatmap(B, Heatmap(H, W, cell=CELL, radius=RADIUS), dev)
    d = [[torch.from_numpy(a).to(dev) for a in fr] for fr in seq]

    def step(fr, ev=None):
        ids = trk.update(*fr)
        inside = zon.update(fr[1], fr[2], fr[3], ids)["det_inside"]
        if ev:
            ev[0].record()
        out = dw.update(fr[3], ids, inside)
        if ev:
            ev[1].record()
        hm.update(fr[1], fr[2], fr[3], ids)
        if ev:
            ev[2].record()
        return ids, inside, out

    for fr in d[:warmup]:                        # code object load, allocator
        step(fr)
    trk.reset(), zon.reset(), dw.reset(), hm.reset()
    rdw, rhm = DR.RefDwell([[k for _, k in rows] for rows in dw.rows], trk.config.max_tracks), HR.RefHeat(B, H, W, cell=CELL, radius=RADIUS)
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in d]
    equal = True
    for f, (fr, ev) in enumerate(zip(d, evs)):
        ids, inside, out = step(fr, ev)
        if f < host_frames:                      # the restatements alongside, on the tracker's own ids
            want = rdw.update(seq[f][3], ids.cpu().numpy(), inside.cpu().numpy(), trk.state()["id"])
            rhm.update(seq[f][1], seq[f][2], seq[f][3])
            equal = equal and np.array_equal(out.cpu().numpy(), want) and all(np.array_equal(v, hm.state()[k]) for k, v in rhm.state().items())
    torch.cuda.synchronize()
    dwell_ms, heat_ms = [e[0].elapsed_time(e[1]) for e in evs], [e[1].elapsed_time(e[2]) for e in evs]
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    for _ in range(3):
        hm.render(frames)
    torch.cuda.synchronize()
    dev_evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(draw_reps)]
    for e0, e1 in dev_evs:
        e0.record()
        hm.render(frames)
        e1.record()
    torch.cuda.synchronize()
    st = dw.state()
    return {"dwell_update_ms_per_batch_hip_events": stats(dwell_ms), "heat_update_ms_per_batch_hip_events": stats(heat_ms),
            "heat_render_ms_per_32_frames_1920x1080_hip_events": stats([e0.elapsed_time(e1) for e0, e1 in dev_evs]),
            "dwell_rows_per_stream": int(dw.D // B), "visits": int(st["visits"].sum()), "longest_visit_frames": int(st["dwell_max"].max()),
            "heat_grid": list(hm.config.grid_shape), "heat_max_hits": round(float(hm.state()["heat_max"].max()) / 256, 1),
            "host_frames": host_frames, "equal_to_restatements": bool(equal)}


def bench_stream(frames_n, warmup_n, reps):
    from focoos_amd.annotate import Overlay
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    zs = regions(640)
    new = lambda: dict(dwell=True, heatmap=Heatmap(640, 640, cell=CELL, radius=RADIUS))      # noqa: E731
    modes = (("track_zones", lambda: {}), ("track_zones_dwell_heat", new),
             ("track_zones_no_detections", lambda: dict(detections=False)), ("track_zones_dwell_heat_no_detections", lambda: dict(detections=False, **new())),
             ("overlay_traces30", lambda: dict(annotate=Overlay(traces=30))), ("overlay_traces30_heat", lambda: dict(annotate=Overlay(traces=30, heat=True), **new())))
    out = {}
    for rep in range(reps):                      # the modes alternate in one process
        for key, kw in modes:
            for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, track=True, zones=zs, **kw()):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in fm.infer_stream([batch] * frames_n, threshold=0.3, track=True, zones=zs, **kw()):
                pass
            out.setdefault(key, []).append(round(32 * frames_n / (time.perf_counter() - t0), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--objects", type=int, default=60)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--draw-reps", type=int, default=50)
    ap.add_argument("--stream-batches", type=int, default=30)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heat_dwell needs a GPU (no CPU fallback, no figure without one)")
    seq = sequence(a.frames, a.objects)
    out = {"bench": "heat_dwell", "streams": B, "T": T, "frames": a.frames, "objects_per_stream": a.objects, "regions_per_stream": 8,
           "frame": [H, W], "cell": CELL, "radius": RADIUS}
    out.update(bench_device(seq, a.warmup, min(a.host_frames, a.frames), a.draw_reps, torch.device("cuda:0")))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_img_per_s"] = bench_stream(a.stream_batches, 3, a.stream_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
