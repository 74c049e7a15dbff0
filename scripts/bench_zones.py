#!/usr/bin/env python
"""First measurements of the device zone / line counter (focoos_amd/zones.py, csrc/zone_ops.hip): 32 streams of synthetic
moving boxes (the generator of scripts/bench_track.py), T = 300 slots per stream, 8 regions per stream (6 zones of 4..12 vertices and 2 lines).
    python scripts/bench_zones.py [--frames 200] [--warmup 10] [--objects 60] [--host-frames 5] [--no-host] [--no-stream]
Reports, as one JSON line:
  * DeviceZones.update per batch of 32 streams by HIP events (median / mean / max over the frames of the sequence, tracker and zone state
    evolving as they would on video), and update + fetch() by the host wall clock (what infer_stream adds per batch);
  * the restatement (tests/zones_ref.py) on the host for the first --host-frames frames, per batch, and whether its outputs equal the
    device's - it is the only host counter this project has and is not tuned code;
  * unless --no-stream: FocoosModel.infer_stream images/s for RT-DETR-L at 640 x 640, batch 32, seeded synthetic weights, the three modes
    track=True / track=True, zones=... / track=True, zones=..., detections=False alternating in one process.
Nothing gates on these numbers."""
from __future__ import annotations

import argparse
import json
import math
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
from focoos_amd.zones import DeviceZones, Line, Zone  # noqa: E402
from scripts.bench_track import B, FRAME, T, sequence  # noqa: E402
from tests import zones_ref as R  # noqa: E402


def regions(frame=FRAME):
    """8 regions shared by every stream: 6 zones of 4, 5, 6, 8, 10 and 12 vertices (regular polygons of different sizes spread over the
    frame, two of them with a class filter) and 2 lines (a vertical and a diagonal one)."""
    out = []
    for i, n in enumerate((4, 5, 6, 8, 10, 12)):
        cx, cy, rad = frame * (0.25 + 0.25 * (i % 3)), frame * (0.3 + 0.4 * (i // 3)), frame * (0.12 + 0.03 * i)
        poly = [(int(cx + rad * math.cos(2 * math.pi * k / n)), int(cy + rad * math.sin(2 * math.pi * k / n))) for k in range(n)]
        out.append(Zone(f"zone{n}", poly, classes=[0, 1, 2, 3] if i % 3 == 2 else None, anchor="bottom_center" if i % 2 else "center"))
    out.append(Line("gate", (frame // 2, 0), (frame // 2, frame), anchor="center"))
    out.append(Line("diag", (0, 0), (frame, frame)))
    return out


def bench_device(seq, warmup, dev):
    trk = DeviceTracker(B, TrackerConfig(), dev)
    zon = DeviceZones(B, regions(), trk)
    d = [[torch.from_numpy(a).to(dev) for a in fr] for fr in seq]
    for fr in d[:warmup]:                        # code object load, allocator
        zon.update(fr[1], fr[2], fr[3], trk.update(*fr))
    trk.reset(), zon.reset()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in d]
    outs, tracked = [], []
    for fr, (e0, e1) in zip(d, ev):
        ids = trk.update(*fr)
        e0.record()
        out = zon.update(fr[1], fr[2], fr[3], ids)
        e1.record()
        outs.append({k: out[k].clone() for k in ("now", "det_inside", "det_in", "det_out")})
        tracked.append((ids, trk.id.clone()))
    torch.cuda.synchronize()
    kern = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    totals = zon.state()
    trk.reset(), zon.reset()
    torch.cuda.synchronize()
    wall = []
    for fr in d:                                 # what a serving loop pays per batch: launch + one copy + the dicts
        ids = trk.update(*fr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zon.update(fr[1], fr[2], fr[3], ids)
        zon.fetch()
        wall.append(time.perf_counter() - t0)
    return outs, tracked, kern, np.array(wall) * 1e3, totals, int(zon._io.numel() * 4)


def bench_host(seq, tracked, nframes, max_tracks):
    ref, outs = R.RefZones(B, regions(), max_tracks), []
    ids = [(i.cpu().numpy(), t.cpu().numpy()) for i, t in tracked[:nframes]]
    t0 = time.perf_counter()
    for fr, (i, t) in zip(seq[:nframes], ids):
        outs.append(ref.update(fr[1], fr[2], fr[3], i, t))
    return outs, (time.perf_counter() - t0) / max(nframes, 1) * 1e3


def bench_stream(frames_n, warmup_n, reps):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    zs = regions(640)
    modes = (("track", dict(track=True)), ("track_zones", dict(track=True, zones=zs)),
             ("track_zones_no_detections", dict(track=True, zones=zs, detections=False)))
    out = {}
    for rep in range(reps):                      # the three modes alternate in one process
        for key, kw in modes:
            for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, **kw):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inside = 0
            for res in fm.infer_stream([batch] * frames_n, threshold=0.3, **kw):
                if "zones" in kw:
                    inside += sum(z["count"] for r in res for z in r.zones.values())
            out.setdefault(key, []).append(round(32 * frames_n / (time.perf_counter() - t0), 1))
            if "zones" in kw:
                out["zone_memberships_per_image"] = round(inside / (32 * frames_n), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--objects", type=int, default=60)
    ap.add_argument("--host-frames", type=int, default=5)
    ap.add_argument("--stream-batches", type=int, default=30)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_zones needs a GPU (no CPU fallback, no figure without one)")
    dev = torch.device("cuda:0")
    seq = sequence(a.frames, a.objects)
    outs, tracked, kern, wall, totals, nbytes = bench_device(seq, a.warmup, dev)
    out = {"bench": "zones", "streams": B, "T": T, "frames": a.frames, "objects_per_stream": a.objects, "regions_per_stream": 8,
           "detections_per_stream": round(float(np.mean([fr[3].mean() for fr in seq])), 1),
           "inside_per_stream_and_frame": round(float(np.mean([int(o["now"].sum()) for o in outs])) / B, 1),
           "events_in": int(totals["in_total"].sum()), "events_out": int(totals["out_total"].sum()), "copy_back_bytes_per_batch": nbytes,
           "update_ms_per_batch_hip_events": {"median": round(float(np.median(kern)), 4), "mean": round(float(kern.mean()), 4),
                                              "max": round(float(kern.max()), 4)},
           "update_plus_fetch_ms_per_batch": {"median": round(float(np.median(wall)), 4), "mean": round(float(wall.mean()), 4)}}
    if not a.no_host:
        n = min(a.host_frames, a.frames)
        houts, ms = bench_host(seq, tracked, n, TrackerConfig().max_tracks)
        out["host_restatement_ms_per_batch"] = round(ms, 1)
        out["host_frames"] = n
        out["equal_to_host"] = bool(all(np.array_equal(h[k].astype(np.int64) & 0xFFFFFFFF, g[k].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
                                        for h, g in zip(houts, outs) for k in h))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_img_per_s"] = bench_stream(a.stream_batches, 3, a.stream_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
