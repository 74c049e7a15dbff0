#!/usr/bin/env python
"""First measurements of the device tracker (focoos_amd/tracking.py, csrc/track_ops.hip): 32 streams of synthetic moving
boxes, T = 300 slots per stream.
    python scripts/bench_track.py [--frames 200] [--warmup 10] [--objects 60] [--host-frames 20] [--no-host] [--no-stream]
Reports, as one JSON line:
  * DeviceTracker.update per batch of 32 streams by HIP events (median / mean / max over the frames of the sequence, the state evolving as it
    would on video), and the same with the ids copied to the host (host wall clock, which is what infer_stream adds per batch);
  * the numpy restatement (tests/tracking_ref.py) on the host for the first --host-frames frames, per batch, and whether its ids equal the
    device's - it is the only host tracker this project has and is not tuned code;
  * unless --no-stream: FocoosModel.infer_stream images/s with and without track=True for RT-DETR-L at 640 x 640, batch 32, seeded synthetic
    weights.
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
from tests import tracking_ref as R  # noqa: E402

B, T, FRAME = 32, 300, 1080


def sequence(frames, objects, seed=0):
    """[frames] x (scores [B, T], labels, boxes, count): per stream ``objects`` boxes of 40..200 pixels drifting by up to 6 pixels a frame inside
    a 1080 x 1080 picture, 8 classes, a persistent confidence per object plus per-frame noise (so detections move between the high and the
    low class), 5 % missed per frame, sorted by score as the engine packs them."""
    rs = np.random.RandomState(seed)
    pos = rs.uniform(0, FRAME - 200, (B, objects, 2))
    size = rs.randint(40, 200, (B, objects, 2))
    vel = rs.uniform(-6, 6, (B, objects, 2))
    lab = rs.randint(0, 8, (B, objects)).astype(np.int32)
    conf = rs.uniform(0.2, 0.95, (B, objects))
    out = []
    for f in range(frames):
        p = np.clip(pos + f * vel, 0, FRAME - 1)
        s = np.clip(conf + rs.normal(0, 0.15, (B, objects)), 0.01, 0.99).astype(np.float32)
        s[rs.rand(B, objects) < 0.05] = 0.0
        order = np.argsort(-s, axis=1, kind="stable")
        sc, lb, bx = np.zeros((B, T), np.float32), np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
        box = np.concatenate([p, np.minimum(p + size, FRAME)], -1).astype(np.int32)
        n = min(objects, T)
        sc[:, :n] = np.take_along_axis(s, order, 1)[:, :n]
        lb[:, :n] = np.take_along_axis(lab, order, 1)[:, :n]
        bx[:, :n] = np.take_along_axis(box, order[:, :, None], 1)[:, :n]
        out.append((sc, lb, bx, (sc > 0.05).sum(1).astype(np.int32)))
    return out


def bench_device(seq, warmup, dev):
    trk = DeviceTracker(B, TrackerConfig(), dev)
    d = [[torch.from_numpy(a).to(dev) for a in fr] for fr in seq]
    for fr in d[:warmup]:                        # code object load, allocator
        trk.update(*fr)
    trk.reset()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in d]
    ids = []
    for fr, (e0, e1) in zip(d, ev):
        e0.record()
        ids.append(trk.update(*fr))
        e1.record()
    torch.cuda.synchronize()
    kern = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    live = int((trk.state()["id"] != 0).sum())
    trk.reset()
    torch.cuda.synchronize()
    wall = []
    for fr in d:                                 # what a serving loop pays per batch: launch + the ids on the host
        t0 = time.perf_counter()
        trk.update(*fr).cpu()
        wall.append(time.perf_counter() - t0)
    return [i.cpu().numpy() for i in ids], kern, np.array(wall) * 1e3, live, trk.status()


def bench_host(seq, nframes):
    ref, ids = R.RefTracker(B, TrackerConfig()), []
    t0 = time.perf_counter()
    for fr in seq[:nframes]:
        ids.append(ref.update(*fr))
    return ids, (time.perf_counter() - t0) / max(nframes, 1) * 1e3


def bench_stream(frames_n, warmup_n):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    out = {}
    for rep in range(2):                         # plain, tracked, plain, tracked: the two alternate in one process
        for key, track in (("plain", None), ("track", True)):
            for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, track=track):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dets = tracked = 0
            for res in fm.infer_stream([batch] * frames_n, threshold=0.3, track=track):
                dets += sum(len(r.detections) for r in res)
                tracked += sum(d.track_id is not None for r in res for d in r.detections)
            out.setdefault(key, []).append(round(32 * frames_n / (time.perf_counter() - t0), 1))
            out["detections_per_image"] = round(dets / (32 * frames_n), 1)
            if track:
                out["tracked_per_image"] = round(tracked / (32 * frames_n), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--objects", type=int, default=60)
    ap.add_argument("--host-frames", type=int, default=20)
    ap.add_argument("--stream-batches", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track needs a GPU (no CPU fallback, no figure without one)")
    dev = torch.device("cuda:0")
    seq = sequence(a.frames, a.objects)
    ids, kern, wall, live, status = bench_device(seq, a.warmup, dev)
    out = {"bench": "track", "streams": B, "T": T, "frames": a.frames, "objects_per_stream": a.objects,
           "detections_per_stream": round(float(np.mean([fr[3].mean() for fr in seq])), 1), "live_tracks_at_end": live,
           "dropped_births": int(status.sum()),
           "update_ms_per_batch_hip_events": {"median": round(float(np.median(kern)), 4), "mean": round(float(kern.mean()), 4),
                                              "max": round(float(kern.max()), 4)},
           "update_plus_ids_to_host_ms_per_batch": {"median": round(float(np.median(wall)), 4), "mean": round(float(wall.mean()), 4)}}
    if not a.no_host:
        hids, ms = bench_host(seq, min(a.host_frames, a.frames))
        out["host_numpy_ms_per_batch"] = round(ms, 2)
        out["host_frames"] = len(hids)
        out["equal_to_host"] = bool(all(np.array_equal(h, g) for h, g in zip(hids, ids)))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_img_per_s"] = bench_stream(a.stream_batches, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
