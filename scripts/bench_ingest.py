#!/usr/bin/env python
"""First measurements of the video frame ingest (focoos_amd/frames.py, csrc/frame_ops.hip): one batch = 32 synthetic
1920 x 1080 camera frames -> the 640 x 640 float32 engine input.
    python scripts/bench_ingest.py [--reps 20] [--warmup 3] [--stream-batches 20] [--stream-reps 2] [--no-stream]
Three paths alternate in one process, after warm-up:
  (a) rgb_host     host RGB arrays through processor.preprocess: 32 pageable uploads and 32 launches of fx_resize_bilinear_u8
  (b) nv12_host    host NV12 frames through FrameBatch: one packed upload and one launch of fx_frames_ingest
  (c) nv12_device  device-resident NV12 surfaces with a 2048-byte pitch through FrameBatch: one descriptor upload and one launch
Per path: HIP events around the device work of the call, and the host wall clock around the whole call ending in a synchronise; reported as
median / min / max over the alternations, and (b), (c) against (a) of the same run.  Unless --no-stream: FocoosModel.infer_stream(track=True,
zones=..., detections=False) images/s for RT-DETR-L, batch 32, seeded synthetic weights, on (a) against (c).  One JSON line; nothing gates
on these numbers."""
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

from focoos_amd.frames import Frame, FrameBatch  # noqa: E402
from focoos_amd.processor import DETRProcessor  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402
from tests import frames_ref as R  # noqa: E402

B, H, W, PITCH, SIZE = 32, 1080, 1920, 2048, 640


def material(dev):
    """32 frames from 4 synthetic pictures (rolled, so no two frames are equal): RGB arrays by the restatement, NV12 host buffers, NV12
    device surfaces at PITCH."""
    ch = (H + 1) // 2
    base = []
    for i in range(4):
        y, u, v = R.rgb_to_yuv_planes(synth_image_structured(i, H, W), i)
        uv = np.ascontiguousarray(np.stack([u, v], -1))
        base.append((y, uv, R.to_rgb("nv12", [y, uv], H, W)))
    rgbs, host, device = [], [], []
    for b in range(B):
        s = 40 * (b // 4)                        # an even shift: luma by s, the chroma pairs by s / 2, the RGB picture by s
        y, uv = np.roll(base[b % 4][0], s, axis=1), np.ascontiguousarray(np.roll(base[b % 4][1], s // 2, axis=1))
        rgbs.append(np.ascontiguousarray(np.roll(base[b % 4][2], s, axis=1)))
        host.append(np.concatenate([y.reshape(-1), uv.reshape(-1)]))
        surf = np.zeros((H + ch, PITCH), np.uint8)
        surf[:H, :W], surf[H:, :W] = y, uv.reshape(ch, W)
        device.append(torch.from_numpy(surf.reshape(-1)).to(dev))
    return rgbs, host, device


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def bench_preprocess(rgbs, host, device, dev, reps, warmup):
    proc = DETRProcessor({}, SIZE)
    paths = {
        "rgb_host": lambda: proc.preprocess(rgbs, dev)[0],
        "nv12_host": lambda: proc.preprocess(FrameBatch([Frame.from_nv12(h, H, W) for h in host]), dev)[0],
        "nv12_device": lambda: proc.preprocess(FrameBatch([Frame.from_nv12(d, H, W, PITCH) for d in device]), dev)[0],
    }
    outs = {k: f().cpu() for k, f in paths.items()}
    equal = bool(torch.equal(outs["rgb_host"], outs["nv12_host"]) and torch.equal(outs["rgb_host"], outs["nv12_device"]))
    del outs
    for _ in range(warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    ev_ms, wall_ms = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(reps):                        # the three paths alternate
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            wall_ms[k].append((time.perf_counter() - t0) * 1e3)
            ev_ms[k].append(e0.elapsed_time(e1))
    out = {"equal_outputs": equal}
    for k in paths:
        out[k] = {"hip_events_ms": stats(ev_ms[k]), "wall_ms": stats(wall_ms[k])}
    for k in ("nv12_host", "nv12_device"):
        out[k]["wall_speedup_over_rgb_host"] = stats(np.array(wall_ms["rgb_host"]) / np.array(wall_ms[k]))
    return out


def bench_stream(rgbs, device, batches, reps):
    from focoos_amd.model import ModelManager
    from scripts.bench_zones import regions

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    zs = regions(H)
    feeds = {"rgb_host": lambda n: (rgbs for _ in range(n)),
             "nv12_device": lambda n: (FrameBatch([Frame.from_nv12(d, H, W, PITCH) for d in device]) for _ in range(n))}
    out, counts = {}, {}
    for rep in range(reps):                      # the two feeds alternate in one process
        for key, feed in feeds.items():
            for _ in fm.infer_stream(feed(3), threshold=0.3, track=True, zones=zs, detections=False):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inside = 0
            for res in fm.infer_stream(feed(batches), threshold=0.3, track=True, zones=zs, detections=False):
                inside += sum(z["count"] for r in res for z in r.zones.values())
            out.setdefault(key, []).append(round(B * batches / (time.perf_counter() - t0), 1))
            counts[key] = inside
    out["equal_zone_counts"] = counts["rgb_host"] == counts["nv12_device"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-batches", type=int, default=20)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest needs a GPU (no CPU fallback, no figure without one)")
    dev = torch.device("cuda:0")
    rgbs, host, device = material(dev)
    out = {"bench": "ingest", "frames": B, "frame": [H, W], "target": [SIZE, SIZE], "device_pitch": PITCH, "reps": a.reps,
           # derived from byte counts, not measured: what crosses PCIe per batch, and what the kernel reads (Y + UV once) and writes
           "derived_bytes": {"rgb_host_upload": B * H * W * 3, "nv12_host_upload": B * (H * W + ((H + 1) // 2) * W),
                             "kernel_in": B * (H * W + ((H + 1) // 2) * W), "kernel_out": B * SIZE * SIZE * 3 * 4}}
    out["preprocess"] = bench_preprocess(rgbs, host, device, dev, a.reps, a.warmup)
    if not a.no_stream:
        out["infer_stream_rtdetr_l_bs32_track_zones_no_detections_img_per_s"] = bench_stream(rgbs, device, a.stream_batches, a.stream_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
