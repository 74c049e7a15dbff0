#!/usr/bin/env python
"""Throughput of FocoosModel.infer_stream(tiling=...) on 32 synthetic 1920 x 1080 NV12 camera frames that are already on the device (tile 640,
overlap 0.2, the whole frame as one more view: 9 views per frame, 288 per frame batch, 9 engine chunks of 32), next to the only route without
it: a loop of FocoosModel.infer_tiled over the same frames converted to RGB arrays (the conversion itself is not timed).  Seeded synthetic
weights, so the number of candidates is arbitrary - it is printed, and --threshold moves it.
    python scripts/bench_tiled_stream.py [--model fai-detr-l-coco] [--batches 30] [--warmup 2] [--threshold 0.05] [--no-loop]
Frames per second: host wall clock around a whole call that ends in a device synchronise, one run each; the analytics-only figure
(detections=False, track, one zone) and the figure with the detection objects built.  The gather and the merge are timed by HIP events
around the launches alone, median over --events repeats; the merge comparison is 32 launches of the single-frame merge on the same packed
results."""
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
from focoos_amd.frames import Frame, FrameBatch  # noqa: E402
from focoos_amd.model import ModelManager  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402
from focoos_amd.zones import Zone  # noqa: E402


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
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled_stream needs a GPU (no CPU fallback, no figure without one)")
    if a.height % 2 or a.width % 2:
        raise SystemExit("bench_tiled_stream builds its NV12 frames from even sizes")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get(a.model, seed=0)
    dev = fm.model.device
    S, H, W = a.streams, a.height, a.width
    tiling = tiled.Tiling(tile=a.tile, overlap=a.overlap)
    wins = tiled.views_of(H, W, a.tile, a.tile, a.overlap, True)
    V = len(wins)
    bs, chunks = tiled.view_chunks(S, V, None)

    # 4 distinct pictures, cycled over the streams; the planes live on the device as a decoder would leave them
    planes = [nv12_of(synth_image_structured(i, H, W)) for i in range(4)]
    dev_planes = [(torch.from_numpy(y).to(dev), torch.from_numpy(uv).to(dev)) for y, uv in planes]

    def frame_batch():
        return FrameBatch([Frame("nv12", list(dev_planes[s % 4]), H, W) for s in range(S)])

    zone = Zone("centre", [(W // 4, H // 4), (3 * W // 4, H // 4), (3 * W // 4, 3 * H // 4), (W // 4, 3 * H // 4)])

    def run(n, detections):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = dets = 0
        for out in fm.infer_stream((frame_batch() for _ in range(n)), threshold=a.threshold, tiling=tiling, track=True, zones=[zone],
                                   detections=detections):
            k += len(out)
            dets += sum(len(o.detections) for o in out)
        torch.cuda.synchronize()
        return k / (time.perf_counter() - t0), dets / max(k, 1)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # the suppression-cap and tracker-slot warnings of arbitrary weights
        run(a.warmup, True)
        run(a.warmup, False)
        fps_analytics, _ = run(a.batches, False)
        fps_dets, per_frame = run(a.batches, True)
    out = {"bench": "tiled_stream", "model": a.model, "streams": S, "frame": [H, W], "format": "nv12 (device)", "tile": a.tile, "overlap": a.overlap,
           "views_per_frame": V, "views_per_batch": S * V, "batch_size": bs, "chunks": len(chunks), "threshold": a.threshold,
           "frame_batches": a.batches, "detections_per_frame": round(per_frame, 1),
           "stream_frames_per_s": {"analytics_only_track_zone": round(fps_analytics, 1), "with_detections_track_zone": round(fps_dets, 1)},
           "view_buffer_bytes": {"float32": S * V * a.tile * a.tile * 12, "uint8_follow_up": S * V * a.tile * a.tile * 3}}

    # HIP events around the gather and around the merge: the launches alone
    lib = _lib.load("bf16")
    fb = frame_batch()
    fb._descriptors(dev)
    wh = torch.from_numpy(wins)
    wd = wh.to(dev)
    Npad = len(chunks) * bs
    views = torch.zeros(Npad, a.tile, a.tile, 3, dtype=torch.float32, device=dev)
    sizes = torch.from_numpy(tiled.view_sizes(wins, S, Npad, a.tile, a.tile)).to(dev)
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
        return round(float(np.median(ts)), 3)

    gather_ms = events(lambda: tiled.gather_stream_views(lib, fb, dev, wh, wd, views))
    s, l, b, c = tiled.detect_views(fm.model, views, sizes, bs, a.threshold)
    torch.cuda.synchronize()
    status = torch.zeros(S, dtype=torch.int32, device=dev)
    T = s.shape[1]
    ws = torch.empty(int(lib.fx_merge_detections_batched_workspace_bytes(S, V, T)), dtype=torch.uint8, device=dev)
    merge_ms = events(lambda: tiled.merge_batched(lib, s, l, b, c, wd, S, V, (H, W), tiling, status, ws))

    def single_merges():
        for st in range(S):
            sl = slice(st * V, (st + 1) * V)
            tiled.merge_detections(lib, s[sl], l[sl], b[sl], c[sl], wd, V, (H, W), tiling.merge_threshold, tiling.merge_metric, tiling.max_detections)

    single_ms = events(single_merges)
    out["candidates_per_batch"] = int(c[:S * V].sum())
    out["event_ms_median"] = {"gather_all_views": gather_ms, "merge_batched": merge_ms, f"merge_{S}_single_frame_calls": single_ms}
    # float32 written, one byte of luma and half a byte of chroma read per source pixel at least (taps overlap in cache)
    out["gather_GB_per_s_written"] = round(S * V * a.tile * a.tile * 12 / (gather_ms * 1e-3) / 1e9, 1)

    if not a.no_loop:
        # the route without tiling=: one infer_tiled call per frame, on RGB arrays (converted once, outside the timed window)
        rgbs = [t.cpu().numpy() for t in frame_batch().rgb_frames(dev)]
        kw = dict(tile=a.tile, overlap=a.overlap, threshold=a.threshold)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for r in rgbs[:3]:
                fm.infer_tiled(r, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(len(fm.infer_tiled(r, **kw).detections) for r in rgbs)
            torch.cuda.synchronize()
            out["infer_tiled_loop_frames_per_s"] = round(len(rgbs) / (time.perf_counter() - t0), 1)
            out["infer_tiled_loop_detections_per_frame"] = round(n / len(rgbs), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
