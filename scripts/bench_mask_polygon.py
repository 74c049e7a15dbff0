#!/usr/bin/env python
"""First measurements of mask_format="polygon" (focoos_amd/mask_polygon.py, csrc/mask_polygon.hip), on the fixed scene
of scripts/bench_mask_rle.py: 16 images of 800 x 800, 20 filled ellipses each (semi-axes 30..150 pixels, seeded), written into a mask_words
tensor of Q = 100 slots with their tight boxes.
    python scripts/bench_mask_polygon.py [--reps 5] [--kernel-reps 50] [--kernels-only N]
Reports, as one JSON line:
  * fx_mask_polygon_encode per batch by HIP events (its three launches together; --kernels-only N just runs it N times, for a kernel trace
    that splits it into scan / rank / emit);
  * device-to-host bytes per batch of pack_detections for "polygon", "rle" and the host path (computed from what each path copies);
  * host wall time per batch, the three alternating in one process (median, min and max over --reps): pack_detections with "polygon", with
    "rle", and the host path a user had before - the bit planes copied back, unpack_masks and trace_mask_numpy per detection.
One run, no gate: nothing depends on these figures."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mask_rle import B, H, OBJECTS, Q, W, scene, stats  # noqa: E402

from focoos_amd.mask_polygon import MaskPolygonEncoder, trace_mask_numpy  # noqa: E402


def bench_kernel(res, reps, dev):
    enc = MaskPolygonEncoder(B, Q, H, W, dev)
    for _ in range(5):
        enc.encode(res)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        enc.encode(res)
        e1.record()
    torch.cuda.synchronize()
    polys = enc.fetch()
    verts = [sum(len(r) // 2 for r in p) for img in polys for p in img]
    rings = [len(p) for img in polys for p in img]
    return stats([e0.elapsed_time(e1) for e0, e1 in ev], 4), enc, polys, {
        "masks": len(verts), "vertices_per_mask_mean": round(float(np.mean(verts)), 1), "vertices_per_mask_max": int(max(verts)),
        "rings_per_mask_max": int(max(rings)), "fell_back": enc.last_fallback}


def host_path(proc, res):
    """what a user had before: the kept bit planes cross to the host, are unpacked, and every mask is traced there"""
    n = res.det_count.cpu().tolist()
    out = []
    for i, ni in enumerate(n):
        masks = proc.unpack_masks(res.mask_words[i, :ni], H, W)
        out.append([trace_mask_numpy(m) for m in masks])
    return out


def bench_pack(res, reps, polys):
    from focoos_amd.processor import MaskFormerProcessor
    from focoos_amd.registry import ModelRegistry

    proc = MaskFormerProcessor(ModelRegistry.get_model_info("fai-mf-l-coco-ins")["config"])
    names = [str(i) for i in range(80)]
    wall = {"polygon": [], "rle": [], "host": []}
    for rep in range(reps + 1):      # the first round warms up (code objects, pinned buffers)
        for fmt in wall:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if fmt == "host":
                out = host_path(proc, res)
                assert out == polys      # the same rings
            else:
                out = proc.pack_detections(res, names, mask_format=fmt)
                assert sum(len(o.detections) for o in out) == B * OBJECTS
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                wall[fmt].append(dt)
    small = B * Q * (4 + 4 + 16)      # scores, labels, boxes
    d2h = {"host": B * 4 + B * OBJECTS * H * ((W + 31) // 32) * 4, "rle": small + proc._rle_encoder.last_d2h_bytes,
           "polygon": small + proc._polygon_encoder.last_d2h_bytes}
    return {k: stats(v) for k, v in wall.items()}, d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--kernels-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_polygon needs a GPU (no CPU fallback, no figure without one)")
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    dev = torch.device("cuda:0")
    res = scene(dev)
    if a.kernels_only:
        enc = MaskPolygonEncoder(B, Q, H, W, dev)
        for _ in range(a.kernels_only):
            enc.encode(res)
        torch.cuda.synchronize()
        return
    kern, enc, polys, shape = bench_kernel(res, a.kernel_reps, dev)
    wall, d2h = bench_pack(res, a.reps, polys)
    out = {"bench": "mask_polygon", "scene": f"{B} images {H} x {W}, {OBJECTS} filled ellipses each (semi-axes 30..150), Q = {Q} slots, tight boxes",
           "capacity_per_image": enc.capacity, "max_edges_per_image": enc.max_edges, "workspace_bytes": int(enc.workspace.numel()), **shape,
           "encode_ms_per_batch_hip_events": kern, "d2h_bytes_per_batch": d2h, "ms_per_batch": wall}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
