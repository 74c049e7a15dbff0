#!/usr/bin/env python
"""First measurements of mask_format="rle" (focoos_amd/mask_rle.py, csrc/mask_rle.hip).  Masks of random weights are
noise, so the post-process is measured on a fixed synthetic scene: 16 images of 800 x 800, 20 filled ellipses each (semi-axes 30..150
pixels, seeded), written into a mask_words tensor of Q = 100 slots with their tight boxes.
    python scripts/bench_mask_rle.py [--reps 5] [--kernel-reps 50] [--stream-batches 6] [--no-stream] [--kernels-only N]
Reports, as one JSON line:
  * fx_mask_rle_encode per batch by HIP events (its three launches together; --kernels-only N just runs it N times, for a kernel trace that
    splits it into count / scan / emit);
  * device-to-host bytes per batch of pack_detections for "rle" and "png" (computed from what each path copies);
  * host wall time of MaskFormerProcessor.pack_detections per batch for "png" (the parent's path, the baseline), "rle" and "none", the three
    alternating in one process: median, min and max over --reps;
  * unless --no-stream: FocoosModel.infer_stream images/s for fai-mf-l-coco-ins at 800 x 800, batch 16, seeded synthetic weights (its masks
    are noise), for the three formats, and how many slots fell back to the host.
The one relation the feature stands on: "rle" post-process wall time below "png" in this run (rle_faster_than_png)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd.mask_rle import MaskRleEncoder  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402

B, Q, H, W, OBJECTS = 16, 100, 800, 800, 20


def scene(dev, seed=0):
    """The packed device results of the ellipse scene, as the engine would leave them."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    W32 = (W + 31) // 32
    words = np.zeros((B, Q, H, W32), np.int32)
    boxes, area = np.zeros((B, Q, 4), np.int32), np.zeros((B, Q), np.int32)
    for b in range(B):
        for j in range(OBJECTS):
            a, c = rs.uniform(30, 150, 2)
            cx, cy = rs.uniform(a, W - a), rs.uniform(c, H - c)
            m = ((xx - cx) / a) ** 2 + ((yy - cy) / c) ** 2 <= 1.0
            words[b, j] = np.packbits(np.pad(m, ((0, 0), (0, W32 * 32 - W))), axis=-1, bitorder="little").view(np.int32)
            ys, xs = np.nonzero(m)
            boxes[b, j], area[b, j] = (xs.min(), ys.min(), xs.max(), ys.max()), m.sum()
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    scores = np.tile(np.linspace(0.95, 0.3, Q, dtype=np.float32), (B, 1))
    return SimpleNamespace(mask_words=t(words), mask_width=W, det_count=t(np.full(B, OBJECTS, np.int32)), det_boxes=t(boxes), det_area=t(area),
                           det_scores=t(scores), det_labels=t((np.arange(B * Q, dtype=np.int32) % 80).reshape(B, Q)),
                           det_query=t(np.tile(np.arange(Q, dtype=np.int32), (B, 1))))


def stats(v, nd=3):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd), "n": int(v.size)}


def bench_kernel(res, reps, dev):
    enc = MaskRleEncoder(B, Q, H, W, dev)
    for _ in range(5):
        enc.encode(res)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        enc.encode(res)
        e1.record()
    torch.cuda.synchronize()
    rles = enc.fetch()
    counts = [len(r["counts"]) for img in rles for r in img]
    return stats([e0.elapsed_time(e1) for e0, e1 in ev], 4), enc, {"masks": len(counts), "counts_per_mask_mean": round(float(np.mean(counts)), 1),
                                                                    "counts_per_mask_max": int(max(counts)), "fell_back": enc.last_fallback}


def bench_pack(res, reps):
    from focoos_amd.processor import MaskFormerProcessor
    from focoos_amd.registry import ModelRegistry

    proc = MaskFormerProcessor(ModelRegistry.get_model_info("fai-mf-l-coco-ins")["config"])
    names = [str(i) for i in range(80)]
    wall = {"png": [], "rle": [], "none": []}
    for rep in range(reps + 1):      # the first round warms up (code objects, pinned buffer, zlib)
        for fmt in wall:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = proc.pack_detections(res, names, mask_format=fmt)
            dt = (time.perf_counter() - t0) * 1e3
            assert sum(len(o.detections) for o in out) == B * OBJECTS
            if rep:
                wall[fmt].append(dt)
    small = B * 4 + B * Q * (4 + 4 + 16)      # det_count, scores, labels, boxes
    d2h = {"none": small, "png": small + B * OBJECTS * H * ((W + 31) // 32) * 4,
           "rle": small - B * 4 + proc._rle_encoder.last_d2h_bytes}
    return {k: stats(v) for k, v in wall.items()}, d2h


def bench_stream(nbatches, reps):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-mf-l-coco-ins", seed=0)
    batch = [synth_image_structured(i, H, W) for i in range(B)]
    out = {"img_per_s": {"png": [], "rle": [], "none": []}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # the fallback is counted below instead
        for rep in range(reps + 1):      # formats alternate in one process; the first round warms up
            for fmt in out["img_per_s"]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dets, n = 0, nbatches if rep else min(2, nbatches)
                for r in fm.infer_stream([batch] * n, mask_format=fmt):
                    dets += sum(len(x.detections) for x in r)
                dt = time.perf_counter() - t0
                if rep:
                    out["img_per_s"][fmt].append(B * n / dt)
                out["detections_per_image"] = round(dets / (B * n), 1)
                print(f"stream round {rep} {fmt}: {B * n / dt:.1f} img/s", file=sys.stderr, flush=True)
    enc = fm.processor._rle_encoder
    out["img_per_s"] = {k: stats(v, 1) for k, v in out["img_per_s"].items()}
    out["rle_masks"], out["rle_fell_back"], out["rle_capacity_per_image"] = enc.total_masks, enc.total_fallback, enc.capacity
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--kernels-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_rle needs a GPU (no CPU fallback, no figure without one)")
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    dev = torch.device("cuda:0")
    res = scene(dev)
    if a.kernels_only:
        enc = MaskRleEncoder(B, Q, H, W, dev)
        for _ in range(a.kernels_only):
            enc.encode(res)
        torch.cuda.synchronize()
        return
    kern, enc, shape = bench_kernel(res, a.kernel_reps, dev)
    wall, d2h = bench_pack(res, a.reps)
    out = {"bench": "mask_rle", "scene": f"{B} images {H} x {W}, {OBJECTS} filled ellipses each (semi-axes 30..150), Q = {Q} slots, tight boxes",
           "capacity_per_image": enc.capacity, **shape, "encode_ms_per_batch_hip_events": kern, "d2h_bytes_per_batch": d2h,
           "pack_detections_ms_per_batch": wall, "rle_faster_than_png": bool(wall["rle"]["median"] < wall["png"]["median"])}
    if not a.no_stream:
        out["infer_stream_fai_mf_l_800_bs16"] = bench_stream(a.stream_batches, max(3, a.reps - 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
