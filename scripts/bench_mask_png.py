#!/usr/bin/env python
"""First measurements of mask_format="png_device" (focoos_amd/mask_png.py, csrc/mask_png.hip) on the ellipse scene of
scripts/bench_mask_rle.py: 16 images of 800 x 800, 20 filled ellipses each, Q = 100 slots, tight boxes (masks of random weights are noise).
    python scripts/bench_mask_png.py [--reps 5] [--kernel-reps 50] [--stream-batches 6] [--no-stream]
Reports, as one JSON line:
  * fx_mask_png_encode per batch by HIP events (its two launches together): median, min, max;
  * device-to-host bytes per batch of pack_detections for each format (computed from what each path copies);
  * host wall time of MaskFormerProcessor.pack_detections per batch for "png" (the parent's path, the baseline), "png_device", "rle" and
    "none", alternating in one process after a warm-up round: median, min and max over --reps;
  * the bytes of the two encoders' IDAT payloads over the scene;
  * unless --no-stream: FocoosModel.infer_stream images/s for fai-mf-l-coco-ins at 800 x 800, batch 16, seeded synthetic weights (its masks
    are noise), for "png" and "png_device", and how many slots fell back to the host.
The one relation the feature stands on: "png_device" post-process wall time below "png" in this run (png_device_faster_than_png)."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_mask_rle import B, H, OBJECTS, Q, W, scene, stats  # noqa: E402
from focoos_amd.mask_png import MaskPngEncoder, decode_png  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402

FORMATS = ("png", "png_device", "rle", "none")


def idat_bytes(b64):
    import base64
    import struct

    png, at, n = base64.b64decode(b64), 8, 0
    while at < len(png):
        size, tag = struct.unpack(">I4s", png[at:at + 8])
        n += size if tag == b"IDAT" else 0
        at += 12 + size
    return n


def bench_kernel(res, reps, dev):
    enc = MaskPngEncoder(B, Q, H, W, dev)
    for _ in range(5):
        enc.encode(res)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        enc.encode(res)
        e1.record()
    torch.cuda.synchronize()
    texts = [t for img in enc.fetch() for t in img]
    return stats([e0.elapsed_time(e1) for e0, e1 in ev], 4), enc, {"masks": len(texts), "base64_chars_per_mask_mean": round(float(np.mean([len(t) for t in texts])), 1),
                                                                    "base64_chars_per_mask_max": max(len(t) for t in texts), "fell_back": enc.last_fallback}


def bench_pack(res, reps):
    from focoos_amd.processor import MaskFormerProcessor
    from focoos_amd.registry import ModelRegistry

    proc = MaskFormerProcessor(ModelRegistry.get_model_info("fai-mf-l-coco-ins")["config"])
    names = [str(i) for i in range(80)]
    wall, last = {f: [] for f in FORMATS}, {}
    for rep in range(reps + 1):      # the first round warms up (code objects, pinned buffers, zlib)
        for fmt in FORMATS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = proc.pack_detections(res, names, mask_format=fmt)
            dt = (time.perf_counter() - t0) * 1e3
            assert sum(len(o.detections) for o in out) == B * OBJECTS
            last[fmt] = out
            if rep:
                wall[fmt].append(dt)
    same = all(np.array_equal(decode_png(p.mask), decode_png(d.mask)) for po, do in zip(last["png"], last["png_device"])
               for p, d in zip(po.detections, do.detections))
    payload = {f: sum(idat_bytes(d.mask) for o in last[f] for d in o.detections) for f in ("png", "png_device")}
    small = B * 4 + B * Q * (4 + 4 + 16)      # det_count, scores, labels, boxes
    d2h = {"none": small, "png": small + B * OBJECTS * H * ((W + 31) // 32) * 4, "rle": small - B * 4 + proc._rle_encoder.last_d2h_bytes,
           "png_device": small - B * 4 + proc._png_encoder.last_d2h_bytes}
    return {k: stats(v) for k, v in wall.items()}, d2h, payload, same


def bench_stream(nbatches, reps):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-mf-l-coco-ins", seed=0)
    batch = [synth_image_structured(i, H, W) for i in range(B)]
    out = {"img_per_s": {"png": [], "png_device": []}}
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
    enc = fm.processor._png_encoder
    out["img_per_s"] = {k: stats(v, 1) for k, v in out["img_per_s"].items()}
    out["png_device_masks"], out["png_device_fell_back"], out["png_device_capacity_per_image"] = enc.total_masks, enc.total_fallback, enc.capacity
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_png needs a GPU (no CPU fallback, no figure without one)")
    if a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    dev = torch.device("cuda:0")
    res = scene(dev)
    kern, enc, shape = bench_kernel(res, a.kernel_reps, dev)
    wall, d2h, payload, same = bench_pack(res, a.reps)
    out = {"bench": "mask_png", "scene": f"{B} images {H} x {W}, {OBJECTS} filled ellipses each (semi-axes 30..150), Q = {Q} slots, tight boxes",
           "capacity_per_image": enc.capacity, **shape, "encode_ms_per_batch_hip_events": kern, "d2h_bytes_per_batch": d2h,
           "pack_detections_ms_per_batch": wall, "idat_payload_bytes": payload, "decodes_equal_to_png": bool(same),
           "png_device_faster_than_png": bool(wall["png_device"]["median"] < wall["png"]["median"])}
    if not a.no_stream:
        out["infer_stream_fai_mf_l_800_bs16"] = bench_stream(a.stream_batches, max(3, a.reps - 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
