#!/usr/bin/env python
"""First measurements of components= (focoos_amd/components.py, csrc/mask_components.hip) on synthetic blob scenes:
32 images of 640 x 640, --blobs discs per image (radius 3..14, seeded) spread over four class masks in a result of Q = 150 slots.
    python scripts/bench_components.py [--reps 20] [--blobs 300] [--stream N] [--tiled]
Reports, as one JSON line:
  * fx_mask_components per batch by HIP events (its six launches together; a kernel trace of this script splits them), against
    label_components and, where it imports, scipy.ndimage.label on 16 threads, both from the bit words copied to the host;
  * --stream N: images/s of infer_stream over N batches of the same pictures drawn as blobs (bisenetformer-l-ade, seeded weights) with and
    without components=True, alternating;
  * --tiled: one segment_tiled 4000 x 3000 frame with and without components=True (frame-sized planes: the workspace path).
One run, no gate: nothing depends on these figures."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from focoos_amd import components as CC  # noqa: E402
from focoos_amd.mask_pool import unpack_words  # noqa: E402

B, Q, H, W, CLASSES = 32, 150, 640, 640, 4


def blobs(seed, n, h=H, w=W):
    """[CLASSES, h, w] bool: n discs, disc i in the mask of class i % CLASSES"""
    rs = np.random.RandomState(seed)
    out = np.zeros((CLASSES, h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.randint(3, 15)
        out[i % CLASSES] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return out


def scene(dev, n):
    words = np.zeros((B, Q, H, (W + 31) // 32), np.int32)
    boxes = np.zeros((B, Q, 4), np.int32)
    for b in range(B):
        m = blobs(b, n)
        words[b, :CLASSES] = np.packbits(m, axis=-1, bitorder="little").view("<i4")
        boxes[b, :CLASSES] = (0, 0, W - 1, H - 1)
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return SimpleNamespace(mask_words=t(words), det_count=torch.full((B,), CLASSES, dtype=torch.int32, device=dev), det_boxes=t(boxes),
                           det_scores=torch.rand(B, Q, device=dev), det_labels=t(np.tile(np.arange(Q, dtype=np.int32), (B, 1))), mask_width=W), words


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--stream", type=int, default=0)
    ap.add_argument("--tiled", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_components needs a GPU (no CPU fallback, no figure without one)")
    dev = torch.device("cuda:0")
    res, words = scene(dev, a.blobs)
    dc = CC.DeviceComponents(B, Q, H, W, dev, CC.Components(max_components=512))
    for _ in range(3):
        o = dc.split(res)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for e0, e1 in ev:
        e0.record()
        dc.split(res)
        e1.record()
    torch.cuda.synchronize()
    out = {"bench": "components", "scene": f"{B} images {H} x {W}, {a.blobs} discs each over {CLASSES} class masks, Q = {Q}, M = 512",
           "components_per_image_mean": round(float(o.det_count.float().mean()), 1), "fell_back": dc.last_fallback, "dropped": dc.last_dropped,
           "run_capacity": dc.run_capacity, "workspace_bytes": int(dc.workspace.numel()),
           "split_ms_per_batch_hip_events_with_status_copy": med([e0.elapsed_time(e1) for e0, e1 in ev])}

    def host(label):      # what a user does today: the planes cross to the host, are unpacked and labelled there
        t0 = time.perf_counter()
        w = res.mask_words[:, :CLASSES].cpu().numpy()
        with ThreadPoolExecutor(16) as ex:
            n = sum(ex.map(lambda p: int(label(unpack_words(p, W))), w.reshape(-1, H, w.shape[-1])))
        return (time.perf_counter() - t0) * 1e3, n

    ms, n = host(lambda m: CC.label_components(m, 8).max())
    out["host_label_components_ms_per_batch"], out["components"] = round(ms, 1), n
    try:
        from scipy import ndimage

        times = [host(lambda m: ndimage.label(m, structure=np.ones((3, 3)))[1]) for _ in range(3)]
        assert times[0][1] == n
        out["host_scipy_16_threads_ms_per_batch"] = med([t for t, _ in times])
    except ImportError:
        out["host_scipy_16_threads_ms_per_batch"] = None
    if a.stream or a.tiled:
        from focoos_amd.model import ModelManager

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fm = ModelManager.get("bisenetformer-l-ade", device=str(dev), seed=3)
    if a.stream:
        imgs = [np.repeat((blobs(b, a.blobs).any(0) * 255).astype(np.uint8)[..., None], 3, -1) for b in range(B)]
        rates = {"plain": [], "components": []}
        fm.processor.components_run_capacity = 1 << 21      # seeded weights give ragged masks: keep them off the host fallback
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for rep in range(3):
                for k in rates:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in fm.infer_stream(iter([imgs] * a.stream), mask_format="rle", components=True if k == "components" else None):
                        pass
                    if rep:
                        rates[k].append(B * a.stream / (time.perf_counter() - t0))
        out["infer_stream_images_per_s"] = {k: med(v) for k, v in rates.items()}
    if a.tiled:
        frame = np.repeat((blobs(99, 2000, 3000, 4000).any(0) * 255).astype(np.uint8)[..., None], 3, -1)
        wall = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for k in ("plain", "components", "plain", "components"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fm.segment_tiled(frame, mask_format="rle", components=CC.Components(min_area=16, max_components=128) if k == "components" else None)
                wall[k] = (round((time.perf_counter() - t0) * 1e3, 1), len(r.detections))
        out["segment_tiled_4000x3000_ms_and_detections"] = wall
    print(json.dumps(out))


if __name__ == "__main__":
    main()
