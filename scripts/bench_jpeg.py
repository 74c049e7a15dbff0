#!/usr/bin/env python
"""First measurements of the device JPEG encoder (focoos_amd/jpeg.py, csrc/jpeg.hip): 32 frames of 1920 x 1080,
quality 85, 4:2:0, 32 MCUs per restart interval.
    python scripts/bench_jpeg.py [--reps 30] [--warmup 3] [--stream-batches 6] [--stream-reps 2] [--no-stream]
Reports, as one JSON line:
  * launch A (fx_jpeg_scan_sizes: sizes and scan) and launch B (fx_jpeg_encode) by HIP events (median / mean / max of --reps), whether the
    first file equals the restatement (tests/jpeg_ref.py), the bytes that cross the bus against the raw copy's;
  * the wall time of what stands where ``to_host`` stood: ``annotate.to_host`` (the raw pinned copy, unchanged by this feature: the
    baseline) and ``jpeg.images_to_host`` (both launches, the small copy, the copy of the files), alternating;
  * unless --no-stream: FocoosModel.infer_stream images/s for RT-DETR-L, batches of 32 frames of 1920 x 1080, seeded synthetic weights,
    annotate=True with image_format="array", with "jpeg", and with "array" followed by Pillow's encoder on 16 threads (what a user does
    today); the modes alternate --stream-reps times in one process.
Nothing gates on these numbers."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd.synth import synth_image_structured  # noqa: E402

B, H, W = 32, 1080, 1920


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "mean": round(float(ms.mean()), 4), "max": round(float(ms.max()), 4)}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return stats([e0.elapsed_time(e1) for e0, e1 in evs])


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return stats(ms)


def frames_host():
    four = [synth_image_structured(i, H, W) for i in range(4)]
    return [four[i % 4] for i in range(B)]


def bench_device(reps, warmup, dev):
    from focoos_amd import jpeg as J
    from focoos_amd.annotate import to_host
    from tests import jpeg_ref as R

    enc, jp = J.DeviceJpegEncoder(dev), J.Jpeg()
    host = frames_host()
    frames = torch.from_numpy(np.stack(host)).to(dev)
    files = enc.encode(frames, jp)                       # uploads the header and the tables
    lib, stream = enc.lib, torch.cuda.current_stream(dev).cuda_stream
    n = lib.fx_jpeg_intervals(H, W, 1, jp.mcus)
    tables, header = enc._tables[jp.quality], enc._headers[(H, W, jp)]
    sizes = torch.empty(B * n, dtype=torch.int32, device=dev)
    ioff, foff = torch.empty(B * n, dtype=torch.int64, device=dev), torch.empty(B + 1, dtype=torch.int64, device=dev)
    args = (frames.data_ptr(), B, H, W, 0, B, 1, jp.mcus, tables.data_ptr())

    def launch_a():
        assert lib.fx_jpeg_scan_sizes(*args, header.numel(), sizes.data_ptr(), ioff.data_ptr(), foff.data_ptr(), stream) == 0

    launch_a()
    total = int(foff[-1].item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def launch_b():
        assert lib.fx_jpeg_encode(*args, header.data_ptr(), header.numel(), ioff.data_ptr(), foff.data_ptr(), out.data_ptr(), total, stream) == 0

    res = {"launch_a_sizes_and_scan_ms_hip_events": timed(launch_a, reps, warmup), "launch_b_encode_ms_hip_events": timed(launch_b, reps, warmup),
           "first_file_equals_restatement": files[0] == R.encode(host[0]), "intervals_per_frame": n,
           "bytes_to_host_jpeg": sum(len(f) for f in files) + 8 * (B + 1), "bytes_to_host_raw": B * H * W * 3}
    raw, jpg = [], []
    for _ in range(3):                                    # alternating, after one warm-up each
        to_host(frames), J.images_to_host(frames, (jp, False))
        raw.append(wall(lambda: to_host(frames), max(3, reps // 3))["median"])
        jpg.append(wall(lambda: J.images_to_host(frames, (jp, False)), max(3, reps // 3))["median"])
    res.update(to_host_raw_wall_ms_medians=raw, images_to_host_jpeg_wall_ms_medians=jpg)
    return res


def pillow_encode(results, pool):
    from PIL import Image

    def one(r):
        buf = io.BytesIO()
        Image.fromarray(r.image).save(buf, "JPEG", quality=85, subsampling="4:2:0")
        return buf.getvalue()

    return list(pool.map(one, results))


def bench_stream(batches_n, reps):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = frames_host()
    pool = ThreadPoolExecutor(16)
    modes = [("array", "array", False), ("jpeg", "jpeg", False), ("array_then_pillow_16_threads", "array", True)]
    out = {}
    for rep in range(reps):                              # the modes alternate in one process
        for key, fmt, pil in modes:
            for _ in fm.infer_stream([batch] * 2, threshold=0.3, annotate=True, image_format=fmt):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for res in fm.infer_stream([batch] * batches_n, threshold=0.3, annotate=True, image_format=fmt):
                if pil:
                    pillow_encode(res, pool)
            out.setdefault(key, []).append(round(B * batches_n / (time.perf_counter() - t0), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg needs a GPU (no CPU fallback, no figure without one)")
    out = {"bench": "jpeg", "frames": B, "frame": [H, W], "quality": 85, "subsampling": "420", "restart_mcus": 32}
    out.update(bench_device(a.reps, a.warmup, torch.device("cuda:0")))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_1080p_bs32_annotate_img_per_s"] = bench_stream(a.stream_batches, a.stream_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
