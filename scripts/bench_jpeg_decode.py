#!/usr/bin/env python
"""First measurements of the device JPEG decoder (focoos_amd/jpeg.py, csrc/jpeg_decode.hip): 32 synthetic files of
1920 x 1080, quality 85, 4:2:0, written by Pillow (no restart markers) and by the project's own encoder (DRI 32).
    python scripts/bench_jpeg_decode.py [--reps 20] [--warmup 3] [--stream-batches 6] [--stream-reps 2] [--no-stream]
Reports, as one JSON line and per kind of file:
  * fx_jpeg_decode (its six launches together) by HIP events on staged files, median / mean / max of --reps; the split per kernel comes from
    ``rocprofv3 --kernel-trace --stats -- python scripts/bench_jpeg_decode.py --no-stream`` in a run of its own (kernels jd_*);
  * the wall time of ``FrameBatch.from_jpeg`` (host parse, packing, the one upload, the launches, the status copy) against Pillow decoding
    the same files on 16 threads, alternating; the bytes uploaded against the raw RGB upload's;
  * unless --no-stream: FocoosModel.infer_stream(track=True, zones=..., detections=False) images/s for RT-DETR-L, batches of 32 files, seeded synthetic
    weights, fed by ``from_jpeg`` against Pillow on 16 threads into ``Frame.from_rgb``; the feeds alternate --stream-reps times in one process.
Nothing gates on these numbers."""
from __future__ import annotations

import argparse
import ctypes
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


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return stats(ms)


def make_files(dev):
    from PIL import Image

    from focoos_amd import jpeg as J

    four = [synth_image_structured(i, H, W) for i in range(4)]
    pil = []
    for im in four:
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, "JPEG", quality=85, subsampling="4:2:0")
        pil.append(buf.getvalue())
    own = J.DeviceJpegEncoder(dev).encode(torch.from_numpy(np.stack(four)).to(dev), J.Jpeg())
    return {"pillow_no_dri": [pil[i % 4] for i in range(B)], "own_encoder_dri32": [own[i % 4] for i in range(B)]}


def pillow_decode(files, pool):
    from PIL import Image

    return list(pool.map(lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), files))


def bench_device(files, reps, warmup, dev, pool):
    from focoos_amd import jpeg as J
    from focoos_amd.frames import FrameBatch

    dec = J.decoder_for(dev)
    real = dec.lib.fx_jpeg_decode
    calls = []
    dec.lib.fx_jpeg_decode = lambda *a: calls.append(a) or real(*a)      # the arguments of one staged call, to replay under events
    fb = FrameBatch.from_jpeg(files, dev)
    dec.lib.fx_jpeg_decode = real
    args = calls[0]
    for _ in range(warmup):
        real(*args)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record()
        assert real(*args) == 0
        e1.record()
    torch.cuda.synchronize()
    res = {"fx_jpeg_decode_ms_hip_events": stats([e0.elapsed_time(e1) for e0, e1 in evs]), "bytes_uploaded": int(args[4]),
           "bytes_raw_rgb_upload": B * H * W * 3, "frames": len(fb)}
    dev_ms, pil_ms = [], []
    for _ in range(3):                                    # alternating
        dev_ms.append(wall(lambda: FrameBatch.from_jpeg(files, dev), max(3, reps // 4))["median"])
        pil_ms.append(wall(lambda: pillow_decode(files, pool), max(3, reps // 4))["median"])
    res.update(from_jpeg_wall_ms_medians=dev_ms, pillow_16_threads_decode_wall_ms_medians=pil_ms)
    return res


def bench_stream(files, batches_n, reps, dev, pool):
    from focoos_amd.frames import Frame, FrameBatch
    from focoos_amd.model import ModelManager
    from scripts.bench_zones import regions

    zs = regions(H)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    feeds = {"from_jpeg": lambda n: (FrameBatch.from_jpeg(files, dev) for _ in range(n)),
             "pillow_16_threads_from_rgb": lambda n: (FrameBatch([Frame.from_rgb(a) for a in pillow_decode(files, pool)]) for _ in range(n))}
    out = {}
    for rep in range(reps):                               # the feeds alternate in one process
        for key, feed in feeds.items():
            for _ in fm.infer_stream(feed(2), threshold=0.3, track=True, zones=zs, detections=False):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in fm.infer_stream(feed(batches_n), threshold=0.3, track=True, zones=zs, detections=False):
                pass
            out.setdefault(key, []).append(round(B * batches_n / (time.perf_counter() - t0), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-batches", type=int, default=6)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode needs a GPU (no CPU fallback, no figure without one)")
    dev, pool = torch.device("cuda:0"), ThreadPoolExecutor(16)
    out = {"bench": "jpeg_decode", "files": B, "frame": [H, W], "quality": 85, "subsampling": "420"}
    kinds = make_files(dev)
    for kind, files in kinds.items():
        out[kind] = dict(file_bytes=sum(len(f) for f in files), **bench_device(files, a.reps, a.warmup, dev, pool))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_1080p_bs32_track_img_per_s"] = {k: bench_stream(f, a.stream_batches, a.stream_reps, dev, pool) for k, f in kinds.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
