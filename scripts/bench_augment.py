#!/usr/bin/env python
"""Throughput of the device augmenter (focoos_amd/augment.py) on 64 synthetic ADE-sized uint8 images -> 640^2 with the default detection and
semantic augmentations, upload included, next to the same parameter records applied on the host with PIL + numpy on 16 threads.  The default
detection preset carries square=1.0, which the augmenter refuses: it is benchmarked with square reset to 0.0 (stated in the output).
    python scripts/bench_augment.py [--n 64] [--iters 20] [--host-threads 16]
Kernel times come from a run of its own:  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_augment.py --iters 5 --no-host
The compulsory bytes of a batch (printed) are every source byte inside a window read once plus every output byte written once."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd import augment as A  # noqa: E402
from focoos_amd.ports import Boxes, DatasetEntry, Instances, SemanticSegmentationDatasetEntry  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402

ORIG = [(512, 683), (512, 768), (683, 512), (512, 512), (384, 512), (512, 640), (640, 512), (427, 640)]   # ADE20K-like original sizes


def entries(n, task):
    rs = np.random.RandomState(0)
    out = []
    for i in range(n):
        h, w = ORIG[i % len(ORIG)]
        img = synth_image_structured(i, h, w)
        if task == "detection":
            t = 8
            x0, y0 = rs.uniform(0, 0.6, t) * w, rs.uniform(0, 0.6, t) * h
            xyxy = np.stack([x0, y0, x0 + rs.uniform(0.1, 0.4, t) * w, y0 + rs.uniform(0.1, 0.4, t) * h], -1).astype(np.float32)
            out.append(DatasetEntry(image=img, height=h, width=w, instances=Instances((h, w), boxes=Boxes(torch.from_numpy(xyxy)),
                                                                                      classes=torch.from_numpy(rs.randint(0, 80, t)))))
        else:
            lab = rs.randint(0, 150, (h // 64 + 1, w // 64 + 1)).repeat(64, 0).repeat(64, 1)[:h, :w].astype(np.uint8)
            out.append(SemanticSegmentationDatasetEntry(image=img, height=h, width=w, sem_seg=lab))
    return out


def host_apply(img, rec):
    """The same record with PIL + numpy, the reference's order: flip, resize (BILINEAR), crop, colour blends, pad."""
    from PIL import Image

    if rec.hflip:
        img = img[:, ::-1]
    if rec.vflip:
        img = img[::-1]
    im = np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((rec.res_w, rec.res_h), Image.BILINEAR))
    im = im[rec.crop_y:rec.crop_y + rec.crop_h, rec.crop_x:rec.crop_x + rec.crop_w].astype(np.float32)
    if rec.order:
        mean = float(img.mean())
        im = im * rec.brightness
        ops = [lambda v: mean * (1 - rec.contrast) + rec.contrast * v,
               lambda v: (v @ np.array([0.299, 0.587, 0.114], np.float32))[..., None] * (1 - rec.saturation) + rec.saturation * v]
        for f in (ops if rec.order == 1 else ops[::-1]):
            im = f(im)
    out = np.zeros((rec.out_h, rec.out_w, 3), np.uint8)
    out[rec.pad_y:rec.pad_y + rec.crop_h, rec.pad_x:rec.pad_x + rec.crop_w] = np.clip(np.floor(im + 0.5), 0, 255).astype(np.uint8)
    return out


def compulsory_bytes(recs):
    src = sum(min(r.src_w, r.crop_w * r.sx) * min(r.src_h, r.crop_h * r.sy) * 3 for r in recs)
    return src + sum(r.out_h * r.out_w * 3 for r in recs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment.py measures on the GPU"
    dev = torch.device("cuda", 0)
    for task in ("detection", "semseg"):
        augs, _ = A.get_default_by_task(task, 640)
        note = ""
        if augs.square:
            augs.square, note = 0.0, " (square reset to 0.0: refused field)"
        data = entries(a.n, task)
        aug = A.DeviceAugmenter(augs, task, dev)
        gen = torch.Generator()
        gen.manual_seed(0)
        for _ in range(3):
            aug(data, gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nbytes = 0
        for _ in range(a.iters):
            aug(data, gen)
            nbytes += compulsory_bytes(aug.last_records)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        line = {"bench": "augment", "task": task, "augmentations": f"get_default_by_task({task}, 640){note}", "images": a.n, "iters": a.iters,
                "device_img_per_s": round(a.n * a.iters / dt, 1), "ms_per_batch": round(dt / a.iters * 1e3, 3),
                "compulsory_MB_per_batch": round(nbytes / a.iters / 1e6, 2)}
        if not a.no_host:
            recs = aug.last_records
            srcs = [A._hwc_u8(e.image) for e in data]
            with ThreadPoolExecutor(a.host_threads) as ex:
                list(ex.map(host_apply, srcs, recs))
                t0 = time.perf_counter()
                for _ in range(3):
                    list(ex.map(host_apply, srcs, recs))
                line["host_pil_img_per_s"] = round(3 * a.n / (time.perf_counter() - t0), 1)
                line["host_threads"] = a.host_threads
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
