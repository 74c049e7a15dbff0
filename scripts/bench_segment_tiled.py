#!/usr/bin/env python
"""Wall time of FocoosModel.segment_tiled on one synthetic 4000 x 3000 uint8 frame (tile 640, overlap 0.2; seeded synthetic
bisenetformer-l-ade weights), upload and the packed copy back included, and the gather, inference and merge launches by HIP events around
the same calls segment_tiled makes.  --host also times the host composition of the same work at the same commit: numpy crops ->
``model.forward`` per chunk (the plan with ``full_masks``, the [B, Q, H, W] tensor copied to the host; ``infer_batch`` hands out no full
masks) -> the merge of the definition in numpy float32, class by class (one [Hf, Wf] accumulator at a time; a view keeps one 640 x 640 map per
class it holds).  ``host_label_agreement`` is the share of pixels where its label map equals segment_tiled's.
    python scripts/bench_segment_tiled.py [--model bisenetformer-l-ade] [--frames 10] [--warmup 2] [--host] [--host-frames 2]
Not a leg of bench.py; first measurements, nothing gates on them (profiles/segment_tiled_bench.txt)."""
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

from focoos_amd import _lib, tiled, tiled_seg  # noqa: E402
from focoos_amd.model import ModelManager  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402


def host_path(fm, frame, wins, chunk, K):
    """numpy crops -> full-resolution masks per chunk on the host -> per view and class the best score x probability -> summed per class over
    the covering views -> per-pixel argmax.  Returns the label map."""
    Hf, Wf = frame.shape[:2]
    per_view = []                     # per view: {class: S(n, c) [wh, ww] float32}
    for c0 in range(0, len(wins), chunk):
        part = wins[c0:c0 + chunk].tolist()
        crops = np.stack([frame[y0:y0 + h, x0:x0 + w] for x0, y0, w, h in part])
        out = fm.model(torch.from_numpy(crops).to(fm.model.device))
        masks, (score, label) = out.masks.cpu().numpy(), (t.cpu().numpy() for t in out.logits.max(-1))
        for i in range(len(part)):
            P = masks[i] * score[i][:, None, None]
            per_view.append({int(c): P[label[i] == c].max(0) for c in np.unique(label[i])})
    best, lab = np.zeros((Hf, Wf), np.float32), np.zeros((Hf, Wf), np.uint8)
    for c in range(K):
        A = np.zeros((Hf, Wf), np.float32)
        for (x0, y0, w, h), S in zip(wins.tolist(), per_view):
            if c in S:
                A[y0:y0 + h, x0:x0 + w] += S[c]
        upd = A > best
        best[upd], lab[upd] = A[upd], c
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bisenetformer-l-ade")
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-frames", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_tiled needs a GPU (no CPU fallback, no figure without one)")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get(a.model, seed=0)
    dev, K = fm.model.device, fm.model.num_classes
    frame = synth_image_structured(0, a.height, a.width)
    wins = tiled.tile_grid(a.height, a.width, a.tile, a.tile, a.overlap)
    N, bs = len(wins), min(len(wins), a.batch_size)
    kw = dict(tile=a.tile, overlap=a.overlap, threshold=0.0, batch_size=bs, mask_format="none", return_label_map=True)

    def timed(fn, warmup, runs):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"median": round(float(np.median(ts)) * 1e3, 2), "min": round(min(ts) * 1e3, 2), "max": round(max(ts) * 1e3, 2), "runs": runs}

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, res_map = fm.segment_tiled(frame, **kw)
        out = {"bench": "segment_tiled", "model": a.model, "frame": [a.height, a.width], "tile": a.tile, "overlap": a.overlap, "views": N,
               "batch_size": bs, "classes_kept": len(res.detections), "wall_ms": timed(lambda: fm.segment_tiled(frame, **kw), a.warmup, a.frames)}

    lib = _lib.load("bf16")
    Npad = -(-N // bs) * bs
    wins_h = torch.from_numpy(wins)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    phases = []
    for it in range(a.warmup + a.frames):
        ev[0].record()
        frame_d, wins_d = torch.from_numpy(frame).to(dev), wins_h.to(dev)
        ev[1].record()
        views = torch.empty(Npad, a.tile, a.tile, 3, dtype=torch.float32, device=dev)
        views[N:].zero_()
        tiled.gather_views(lib, frame_d, wins_h, wins_d, views)
        ev[2].record()
        probs, score, label = tiled_seg.segment_views(fm.model, views, bs)
        ev[3].record()
        tiled_seg.merge_views(lib, probs, score, label, wins_h, wins_d, (a.height, a.width), K, 0.0, K)
        ev[4].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            phases.append([ev[i].elapsed_time(ev[i + 1]) for i in range(4)])
    ph = np.median(np.array(phases), 0)
    out["phase_ms_median"] = dict(zip(("upload", "gather", "inference", "merge_with_allocations"), (round(float(v), 3) for v in ph)))
    if a.host:
        lab = host_path(fm, frame, wins, bs, K)
        out["host_wall_ms"] = timed(lambda: host_path(fm, frame, wins, bs, K), 0, a.host_frames)
        out["host_label_agreement"] = round(float((lab == res_map).mean()), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
