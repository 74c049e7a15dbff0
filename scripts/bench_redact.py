#!/usr/bin/env python
"""First measurements of on-device redaction (focoos_amd/annotate.py Redact, csrc/redact.hip) in the setting of
scripts/bench_overlay.py / bench_heat_dwell.py: 32 frames of 1920 x 1080 with 20 detections each, T = 300 slots per stream, a tracker of
256 slots per stream.
    python scripts/bench_redact.py [--reps 200] [--warmup 10] [--stream-batches 30] [--stream-reps 2] [--no-stream] [--only-true]
Reports, as one JSON line:
  * fx_redact_regions and fx_redact_u8 by HIP events (median / mean / max of --reps) for every mode - fill and pixelate (cell 16) in place,
    blur (radius 16) into a second buffer - and whether regions and pixels of the first frame equal the restatement (tests/redact_ref.py);
  * unless --no-stream: FocoosModel.infer_stream images/s for RT-DETR-L at 640 x 640, batch 32, seeded synthetic weights, track=True:
    annotate=True, annotate=Overlay(zones=False), the same with redact=Redact() and with redact=Redact(mode="blur"); the modes alternate
    --stream-reps times in one process, so the new cost can be read against the spread between identical rounds.  --only-true runs the
    annotate=True mode alone (the one figure a tree without this feature can give as well).
Nothing gates on these numbers."""
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

from focoos_amd.synth import synth_image_structured  # noqa: E402

B, T, M, H, W, N = 32, 300, 256, 1080, 1920, 20


def stats(ms):
    ms = np.asarray(ms)
    return {"median": round(float(np.median(ms)), 4), "mean": round(float(ms.mean()), 4), "max": round(float(ms.max()), 4)}


def scene(seed=0):
    """20 boxes per stream between 60 and 360 pixels on a side, two labels."""
    rs = np.random.RandomState(seed)
    labels, boxes, count = np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32), np.full(B, N, np.int32)
    x0, y0 = rs.randint(0, W - 60, (B, N)), rs.randint(0, H - 60, (B, N))
    boxes[:, :N] = np.stack([x0, y0, x0 + rs.randint(60, 360, (B, N)), y0 + rs.randint(60, 360, (B, N))], -1)
    labels[:, :N] = rs.randint(0, 2, (B, N))
    return labels, boxes, count


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


def bench_device(reps, warmup, dev):
    from focoos_amd import _lib
    from focoos_amd.annotate import REDACT_MODES
    from focoos_amd.tracking import DeviceTracker, TrackerConfig
    from tests import redact_ref as RR

    lib = _lib.load("bf16")
    stream = torch.cuda.current_stream(dev).cuda_stream
    labels, boxes, count = scene()
    dl, dbx, dc = (torch.from_numpy(a).to(dev) for a in (labels, boxes, count))
    trk = DeviceTracker(B, TrackerConfig(max_tracks=M), dev)
    trk.update(torch.full((B, T), 0.9, device=dev), dl, dbx, dc)                 # every box becomes a track ...
    trk.update(torch.full((B, T), 0.9, device=dev), dl, dbx, torch.zeros_like(dc))      # ... and is missed in the next frame: 20 coasting slots
    R = T + M
    i32 = dict(dtype=torch.int32, device=dev)
    reg, slot, cnt = torch.zeros(B, R, 4, **i32), torch.zeros(B, R, **i32), torch.zeros(B, **i32)

    def regions(hold):
        rc = lib.fx_redact_regions(dl.data_ptr(), dbx.data_ptr(), dc.data_ptr(), B, T, None, 0, trk.id.data_ptr(), trk.label.data_ptr(), trk.tsu.data_ptr(),
                                   trk.box.data_ptr(), M, hold, 0, 256, reg.data_ptr(), slot.data_ptr(), cnt.data_ptr(), stream)
        assert rc == 0

    out = {"regions_ms_per_batch_hold2_hip_events": timed(lambda: regions(2), reps, warmup)}
    out["regions_per_stream_hold2"] = int(cnt.max())
    regions(0)                                                                   # the pixels below: the 20 detections alone
    torch.cuda.synchronize()
    wreg, wslot, wcnt = RR.regions(labels, boxes, count, None, 0, trk.state(), 0)
    equal = bool(np.array_equal(reg.cpu().numpy(), wreg) and np.array_equal(cnt.cpu().numpy(), wcnt))
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    other = torch.empty_like(frames)
    host0 = frames[:1].cpu().numpy()
    for mode, inplace in (("fill", True), ("pixelate", True), ("pixelate", False), ("blur", False)):
        work = frames.clone() if inplace else frames
        dst = work if inplace else other

        def cover():
            rc = lib.fx_redact_u8(work.data_ptr(), dst.data_ptr(), B, H, W, 0, reg.data_ptr(), slot.data_ptr(), cnt.data_ptr(), R, None, 0, 0, T,
                                  REDACT_MODES[mode], 0, 16, 16, 0x204060, stream)
            assert rc == 0

        if not inplace:                                                          # in place the frame changes with every repetition: timed only
            cover()
            torch.cuda.synchronize()
            want = RR.redact(host0, 0, wreg, wslot, wcnt, REDACT_MODES[mode], RR.BOX, 16, 16, 0x204060)
            equal = equal and bool(np.array_equal(dst[:1].cpu().numpy(), want))
        out[f"{mode}_{'in_place' if inplace else 'out_of_place'}_ms_per_32_frames_1920x1080_hip_events"] = timed(cover, reps, warmup)
    covered = RR.covered(H, W, wreg[0], wslot[0], wcnt[0])
    out.update(covered_share_of_frame_0=round(float(covered.mean()), 3), equal_to_restatement=equal)
    return out


def bench_stream(frames_n, warmup_n, reps, only_true):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fm = ModelManager.get("fai-detr-l-coco", seed=0)
    batch = [synth_image_structured(i, 640, 640) for i in range(32)]
    modes = [("annotate_true", lambda: True)]
    if not only_true:
        from focoos_amd.annotate import Overlay, Redact

        modes += [("overlay", lambda: Overlay(zones=False)), ("overlay_redact_pixelate", lambda: Overlay(zones=False, redact=Redact())),
                  ("overlay_redact_blur", lambda: Overlay(zones=False, redact=Redact(mode="blur")))]
    out = {}
    for rep in range(reps):                      # the modes alternate in one process
        for key, ann in modes:
            for _ in fm.infer_stream([batch] * warmup_n, threshold=0.3, track=True, annotate=ann()):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in fm.infer_stream([batch] * frames_n, threshold=0.3, track=True, annotate=ann()):
                pass
            out.setdefault(key, []).append(round(32 * frames_n / (time.perf_counter() - t0), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stream-batches", type=int, default=30)
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--only-true", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_redact needs a GPU (no CPU fallback, no figure without one)")
    out = {"bench": "redact", "streams": B, "T": T, "max_tracks": M, "frame": [H, W], "detections_per_stream": N, "cell": 16, "radius": 16}
    if not a.only_true:
        out.update(bench_device(a.reps, a.warmup, torch.device("cuda:0")))
    if not a.no_stream:
        out["infer_stream_rtdetr_l_640_bs32_track_img_per_s"] = bench_stream(a.stream_batches, 3, a.stream_reps, a.only_true)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
