"""Tiled RT-DETR inference of one large frame (``FocoosModel.infer_tiled``).

``infer`` squashes the whole picture to the model's input size; on a 4000 x 3000 frame a 20-pixel object shrinks to 3 pixels.  Here the
frame is cut into overlapping windows of the model's size, every window (plus, optionally, the whole frame resized) is one image of an
engine batch, the boxes are moved back into frame coordinates and duplicates across windows are suppressed - all on the device:

  frame (uint8 HWC, uploaded once) -> fx_tile_gather_u8_f32 -> float32 views -> FAIDetr.detect per chunk -> packed results [N][T]
                                   -> fx_merge_detections_nms -> one packed list -> DETRProcessor.pack_detections (the one D2H copy)

The reference has no counterpart (like ``infer_stream``); ``tile_grid`` is pure host code."""
from __future__ import annotations

import math
import os
import warnings
from time import perf_counter
from typing import Optional, Tuple, Union

import numpy as np
import torch

MERGE_METRICS = {"iou": 0, "ios": 1}   # include/focoos_amd.h FX_MERGE_IOU / FX_MERGE_IOS
NMS_CAP = 4096                          # include/focoos_amd.h FX_MERGE_NMS_CAP
MIN_TILE = 32


def _axis_windows(extent: int, t: int, overlap: float):
    if extent <= t:                    # an axis no longer than the tile: one window of the frame's own extent (the gather enlarges it)
        return [(0, extent)]
    stride = max(1, math.floor(t * (1.0 - overlap)))
    origins, o = [], 0
    while o + t < extent:
        origins.append(o)
        o += stride
    if not origins or origins[-1] != extent - t:
        origins.append(extent - t)     # the last window is snapped to the border
    return [(o, t) for o in origins]


def tile_grid(H: int, W: int, th: int, tw: int, overlap: float) -> np.ndarray:
    """The windows of an H x W frame for tiles of (th, tw): int32 [N, 4] rows (x0, y0, w, h), row-major (y outer, x inner).  Per axis the
    stride is max(1, floor(t * (1 - overlap))), origins are 0, stride, 2 stride ... while origin + t < extent, and one last window is
    snapped to extent - t; an axis no longer than the tile gets one window of its own extent.  Windows never leave the frame, their union
    is the frame and neighbours share at least ``overlap`` of a tile."""
    H, W, th, tw = int(H), int(W), int(th), int(tw)
    if H < 1 or W < 1 or th < 1 or tw < 1:
        raise ValueError(f"tile_grid: frame {H} x {W} and tile {th} x {tw} must be positive")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"tile_grid: overlap must be in [0, 1), got {overlap}")
    xs, ys = _axis_windows(W, tw, overlap), _axis_windows(H, th, overlap)
    return np.array([[x0, y0, w, h] for (y0, h) in ys for (x0, w) in xs], dtype=np.int32).reshape(-1, 4)


def check_supported(focoos_model) -> None:
    fam = focoos_model.model.family
    if fam != "fai_detr":
        raise NotImplementedError(f"FocoosModel.infer_tiled: tiled inference is built for the fai_detr family only, not {fam!r} "
                                  "(merging masks or class scores across tiles is a different problem)")


def check_arguments(tile, overlap, merge_threshold, merge_metric, batch_size, max_detections, default_tile) -> Tuple[int, int]:
    """ValueError for anything outside the contract; returns the tile as (h, w)."""
    if tile is None:
        tile = default_tile
    th, tw = (int(tile), int(tile)) if isinstance(tile, (int, np.integer)) else (int(tile[0]), int(tile[1]))
    if th < MIN_TILE or tw < MIN_TILE:
        raise ValueError(f"infer_tiled: tile must be at least {MIN_TILE} pixels a side, got {(th, tw)}")
    if not 0.0 <= float(overlap) < 1.0:
        raise ValueError(f"infer_tiled: overlap must be in [0, 1), got {overlap}")
    if not 0.0 < float(merge_threshold) <= 1.0:
        raise ValueError(f"infer_tiled: merge_threshold must be in (0, 1], got {merge_threshold}")
    if merge_metric not in MERGE_METRICS:
        raise ValueError(f"infer_tiled: merge_metric must be one of {sorted(MERGE_METRICS)}, got {merge_metric!r}")
    if int(max_detections) < 1:
        raise ValueError(f"infer_tiled: max_detections must be at least 1, got {max_detections}")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError(f"infer_tiled: batch_size must be at least 1, got {batch_size}")
    return th, tw


def frame_tensor(image) -> torch.Tensor:
    """One picture (path, PIL image, HWC uint8 ndarray, HWC / CHW uint8 tensor) as a contiguous uint8 [H, W, 3] tensor (where it lives)."""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image

        image = np.array(Image.open(image).convert("RGB"))
    if not isinstance(image, (np.ndarray, torch.Tensor)):
        image = np.array(image)        # PIL image
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if image.dim() != 3:
        raise ValueError("infer_tiled takes one picture: [H, W, 3] or [3, H, W] uint8")
    if image.shape[0] == 3 and image.shape[-1] != 3:   # CHW -> HWC
        image = image.permute(1, 2, 0)
    if image.shape[-1] != 3 or image.dtype != torch.uint8:
        raise ValueError(f"infer_tiled takes a uint8 RGB picture, got {tuple(image.shape)} {image.dtype}")
    return image.contiguous()


def views_of(H: int, W: int, th: int, tw: int, overlap: float, include_full: bool) -> np.ndarray:
    """tile_grid plus, when asked and not already there, the whole frame as one more window."""
    wins = tile_grid(H, W, th, tw, overlap)
    full = np.array([[0, 0, W, H]], dtype=np.int32)
    if include_full and not (wins == full).all(1).any():
        wins = np.concatenate([wins, full], 0)
    return wins


def gather_views(lib, frame: torch.Tensor, wins_host: torch.Tensor, wins_dev: torch.Tensor, out: torch.Tensor) -> None:
    """fx_tile_gather_u8_f32: ``out`` [>= N, Ho, Wo, 3] float32 receives the N views of the device frame [H, W, 3] uint8."""
    from ._lib import check

    N = wins_host.shape[0]
    assert frame.is_cuda and frame.is_contiguous() and out.is_contiguous() and out.shape[0] >= N and wins_host.dtype == torch.int32
    check(lib.fx_tile_gather_u8_f32(frame.data_ptr(), frame.shape[0], frame.shape[1], wins_dev.data_ptr(), wins_host.data_ptr(), N, out.data_ptr(),
                                    out.shape[1], out.shape[2], torch.cuda.current_stream(frame.device).cuda_stream), "fx_tile_gather_u8_f32")


def merge_detections(lib, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor, count: torch.Tensor, wins_dev: torch.Tensor, N: int,
                     frame_hw: Tuple[int, int], merge_threshold: float, merge_metric: str, max_detections: int):
    """fx_merge_detections_nms on the first N views of the packed buffers [>= N][T].  Returns (scores [1, D], labels [1, D], boxes [1, D, 4],
    count_status [2]: the number of detections and the number of candidates dropped by the cap), all on the device."""
    from ._lib import check

    dev, T = scores.device, scores.shape[1]
    D = int(max_detections)
    o_s = torch.empty(1, D, dtype=torch.float32, device=dev)
    o_l = torch.empty(1, D, dtype=torch.int32, device=dev)
    o_b = torch.empty(1, D, 4, dtype=torch.int32, device=dev)
    cs = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.fx_merge_detections_workspace_bytes(N, T)), dtype=torch.uint8, device=dev)
    check(lib.fx_merge_detections_nms(scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), count.data_ptr(), wins_dev.data_ptr(), N, T,
                                      int(frame_hw[0]), int(frame_hw[1]), float(merge_threshold), MERGE_METRICS[merge_metric], D, o_s.data_ptr(),
                                      o_l.data_ptr(), o_b.data_ptr(), cs.data_ptr(), cs.data_ptr() + 4, ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream), "fx_merge_detections_nms")
    return o_s, o_l, o_b, cs


def detect_views(model, views: torch.Tensor, sizes: torch.Tensor, batch_size: int, threshold: float):
    """Run the views [Npad, th, tw, 3] (Npad a multiple of batch_size) through ``model.detect`` chunk by chunk on ONE plan and collect the
    packed results device to device: (det_scores [Npad, T], det_labels, det_boxes [Npad, T, 4], det_count [Npad])."""
    Npad = views.shape[0]
    bufs = None
    for c0 in range(0, Npad, batch_size):
        pl = model.detect(views[c0:c0 + batch_size], sizes=sizes[c0:c0 + batch_size], threshold=threshold)
        if bufs is None:
            T = pl.det_scores.shape[1]
            bufs = (torch.empty(Npad, T, dtype=torch.float32, device=views.device), torch.empty(Npad, T, dtype=torch.int32, device=views.device),
                    torch.empty(Npad, T, 4, dtype=torch.int32, device=views.device), torch.empty(Npad, dtype=torch.int32, device=views.device))
        for dst, src in zip(bufs, (pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)):
            dst[c0:c0 + batch_size].copy_(src, non_blocking=True)
    return bufs


def infer_tiled(fm, image, tile: Union[None, int, Tuple[int, int]] = None, overlap: float = 0.2, threshold: Optional[float] = None,
                merge_threshold: float = 0.5, merge_metric: str = "iou", include_full: bool = True, batch_size: Optional[int] = None,
                max_detections: int = 300, annotate: bool = False):
    """FocoosModel.infer_tiled (see there)."""
    from ._lib import load
    from .ports import InferLatency

    check_supported(fm)
    im = fm.model_info.im_size
    th, tw = check_arguments(tile, overlap, merge_threshold, merge_metric, batch_size, max_detections, im)
    if annotate and int(max_detections) > 1024:
        raise ValueError(f"infer_tiled: annotate=True draws at most 1024 detections, got max_detections={max_detections}")
    t0 = perf_counter()
    frame = frame_tensor(image)
    H, W = int(frame.shape[0]), int(frame.shape[1])
    wins = views_of(H, W, th, tw, float(overlap), include_full)
    N = wins.shape[0]
    bs = min(N, 32) if batch_size is None else int(batch_size)
    Npad = -(-N // bs) * bs
    dev = fm.model.device
    lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
    thr = threshold or fm.processor.threshold
    frame_d = frame.to(dev, non_blocking=True)
    wins_h = torch.from_numpy(wins)
    wins_d = wins_h.to(dev, non_blocking=True)
    sizes_np = np.full((Npad, 2), (th, tw), dtype=np.int32)
    sizes_np[:N] = wins[:, [3, 2]]     # each window's own (h, w): boxes come back in window pixels
    sizes_d = torch.from_numpy(sizes_np).to(dev, non_blocking=True)
    views = torch.empty(Npad, th, tw, 3, dtype=torch.float32, device=dev)
    views[N:].zero_()                  # the padding of the last chunk: zero views whose results are ignored
    gather_views(lib, frame_d, wins_h, wins_d, views)
    t1 = perf_counter()
    scores, labels, boxes, count = detect_views(fm.model, views, sizes_d, bs, thr)
    o_s, o_l, o_b, cs = merge_detections(lib, scores, labels, boxes, count, wins_d, N, (H, W), merge_threshold, merge_metric, max_detections)
    torch.cuda.current_stream(dev).synchronize()
    t2 = perf_counter()
    out = fm.processor.pack_detections(o_s, o_l, o_b, cs[:1], fm.model_info.classes)[0]
    dropped = int(cs[1].item())
    if dropped:
        warnings.warn(f"infer_tiled: {dropped} of {dropped + NMS_CAP} candidates were dropped before suppression (only the {NMS_CAP} best enter "
                      "it): raise the threshold")
    t3 = perf_counter()
    if annotate:       # the frame is resident: draw the merged, frame-pixel detections on it (a caller's own device tensor stays untouched)
        from types import SimpleNamespace

        from .annotate import annotator_of, to_host

        res = SimpleNamespace(det_scores=o_s, det_labels=o_l, det_boxes=o_b, det_count=cs[:1])
        drawn = annotator_of(fm).annotate(frame_d[None], res, 0, out=torch.empty_like(frame_d[None]) if frame.is_cuda else None)
        out.image = to_host(drawn)[0]
    t4 = perf_counter()
    # host wall clock: the gather is enqueued in `preprocess`, the device drains it, the engine and the merge in `inference`
    out.latency = InferLatency(preprocess=round(t1 - t0, 3), inference=round(t2 - t1, 3), postprocess=round(t3 - t2, 3),
                               annotate=round(t4 - t3, 3) if annotate else None)
    return out
