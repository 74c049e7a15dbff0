"""Tiled semantic segmentation of one large frame (``FocoosModel.segment_tiled``).

The segmentation families run at the picture's own size, so a 4000 x 3000 frame is one huge plan at batch 1.  Here the frame is cut into
the overlapping windows of ``tiled.tile_grid``, every window is one image of an engine batch, and the views' low-resolution query maps are
merged per class into one frame-sized label map and one packed mask per class - all on the device:

  frame (uint8 HWC, uploaded once) -> fx_tile_gather_u8_f32 -> float32 views -> BisenetFormer.detect per chunk -> mask_probs / cls_score /
  cls_label [Npad] -> fx_seg_merge_views -> label map + packed result [1][max_classes] -> pack_detections or a mask encoder (the D2H copy)

Queries mean different things in different views, so the merge goes through classes (the definition is in include/focoos_amd.h).  The
packed result has the layout of ``fx_seg_postprocess``: the RLE, polygon, PNG, annotate and redact paths read it unchanged.

Memory: a mask plane takes ``Hf * ceil(Wf / 32) * 4`` bytes and ``max_classes`` (default ``num_classes``) planes are allocated - 225 MB for
a 4000 x 3000 frame and the 150 ADE classes; classes beyond ``max_classes`` (ascending class id) are dropped with a warning."""
from __future__ import annotations

import warnings
from time import perf_counter
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .tiled import MIN_TILE, frame_tensor, gather_views, tile_grid

MAX_CLASSES = 255      # include/focoos_amd.h: K and max_classes of fx_seg_merge_views (labels are bytes, 255 slots)
MAX_OVERLAP = 0.5      # FX_SEG_MERGE_MAX_COVER = 9 views per pixel holds for tile_grid up to here


def check_supported(fm) -> None:
    """NotImplementedError, by name, for everything but a semantic BiSeNetFormer (``predict_all_pixels``).  Host only."""
    fam = fm.model.family
    if fam != "bisenetformer":
        raise NotImplementedError(f"FocoosModel.segment_tiled: tiled segmentation is built for the bisenetformer family only, not {fam!r}")
    if not bool(fm.model_info.config.get("predict_all_pixels", False)):
        raise NotImplementedError("FocoosModel.segment_tiled: tiled segmentation merges per-pixel classes: a bisenetformer without "
                                  "predict_all_pixels (instance mode) is not built")


def check_arguments(tile, overlap, batch_size, max_classes, default_tile, num_classes) -> tuple:
    """ValueError for anything outside the contract; returns (tile, max_classes)."""
    tile = default_tile if tile is None else tile
    if not isinstance(tile, (int, np.integer)) or int(tile) < MIN_TILE or int(tile) % 32:
        raise ValueError(f"segment_tiled: tile must be a multiple of 32 and at least {MIN_TILE}, got {tile!r}")
    if not 0.0 <= float(overlap) <= MAX_OVERLAP:
        raise ValueError(f"segment_tiled: overlap must be in [0, {MAX_OVERLAP}], got {overlap}")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError(f"segment_tiled: batch_size must be at least 1, got {batch_size}")
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"segment_tiled: the merge serves 1 .. {MAX_CLASSES} classes, the model has {num_classes}")
    max_classes = int(num_classes) if max_classes is None else int(max_classes)
    if not 1 <= max_classes <= MAX_CLASSES:
        raise ValueError(f"segment_tiled: max_classes must be in 1 .. {MAX_CLASSES}, got {max_classes}")
    return int(tile), max_classes


def segment_views(model, views: torch.Tensor, batch_size: int):
    """Run the views [Npad, t, t, 3] through ``model.detect`` chunk by chunk on ONE plan and collect, device to device, what the merge
    reads: (mask_probs [Npad, Q, h, w], cls_score [Npad, Q], cls_label [Npad, Q])."""
    Npad, bufs = views.shape[0], None
    for c0 in range(0, Npad, batch_size):
        pl = model.detect(views[c0:c0 + batch_size])
        src = (pl.mask_probs, pl.cls_score, pl.cls_label)
        if bufs is None:
            bufs = tuple(torch.empty((Npad,) + tuple(s.shape[1:]), dtype=s.dtype, device=views.device) for s in src)
        for dst, s in zip(bufs, src):
            dst[c0:c0 + batch_size].copy_(s, non_blocking=True)
    return bufs


def merge_views(lib, mask_probs: torch.Tensor, score: torch.Tensor, label: torch.Tensor, wins_host: torch.Tensor, wins_dev: torch.Tensor,
                frame_hw, num_classes: int, threshold: float, max_classes: int, want_conf: bool = False):
    """fx_seg_merge_views on the first N = len(wins_host) views of the buffers [>= N]: the packed result in the plan's field names
    (``det_count`` [1], ``det_scores`` / ``det_labels`` / ``det_area`` [1, max_classes], ``det_boxes`` [1, max_classes, 4], ``mask_words``
    [1, max_classes, Hf, ceil(Wf / 32)], ``mask_width``) plus ``label_map`` uint8 [Hf, Wf], ``status`` int32 [1] (kept classes that found
    no slot) and, when asked, ``conf`` float32 [Hf, Wf]; all on the device."""
    from ._lib import check

    dev, N = mask_probs.device, int(wins_host.shape[0])
    Q, h, w = (int(v) for v in mask_probs.shape[1:])
    Hf, Wf, M = int(frame_hw[0]), int(frame_hw[1]), int(max_classes)
    assert mask_probs.is_contiguous() and score.is_contiguous() and label.is_contiguous() and label.dtype == torch.int32
    assert mask_probs.shape[0] >= N and wins_host.dtype == torch.int32 and wins_host.is_contiguous() and wins_dev.is_contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    res = SimpleNamespace(det_count=torch.zeros(1, **i32), det_labels=torch.zeros(1, M, **i32), det_boxes=torch.zeros(1, M, 4, **i32),
                          det_area=torch.zeros(1, M, **i32), det_scores=torch.zeros(1, M, dtype=torch.float32, device=dev),
                          mask_words=torch.zeros(1, M, Hf, (Wf + 31) // 32, **i32), mask_width=Wf,
                          label_map=torch.empty(Hf, Wf, dtype=torch.uint8, device=dev), status=torch.zeros(1, **i32),
                          conf=torch.empty(Hf, Wf, dtype=torch.float32, device=dev) if want_conf else None)
    ws = torch.empty(int(lib.fx_seg_merge_workspace_bytes(N, Q, h, w, Hf, Wf, int(num_classes), M)), dtype=torch.uint8, device=dev)
    check(lib.fx_seg_merge_views(mask_probs.data_ptr(), score.data_ptr(), label.data_ptr(), wins_dev.data_ptr(), wins_host.data_ptr(), N, Q, h, w,
                                 Hf, Wf, int(num_classes), float(threshold), M, ws.data_ptr(), ws.numel(), res.label_map.data_ptr(),
                                 None if res.conf is None else res.conf.data_ptr(), res.det_count.data_ptr(), res.det_labels.data_ptr(),
                                 res.det_scores.data_ptr(), res.det_boxes.data_ptr(), res.det_area.data_ptr(), res.mask_words.data_ptr(),
                                 res.status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "fx_seg_merge_views")
    return res


def segment_tiled(fm, image, tile: Optional[int] = None, overlap: float = 0.2, threshold: Optional[float] = None,
                  batch_size: Optional[int] = None, max_classes: Optional[int] = None, mask_format: str = "png", annotate: bool = False,
                  return_label_map: bool = False, components=None, image_format=None):
    """FocoosModel.segment_tiled (see there).  ``image_format``: None, or what ``jpeg.check_image_format`` returned."""
    from ._lib import load
    from .mask_rle import check_mask_format
    from .ports import InferLatency

    check_supported(fm)
    check_mask_format(mask_format, fm.model.family, "segment_tiled")
    if components is not None:
        from . import components as CC

        components = CC.check(components, fm.model.family, fm.model_info.classes, mask_format, True, bool(annotate), "segment_tiled")
    K = int(fm.model_info.config["num_classes"])
    t, M = check_arguments(tile, overlap, batch_size, max_classes, fm.model_info.im_size, K)
    t0 = perf_counter()
    frame = frame_tensor(image, "segment_tiled")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    wins = tile_grid(H, W, t, t, float(overlap))
    N = wins.shape[0]
    bs = min(N, 32) if batch_size is None else int(batch_size)
    Npad = -(-N // bs) * bs
    dev = fm.model.device
    lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
    thr = fm.processor.threshold if threshold is None else float(threshold)
    frame_d = frame.to(dev, non_blocking=True)
    wins_h = torch.from_numpy(wins)
    wins_d = wins_h.to(dev, non_blocking=True)
    views = torch.empty(Npad, t, t, 3, dtype=torch.float32, device=dev)
    views[N:].zero_()                  # the padding of the last chunk: zero views whose results are ignored
    gather_views(lib, frame_d, wins_h, wins_d, views)
    t1 = perf_counter()
    probs, score, label = segment_views(fm.model, views, bs)
    res = merged = merge_views(lib, probs, score, label, wins_h, wins_d, (H, W), K, thr, M)
    if components is not None:      # behind the merge: one slot per connected component of every class mask; cached like the encoders below
        fm._tiled_seg_components = CC.splitter_for(getattr(fm, "_tiled_seg_components", None), res, components,
                                                   CC.split_table(components.classes, fm.model_info.classes, "segment_tiled"),
                                                   fm.processor.components_run_capacity)
        res = fm._tiled_seg_components.split(res)
    torch.cuda.current_stream(dev).synchronize()
    t2 = perf_counter()
    # the device mask encoders are cached per shape on the processor: the frame-shaped ones live on the model, so that a caller who
    # alternates infer_batch and segment_tiled keeps both sets
    proc, names = fm.processor, ("_rle_encoder", "_polygon_encoder", "_png_encoder")
    theirs = [getattr(proc, n) for n in names]
    for n, enc in zip(names, getattr(fm, "_tiled_seg_encoders", (None, None, None))):
        setattr(proc, n, enc)
    try:
        out = proc.pack_detections(res, fm.model_info.classes, mask_format=mask_format)[0]
    finally:
        fm._tiled_seg_encoders = [getattr(proc, n) for n in names]
        for n, enc in zip(names, theirs):
            setattr(proc, n, enc)
    dropped = int(merged.status.item())
    if dropped:
        warnings.warn(f"segment_tiled: {dropped} classes present in the frame found no mask plane (max_classes = {M}; classes take the "
                      "planes in ascending class id): raise max_classes")
    label_map = merged.label_map.cpu().numpy() if return_label_map else None
    t3 = perf_counter()
    if annotate:       # the frame is resident: draw the merged classes on it (a caller's own device tensor stays untouched)
        from .annotate import annotate_results

        annotate_results(fm, [frame], frame_d.clone()[None] if frame.is_cuda else frame_d[None], res, [out], None, image_format)
    t4 = perf_counter()
    out.latency = InferLatency(preprocess=round(t1 - t0, 3), inference=round(t2 - t1, 3), postprocess=round(t3 - t2, 3),
                               annotate=round(t4 - t3, 3) if annotate else None)
    return (out, label_map) if return_label_map else out      # FocoosDetections' fields are pinned: the map travels beside it
