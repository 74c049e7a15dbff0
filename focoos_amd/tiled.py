"""Tiled RT-DETR inference of one large frame (``FocoosModel.infer_tiled``).

``infer`` squashes the whole picture to the model's input size; on a 4000 x 3000 frame a 20-pixel object shrinks to 3 pixels.  Here the
frame is cut into overlapping windows of the model's size, every window (plus, optionally, the whole frame resized) is one image of an
engine batch, the boxes are moved back into frame coordinates and duplicates across windows are suppressed - all on the device:

  frame (uint8 HWC, uploaded once) -> fx_tile_gather_u8_f32 -> float32 views -> FAIDetr.detect per chunk -> packed results [N][T]
                                   -> fx_merge_detections_nms -> one packed list -> DETRProcessor.pack_detections (the one D2H copy)

The reference has no counterpart (like ``infer_stream``); ``tile_grid`` is pure host code.

Tiled inference of video streams (``infer_stream(tiling=Tiling(...))`` / ``infer_batch(tiling=)``) is the batched form: S
frames of one size, one per camera, and one packed result per stream that stays on the device for the tracker, the zones and the overlay:

  FrameBatch (NV12 / I420 / BGR / RGB planes) -> fx_frames_tile_gather_f32 -> views [S * V] -> engine pipeline, chunks of batch_size
                                              -> packed results [S * V][T] -> fx_merge_detections_nms_batched -> det_* [S][D], frame pixels"""
from __future__ import annotations

import math
import os
import warnings
from dataclasses import dataclass
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


# ---------------------------------------------------------------- tiled inference of video streams
MAX_STREAM_DETECTIONS = 1024            # the tracker's and the annotator's slot limit (tracking.MAX_SLOTS)


@dataclass(frozen=True)
class Tiling:
    """``infer_stream(tiling=...)`` / ``infer_batch(tiling=...)``: every input of a batch is a large frame of stream b, cut into the windows
    of ``views_of`` and merged per stream on the device.  The fields mean what the arguments of ``infer_tiled`` mean and are checked here
    by the same rules (a ValueError names the field); ``max_detections`` is also the slot count of the merged packed result that the
    tracker, the zones and the annotator read, so it may not exceed 1024."""
    tile: Union[None, int, Tuple[int, int]] = None
    overlap: float = 0.2
    merge_threshold: float = 0.5
    merge_metric: str = "iou"
    include_full: bool = True
    max_detections: int = 300
    batch_size: Optional[int] = None

    def __post_init__(self):
        check_arguments(self.tile, self.overlap, self.merge_threshold, self.merge_metric, self.batch_size, self.max_detections, MIN_TILE)
        if int(self.max_detections) > MAX_STREAM_DETECTIONS:
            raise ValueError(f"Tiling: max_detections must be at most {MAX_STREAM_DETECTIONS} (the slots the tracker, the zones and the "
                             f"annotator read per stream), got {self.max_detections}")


def check_tiling(fm, tiling, what: str) -> None:
    """The refusals that need no input: family (NotImplementedError by name, as ``check_supported``) and the argument's type."""
    fam = fm.model.family
    if fam != "fai_detr":
        raise NotImplementedError(f"{what}(tiling=): tiled inference is built for the fai_detr family only, not {fam!r} "
                                  "(merging masks or class scores across tiles is a different problem)")
    if not isinstance(tiling, Tiling):
        raise TypeError(f"{what}: tiling must be a tiled.Tiling, not {type(tiling).__name__}")


def stream_frames(inputs, what: str):
    """One batch of ``tiling=`` inputs as a FrameBatch of ONE (H, W): a FrameBatch, a Frame, or a list of Frames and / or uint8 RGB arrays
    or tensors [H, W, 3] (wrapped as RGB24 frames).  ValueError for anything else; host only."""
    from .frames import wrap_frames

    fb = wrap_frames(inputs, f"{what}(tiling=)")
    sizes = fb.sizes
    for i, s in enumerate(sizes):
        if s != sizes[0]:
            raise ValueError(f"{what}(tiling=): the frames of one batch must share one (H, W): frame 0 is {sizes[0]}, frame {i} is {s}")
    return fb


def view_chunks(S: int, V: int, batch_size: Optional[int] = None):
    """The flat view and chunk plan of S streams of V views: view (s, v) has flat index s * V + v, the flat list is cut into consecutive
    chunks of ``batch_size`` (default min(S * V, 32)) and the last chunk is padded.  Returns (batch_size, [(first flat index, views of the
    chunk that are real)]); a chunk's padding is batch_size minus the second number."""
    S, V = int(S), int(V)
    if S < 1 or V < 1:
        raise ValueError(f"view_chunks: S = {S} streams of V = {V} views must be positive")
    N = S * V
    bs = min(N, 32) if batch_size is None else int(batch_size)
    if bs < 1:
        raise ValueError(f"view_chunks: batch_size must be at least 1, got {batch_size}")
    return bs, [(c0, min(bs, N - c0)) for c0 in range(0, N, bs)]


def view_sizes(wins: np.ndarray, S: int, Npad: int, th: int, tw: int) -> np.ndarray:
    """``sizes`` of the padded flat view list, int32 [Npad, 2]: a view's own window (h, w), the tile's for the padding."""
    sizes = np.full((Npad, 2), (th, tw), dtype=np.int32)
    sizes[:S * len(wins)] = np.tile(wins[:, [3, 2]], (S, 1))
    return sizes


def gather_stream_views(lib, fb, device, wins_host: torch.Tensor, wins_dev: torch.Tensor, out: torch.Tensor) -> None:
    """fx_frames_tile_gather_f32: ``out`` [>= S * V, Ho, Wo, 3] float32 receives view s * V + v = window v of frame s, on the current stream."""
    import ctypes

    from ._lib import check

    S, V = len(fb), wins_host.shape[0]
    assert out.is_contiguous() and out.shape[0] >= S * V and wins_host.dtype == torch.int32
    descs, host = fb._descriptors(device)
    check(lib.fx_frames_tile_gather_f32(descs.data_ptr(), ctypes.addressof(host), S, wins_dev.data_ptr(), wins_host.data_ptr(), V, out.data_ptr(),
                                        out.shape[1], out.shape[2], torch.cuda.current_stream(torch.device(device)).cuda_stream),
          "fx_frames_tile_gather_f32")


def merge_batched(lib, scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor, count: torch.Tensor, wins_dev: torch.Tensor, S: int,
                  V: int, frame_hw: Tuple[int, int], tiling: Tiling, status: torch.Tensor, ws: Optional[torch.Tensor] = None):
    """fx_merge_detections_nms_batched on the first S * V views of the packed buffers [>= S * V][T]: the merged packed result in frame
    pixels, in the plan's own field names (``det_scores`` [S, D], ``det_labels``, ``det_boxes`` [S, D, 4], ``det_count`` [S]), on the
    device.  ``status`` int32 [S] has the candidates dropped by the cap ADDED to it."""
    from types import SimpleNamespace

    from ._lib import check

    dev, T, D = scores.device, scores.shape[1], int(tiling.max_detections)
    res = SimpleNamespace(det_scores=torch.empty(S, D, dtype=torch.float32, device=dev), det_labels=torch.empty(S, D, dtype=torch.int32, device=dev),
                          det_boxes=torch.empty(S, D, 4, dtype=torch.int32, device=dev), det_count=torch.empty(S, dtype=torch.int32, device=dev))
    if ws is None:
        ws = torch.empty(int(lib.fx_merge_detections_batched_workspace_bytes(S, V, T)), dtype=torch.uint8, device=dev)
    check(lib.fx_merge_detections_nms_batched(scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), count.data_ptr(), wins_dev.data_ptr(), S, V, T,
                                              int(frame_hw[0]), int(frame_hw[1]), float(tiling.merge_threshold), MERGE_METRICS[tiling.merge_metric],
                                              D, res.det_scores.data_ptr(), res.det_labels.data_ptr(), res.det_boxes.data_ptr(),
                                              res.det_count.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream(dev).cuda_stream), "fx_merge_detections_nms_batched")
    return res


def warn_dropped(status: torch.Tensor, what: str) -> None:
    """The once-per-call warning of candidates that the cap kept out of suppression (``status`` accumulates over the call's merges)."""
    dropped = int(status.sum().item())
    if dropped:
        warnings.warn(f"{what}(tiling=): {dropped} candidates were dropped before suppression (only the {NMS_CAP} best of a stream's frame "
                      "enter it): raise the threshold")


class StreamTiler:
    """What one call of ``infer_stream(tiling=)`` / ``infer_batch(tiling=)`` keeps on the device: the windows and view sizes of the current
    (S, H, W), ``ring`` view buffers (the padding of the last chunk zeroed once), the merge workspace and the dropped-candidates counter."""

    def __init__(self, fm, tiling: Tiling, ring: int):
        from ._lib import load

        self.fm, self.tiling, self.ring = fm, tiling, ring
        self.dev = fm.model.device
        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
        self.th, self.tw = check_arguments(tiling.tile, tiling.overlap, tiling.merge_threshold, tiling.merge_metric, tiling.batch_size,
                                           tiling.max_detections, fm.model_info.im_size)
        self.key = None
        self.status = None
        self.turn = 0

    def changed(self, S: int, H: int, W: int) -> bool:
        """Whether (S, H, W) differs from the current shape: the caller then drains what is in flight and calls ``reshape``."""
        return self.key != (S, H, W)

    def reshape(self, S: int, H: int, W: int) -> None:
        t = self.tiling
        self.key, self.S, self.H, self.W = (S, H, W), S, H, W
        wins = views_of(H, W, self.th, self.tw, float(t.overlap), t.include_full)
        self.V = wins.shape[0]
        self.N = S * self.V
        self.bs, self.chunks = view_chunks(S, self.V, t.batch_size)
        self.Npad = len(self.chunks) * self.bs
        self.wins_h = torch.from_numpy(wins)
        self.wins_d = self.wins_h.to(self.dev, non_blocking=True)
        self.sizes = torch.from_numpy(view_sizes(wins, S, self.Npad, self.th, self.tw)).to(self.dev, non_blocking=True)
        self.views = []
        for _ in range(self.ring):
            v = torch.empty(self.Npad, self.th, self.tw, 3, dtype=torch.float32, device=self.dev)
            v[self.N:].zero_()         # the padding of the last chunk: zero views whose results are ignored; the gather never writes them
            self.views.append(v)
        self.ws = None
        if self.status is None or self.status.shape[0] != S:
            if self.status is not None:
                warn_dropped(self.status, "infer_stream")
            self.status = torch.zeros(S, dtype=torch.int32, device=self.dev)

    def gather(self, fb) -> torch.Tensor:
        """The next view buffer of the ring, filled from the frames in one launch on the current stream."""
        views = self.views[self.turn % self.ring]
        self.turn += 1
        gather_stream_views(self.lib, fb, self.dev, self.wins_h, self.wins_d, views)
        return views

    def collect_buffers(self, T: int):
        dev = self.dev
        return (torch.empty(self.Npad, T, dtype=torch.float32, device=dev), torch.empty(self.Npad, T, dtype=torch.int32, device=dev),
                torch.empty(self.Npad, T, 4, dtype=torch.int32, device=dev), torch.empty(self.Npad, dtype=torch.int32, device=dev))

    def merge(self, bufs):
        scores, labels, boxes, count = bufs
        if self.ws is None:
            self.ws = torch.empty(int(self.lib.fx_merge_detections_batched_workspace_bytes(self.S, self.V, scores.shape[1])), dtype=torch.uint8,
                                  device=self.dev)
        return merge_batched(self.lib, scores, labels, boxes, count, self.wins_d, self.S, self.V, (self.H, self.W), self.tiling, self.status,
                             self.ws)

    def rgb(self, fb) -> torch.Tensor:
        """The frames as one uint8 RGB device tensor [S, H, W, 3]: what the overlay draws on (the planes are resident already)."""
        return fb._ingest(self.dev, 0, self.S, torch.empty(self.S, self.H, self.W, 3, dtype=torch.uint8, device=self.dev), False)


def infer_batch_tiled(fm, fb, tiling: Tiling, thr: float):
    """The device side of ``infer_batch(tiling=)`` up to the merged packed result: (result, tiler).  The chunks run through ``model.detect``
    one after the other on one plan, collected device to device, then one batched merge."""
    tl = StreamTiler(fm, tiling, 1)
    H, W = fb.sizes[0]
    tl.reshape(len(fb), H, W)
    views = tl.gather(fb)
    return tl.merge(detect_views(fm.model, views, tl.sizes, tl.bs, thr)), tl


def infer_stream_tiled(fm, batches, tiling: Tiling, thr: float, depth: Optional[int], an):
    """The loop of ``infer_stream(tiling=)``.  Every chunk of every frame batch is one submit on ONE engine pipeline of (batch_size, th, tw);
    a lane's packed results are copied out device to device (after ``wait``, on the current stream, which the lane's next submit waits
    for) before that lane is submitted to again; a frame batch is finished - merged, then ``analyse``d like an engine plan's result - once
    the next one has been submitted, so its chunks run while this one is merged and packed.  Two view buffers alternate: the gather of
    frame batch i + 2 overwrites what the chunks of batch i read, and batch i has been finished (every chunk waited for) by then.
    ``an``: the call's ``analytics.StreamAnalytics`` - ``an.prepare(fb, S)`` checks the batch and creates the per-call state
    (called before anything here loads the library), ``an.analyse(result, S, fb)`` and ``an.draw`` are the tail every entry point runs;
    ``fb`` are the batch's frames, which ``classify=`` crops from."""
    from collections import deque

    tl, pipe, T = None, None, 0      # the tiler loads the library: created once the first batch has passed the host checks
    pending = deque()          # frame batches in flight: {"fb": the frames (kept alive), "bufs": the collected packed results [Npad][T]}
    outstanding = deque()      # submitted chunks whose lane still holds the result: (ticket, frame batch record, first flat index)

    def collect():
        ticket, rec, c0 = outstanding.popleft()
        pl = pipe.wait(ticket)
        for dst, src in zip(rec["bufs"], (pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)):
            dst[c0:c0 + tl.bs].copy_(src, non_blocking=True)

    def finish():
        rec = pending.popleft()
        while outstanding and outstanding[0][1] is rec:
            collect()
        res = tl.merge(rec["bufs"])
        drawn = (rec["fb"], tl.rgb(rec["fb"])) if an.annotate else None
        out = an.analyse(res, tl.S, rec["fb"])
        if drawn is not None:
            an.draw(drawn, res, out)
        return out

    for inputs in batches:
        fb = an.frames(inputs)
        S, (H, W) = len(fb), fb.sizes[0]
        an.prepare(fb, S)
        if tl is None:
            tl = StreamTiler(fm, tiling, 2)
        if tl.changed(S, H, W):
            while pending:
                yield finish()
            tl.reshape(S, H, W)
            if pipe is None or pipe.B != tl.bs:
                pipe = fm.model.engine.pipeline(tl.bs, tl.th, tl.tw, depth, True)
                T = int(pipe.lanes[0][0].det_scores.shape[1])
        views = tl.gather(fb)            # at most one frame batch is pending here, and it read the OTHER view buffer
        rec = {"fb": fb, "bufs": tl.collect_buffers(T)}
        pending.append(rec)
        for c0, _ in tl.chunks:
            while len(outstanding) >= pipe.depth:      # the lane about to be reused still holds an uncollected result
                collect()
            outstanding.append((pipe.submit(views[c0:c0 + tl.bs], tl.sizes[c0:c0 + tl.bs], thr), rec, c0))
        if len(pending) > 1:             # the batch before this one: its chunks were all submitted before this batch's
            yield finish()
    while pending:
        yield finish()
    if tl is not None and tl.status is not None:
        warn_dropped(tl.status, "infer_stream")


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
