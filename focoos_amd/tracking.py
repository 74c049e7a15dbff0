"""Identity across frames on the device (``FocoosModel.infer_stream(track=...)``).

A ByteTrack-shaped tracker (high scores first, low scores rescue tracks; class-aware greedy IoU association) over the packed results that
every box family leaves on the device.  Batch index b is stream b (camera b): one ``fx_track_update`` launch per batch, one workgroup per
stream (csrc/track_ops.hip; the contract is in include/focoos_amd.h), and one small int32 array more in the copy back.  The reference has
no counterpart.  Left out on purpose: the Kalman covariance, score fusion into the cost, Hungarian assignment, duplicate-track removal and
re-identification by appearance."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, fields
from typing import Dict, List, Optional

import numpy as np
import torch

MAX_SLOTS = 1024       # include/focoos_amd.h FX_TRACK_MAX_SLOTS: slots per stream and detections per stream
MAX_STREAMS = 65535    # FX_TRACK_MAX_STREAMS
BOX_FAMILIES = ("fai_detr", "fai_mf", "bisenetformer")


@dataclass(frozen=True)
class TrackerConfig:
    """ByteTrack's defaults restated as IoU.  ``high`` / ``low``: score classes of stage 1 / stage 2; ``new_thresh``: least score of a new
    track; ``match_iou`` / ``second_iou``: a pair is eligible when its IoU EXCEEDS the value; ``track_buffer``: frames a lost track is
    kept; ``min_hits``: matches before an id is reported; ``alpha``: gain of the velocity update; ``max_tracks``: slots per stream.
    Validated at construction: ValueError names the field."""
    high: float = 0.5
    low: float = 0.1
    new_thresh: float = 0.6
    match_iou: float = 0.2
    second_iou: float = 0.5
    track_buffer: int = 30
    min_hits: int = 1
    alpha: float = 0.5
    max_tracks: int = 256

    def __post_init__(self):
        def bad(name, why):
            raise ValueError(f"TrackerConfig.{name} = {getattr(self, name)!r}: {why}")

        for f in fields(self):
            v = getattr(self, f.name)
            if f.name in ("track_buffer", "min_hits", "max_tracks"):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    bad(f.name, "must be an integer")
            elif isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                bad(f.name, "must be a finite number")
        # compared as the float32 values the kernel receives
        f32 = {n: float(np.float32(getattr(self, n))) for n in ("high", "low", "new_thresh", "match_iou", "second_iou", "alpha")}
        if not 0.0 < f32["low"]:
            bad("low", "must be > 0")
        if not f32["low"] <= f32["high"]:
            bad("low", "must be <= high")
        if not f32["high"] <= 1.0:
            bad("high", "must be <= 1")
        if not f32["new_thresh"] >= f32["high"]:
            bad("new_thresh", "must be >= high")
        for n in ("match_iou", "second_iou"):
            if not 0.0 < f32[n] <= 1.0:
                bad(n, "must be in (0, 1]")
        if self.track_buffer < 0 or self.track_buffer > 2 ** 30:
            bad("track_buffer", "must be >= 0")
        if self.min_hits < 1 or self.min_hits > 2 ** 30:
            bad("min_hits", "must be >= 1")
        if not 0.0 <= f32["alpha"] <= 1.0:
            bad("alpha", "must be in [0, 1]")
        if not 1 <= self.max_tracks <= MAX_SLOTS:
            bad("max_tracks", f"must be in 1..{MAX_SLOTS}")


def check_family(family: str, what: str = "infer_stream") -> None:
    """NotImplementedError, by name, for a family without boxes.  Host only: nothing is loaded or launched."""
    if family not in BOX_FAMILIES:
        raise NotImplementedError(f"{what}: tracking needs boxes; model family {family!r} has none (supported: {', '.join(BOX_FAMILIES)})")


class DeviceTracker:
    """The state of ``streams`` independent trackers on ``device`` and their update, one launch per batch on the current stream.  The state
    arrays (structure of arrays, [streams, max_tracks]) belong to this object; ``track_ids`` of an update is a fresh device tensor."""

    STATE = ("id", "label", "tsu", "hits", "box", "vel", "next_id", "status")

    def __init__(self, streams: int, config: Optional[TrackerConfig] = None, device="cuda"):
        from ._lib import load

        if isinstance(streams, bool) or not isinstance(streams, (int, np.integer)) or not 1 <= streams <= MAX_STREAMS:
            raise ValueError(f"DeviceTracker: streams = {streams!r} must be in 1..{MAX_STREAMS}")
        if config is None:
            config = TrackerConfig()
        if not isinstance(config, TrackerConfig):
            raise TypeError(f"DeviceTracker: config must be a TrackerConfig, not {type(config).__name__}")
        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned (the kernel is the same in both)
        self.device = torch.device(device)
        self.streams, self.config = int(streams), config
        B, M = self.streams, config.max_tracks
        i32 = dict(dtype=torch.int32, device=self.device)
        self.id, self.label = torch.zeros(B, M, **i32), torch.zeros(B, M, **i32)
        self.tsu, self.hits = torch.zeros(B, M, **i32), torch.zeros(B, M, **i32)
        self.box = torch.zeros(B, M, 4, dtype=torch.float32, device=self.device)
        self.vel = torch.zeros(B, M, 4, dtype=torch.float32, device=self.device)
        self.next_id, self.status_words = torch.ones(B, **i32), torch.zeros(B, **i32)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _state_ptrs(self):
        return (self.id.data_ptr(), self.label.data_ptr(), self.tsu.data_ptr(), self.hits.data_ptr(), self.box.data_ptr(), self.vel.data_ptr(),
                self.next_id.data_ptr(), self.status_words.data_ptr())

    def update(self, det_scores: torch.Tensor, det_labels: torch.Tensor, det_boxes: torch.Tensor, det_count: torch.Tensor) -> torch.Tensor:
        """One frame of every stream: the packed device results (f32 [B, T], i32 [B, T], i32 xyxy [B, T, 4], i32 [B]) -> track_ids i32 [B, T]
        on the device (-1 = no id).  B must be ``streams``; T <= 1024."""
        from ._lib import check

        if det_scores.dim() != 2:
            raise ValueError(f"DeviceTracker.update: det_scores must be [B, T], got {tuple(det_scores.shape)}")
        B, T = int(det_scores.shape[0]), int(det_scores.shape[1])
        if B != self.streams:
            raise ValueError(f"DeviceTracker.update: a batch of {B} for a tracker of {self.streams} streams (batch index b is stream b)")
        if not 1 <= T <= MAX_SLOTS:
            raise ValueError(f"DeviceTracker.update: T = {T} detections per stream, must be in 1..{MAX_SLOTS}")
        for name, t, dt, shape in (("det_scores", det_scores, torch.float32, (B, T)), ("det_labels", det_labels, torch.int32, (B, T)),
                                   ("det_boxes", det_boxes, torch.int32, (B, T, 4)), ("det_count", det_count, torch.int32, (B,))):
            if tuple(t.shape) != shape or t.dtype != dt or t.device != self.id.device or not t.is_contiguous():
                raise ValueError(f"DeviceTracker.update: {name} must be a contiguous {dt} tensor {shape} on {self.id.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        c = self.config
        ids = torch.empty(B, T, dtype=torch.int32, device=self.device)
        check(self.lib.fx_track_update(det_scores.data_ptr(), det_labels.data_ptr(), det_boxes.data_ptr(), det_count.data_ptr(), B, T,
                                       *self._state_ptrs(), c.max_tracks, c.high, c.low, c.new_thresh, c.match_iou, c.second_iou,
                                       int(c.track_buffer), int(c.min_hits), c.alpha, ids.data_ptr(), self._stream()), "fx_track_update")
        return ids

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget every track of ``stream`` (all streams when None): free slots, ids from 1 again, drop counter 0."""
        from ._lib import check

        if stream is not None and (isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceTracker.reset: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        check(self.lib.fx_track_reset(*self._state_ptrs(), self.streams, self.config.max_tracks, -1 if stream is None else int(stream),
                                      self._stream()), "fx_track_reset")

    def status(self) -> np.ndarray:
        """int32 [streams]: the births dropped for want of a free slot since the last call; reads and clears the counters."""
        out = self.status_words.cpu().numpy().copy()
        self.status_words.zero_()
        return out

    def state(self) -> Dict[str, np.ndarray]:
        """Host copies of every state array (id, label, tsu, hits, box, vel, next_id, status); the counters are not cleared."""
        src = dict(id=self.id, label=self.label, tsu=self.tsu, hits=self.hits, box=self.box, vel=self.vel, next_id=self.next_id,
                   status=self.status_words)
        return {k: src[k].cpu().numpy().copy() for k in self.STATE}


def resolve(track, family: str, device, what: str = "infer_stream", device_only: bool = False):
    """What ``track=`` of infer_stream means: None / False -> no tracking; True / a TrackerConfig -> a tracker created with the first
    batch (returned as the config until then); a DeviceTracker -> itself, its state outlives the call.  ``device_only``
    (``tracker=`` of infer_batch, which sees one batch per call): a DeviceTracker or nothing."""
    if track is None or track is False:
        return None
    check_family(family, what)
    if device_only and not isinstance(track, DeviceTracker):
        raise TypeError(f"{what}: tracker must be a DeviceTracker, not {type(track).__name__}")
    if track is True:
        return TrackerConfig()
    if isinstance(track, (TrackerConfig, DeviceTracker)):
        return track
    raise TypeError(f"{what}: track must be None, True, a TrackerConfig or a DeviceTracker, not {type(track).__name__}")


def for_batch(track, B: int, device, what: str = "infer_stream") -> DeviceTracker:
    """The tracker of a batch of B: created from the config with the first batch, which fixes B; another size is a ValueError."""
    if isinstance(track, TrackerConfig):
        return DeviceTracker(B, track, device)
    if track.streams != B:
        raise ValueError(f"{what}: a batch of {B} images for a tracker of {track.streams} streams (the first batch fixes the batch size; "
                         f"batch index b is stream b)")
    return track


def attach_ids(out: List, ids) -> None:
    """Set ``track_id`` of the detections of one packed batch from its ids (host list [B][T]); -1 stays None."""
    for dets, row in zip(out, ids):
        for d, i in zip(dets.detections, row):
            if i >= 0:
                d.track_id = int(i)


def warn_drops(tracker: Optional[DeviceTracker], what: str = "infer_stream") -> None:
    """One warning when births were dropped for want of a free slot (reads and clears the counters)."""
    if tracker is None:
        return
    st = tracker.status()
    if st.any():
        warnings.warn(f"{what}: {int(st.sum())} new tracks dropped on {int((st != 0).sum())} of {tracker.streams} streams: every one of "
                      f"max_tracks = {tracker.config.max_tracks} slots was taken (raise TrackerConfig.max_tracks)", RuntimeWarning, stacklevel=4)
