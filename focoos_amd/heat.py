"""Heat maps on the device (``FocoosModel.infer_stream(heatmap=...)``).

Where the detections of a camera have been standing: every frame each detection deposits a disc of cells around its anchor on a coarse
grid, the grid optionally decays, and ``annotate=Overlay(heat=True)`` (or ``DeviceHeatmap.render``) blends the map into the frame through a
256-entry colour table - the ``HeatMapAnnotator`` of the ``supervision`` stack that DESIGN.md section 20 names as the model of this line of
work.  The packed results are already on the device when a lane finishes, so the update is one ``fx_heat_update`` call per batch
(csrc/heat_ops.hip; the contract is in include/focoos_amd.h) and nothing is copied back per frame: ``grid()`` reads the map when the caller
wants it.  Batch index b is stream b (camera b).  All decisions are integer ones; tests/heat_ref.py restates them and the GPU tests ask
for equality.  Left out on purpose: per-class maps in one object (use several ``DeviceHeatmap``), blur beyond the bilinear read,
``infer_tiled`` and ``fai_cls``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .tracking import BOX_FAMILIES, MAX_SLOTS, MAX_STREAMS
from .zones import ANCHORS, _is_int

ONE = 256              # include/focoos_amd.h FX_HEAT_ONE: one hit
CLAMP = 1 << 30        # a cell saturates here
CELLS = (4, 8, 16, 32)
MAX_RADIUS = 16
MAX_DIM = 16384
MAX_SCALE = 1 << 22    # 256 full_scale <= 2^30
FLAG_ANY_CLASS, FLAG_TRACKED_ONLY = 1, 2


def default_lut(opacity: float = 0.6) -> np.ndarray:
    """The default colour table, uint32 [256] of R | G << 8 | B << 16 | A << 24, in integers: a blue - cyan - green - yellow - red ramp
    R = clamp(384 - |4 i - 768|, 0, 255), G = clamp(384 - |4 i - 512|, 0, 255), B = clamp(384 - |4 i - 256|, 0, 255), and an alpha that
    fades in over the first quarter, A = (int(255 opacity + 0.5) * min(255, 4 i)) // 255, so lut[0].A = 0: a cell nobody stood in stays
    undrawn."""
    i = np.arange(256, dtype=np.int64)
    r, g, b = (np.clip(384 - np.abs(4 * i - c), 0, 255) for c in (768, 512, 256))
    a = (int(255 * float(opacity) + 0.5) * np.minimum(255, 4 * i)) // 255
    return (r | (g << 8) | (b << 16) | (a << 24)).astype(np.uint32)


@dataclass(frozen=True, eq=False)      # compared by identity: the table is an array
class Heatmap:
    """The configuration of a heat map of ``height`` x ``width`` frames (original pixels, 1..16384): ``cell`` - pixels per grid cell
    (4, 8, 16 or 32); ``radius`` - a detection heats the cells within this many cells of its anchor's (0..16); ``anchor`` / ``classes`` as
    in ``zones.Zone``; ``decay_shift`` - every update first takes h >> decay_shift off every cell (0 = no decay, 1..15);
    ``tracked_only`` - only detections with a track id count (needs a tracker); ``full_scale`` - the number of hits drawn in the last
    colour (0 = the stream's current maximum); ``lut`` - uint32 [256] of R | G << 8 | B << 16 | A << 24 (None: ``default_lut(opacity)``);
    ``opacity`` - of the default table, 0..1.  Validated at construction: ValueError names the field."""
    height: int
    width: int
    cell: int = 8
    radius: int = 2
    anchor: str = "bottom_center"
    classes: Optional[Sequence[int]] = None
    decay_shift: int = 0
    tracked_only: bool = False
    full_scale: int = 0
    lut: Optional[np.ndarray] = None
    opacity: float = 0.6

    def __post_init__(self):
        for f in ("height", "width"):
            v = getattr(self, f)
            if not _is_int(v) or not 1 <= v <= MAX_DIM:
                raise ValueError(f"Heatmap.{f} = {v!r}: must be an integer in 1..{MAX_DIM} (the frame size in original pixels)")
        if not _is_int(self.cell) or self.cell not in CELLS:
            raise ValueError(f"Heatmap.cell = {self.cell!r}: must be one of {CELLS}")
        if not _is_int(self.radius) or not 0 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"Heatmap.radius = {self.radius!r}: must be an integer in 0..{MAX_RADIUS} (cells)")
        if self.anchor not in ANCHORS:
            raise ValueError(f"Heatmap.anchor = {self.anchor!r}: must be one of {', '.join(ANCHORS)}")
        if self.classes is not None:
            try:
                cl = list(self.classes)
            except TypeError:
                raise ValueError(f"Heatmap.classes = {self.classes!r}: must be None (every class) or a collection of class ids") from None
            if isinstance(self.classes, (str, bytes)) or not all(_is_int(c) and 0 <= c <= 255 for c in cl):
                raise ValueError(f"Heatmap.classes = {self.classes!r}: class ids must be integers in 0..255")
            object.__setattr__(self, "classes", tuple(sorted({int(c) for c in cl})))
        if not _is_int(self.decay_shift) or not 0 <= self.decay_shift <= 15:
            raise ValueError(f"Heatmap.decay_shift = {self.decay_shift!r}: must be an integer in 0..15 (0 = no decay)")
        if not isinstance(self.tracked_only, (bool, np.bool_)):
            raise ValueError(f"Heatmap.tracked_only = {self.tracked_only!r}: must be True or False")
        if not _is_int(self.full_scale) or not 0 <= self.full_scale <= MAX_SCALE:
            raise ValueError(f"Heatmap.full_scale = {self.full_scale!r}: must be an integer in 0..{MAX_SCALE} (hits; 0 = the current maximum)")
        if isinstance(self.opacity, bool) or not isinstance(self.opacity, (int, float, np.integer, np.floating)) or not 0 <= self.opacity <= 1:
            raise ValueError(f"Heatmap.opacity = {self.opacity!r}: must be a number in 0..1")
        if self.lut is not None:
            lut = self.lut
            if not isinstance(lut, np.ndarray) or lut.dtype != np.uint32 or lut.shape != (256,):
                raise ValueError("Heatmap.lut: must be None or a numpy uint32 array [256] of R | G << 8 | B << 16 | A << 24")
            lut = np.ascontiguousarray(lut).copy()
            lut.setflags(write=False)
            object.__setattr__(self, "lut", lut)

    @property
    def grid_shape(self):
        """(Gh, Gw): cells along y and x."""
        return (self.height + self.cell - 1) // self.cell, (self.width + self.cell - 1) // self.cell

    @property
    def table(self) -> np.ndarray:
        """The colour table that is uploaded."""
        return self.lut if self.lut is not None else default_lut(self.opacity)

    def class_words(self) -> np.ndarray:
        words = np.zeros(8, np.uint32)
        for c in self.classes or ():
            words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
        return words


def check_family(family: str, what: str = "infer_stream") -> None:
    """NotImplementedError, by name, for a family without boxes.  Host only: nothing is loaded or launched."""
    if family not in BOX_FAMILIES:
        raise NotImplementedError(f"{what}: a heat map needs boxes; model family {family!r} has none (supported: {', '.join(BOX_FAMILIES)})")


class DeviceHeatmap:
    """The heat maps of ``streams`` cameras on ``device`` and the update of one batch.  The state belongs to this object and outlives the
    ``infer_stream`` calls it is passed to."""

    STATE = ("heat", "heat_max")

    def __init__(self, streams: int, config: Heatmap, device=None):
        if not _is_int(streams) or not 1 <= streams <= MAX_STREAMS:
            raise ValueError(f"DeviceHeatmap: streams = {streams!r} must be in 1..{MAX_STREAMS}")
        if not isinstance(config, Heatmap):
            raise TypeError(f"DeviceHeatmap: config must be a Heatmap, not {type(config).__name__}")
        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library (the kernels are the same in both)
        self.streams, self.config = int(streams), config
        self.device = torch.device(device if device is not None else "cuda")
        self.Gh, self.Gw = config.grid_shape
        i32 = dict(dtype=torch.int32, device=self.device)
        self.heat, self.heat_max = torch.zeros(self.streams, self.Gh, self.Gw, **i32), torch.zeros(self.streams, **i32)
        self._part = torch.zeros(self.streams, int(self.lib.fx_heat_tiles(config.height, config.width, config.cell)), **i32)
        self._words = config.class_words()      # host memory, read by every update
        self._flags = (FLAG_ANY_CLASS if config.classes is None else 0) | (FLAG_TRACKED_ONLY if config.tracked_only else 0)
        self._lut = torch.from_numpy(config.table.view(np.int32).copy()).to(self.device)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def update(self, det_labels: torch.Tensor, det_boxes: torch.Tensor, det_count: torch.Tensor, track_ids: Optional[torch.Tensor] = None) -> None:
        """One frame of every stream: the packed device results (i32 [B, T], i32 xyxy [B, T, 4] in original pixels, i32 [B]) and, for
        ``tracked_only``, the ids the tracker gave them in this frame (i32 [B, T]).  B must be ``streams``; T <= 1024."""
        from ._lib import check

        if det_labels.dim() != 2:
            raise ValueError(f"DeviceHeatmap.update: det_labels must be [B, T], got {tuple(det_labels.shape)}")
        B, T = int(det_labels.shape[0]), int(det_labels.shape[1])
        if B != self.streams:
            raise ValueError(f"DeviceHeatmap.update: a batch of {B} for heat maps of {self.streams} streams (batch index b is stream b)")
        if not 1 <= T <= MAX_SLOTS:
            raise ValueError(f"DeviceHeatmap.update: T = {T} detections per stream, must be in 1..{MAX_SLOTS}")
        if self.config.tracked_only and track_ids is None:
            raise ValueError("DeviceHeatmap.update: Heatmap.tracked_only = True needs track_ids")
        args = [("det_labels", det_labels, (B, T)), ("det_boxes", det_boxes, (B, T, 4)), ("det_count", det_count, (B,))]
        if track_ids is not None:
            args.append(("track_ids", track_ids, (B, T)))
        for name, t, shape in args:
            if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.heat.device or not t.is_contiguous():
                raise ValueError(f"DeviceHeatmap.update: {name} must be a contiguous torch.int32 tensor {shape} on {self.heat.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        c = self.config
        check(self.lib.fx_heat_update(det_labels.data_ptr(), det_boxes.data_ptr(), det_count.data_ptr(),
                                      None if track_ids is None else track_ids.data_ptr(), B, T, c.height, c.width, c.cell, c.radius,
                                      ANCHORS.index(c.anchor), c.decay_shift, self._flags, self._words.ctypes.data, self.heat.data_ptr(),
                                      self.heat_max.data_ptr(), self._part.data_ptr(), self._stream()), "fx_heat_update")

    def check_frame(self, H: int, W: int, what: str = "DeviceHeatmap.render") -> None:
        if (int(H), int(W)) != (self.config.height, self.config.width):
            raise ValueError(f"{what}: a frame of {int(H)} x {int(W)} for a heat map of {self.config.height} x {self.config.width} (height x width)")

    def render(self, frames: torch.Tensor, b0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fx_annotate_heat_u8: the maps of streams b0 .. b0+B-1 blended into ``frames`` (device uint8 [B, H, W, 3] of the heat map's
        size), in place or into ``out``.  A stream whose map is still cold (and ``full_scale`` = 0) keeps its bytes."""
        from ._lib import check

        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3
                and frames.is_contiguous()):
            raise ValueError("DeviceHeatmap.render takes contiguous device uint8 frames [B, H, W, 3]")
        B, H, W, _ = frames.shape
        self.check_frame(H, W)
        if not _is_int(b0) or b0 < 0 or b0 + B > self.streams:
            raise ValueError(f"DeviceHeatmap.render: frames {b0} .. {b0 + B - 1} of {self.streams} streams")
        dst = frames if out is None else out
        if out is not None and (out.shape != frames.shape or out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous()):
            raise ValueError("DeviceHeatmap.render: out must be a contiguous device uint8 tensor of the frames' shape")
        check(self.lib.fx_annotate_heat_u8(frames.data_ptr(), dst.data_ptr(), B, H, W, int(b0), self.streams, self.heat.data_ptr(),
                                           self.heat_max.data_ptr(), self.config.cell, self.config.full_scale, self._lut.data_ptr(),
                                           self._stream()), "fx_annotate_heat_u8")
        return dst

    def grid(self, stream: Optional[int] = None) -> np.ndarray:
        """The map in hits (heat / 256) as float32 on the host, copied on demand: [Gh, Gw] of ``stream``, or [streams, Gh, Gw]."""
        if stream is not None and (not _is_int(stream) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceHeatmap.grid: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        h = (self.heat if stream is None else self.heat[int(stream)]).cpu().numpy()
        return (h.astype(np.float64) / ONE).astype(np.float32)

    def reset(self, stream: Optional[int] = None) -> None:
        """Cool the map of ``stream`` (all streams when None) down to zero."""
        if stream is not None and (not _is_int(stream) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceHeatmap.reset: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        if stream is None:
            self.heat.zero_(), self.heat_max.zero_()
        else:
            self.heat[int(stream)].zero_(), self.heat_max[int(stream)].zero_()

    def state(self) -> Dict[str, np.ndarray]:
        """Host copies of the state arrays: heat [streams, Gh, Gw], heat_max [streams]."""
        return dict(heat=self.heat.cpu().numpy().copy(), heat_max=self.heat_max.cpu().numpy().copy())


def resolve(heatmap, tracked: bool, family: str, what: str = "infer_stream", device_only: bool = False):
    """What ``heatmap=`` means, decided on the host before anything touches the GPU: None -> None; a Heatmap (not with ``device_only``,
    which is infer_batch: the DeviceHeatmap is created with the first batch) or a DeviceHeatmap, whose ``tracked_only`` needs a tracker."""
    if heatmap is None:
        return None
    check_family(family, what)
    if not isinstance(heatmap, DeviceHeatmap if device_only else (Heatmap, DeviceHeatmap)):
        raise TypeError(f"{what}: heatmap must be a " + ("DeviceHeatmap" if device_only else "Heatmap or a DeviceHeatmap") +
                        f", not {type(heatmap).__name__}")
    cfg = heatmap.config if isinstance(heatmap, DeviceHeatmap) else heatmap
    if cfg.tracked_only and not tracked:
        raise ValueError(f"{what}: Heatmap.tracked_only = True needs a tracker (pass track= / tracker=)")
    return heatmap


def for_batch(heatmap, B: int, device, what: str = "infer_stream") -> DeviceHeatmap:
    """The DeviceHeatmap of a batch of B: created from the Heatmap with the first batch, which fixes B; another size is a ValueError."""
    if not isinstance(heatmap, DeviceHeatmap):
        return DeviceHeatmap(B, heatmap, device)
    if heatmap.streams != B:
        raise ValueError(f"{what}: a batch of {B} images for heat maps of {heatmap.streams} streams (batch index b is stream b)")
    return heatmap


def check_sizes(heatmap, sizes, what: str = "infer_stream") -> None:
    """Every frame of the batch must have the heat map's size (the boxes are in original pixels): ValueError before the launch."""
    cfg = heatmap.config if isinstance(heatmap, DeviceHeatmap) else heatmap
    for i, (h, w) in enumerate(sizes):
        if (int(h), int(w)) != (cfg.height, cfg.width):
            raise ValueError(f"{what}: heatmap: input {i} is {int(h)} x {int(w)}, the heat map is {cfg.height} x {cfg.width} (height x width)")
