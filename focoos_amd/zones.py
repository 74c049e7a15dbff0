"""Zone and line counting on the device (``FocoosModel.infer_stream(zones=...)``).

How many detections stand in a polygon now, and how many tracks crossed into / out of it or over a line: the ``PolygonZone`` / ``LineZone``
analytics a camera deployment asks for after identity.  Everything the counter needs is already on the device - the packed results every
box family leaves there and the tracker's ids (tracking.py) - so it is one ``fx_zone_update`` launch per batch, one workgroup per stream
(csrc/zone_ops.hip; the contract is in include/focoos_amd.h), and a few hundred bytes more in the copy back.  Batch index b is stream b
(camera b).  All decisions are integer ones; tests/zones_ref.py restates them and the GPU tests ask for equality.  The reference has no
counterpart.  Left out on purpose: ``infer_tiled``; the regions and their counts are drawn by ``annotate=Overlay(...)`` (annotate.py,
DESIGN.md section 22); how long a track stays in a zone is ``DeviceDwell`` below (``infer_stream(dwell=...)``) and
where the detections stand over time is heat.py.

A detection is represented by its anchor, one of nine points of its integer box.  A ``Zone`` is an even-odd polygon (an axis-aligned
rectangle is half-open: left and top edges inside, right and bottom edges outside); a ``Line`` from ``start`` to ``end`` observes the side
of the anchor (positive = to the right of the direction of travel start -> end in image coordinates, y down) while the anchor projects
onto the segment.  A track whose observed side flips is an event: into a zone / onto the positive side = "entered", the other way =
"exited".  The first observation of a track only records its side, and a detection without an id takes part in the occupancy only.

After ``DeviceTracker.reset(b)`` the ids of stream b restart at 1, so they would meet the sides stored for the old ids:
``DeviceZones.reset(b, counters=False)`` must follow it, and so must ``DeviceDwell.reset(b, totals=False)`` (the visits in progress are
keyed by the old ids).  ``infer_stream`` never resets any of them."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .tracking import BOX_FAMILIES, MAX_SLOTS, MAX_STREAMS, DeviceTracker

MAX_REGIONS = 32       # include/focoos_amd.h FX_ZONE_MAX_REGIONS: regions per stream, one bit each in the per-detection masks
MAX_VERTS = 64         # FX_ZONE_MAX_VERTS
COORD = 32768          # |vertex coordinate| <=
ANCHORS = ("top_left", "top_center", "top_right", "center_left", "center", "center_right", "bottom_left", "bottom_center", "bottom_right")
KIND_ZONE, KIND_LINE = 0, 1
REC_WORDS = 16         # fx_zone_region: kind, anchor, flags, vert_first, vert_count, class_words[8], reserved[3]
KEYS = ("kind", "count", "detections", "entered", "exited", "crossed_in", "crossed_out")
DWELL_KEYS = ("dwell", "visits", "dwell_total", "dwell_max", "dwell_mean")      # added to a dwell zone's dict; with fps also "dwell_seconds"


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _point(cls: str, field: str, p) -> Tuple[int, int]:
    try:
        x, y = p
    except (TypeError, ValueError):
        raise ValueError(f"{cls}.{field}: {p!r} is not an (x, y) pair") from None
    if not (_is_int(x) and _is_int(y)) or not (-COORD <= x <= COORD and -COORD <= y <= COORD):
        raise ValueError(f"{cls}.{field}: ({x!r}, {y!r}) must be integer pixels in [{-COORD}, {COORD}]")
    return int(x), int(y)


def _common(self, cls: str) -> None:
    """name / stream / classes / anchor of both region kinds; normalises classes to a sorted tuple."""
    if not isinstance(self.name, str) or not self.name:
        raise ValueError(f"{cls}.name = {self.name!r}: must be a non-empty string")
    if self.stream is not None and (not _is_int(self.stream) or not 0 <= self.stream < MAX_STREAMS):
        raise ValueError(f"{cls}.stream = {self.stream!r}: must be None (every stream) or a stream index >= 0")
    if self.classes is not None:
        try:
            cl = list(self.classes)
        except TypeError:
            raise ValueError(f"{cls}.classes = {self.classes!r}: must be None (every class) or a collection of class ids") from None
        if isinstance(self.classes, (str, bytes)) or not all(_is_int(c) and 0 <= c <= 255 for c in cl):
            raise ValueError(f"{cls}.classes = {self.classes!r}: class ids must be integers in 0..255")
        object.__setattr__(self, "classes", tuple(sorted({int(c) for c in cl})))
    if self.anchor not in ANCHORS:
        raise ValueError(f"{cls}.anchor = {self.anchor!r}: must be one of {', '.join(ANCHORS)}")


@dataclass(frozen=True)
class Zone:
    """A polygon zone: ``polygon`` = 3..64 (x, y) integer pixel vertices in [-32768, 32768] (either orientation, even-odd rule);
    ``stream``: None = every stream, or one stream index; ``classes``: None = every class, or class ids in 0..255; ``anchor``: which point
    of a box stands for the detection (``ANCHORS``).  Validated at construction: ValueError names the field."""
    name: str
    polygon: Sequence[Tuple[int, int]]
    stream: Optional[int] = None
    classes: Optional[Sequence[int]] = None
    anchor: str = "bottom_center"

    kind = "zone"

    def __post_init__(self):
        _common(self, "Zone")
        try:
            pts = list(self.polygon)
        except TypeError:
            raise ValueError(f"Zone.polygon = {self.polygon!r}: must be a sequence of (x, y) pairs") from None
        if not 3 <= len(pts) <= MAX_VERTS:
            raise ValueError(f"Zone.polygon: {len(pts)} vertices, must be 3..{MAX_VERTS}")
        object.__setattr__(self, "polygon", tuple(_point("Zone", "polygon", p) for p in pts))

    @property
    def vertices(self) -> Tuple[Tuple[int, int], ...]:
        return self.polygon


@dataclass(frozen=True)
class Line:
    """A counting line from ``start`` to ``end`` ((x, y) integer pixels, different points); the other fields as in ``Zone``.  Needs a
    tracker: a line has no occupancy, only crossings."""
    name: str
    start: Tuple[int, int]
    end: Tuple[int, int]
    stream: Optional[int] = None
    classes: Optional[Sequence[int]] = None
    anchor: str = "bottom_center"

    kind = "line"

    def __post_init__(self):
        _common(self, "Line")
        object.__setattr__(self, "start", _point("Line", "start", self.start))
        object.__setattr__(self, "end", _point("Line", "end", self.end))
        if self.start == self.end:
            raise ValueError(f"Line.end = {self.end!r}: must differ from start")

    @property
    def vertices(self) -> Tuple[Tuple[int, int], ...]:
        return (self.start, self.end)


Region = Union[Zone, Line]


def check_family(family: str, what: str = "infer_stream") -> None:
    """NotImplementedError, by name, for a family without boxes.  Host only: nothing is loaded or launched."""
    if family not in BOX_FAMILIES:
        raise NotImplementedError(f"{what}: zones need boxes; model family {family!r} has none (supported: {', '.join(BOX_FAMILIES)})")


def check_regions(regions, streams: Optional[int] = None, tracked: bool = True, what: str = "DeviceZones") -> List[Region]:
    """The list of regions, validated on the host: Zone / Line objects, at least one, names unique within every stream, at most 32 per
    stream, stream indices below ``streams`` (when known), and no Line without a tracker."""
    if isinstance(regions, (Zone, Line)) or not isinstance(regions, (list, tuple)):
        raise TypeError(f"{what}: regions must be a list of Zone / Line, not {type(regions).__name__}")
    regions = list(regions)
    if not regions:
        raise ValueError(f"{what}: regions is empty")
    for r in regions:
        if not isinstance(r, (Zone, Line)):
            raise TypeError(f"{what}: regions must hold Zone / Line objects, not {type(r).__name__}")
        if isinstance(r, Line) and not tracked:
            raise ValueError(f"{what}: Line {r.name!r} needs a tracker (a line counts crossings of tracked objects): pass track= / tracker=")
        if streams is not None and r.stream is not None and r.stream >= streams:
            raise ValueError(f"{what}: regions: {type(r).__name__} {r.name!r} has stream = {r.stream}, there are {streams} streams")
    shared = [r.name for r in regions if r.stream is None]
    per: Dict[int, List[str]] = {}
    for r in regions:
        if r.stream is not None:
            per.setdefault(int(r.stream), []).append(r.name)
    for s, names in [(None, shared)] + [(s, shared + n) for s, n in sorted(per.items())]:
        dup = sorted({n for n in names if names.count(n) > 1})
        if dup:
            raise ValueError(f"{what}: regions: name {dup[0]!r} is used twice" + ("" if s is None else f" on stream {s}"))
        if len(names) > MAX_REGIONS:
            raise ValueError(f"{what}: regions: {len(names)} regions" + ("" if s is None else f" on stream {s}") + f", at most {MAX_REGIONS} per stream")
    return regions


def build_tables(regions: Sequence[Region], streams: int):
    """The host tables of ``fx_zone_update``: (records int32 [R_total, 16], reg_first int32 [streams + 1], verts int32 [V_total, 2],
    per_stream = for every stream the list of its regions in bit order).  A region's vertices are stored once; a shared region has one
    record per stream, all pointing at them.  Bit order = list order among the regions of the stream."""
    verts, first = [], []
    for r in regions:
        first.append(len(verts))
        verts.extend(r.vertices)
    recs, reg_first, per_stream = [], [0], []
    for b in range(streams):
        mine = [i for i, r in enumerate(regions) if r.stream is None or r.stream == b]
        per_stream.append([regions[i] for i in mine])
        for i in mine:
            r = regions[i]
            words = np.zeros(8, np.uint32)
            for c in r.classes or ():
                words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
            rec = np.zeros(REC_WORDS, np.int32)
            rec[:5] = (KIND_LINE if isinstance(r, Line) else KIND_ZONE, ANCHORS.index(r.anchor), 1 if r.classes is None else 0, first[i],
                       len(r.vertices))
            rec[5:13] = words.view(np.int32)
            recs.append(rec)
        reg_first.append(len(recs))
    return (np.ascontiguousarray(np.stack(recs)), np.asarray(reg_first, np.int32), np.ascontiguousarray(np.asarray(verts, np.int32).reshape(-1, 2)),
            per_stream)


class DeviceZones:
    """The regions of ``streams`` cameras on ``device``, their per-track side state and running totals, and the update of one batch: one
    launch on the current stream.  ``tracker``: the ``DeviceTracker`` whose ids the updates will be given (its ``max_tracks`` sizes the
    state and its slot table tells which slot an id lives in); without one only the occupancy of zones is counted and a ``Line`` raises
    ValueError.  The state belongs to this object and outlives ``infer_stream`` calls it is passed to."""

    STATE = ("st_id", "st_side", "in_total", "out_total")

    def __init__(self, streams: int, regions: Sequence[Region], tracker: Optional[DeviceTracker] = None, device=None):
        if not _is_int(streams) or not 1 <= streams <= MAX_STREAMS:
            raise ValueError(f"DeviceZones: streams = {streams!r} must be in 1..{MAX_STREAMS}")
        if tracker is not None and not isinstance(tracker, DeviceTracker):
            raise TypeError(f"DeviceZones: tracker must be a DeviceTracker, not {type(tracker).__name__}")
        if tracker is not None and tracker.streams != streams:
            raise ValueError(f"DeviceZones: streams = {streams} but the tracker has {tracker.streams}")
        self.regions = check_regions(regions, int(streams), tracker is not None)
        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library (the kernel is the same in both)
        self.streams, self.tracker = int(streams), tracker
        self.device = torch.device(device if device is not None else (tracker.device if tracker is not None else "cuda"))
        if tracker is not None and tracker.id.device != torch.empty(0, device=self.device).device:
            raise ValueError(f"DeviceZones: device {self.device} but the tracker lives on {tracker.id.device}")
        self.max_tracks = tracker.config.max_tracks if tracker is not None else 1
        # the host copies stay alive: the library validates them at every update
        self.records, self.reg_first, self.verts, self.per_stream = build_tables(self.regions, self.streams)
        self.R = int(self.reg_first[-1])
        self._d_records = torch.from_numpy(self.records).to(self.device)
        self._d_reg_first = torch.from_numpy(self.reg_first).to(self.device)
        self._d_verts = torch.from_numpy(self.verts).to(self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.st_id, self.st_side = torch.zeros(self.R, self.max_tracks, **i32), torch.zeros(self.R, self.max_tracks, **i32)
        # one buffer = one copy back: in_total [R] | out_total [R] | now [R] | det_inside [B, T] | det_in [B, T] | det_out [B, T]; the totals
        # persist, the rest is written by every update; reallocated (totals carried over) when T changes
        self._io, self._T = torch.zeros(3 * self.R, **i32), 0

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _views(self) -> Dict[str, torch.Tensor]:
        R, n = self.R, self.streams * self._T
        io, shape = self._io, (self.streams, self._T)
        return dict(entered=io[:R], exited=io[R:2 * R], now=io[2 * R:3 * R], det_inside=io[3 * R:3 * R + n].view(shape),
                    det_in=io[3 * R + n:3 * R + 2 * n].view(shape), det_out=io[3 * R + 2 * n:3 * R + 3 * n].view(shape))

    def update(self, det_labels: torch.Tensor, det_boxes: torch.Tensor, det_count: torch.Tensor,
               track_ids: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One frame of every stream: the packed device results (i32 [B, T], i32 xyxy [B, T, 4], i32 [B]) and the ids the tracker gave them
        in THIS frame (i32 [B, T], -1 = none; None = occupancy only, nothing is remembered).  Returns device tensors, views of one
        buffer that the next update overwrites: ``now`` i32 [R_total], ``entered`` / ``exited`` i32 [R_total] (the running totals),
        ``det_inside`` / ``det_in`` / ``det_out`` i32 [B, T] whose bit k is the k-th region of the stream.  B must be ``streams``; T <= 1024."""
        from ._lib import check

        if det_labels.dim() != 2:
            raise ValueError(f"DeviceZones.update: det_labels must be [B, T], got {tuple(det_labels.shape)}")
        B, T = int(det_labels.shape[0]), int(det_labels.shape[1])
        if B != self.streams:
            raise ValueError(f"DeviceZones.update: a batch of {B} for zones of {self.streams} streams (batch index b is stream b)")
        if not 1 <= T <= MAX_SLOTS:
            raise ValueError(f"DeviceZones.update: T = {T} detections per stream, must be in 1..{MAX_SLOTS}")
        if track_ids is not None and self.tracker is None:
            raise ValueError("DeviceZones.update: track_ids without a tracker (pass tracker= at construction)")
        args = [("det_labels", det_labels, (B, T)), ("det_boxes", det_boxes, (B, T, 4)), ("det_count", det_count, (B,))]
        if track_ids is not None:
            args.append(("track_ids", track_ids, (B, T)))
        for name, t, shape in args:
            if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.st_id.device or not t.is_contiguous():
                raise ValueError(f"DeviceZones.update: {name} must be a contiguous torch.int32 tensor {shape} on {self.st_id.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if T != self._T:
            io = torch.zeros(3 * self.R + 3 * B * T, dtype=torch.int32, device=self.device)
            io[:2 * self.R] = self._io[:2 * self.R]
            self._io, self._T = io, T
        v = self._views()
        check(self.lib.fx_zone_update(det_labels.data_ptr(), det_boxes.data_ptr(), det_count.data_ptr(), B, T,
                                      None if track_ids is None else track_ids.data_ptr(), None if track_ids is None else self.tracker.id.data_ptr(),
                                      self.max_tracks, self._d_records.data_ptr(), self._d_reg_first.data_ptr(), self._d_verts.data_ptr(),
                                      self.records.ctypes.data, self.reg_first.ctypes.data, self.verts.ctypes.data, self.R, int(self.verts.shape[0]),
                                      self.st_id.data_ptr(), self.st_side.data_ptr(), v["entered"].data_ptr(), v["exited"].data_ptr(),
                                      v["now"].data_ptr(), v["det_inside"].data_ptr(), v["det_in"].data_ptr(), v["det_out"].data_ptr(),
                                      self._stream()), "fx_zone_update")
        return v

    def fetch(self) -> List[Dict[str, dict]]:
        """The last update on the host, in one copy: for every stream ``{name: {"kind", "count", "detections", "entered", "exited",
        "crossed_in", "crossed_out"}}`` - ``count`` / ``detections``: this frame's occupancy of a zone and the slots (= indices into the
        packed detections) inside it (0 / [] for a line); ``entered`` / ``exited``: the running totals; ``crossed_in`` / ``crossed_out``: the
        slots of this frame's events."""
        if self._T == 0:
            raise RuntimeError("DeviceZones.fetch: no update yet")
        h = self._io.cpu().numpy()
        R, B, T = self.R, self.streams, self._T
        ent, ext, now = h[:R].tolist(), h[R:2 * R].tolist(), h[2 * R:3 * R].tolist()
        masks = h[3 * R:].view(np.uint32).reshape(3, B, T)
        some = np.bitwise_or.reduce(masks, axis=2).tolist()      # [3][B]: which bits are set anywhere in the stream

        def slots(q, b, k):
            return np.nonzero((masks[q, b] >> np.uint32(k)) & np.uint32(1))[0].tolist() if (some[q][b] >> k) & 1 else []

        out = []
        for b, regs in enumerate(self.per_stream):
            r0, d = int(self.reg_first[b]), {}
            for k, reg in enumerate(regs):
                d[reg.name] = {"kind": reg.kind, "count": now[r0 + k], "detections": slots(0, b, k), "entered": ent[r0 + k], "exited": ext[r0 + k],
                               "crossed_in": slots(1, b, k), "crossed_out": slots(2, b, k)}
            out.append(d)
        return out

    def reset(self, stream: Optional[int] = None, counters: bool = True) -> None:
        """Forget the sides of every track in the regions of ``stream`` (all streams when None); with ``counters`` the running totals
        start at 0 again.  ``reset(b, counters=False)`` is what must follow ``DeviceTracker.reset(b)``: the ids start over."""
        from ._lib import check

        if stream is not None and (not _is_int(stream) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceZones.reset: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        R = self.R
        check(self.lib.fx_zone_reset(self.st_id.data_ptr(), self.st_side.data_ptr(), self._io[:R].data_ptr(), self._io[R:2 * R].data_ptr(),
                                     self.reg_first.ctypes.data, self.streams, self.max_tracks, -1 if stream is None else int(stream),
                                     1 if counters else 0, self._stream()), "fx_zone_reset")

    def state(self) -> Dict[str, np.ndarray]:
        """Host copies of the state arrays: st_id / st_side [R_total, max_tracks], in_total / out_total [R_total]."""
        R = self.R
        src = dict(st_id=self.st_id, st_side=self.st_side, in_total=self._io[:R], out_total=self._io[R:2 * R])
        return {k: src[k].cpu().numpy().copy() for k in self.STATE}


def check_dwell_names(regions: Sequence[Region], names, what: str = "DeviceDwell") -> List[str]:
    """The names of the zones whose dwell is kept (``names`` None / True: every Zone), validated on the host: each must name a Zone of
    ``regions``, once."""
    zone_names = [r.name for r in regions if isinstance(r, Zone)]
    if names is None or names is True:
        if not zone_names:
            raise ValueError(f"{what}: regions: there is no Zone to keep dwell times for (a Line has no inside)")
        return list(dict.fromkeys(zone_names))
    if isinstance(names, (str, bytes)) or not isinstance(names, (list, tuple)):
        raise ValueError(f"{what}: regions = {names!r}: must be None (every Zone) or a list of Zone names")
    out = []
    for n in names:
        if any(r.name == n and isinstance(r, Line) for r in regions) and n not in zone_names:
            raise ValueError(f"{what}: regions: {n!r} is a Line (dwell needs an inside: name a Zone)")
        if n not in zone_names:
            raise ValueError(f"{what}: regions: there is no Zone named {n!r}")
        if n in out:
            raise ValueError(f"{what}: regions: {n!r} is named twice")
        out.append(n)
    if not out:
        raise ValueError(f"{what}: regions is empty")
    return out


def check_fps(fps, what: str = "DeviceDwell") -> Optional[float]:
    if fps is None:
        return None
    if isinstance(fps, bool) or not isinstance(fps, (int, float, np.integer, np.floating)) or not fps > 0 or not np.isfinite(fps):
        raise ValueError(f"{what}: fps = {fps!r}: must be None or a positive number (frames per second of every stream)")
    return float(fps)


def build_dwell_tables(per_stream: Sequence[Sequence[Region]], reg_first: np.ndarray, names: Sequence[str]):
    """The host tables of ``fx_dwell_update``: (dw_first int32 [streams + 1], dw_region int32 [D_total], dw_bit int32 [D_total], rows = for
    every stream the [(name, bit)] of its dwell rows in bit order)."""
    first, region, bit, rows = [0], [], [], []
    for b, regs in enumerate(per_stream):
        mine = [(r.name, k) for k, r in enumerate(regs) if isinstance(r, Zone) and r.name in names]
        rows.append(mine)
        region.extend(int(reg_first[b]) + k for _, k in mine)
        bit.extend(k for _, k in mine)
        first.append(len(bit))
    return np.asarray(first, np.int32), np.asarray(region, np.int32), np.asarray(bit, np.int32), rows


class DeviceDwell:
    """How long every track has been inside the zones ``regions`` (names; None = every ``Zone``) of ``zones``, and per zone the finished
    visits, their total and their longest, in frames: one ``fx_dwell_update`` launch right after ``zones.update`` (csrc/dwell_ops.hip, the
    contract is in include/focoos_amd.h).  Needs ``zones.tracker``: a visit belongs to a track.  A visit lasts from
    its first to its last inside observation, inclusive; a frame in which the track is not detected does not end it.  ``fps`` (constant,
    the same for every stream) adds the seconds.  The state belongs to this object and outlives the ``infer_stream`` calls it is passed to;
    ``reset(b, totals=False)`` must follow ``DeviceTracker.reset(b)``."""

    STATE = ("dw_id", "dw_enter", "dw_last", "visits", "dwell_sum", "dwell_max", "frame")

    def __init__(self, zones: DeviceZones, regions: Optional[Sequence[str]] = None, fps: Optional[float] = None):
        if not isinstance(zones, DeviceZones):
            raise TypeError(f"DeviceDwell: zones must be a DeviceZones, not {type(zones).__name__}")
        if zones.tracker is None:
            raise ValueError("DeviceDwell: zones.tracker is None: dwell times belong to tracks (build the DeviceZones with tracker=)")
        self.names = check_dwell_names(zones.regions, regions)
        self.fps = check_fps(fps)
        self.zones, self.lib, self.device = zones, zones.lib, zones.device
        self.streams, self.max_tracks = zones.streams, zones.max_tracks
        # the host copies stay alive: the library validates them at every update
        self.dw_first, self.dw_region, self.dw_bit, self.rows = build_dwell_tables(zones.per_stream, zones.reg_first, self.names)
        self.D = int(self.dw_first[-1])
        self._d_first, self._d_bit = torch.from_numpy(self.dw_first).to(self.device), torch.from_numpy(self.dw_bit).to(self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        D, M = self.D, self.max_tracks
        self.dw_id, self.dw_enter, self.dw_last = torch.zeros(D, M, **i32), torch.zeros(D, M, **i32), torch.zeros(D, M, **i32)
        self.frame = torch.zeros(self.streams, **i32)
        # one buffer = one copy back: dwell_sum [D] as int64 (2 D words, first: 8-byte aligned) | visits [D] | dwell_max [D] | det_dwell [D, T];
        # the totals persist, det_dwell is written by every update; reallocated (totals carried over) when T changes
        self._io, self._T = torch.zeros(4 * D, **i32), 0

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _views(self) -> Dict[str, torch.Tensor]:
        D, io = self.D, self._io
        return dict(dwell_sum=io[:2 * D].view(torch.int64), visits=io[2 * D:3 * D], dwell_max=io[3 * D:4 * D], det_dwell=io[4 * D:].view(D, self._T))

    def update(self, det_count: torch.Tensor, track_ids: torch.Tensor, det_inside: torch.Tensor) -> torch.Tensor:
        """One frame of every stream: ``det_count`` i32 [B], the ids the tracker gave THIS frame's detections (i32 [B, T]) and the
        ``det_inside`` masks ``zones.update`` returned for it (i32 [B, T]).  Returns ``det_dwell`` i32 [D_total, T] on the device (a view the
        next update overwrites): the frames the track of detection j has been in the zone of row d, 0 when it is not tracked or not inside."""
        from ._lib import check

        if track_ids is None or track_ids.dim() != 2:
            raise ValueError("DeviceDwell.update: track_ids must be the tracker's ids of this frame, [B, T]")
        B, T = int(track_ids.shape[0]), int(track_ids.shape[1])
        if B != self.streams:
            raise ValueError(f"DeviceDwell.update: a batch of {B} for dwell times of {self.streams} streams (batch index b is stream b)")
        if not 1 <= T <= MAX_SLOTS:
            raise ValueError(f"DeviceDwell.update: T = {T} detections per stream, must be in 1..{MAX_SLOTS}")
        for name, t, shape in (("det_count", det_count, (B,)), ("track_ids", track_ids, (B, T)), ("det_inside", det_inside, (B, T))):
            if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.dw_id.device or not t.is_contiguous():
                raise ValueError(f"DeviceDwell.update: {name} must be a contiguous torch.int32 tensor {shape} on {self.dw_id.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if T != self._T:
            io = torch.zeros(4 * self.D + self.D * T, dtype=torch.int32, device=self.device)
            io[:4 * self.D] = self._io[:4 * self.D]
            self._io, self._T = io, T
        v = self._views()
        check(self.lib.fx_dwell_update(det_count.data_ptr(), track_ids.data_ptr(), det_inside.data_ptr(), B, T, self.zones.tracker.id.data_ptr(),
                                       self.max_tracks, self._d_first.data_ptr(), self._d_bit.data_ptr(), self.dw_first.ctypes.data,
                                       self.dw_region.ctypes.data, self.dw_bit.ctypes.data, self.zones.reg_first.ctypes.data, self.D,
                                       self.dw_id.data_ptr(), self.dw_enter.data_ptr(), self.dw_last.data_ptr(), v["visits"].data_ptr(),
                                       v["dwell_sum"].data_ptr(), v["dwell_max"].data_ptr(), self.frame.data_ptr(), v["det_dwell"].data_ptr(),
                                       self._stream()), "fx_dwell_update")
        return v["det_dwell"]

    def fetch(self, zone_dicts: Optional[List[Dict[str, dict]]] = None) -> List[Dict[str, dict]]:
        """The last update on the host, in one copy, merged into ``zone_dicts`` (what ``zones.fetch()`` returned for the same frame; fetched
        when None) and returned: the dict of every dwell zone gets ``dwell`` (frames, aligned with its ``detections``; 0 for an untracked
        detection), ``visits`` / ``dwell_total`` / ``dwell_max`` (finished visits so far, in frames), ``dwell_mean`` = dwell_total / visits
        (0.0 without a visit) and, with ``fps``, ``dwell_seconds`` (``dwell`` divided by fps)."""
        if self._T == 0:
            raise RuntimeError("DeviceDwell.fetch: no update yet")
        if zone_dicts is None:
            zone_dicts = self.zones.fetch()
        h = self._io.cpu().numpy()
        D = self.D
        total = h[:2 * D].view(np.int64).tolist()
        visits, longest = h[2 * D:3 * D].tolist(), h[3 * D:4 * D].tolist()
        det = h[4 * D:].reshape(D, self._T)
        for b, rows in enumerate(self.rows):
            d0 = int(self.dw_first[b])
            for i, (name, _) in enumerate(rows):
                d, z = d0 + i, zone_dicts[b][name]
                z["dwell"] = det[d, z["detections"]].tolist() if z["detections"] else []
                z["visits"], z["dwell_total"], z["dwell_max"] = visits[d], total[d], longest[d]
                z["dwell_mean"] = total[d] / visits[d] if visits[d] else 0.0
                if self.fps is not None:
                    z["dwell_seconds"] = [n / self.fps for n in z["dwell"]]
        return zone_dicts

    def reset(self, stream: Optional[int] = None, totals: bool = True) -> None:
        """Forget the visits in progress of ``stream`` (all streams when None) and start its frame count again; with ``totals`` the
        visits, their total and their longest start at 0 again.  ``reset(b, totals=False)`` is what must follow ``DeviceTracker.reset(b)``."""
        from ._lib import check

        if stream is not None and (not _is_int(stream) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceDwell.reset: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        v = self._views()
        check(self.lib.fx_dwell_reset(self.dw_id.data_ptr(), self.dw_enter.data_ptr(), self.dw_last.data_ptr(), v["visits"].data_ptr(),
                                      v["dwell_sum"].data_ptr(), v["dwell_max"].data_ptr(), self.frame.data_ptr(), self.dw_first.ctypes.data,
                                      self.streams, self.max_tracks, -1 if stream is None else int(stream), 1 if totals else 0, self._stream()),
              "fx_dwell_reset")

    def state(self) -> Dict[str, np.ndarray]:
        """Host copies of the state arrays: dw_id / dw_enter / dw_last [D_total, max_tracks], visits / dwell_max int32 and dwell_sum int64
        [D_total], frame [streams]."""
        v = self._views()
        src = dict(dw_id=self.dw_id, dw_enter=self.dw_enter, dw_last=self.dw_last, visits=v["visits"], dwell_sum=v["dwell_sum"],
                   dwell_max=v["dwell_max"], frame=self.frame)
        return {k: src[k].cpu().numpy().copy() for k in self.STATE}


def resolve_dwell(dwell, zones, track, family: str, what: str = "infer_stream", device_only: bool = False):
    """What ``dwell=`` means, decided on the host before anything touches the GPU (after ``resolve``): None / False -> None; True, a list of
    Zone names or a DeviceDwell need ``zones=`` and a tracker.  Returns None, the DeviceDwell, or (names, None) to build with the first batch.
    ``device_only`` (infer_batch): a DeviceDwell or nothing."""
    if dwell is None or dwell is False:
        return None
    check_family(family, what)
    if zones is None:
        raise ValueError(f"{what}: dwell= needs zones= (dwell times are kept per Zone)")
    if isinstance(dwell, DeviceDwell):
        if dwell.zones is not zones:
            raise ValueError(f"{what}: dwell: the DeviceDwell was built for another DeviceZones: pass that one as zones=")
        return dwell
    if device_only:
        raise TypeError(f"{what}: dwell must be a DeviceDwell, not {type(dwell).__name__}")
    if track is None or (isinstance(zones, DeviceZones) and zones.tracker is None):
        raise ValueError(f"{what}: dwell= needs track= (dwell times belong to tracks; a DeviceZones passed as zones= must be built on a tracker)")
    regions = zones.regions if isinstance(zones, DeviceZones) else zones
    return check_dwell_names(regions, None if dwell is True else dwell, f"{what}: dwell"), None


def check_detections_flag(detections: bool, zones, annotate: bool, mask_format: str, what: str = "infer_stream") -> None:
    """``detections=False`` is the analytics-only mode: it needs zones and hands out neither pictures nor masks."""
    if detections:
        return
    if zones is None:
        raise ValueError(f"{what}: detections=False needs zones= (there would be nothing to return)")
    if annotate:
        raise ValueError(f"{what}: detections=False cannot be combined with annotate=True (nothing to draw)")
    if mask_format != "png":
        raise ValueError(f"{what}: detections=False cannot be combined with mask_format={mask_format!r} (no masks are returned)")


def resolve(zones, track, family: str, what: str = "infer_stream", device_only: bool = False):
    """What ``zones=`` means, decided on the host before anything touches the GPU: returns (zones, track).  None -> no zones; a list of
    Zone / Line -> validated, the DeviceZones is created with the first batch (a Line without ``track`` is a ValueError); a DeviceZones ->
    itself, and its tracker is the one that runs (``track`` must be None or that tracker).  ``device_only`` (infer_batch): a DeviceZones
    or nothing."""
    if zones is None:
        return None, track
    check_family(family, what)
    if device_only and not isinstance(zones, DeviceZones):
        raise TypeError(f"{what}: zones must be a DeviceZones, not {type(zones).__name__}")
    if isinstance(zones, DeviceZones):
        if zones.tracker is not None:
            if track is not None and track is not zones.tracker:
                raise ValueError(f"{what}: the DeviceZones was built for another tracker: pass that tracker, or leave track / tracker unset")
            track = zones.tracker
        return zones, track
    return check_regions(zones, None, track is not None, what), track


def for_batch(zones, B: int, tracker: Optional[DeviceTracker], device, what: str = "infer_stream") -> DeviceZones:
    """The DeviceZones of a batch of B: created from the list with the first batch, which fixes B; another size is a ValueError."""
    if not isinstance(zones, DeviceZones):
        return DeviceZones(B, zones, tracker, device)
    if zones.streams != B:
        raise ValueError(f"{what}: a batch of {B} images for zones of {zones.streams} streams (batch index b is stream b)")
    return zones


def attach(out: List, per_stream: List[Dict[str, dict]]) -> None:
    for o, z in zip(out, per_stream):
        o.zones = z
