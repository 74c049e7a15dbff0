"""Drawing the detections on the frame on the device (``FocoosModel.infer(image, annotate=True)``).

The reference draws with ``supervision`` + ``cv2`` on the host (focoos/utils/vision.py:437-488).  Here the packed device results and the
bit-packed masks never leave the GPU: ``fx_annotate_labels_from_detections`` turns them into label records ("name: NN%", rectangle, colour)
and ``fx_annotate_u8`` draws outlines, half-opacity masks and the labels in one pass over the uint8 frames (csrc/annotate.hip; the contract
is in include/focoos_amd.h).  What is mirrored from the reference is the layer order (outlines, masks, labels), the palette and the class
colouring, the half-opacity masks with the smaller instance on top and the label text; pixel equality with supervision / cv2 is NOT claimed
(a bitmap font in a fixed cell, square label corners).  Keypoints are out of scope.

``annotate=Overlay(ids, zones, traces)`` in ``infer_stream`` / ``infer_batch`` adds the analytics half of the picture from
what is already on the device when a lane finishes: "#17 " in front of a tracked label (``fx_annotate_labels_tracked``), the regions of a
``DeviceZones`` tinted and outlined and its lines stroked, a tail of the last N anchors behind every track (``DeviceTraces``, ``fx_trace_update``;
all three in one geometry pass, ``fx_annotate_overlay_u8``) and "door: 3" / "gate: 12/9" at every region (``fx_annotate_zone_records``, drawn by
``fx_annotate_u8``).  csrc/overlay.hip; tests/overlay_ref.py restates the contracts.  ``Overlay(heat=True)`` puts the call's heat map
underneath all of it (heat.py, ``fx_annotate_heat_u8``).  ``Overlay(redact=Redact(...))`` makes the selected
objects unreadable first, under every other layer: their boxes, and the predicted boxes of tracks the detector has just missed, are
pixelated, blurred or filled from the packed results and the tracker's slots (``fx_redact_regions``, ``fx_redact_u8``, csrc/redact.hip,
DESIGN.md section 26; tests/redact_ref.py restates the contracts), and ``draw=False`` leaves the boxes, masks and labels out.
``annotate=True`` draws exactly what it always drew."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

LNAME = 24      # include/focoos_amd.h FX_ANN_LNAME
LMAX = 32       # FX_ANN_LMAX
GLYPHS = 95     # FX_ANN_GLYPHS: ASCII 32..126
MAX_SLOTS = 1024
FLAG_BOXES, FLAG_MASKS, FLAG_LABELS = 1, 2, 4
RNAME = 16      # FX_OVL_RNAME: glyphs of a region name
MAX_TRACE = 64  # FX_TRACE_MAX_LEN: points kept per track
OVL_FILL, OVL_STROKE, OVL_TRACES = 1, 2, 4
REDACT_MODES = {"pixelate": 0, "blur": 1, "fill": 2}      # FX_REDACT_PIXELATE / _BLUR / _FILL
REDACT_SHAPES = {"box": 0, "ellipse": 1, "mask": 2}       # FX_REDACT_BOX / _ELLIPSE / _MASK
REDACT_CELLS = (4, 8, 16, 32, 64)
REDACT_MAX_RADIUS = 32    # FX_REDACT_MAX_RADIUS
REDACT_MAX_HOLD = 1024    # FX_REDACT_MAX_HOLD
MASK_FAMILIES = ("fai_mf", "bisenetformer")
FOCOOS_PALETTE = ("#015fe6", "#3faebd", "#63dba6", "#a151ff", "#df923a")
# ctypes-free mirror of fx_annotate_record (56 bytes)
REC_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("colour", "<u4"), ("nchar", "<i4"), ("glyph", "u1", (LMAX,))])
TASK_FLAGS = {"detection": FLAG_BOXES, "instseg": FLAG_BOXES | FLAG_MASKS, "semseg": FLAG_MASKS, "classification": 0}

_ATLAS: list = []


def scale_for(H: int, W: int) -> int:
    """Integer drawing scale of an H x W frame: 1 up to 809 pixels on the short side, then one more per 540, at most 4."""
    return max(1, min(4, (min(int(H), int(W)) + 270) // 540))


def palette_colour(i: int) -> int:
    """FOCOOS_PALETTE[i mod 5] as R | G << 8 | B << 16."""
    h = FOCOOS_PALETTE[int(i) % len(FOCOOS_PALETTE)].lstrip("#")
    return int(h[0:2], 16) | (int(h[2:4], 16) << 8) | (int(h[4:6], 16) << 16)


def glyph_atlas() -> Tuple[np.ndarray, int, int]:
    """(atlas uint32 [95, gh], gw, gh): ASCII 32..126 rasterised with Pillow's default font (nominal size 16 where the installed Pillow
    takes one), thresholded at 128, each glyph in the top-left corner of one fixed cell; bit x of row word y = pixel (x, y).  Built once per
    process.  Labels need Pillow; boxes and masks do not."""
    if _ATLAS:
        return _ATLAS[0]
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError as e:
        raise ImportError("focoos_amd.annotate: drawing labels needs Pillow (PIL) to rasterise the glyph atlas; install it or annotate "
                          "with labels=False") from e
    try:
        font = ImageFont.load_default(16)
    except TypeError:          # Pillow < 10.1: the fixed bitmap font
        font = ImageFont.load_default()
    side = 64
    bits = np.zeros((GLYPHS, side, side), dtype=bool)
    for g in range(GLYPHS):
        img = Image.new("L", (side, side), 0)
        ImageDraw.Draw(img).text((0, 0), chr(32 + g), fill=255, font=font)
        bits[g] = np.asarray(img) >= 128
    rows, cols = np.nonzero(bits.any(0).any(1))[0], np.nonzero(bits.any(0).any(0))[0]
    top, bottom, right = int(rows.min()), int(rows.max()), int(cols.max())
    gh, gw = min(32, bottom - top + 1), min(32, right + 2)          # one blank column between neighbours
    cell = bits[:, top:top + gh, :gw]
    atlas = (cell.astype(np.uint64) << np.arange(gw, dtype=np.uint64)).sum(-1).astype(np.uint32)
    _ATLAS.append((np.ascontiguousarray(atlas), gw, gh))
    return _ATLAS[0]


def encode_text(text: str) -> List[int]:
    """Glyph indices (ASCII code - 32) of ``text``; a character outside ASCII 32..126 becomes '?'."""
    return [(ord(c) - 32) if 32 <= ord(c) <= 126 else ord("?") - 32 for c in text]


def name_table(classes: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """The class names as the records kernel reads them: glyph indices uint8 [K, LNAME] (truncated) and lengths int32 [K]."""
    K = len(classes)
    tab, ln = np.zeros((max(K, 1), LNAME), dtype=np.uint8), np.zeros(max(K, 1), dtype=np.int32)
    for k, name in enumerate(classes):
        g = encode_text(str(name))[:LNAME]
        tab[k, :len(g)], ln[k] = g, len(g)
    return tab, ln


def percent(conf: float) -> int:
    """min(100, int(fp32(fp32(conf * 100) + 0.5))): the records kernel's arithmetic in numpy float32."""
    p = np.float32(np.float32(conf) * np.float32(100.0)) + np.float32(0.5)
    return 100 if p >= 100 else (int(p) if p >= 0 else 0)


def classification_records(lines: Sequence[Sequence[Tuple[str, float]]], T: int, s: int, gw: int, gh: int) -> np.ndarray:
    """Host-built records [B, T] of the classification overlay: per image the (label, confidence) lines sorted by confidence descending,
    stacked from (pad, pad) downwards, line i in FOCOOS_PALETTE[i mod 5] (draw_classification_labels' list, vision.py:405-407)."""
    rec = np.zeros((len(lines), T), dtype=REC_DTYPE)
    pad = 2 * s
    h = gh * s + 2 * pad
    for b, ls in enumerate(lines):
        for i, (label, conf) in enumerate(sorted(ls, key=lambda lc: -lc[1])[:T]):
            g = encode_text(str(label))[:LNAME] + encode_text(f": {percent(conf)}%")
            r = rec[b, i]
            r["x0"], r["y0"], r["w"], r["h"] = pad, pad + i * h, len(g) * gw * s + 2 * pad, h
            r["colour"], r["nchar"] = palette_colour(i), len(g)
            r["glyph"][:len(g)] = g
    return rec


class DeviceTraces:
    """The ring of the last ``length`` anchors (bottom centre of the box, doubled pixels) of every slot of ``tracker``, on the device: what
    ``Overlay(traces=...)`` draws as the tail behind a tracked object.  ``update`` is one launch right after the
    tracker's; the state belongs to this object and outlives the ``infer_stream`` calls it is passed to through ``Overlay(traces=this)``.
    After ``DeviceTracker.reset(b)`` the ids of stream b start over: ``reset(b)`` must follow it."""

    STATE = ("id", "label", "len", "head", "xy")

    def __init__(self, tracker, length: int, device=None):
        from .tracking import DeviceTracker

        if not isinstance(tracker, DeviceTracker):
            raise TypeError(f"DeviceTraces: tracker must be a DeviceTracker, not {type(tracker).__name__}")
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not 1 <= length <= MAX_TRACE:
            raise ValueError(f"DeviceTraces: length = {length!r} must be an integer in 1..{MAX_TRACE}")
        self.tracker, self.length = tracker, int(length)
        self.device = torch.device(device if device is not None else tracker.device)
        if tracker.id.device != torch.empty(0, device=self.device).device:
            raise ValueError(f"DeviceTraces: device {self.device} but the tracker lives on {tracker.id.device}")
        self.lib = tracker.lib
        self.streams, self.max_tracks = tracker.streams, tracker.config.max_tracks
        i32 = dict(dtype=torch.int32, device=self.device)
        B, M = self.streams, self.max_tracks
        self.id, self.label = torch.zeros(B, M, **i32), torch.zeros(B, M, **i32)
        self.len, self.head = torch.zeros(B, M, **i32), torch.zeros(B, M, **i32)
        self.xy = torch.zeros(B, M, self.length, 2, **i32)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _state_ptrs(self):
        return self.id.data_ptr(), self.label.data_ptr(), self.len.data_ptr(), self.head.data_ptr()

    def update(self, det_labels: torch.Tensor, det_boxes: torch.Tensor, det_count: torch.Tensor, track_ids: torch.Tensor) -> None:
        """One frame of every stream: the packed device results and the ids the tracker gave them in THIS frame (i32 [B, T])."""
        from ._lib import check

        B, T = self.streams, int(det_labels.shape[-1])
        for name, t, shape in (("det_labels", det_labels, (B, T)), ("det_boxes", det_boxes, (B, T, 4)), ("det_count", det_count, (B,)),
                               ("track_ids", track_ids, (B, T))):
            if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != self.id.device or not t.is_contiguous():
                raise ValueError(f"DeviceTraces.update: {name} must be a contiguous torch.int32 tensor {shape} on {self.id.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        check(self.lib.fx_trace_update(det_labels.data_ptr(), det_boxes.data_ptr(), det_count.data_ptr(), B, T, track_ids.data_ptr(),
                                       self.tracker.id.data_ptr(), self.max_tracks, self.length, *self._state_ptrs(), self.xy.data_ptr(),
                                       self._stream()), "fx_trace_update")

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget the traces of ``stream`` (all streams when None)."""
        from ._lib import check

        if stream is not None and (isinstance(stream, bool) or not isinstance(stream, (int, np.integer)) or not 0 <= stream < self.streams):
            raise ValueError(f"DeviceTraces.reset: stream = {stream!r} must be in 0..{self.streams - 1} or None")
        check(self.lib.fx_trace_reset(*self._state_ptrs(), self.streams, self.max_tracks, -1 if stream is None else int(stream), self._stream()),
              "fx_trace_reset")

    def state(self) -> Dict[str, np.ndarray]:
        """Host copies of the state arrays: id / label / len / head [streams, max_tracks], xy [streams, max_tracks, length, 2]."""
        src = dict(id=self.id, label=self.label, len=self.len, head=self.head, xy=self.xy)
        return {k: src[k].cpu().numpy().copy() for k in self.STATE}


@dataclass(frozen=True)
class Redact:
    """What ``Overlay(redact=...)`` makes unreadable before anything is drawn.  ``classes``: class names or ids,
    None = every class (resolved against the model's classes when the call starts; an unknown name raises ValueError); ``mode``:
    "pixelate" (the mean of the pixel's ``cell`` x ``cell`` cell, grid anchored at the frame origin), "blur" (the mean of the
    (2 ``radius`` + 1)^2 window) or "fill" (``colour``, RGB); ``shape``: "box", "ellipse" (inscribed in the box) or "mask" (the
    instance's own pixels, mask families only); ``pad``: the box grows by this fraction of its width and height on every side; ``top``:
    only the upper fraction of the box is covered (a person detector then hides heads); ``hold``: also cover the predicted boxes of
    tracks of the selected classes that have gone undetected for 1 .. ``hold`` frames (needs a tracker).  Validated at construction:
    ValueError names the field."""
    classes: Optional[Sequence[Union[str, int]]] = None
    mode: str = "pixelate"
    cell: int = 16
    radius: int = 16
    colour: Tuple[int, int, int] = (0, 0, 0)
    shape: str = "box"
    pad: float = 0.0
    top: float = 1.0
    hold: int = 0

    def __post_init__(self):
        def bad(name, why):
            raise ValueError(f"Redact.{name} = {getattr(self, name)!r}: {why}")

        def integer(v):
            return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))

        c = self.classes
        if c is not None:
            if isinstance(c, (str, bytes)) or not isinstance(c, (list, tuple)) or not c:
                bad("classes", "must be None or a non-empty list of class names or ids")
            for v in c:
                if not (isinstance(v, str) or (integer(v) and v >= 0)):
                    bad("classes", "every entry must be a class name or an id >= 0")
            object.__setattr__(self, "classes", tuple(v if isinstance(v, str) else int(v) for v in c))
        if self.mode not in REDACT_MODES:
            bad("mode", f"must be one of {', '.join(REDACT_MODES)}")
        if not integer(self.cell) or self.cell not in REDACT_CELLS:
            bad("cell", f"must be one of {', '.join(str(v) for v in REDACT_CELLS)}")
        if not integer(self.radius) or not 1 <= self.radius <= REDACT_MAX_RADIUS:
            bad("radius", f"must be an integer in 1..{REDACT_MAX_RADIUS}")
        col = self.colour
        if not isinstance(col, (list, tuple)) or len(col) != 3 or not all(integer(v) and 0 <= v <= 255 for v in col):
            bad("colour", "must be three integers (R, G, B) in 0..255")
        object.__setattr__(self, "colour", tuple(int(v) for v in col))
        if self.shape not in REDACT_SHAPES:
            bad("shape", f"must be one of {', '.join(REDACT_SHAPES)}")
        for name, lo_open in (("pad", False), ("top", True)):
            v = getattr(self, name)
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                bad(name, "must be a finite number")
            if not (0 < v <= 1 if lo_open else 0 <= v <= 1):
                bad(name, "must be in (0, 1]" if lo_open else "must be in [0, 1]")
        if not integer(self.hold) or not 0 <= self.hold <= REDACT_MAX_HOLD:
            bad("hold", f"must be an integer in 0..{REDACT_MAX_HOLD}")

    @property
    def pad256(self) -> int:
        """``pad`` as the kernel takes it: round(pad * 256), 0 .. 256."""
        return int(round(float(self.pad) * 256))

    @property
    def top256(self) -> int:
        """``top`` as the kernel takes it: max(1, round(top * 256)), 1 .. 256."""
        return max(1, int(round(float(self.top) * 256)))

    @property
    def colour_word(self) -> int:
        return self.colour[0] | (self.colour[1] << 8) | (self.colour[2] << 16)

    def class_ids(self, classes: Sequence[str]) -> Optional[List[int]]:
        """The ids of ``classes`` (the model's names) this object selects, None for every class; an unknown name or an id past the last
        class raises ValueError and names it."""
        if self.classes is None:
            return None
        names = [str(n) for n in classes or []]
        ids = []
        for v in self.classes:
            if isinstance(v, str):
                if v not in names:
                    raise ValueError(f"Redact.classes: unknown class name {v!r} (the model has {len(names)} classes)")
                ids.append(names.index(v))
            else:
                if v >= len(names):
                    raise ValueError(f"Redact.classes: class id {v} is not in 0..{len(names) - 1}")
                ids.append(v)
        return sorted(set(ids))


def class_words(ids: Sequence[int], K: int) -> np.ndarray:
    """The class bitmap fx_redact_regions reads: uint32 [ceil(K / 32)], bit l & 31 of word l >> 5 set for every id l."""
    w = np.zeros(max(1, (int(K) + 31) // 32), dtype=np.uint32)
    for l in ids:
        w[l >> 5] |= np.uint32(1 << (l & 31))
    return w


@dataclass(frozen=True)
class Overlay:
    """What ``annotate=`` draws beyond ``True`` (boxes, masks, "name: NN%") in ``infer_stream`` / ``infer_batch``: ``ids`` - "#17 " in front
    of the label of a tracked detection; ``zones`` - the regions tinted and outlined, the lines stroked, "door: 3" / "gate: 12/9" at each
    region's first vertex; ``traces`` - the last N (0..64, 0 = off) anchors of every track joined into a tail, or a ``DeviceTraces`` whose
    state then outlives the call; ``heat`` - the heat map of ``heatmap=`` blended in above the redaction and below the rest (heat.py);
    ``redact`` - a ``Redact``: the selected objects are made unreadable first, under every other layer; ``draw`` - False leaves out the
    box outlines, the mask tints and the "name: NN%" labels (``Overlay(ids=False, zones=False, redact=Redact(...), draw=False)`` is the
    anonymised frame alone).  Validated at construction: ValueError names the field."""
    ids: bool = True
    zones: bool = True
    traces: Union[int, DeviceTraces] = 0
    heat: bool = False
    redact: Optional[Redact] = None
    draw: bool = True

    def __post_init__(self):
        if self.redact is not None and not isinstance(self.redact, Redact):
            raise ValueError(f"Overlay.redact = {self.redact!r}: must be None or a Redact")
        for f in ("ids", "zones", "heat", "draw"):
            if not isinstance(getattr(self, f), (bool, np.bool_)):
                raise ValueError(f"Overlay.{f} = {getattr(self, f)!r}: must be True or False")
        t = self.traces
        if not isinstance(t, DeviceTraces) and (isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t <= MAX_TRACE):
            raise ValueError(f"Overlay.traces = {t!r}: must be an integer in 0..{MAX_TRACE} (points kept per track, 0 = off) or a DeviceTraces")

    @property
    def traced(self) -> bool:
        return isinstance(self.traces, DeviceTraces) or self.traces > 0


def check_overlay(annotate, tracked: bool, zoned: bool, family: str, what: str = "infer_stream", heated: bool = False,
                  fm=None, device_only: bool = False) -> Optional[Overlay]:
    """The Overlay of ``annotate=`` (None for True / False), refused on the host, by field, when the call has nothing to draw it from.
    ``fm``: the model, whose class names ``Overlay.redact.classes`` is resolved against.  ``device_only`` (infer_batch, one batch per
    call): the traces must be a DeviceTraces."""
    if not isinstance(annotate, Overlay):
        return None
    if family == "fai_cls":
        raise NotImplementedError(f"{what}: annotate=Overlay(...) draws ids, zones and traces of boxes; model family 'fai_cls' has none")
    if annotate.ids and not tracked:
        raise ValueError(f"{what}: Overlay.ids = True needs a tracker (pass track= / tracker=, or Overlay(ids=False))")
    if annotate.traced and not tracked:
        raise ValueError(f"{what}: Overlay.traces = {annotate.traces!r} needs a tracker (pass track= / tracker=)")
    if annotate.zones and not zoned:
        raise ValueError(f"{what}: Overlay.zones = True needs zones= (or Overlay(zones=False))")
    if annotate.heat and not heated:
        raise ValueError(f"{what}: Overlay.heat = True needs heatmap= (there is no heat map to draw)")
    if device_only and annotate.traced and not isinstance(annotate.traces, DeviceTraces):
        raise ValueError(f"{what}: Overlay.traces = {annotate.traces!r} would start a new trace with every call: pass a DeviceTraces")
    red = annotate.redact
    if red is not None:
        if red.hold > 0 and not tracked:
            raise ValueError(f"{what}: Redact.hold = {red.hold} covers the predicted boxes of missed tracks: it needs a tracker (pass track= / "
                             f"tracker=, or Redact(hold=0))")
        if red.shape == "mask" and family not in MASK_FAMILIES:
            raise NotImplementedError(f"{what}: Redact.shape = 'mask' covers an instance's own pixels; model family {family!r} packs no masks "
                                      f"(supported: {', '.join(MASK_FAMILIES)})")
        if fm is not None:
            red.class_ids(fm.model_info.classes)      # an unknown name is a ValueError now, not at the first batch
    return annotate


def refuse_overlay(annotate, what: str) -> None:
    """``infer`` and ``infer_tiled`` see one picture: no stream, no identity, nothing an Overlay could draw."""
    if isinstance(annotate, Overlay):
        raise ValueError(f"{what}: annotate=Overlay(...) needs a stream identity: use infer_stream or infer_batch ({what} takes annotate=True)")


def traces_for_batch(overlay: Overlay, tracker, what: str = "infer_stream") -> Optional[DeviceTraces]:
    """The DeviceTraces of a call: created for ``tracker`` with the first batch from ``Overlay(traces=N)``, or the caller's own."""
    t = overlay.traces
    if isinstance(t, DeviceTraces):
        if t.tracker is not tracker:
            raise ValueError(f"{what}: Overlay.traces was built for another tracker: pass that tracker as track= / tracker=")
        return t
    return DeviceTraces(tracker, int(t)) if t > 0 else None


@dataclass
class OverlayPass:
    """What one batch's drawing reads beyond the packed results: the Overlay, the ids of this frame and the device state objects."""
    overlay: Overlay
    ids: Optional[torch.Tensor] = None
    zones: Optional[object] = None       # zones.DeviceZones, when Overlay.zones
    traces: Optional[DeviceTraces] = None
    heat: Optional[object] = None        # heat.DeviceHeatmap, when Overlay.heat
    tracker: Optional[object] = None     # tracking.DeviceTracker, when Overlay.redact.hold > 0


def region_name_table(names: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """Region names as the zone-records kernel reads them: glyph indices uint8 [R, RNAME] (truncated) and lengths int32 [R]."""
    tab, ln = np.zeros((max(len(names), 1), RNAME), dtype=np.uint8), np.zeros(max(len(names), 1), dtype=np.int32)
    for k, name in enumerate(names):
        g = encode_text(str(name))[:RNAME]
        tab[k, :len(g)], ln[k] = g, len(g)
    return tab, ln


def check_inputs(inputs, what: str = "infer_batch") -> None:
    """ValueError for anything ``annotate=True`` cannot draw on (only uint8 RGB pictures; float frames are out of scope).  Host only."""
    for i, im in enumerate(inputs if isinstance(inputs, list) else [inputs]):
        dt = getattr(im, "dtype", None)
        if dt is not None and dt not in (np.uint8, torch.uint8):
            raise ValueError(f"{what}(annotate=True) draws on uint8 RGB images: input {i} is {dt}")


class DeviceAnnotator:
    """The device side of ``annotate=True`` for one model: uploads the glyph atlas and the class-name table once, then draws on device
    frames with the two kernels on the current stream.  ``task``: detection (outlines + labels), instseg (outlines, masks, labels),
    semseg (masks + labels, no outlines, as annotate_image), classification (host-built label lines).  ``labels=False`` needs no Pillow."""

    def __init__(self, classes: Sequence[str], task: str, device, labels: bool = True):
        from ._lib import load

        if task not in TASK_FLAGS:
            raise ValueError(f"DeviceAnnotator: unknown task {task!r} (one of {sorted(TASK_FLAGS)})")
        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
        self.device = torch.device(device)
        self.task, self.classes = task, list(classes or [])
        self.flags = TASK_FLAGS[task] | (FLAG_LABELS if labels else 0)
        self.gw = self.gh = 1
        self.atlas = self.names = self.name_len = None
        self._redact_words: dict = {}     # Redact -> its class bitmap on the device (None: every class)
        self._redact_regions: dict = {}   # (rows, R) -> regions, region_slot, region_count
        self._redact_scratch: dict = {}   # frame shape -> the frame blur writes into
        if labels:
            atlas, self.gw, self.gh = glyph_atlas()
            tab, ln = name_table(self.classes)
            self.atlas = torch.from_numpy(atlas.view(np.int32)).to(self.device)
            self.names, self.name_len = torch.from_numpy(tab).to(self.device), torch.from_numpy(ln).to(self.device)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check_frames(self, frames: torch.Tensor) -> None:
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_contiguous()):
            raise ValueError("DeviceAnnotator takes contiguous device uint8 frames [B, H, W, 3]")

    def records(self, results, b0: int, B: int, H: int, W: int, s: int, rec: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fx_annotate_labels_from_detections for images b0 .. b0+B-1 of ``results`` at frame size (H, W): returns the record buffer
        (uint8 [rows of results, T, 56]; only those images' rows are written)."""
        from ._lib import check

        T = int(results.det_scores.shape[1])
        if rec is None:
            rec = torch.zeros(int(results.det_count.shape[0]), T, REC_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        check(self.lib.fx_annotate_labels_from_detections(
            results.det_scores.data_ptr() + 4 * b0 * T, results.det_labels.data_ptr() + 4 * b0 * T, results.det_boxes.data_ptr() + 16 * b0 * T,
            results.det_count.data_ptr() + 4 * b0, B, T, self.names.data_ptr(), self.name_len.data_ptr(), len(self.classes), H, W, s, self.gw,
            self.gh, rec.data_ptr() + REC_DTYPE.itemsize * b0 * T, self._stream()), "fx_annotate_labels_from_detections")
        return rec

    def annotate(self, frames: torch.Tensor, results, b0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draw images b0 .. b0+B-1 of the packed device ``results`` (``det_scores / det_labels / det_boxes / det_count``; with masks also
        ``mask_words`` [., T, H, words per row] and ``det_area``) on ``frames`` (device uint8 [B, H, W, 3]), in place or into ``out``:
        the records kernel, then the draw kernel.  Returns the drawn device frames."""
        self._check_frames(frames)
        B, H, W, _ = frames.shape
        s = scale_for(H, W)
        rec = self.records(results, b0, B, H, W, s) if self.flags & FLAG_LABELS else None
        return self.draw(frames, results, rec, b0, out)

    def draw(self, frames: torch.Tensor, results, rec: Optional[torch.Tensor], b0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fx_annotate_u8 alone, with the records of ``records()``."""
        from ._lib import check

        self._check_frames(frames)
        dst = frames if out is None else out
        B, H, W, _ = frames.shape
        s = scale_for(H, W)
        T = int(results.det_labels.shape[1])
        flags = self.flags
        area = words = None
        wpr = stride = 0
        if flags & FLAG_MASKS:
            words, area = results.mask_words, results.det_area
            if tuple(words.shape[1:3]) != (T, H) or not words.is_contiguous():
                raise ValueError(f"annotate: mask planes {tuple(words.shape)} do not match {T} slots of {H} rows")
            wpr, stride = int(words.shape[3]), int(words.shape[2]) * int(words.shape[3])
        check(self.lib.fx_annotate_u8(frames.data_ptr(), dst.data_ptr(), B, H, W, int(b0), T, results.det_count.data_ptr(),
                                      results.det_labels.data_ptr(), results.det_boxes.data_ptr(), None if area is None else area.data_ptr(),
                                      None if words is None else words.data_ptr(), wpr, stride, None if rec is None else rec.data_ptr(),
                                      None if self.atlas is None else self.atlas.data_ptr(), self.gw, self.gh, s, flags, self._stream()),
              "fx_annotate_u8")
        return dst

    def records_tracked(self, results, ids: torch.Tensor, b0: int, B: int, H: int, W: int, s: int) -> torch.Tensor:
        """fx_annotate_labels_tracked: ``records()`` with "#id " in front of the text of every slot whose ``ids`` (i32 [rows, T]) is >= 0."""
        from ._lib import check

        T = int(results.det_scores.shape[1])
        rec = torch.zeros(int(results.det_count.shape[0]), T, REC_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        check(self.lib.fx_annotate_labels_tracked(
            results.det_scores.data_ptr() + 4 * b0 * T, results.det_labels.data_ptr() + 4 * b0 * T, results.det_boxes.data_ptr() + 16 * b0 * T,
            results.det_count.data_ptr() + 4 * b0, ids.data_ptr() + 4 * b0 * T, B, T, self.names.data_ptr(), self.name_len.data_ptr(),
            len(self.classes), H, W, s, self.gw, self.gh, rec.data_ptr() + REC_DTYPE.itemsize * b0 * T, self._stream()),
            "fx_annotate_labels_tracked")
        return rec

    def _zone_tables(self, zones) -> dict:
        """The region names, region counts and the record buffer of a DeviceZones, uploaded once and kept on it."""
        tab = getattr(zones, "_overlay_tables", None)
        if tab is None:
            from .zones import MAX_REGIONS

            names, ln = region_name_table([r.name for regs in zones.per_stream for r in regs])
            S = zones.streams
            tab = zones._overlay_tables = dict(
                names=torch.from_numpy(names).to(self.device), name_len=torch.from_numpy(ln).to(self.device),
                count=torch.from_numpy(np.diff(zones.reg_first).astype(np.int32)).to(self.device),
                zeros=torch.zeros(S, MAX_REGIONS, 4, dtype=torch.int32, device=self.device),
                rec=torch.zeros(S, MAX_REGIONS, REC_DTYPE.itemsize, dtype=torch.uint8, device=self.device))
        return tab

    def zone_records(self, zones, H: int, W: int, s: int) -> torch.Tensor:
        """fx_annotate_zone_records for every stream of ``zones`` at frame size (H, W): uint8 [streams, 32, 56], the counts read from the
        buffer of the last ``zones.update`` on the device."""
        from ._lib import check

        tab, R = self._zone_tables(zones), zones.R
        io = zones._io
        check(self.lib.fx_annotate_zone_records(
            zones._d_records.data_ptr(), zones._d_reg_first.data_ptr(), zones._d_verts.data_ptr(), zones.records.ctypes.data,
            zones.reg_first.ctypes.data, zones.verts.ctypes.data, R, int(zones.verts.shape[0]), tab["names"].data_ptr(), tab["name_len"].data_ptr(),
            io[:R].data_ptr(), io[R:2 * R].data_ptr(), io[2 * R:3 * R].data_ptr(), zones.streams, H, W, s, self.gw, self.gh, tab["rec"].data_ptr(),
            self._stream()), "fx_annotate_zone_records")
        return tab["rec"]

    def geometry(self, frames: torch.Tensor, b0: int, zones, traces: Optional[DeviceTraces], flags: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fx_annotate_overlay_u8: zone fills, zone outlines / line strokes and traces of streams b0 .. b0+B-1 on ``frames``, in place or
        into ``out``.  ``zones`` (a DeviceZones) is read with OVL_FILL | OVL_STROKE, ``traces`` with OVL_TRACES."""
        from ._lib import check

        self._check_frames(frames)
        dst = frames if out is None else out
        B, H, W, _ = frames.shape
        z = [None] * 6 + [0, 0]
        t = [None] * 6 + [1, 1]
        streams = zones.streams if zones is not None else (traces.streams if traces is not None else b0 + B)
        if flags & (OVL_FILL | OVL_STROKE):
            z = [zones._d_records.data_ptr(), zones._d_reg_first.data_ptr(), zones._d_verts.data_ptr(), zones.records.ctypes.data,
                 zones.reg_first.ctypes.data, zones.verts.ctypes.data, zones.R, int(zones.verts.shape[0])]
        if flags & OVL_TRACES:
            t = [traces.tracker.id.data_ptr(), *traces._state_ptrs(), traces.xy.data_ptr(), traces.max_tracks, traces.length]
        check(self.lib.fx_annotate_overlay_u8(frames.data_ptr(), dst.data_ptr(), B, H, W, int(b0), streams, *z, *t, scale_for(H, W), flags,
                                              self._stream()), "fx_annotate_overlay_u8")
        return dst

    def redact(self, frames: torch.Tensor, results, b0: int, red: Redact, tracker=None) -> torch.Tensor:
        """Cover the selected objects of images b0 .. b0+B-1 of ``results`` on ``frames``: fx_redact_regions over every row of the results
        (with ``tracker``, a DeviceTracker of as many streams, also its coasting slots), then fx_redact_u8 - in place for "fill" and
        "pixelate", into the scratch frame of this frame shape for "blur".  Returns the frames that now hold the picture."""
        from ._lib import check

        self._check_frames(frames)
        B, H, W, _ = frames.shape
        rows, T = int(results.det_labels.shape[0]), int(results.det_labels.shape[1])
        if red not in self._redact_words:      # the class bitmap goes up once per Redact
            ids = red.class_ids(self.classes)
            self._redact_words[red] = None if ids is None else torch.from_numpy(class_words(ids, len(self.classes)).view(np.int32)).to(self.device)
        words = self._redact_words[red]
        trk = [None] * 4 + [0]
        if tracker is not None:
            if tracker.streams != rows:
                raise ValueError(f"redact: a tracker of {tracker.streams} streams for results of {rows} rows (batch index b is stream b)")
            trk = [tracker.id.data_ptr(), tracker.label.data_ptr(), tracker.tsu.data_ptr(), tracker.box.data_ptr(), tracker.config.max_tracks]
        R = T + trk[4]
        if (rows, R) not in self._redact_regions:
            i32 = dict(dtype=torch.int32, device=self.device)
            self._redact_regions[(rows, R)] = (torch.zeros(rows, R, 4, **i32), torch.zeros(rows, R, **i32), torch.zeros(rows, **i32))
        reg, slot, count = self._redact_regions[(rows, R)]
        check(self.lib.fx_redact_regions(results.det_labels.data_ptr(), results.det_boxes.data_ptr(), results.det_count.data_ptr(), rows, T,
                                         None if words is None else words.data_ptr(), len(self.classes) if words is not None else 0, *trk,
                                         red.hold if tracker is not None else 0, red.pad256, red.top256, reg.data_ptr(), slot.data_ptr(),
                                         count.data_ptr(), self._stream()), "fx_redact_regions")
        mw, wpr, stride = None, 0, 0
        if red.shape == "mask":
            mw = results.mask_words
            if tuple(mw.shape[1:3]) != (T, H) or not mw.is_contiguous():
                raise ValueError(f"redact: mask planes {tuple(mw.shape)} do not match {T} slots of {H} rows")
            wpr, stride = int(mw.shape[3]), int(mw.shape[2]) * int(mw.shape[3])
        dst = frames
        if red.mode == "blur":      # cannot run in place: one scratch frame per frame shape, the later layers draw there
            key = tuple(frames.shape)
            if key not in self._redact_scratch:
                self._redact_scratch[key] = torch.empty_like(frames)
            dst = self._redact_scratch[key]
        check(self.lib.fx_redact_u8(frames.data_ptr(), dst.data_ptr(), B, H, W, int(b0), reg.data_ptr(), slot.data_ptr(), count.data_ptr(), R,
                                    None if mw is None else mw.data_ptr(), wpr, stride, T, REDACT_MODES[red.mode], REDACT_SHAPES[red.shape],
                                    red.cell, red.radius, red.colour_word, self._stream()), "fx_redact_u8")
        return dst

    def annotate_overlay(self, frames: torch.Tensor, results, b0: int, ov: OverlayPass) -> torch.Tensor:
        """``annotate()`` with the layers of an Overlay, in place, bottom to top: the redaction (its own pass; "blur" moves the picture to
        the scratch frame, where the rest is then drawn), the heat map (its own pass), zone fills, zone outlines and line strokes, traces
        (one geometry pass), the three layers of ``annotate()`` with the id in the label (left out with ``draw=False``), the region
        count labels."""
        self._check_frames(frames)
        B, H, W, _ = frames.shape
        s = scale_for(H, W)
        if ov.overlay.redact is not None:
            frames = self.redact(frames, results, b0, ov.overlay.redact, ov.tracker)
        if ov.heat is not None:
            ov.heat.render(frames, b0)
        geo = (OVL_FILL | OVL_STROKE if ov.zones is not None else 0) | (OVL_TRACES if ov.traces is not None else 0)
        if geo:
            self.geometry(frames, b0, ov.zones, ov.traces, geo)
        labels = bool(self.flags & FLAG_LABELS)
        if ov.overlay.draw:
            rec = None
            if labels:
                rec = self.records_tracked(results, ov.ids, b0, B, H, W, s) if ov.overlay.ids else self.records(results, b0, B, H, W, s)
            self.draw(frames, results, rec, b0)
        if labels and ov.zones is not None:
            from ._lib import check

            tab = self._zone_tables(ov.zones)
            zrec = self.zone_records(ov.zones, H, W, s)
            check(self.lib.fx_annotate_u8(frames.data_ptr(), frames.data_ptr(), B, H, W, int(b0), int(zrec.shape[1]), tab["count"].data_ptr(),
                                          tab["zeros"].data_ptr(), tab["zeros"].data_ptr(), None, None, 0, 0, zrec.data_ptr(),
                                          self.atlas.data_ptr(), self.gw, self.gh, s, FLAG_LABELS, self._stream()), "fx_annotate_u8")
        return frames

    def annotate_classification(self, frames: torch.Tensor, detections: Sequence, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The classification overlay: ``detections[b]`` (FocoosDetections) gives frame b's lines; the records are built on the host (the
        classifier leaves nothing packed on the device) and drawn by fx_annotate_u8 with only the labels flag."""
        from ._lib import check

        self._check_frames(frames)
        dst = frames if out is None else out
        if not self.flags & FLAG_LABELS:
            if out is not None:
                out.copy_(frames)
            return dst
        B, H, W, _ = frames.shape
        s = scale_for(H, W)
        lines = [[(d.label, d.conf) for d in det.detections if d.conf is not None and d.label is not None] for det in detections]
        T = min(MAX_SLOTS, max(1, max(len(ls) for ls in lines)))
        rec = torch.from_numpy(classification_records(lines, T, s, self.gw, self.gh).view(np.uint8).reshape(B, T, -1)).to(self.device)
        count = torch.tensor([min(len(ls), T) for ls in lines], dtype=torch.int32).to(self.device)
        zeros = torch.zeros(B, T, 4, dtype=torch.int32, device=self.device)
        check(self.lib.fx_annotate_u8(frames.data_ptr(), dst.data_ptr(), B, H, W, 0, T, count.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), None,
                                      None, 0, 0, rec.data_ptr(), self.atlas.data_ptr(), self.gw, self.gh, s, FLAG_LABELS, self._stream()),
              "fx_annotate_u8")
        return dst


def annotator_of(fm) -> DeviceAnnotator:
    """The model's annotator, created on first use (uploads the atlas and the class names once)."""
    ann = getattr(fm, "_annotator", None)
    if ann is None:
        ann = fm._annotator = DeviceAnnotator(fm.model_info.classes, str(getattr(fm.model_info.task, "value", fm.model_info.task)), fm.model.device)
    return ann


def to_host(frames: torch.Tensor) -> np.ndarray:
    """One pinned device-to-host copy of drawn frames [B, H, W, 3]."""
    host = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(frames, non_blocking=True)
    torch.cuda.current_stream(frames.device).synchronize()
    return host.numpy().copy()


def annotate_results(fm, inputs, images: torch.Tensor, results, out: list, overlay: Optional[OverlayPass] = None) -> None:
    """Set ``out[i].image`` (np.uint8 [H, W, 3] at the ORIGINAL size of input i) for one batch: ``images`` is what preprocess returned,
    ``results`` the plan holding the packed device results (ignored for classification, drawn from ``out``'s detections).  When
    preprocess took the uint8 same-size fast path the batch itself is drawn on; otherwise every original goes up once (the boxes are in
    original pixels already) and each run of equal-size images is one kernel call with its ``b0``.  One pinned copy back per call.
    ``overlay``: the layers of an ``Overlay`` as well (``annotate_overlay``); None draws exactly what ``annotate=True`` always drew."""
    ann = annotator_of(fm)
    lst = inputs if isinstance(inputs, list) else [inputs]
    cls = fm.model.family == "fai_cls"
    if images.dtype == torch.uint8:      # preprocess stacks uint8 inputs only when all of them already have the batch's size
        runs = [(0, images.contiguous())]
    else:
        from .tiled import frame_tensor

        frames = [frame_tensor(im) for im in lst]
        runs, i = [], 0
        while i < len(frames):
            j = i + 1
            while j < len(frames) and frames[j].shape == frames[i].shape:
                j += 1
            runs.append((i, torch.stack(frames[i:j], 0).to(fm.model.device, non_blocking=True)))
            i = j
    for b0, fr in runs:
        n = fr.shape[0]
        if cls:
            drawn = ann.annotate_classification(fr, out[b0:b0 + n])
        else:
            drawn = ann.annotate(fr, results, b0) if overlay is None else ann.annotate_overlay(fr, results, b0, overlay)
        host = to_host(drawn)
        for k in range(n):
            out[b0 + k].image = host[k]
