"""Drawing the detections on the frame on the device (``FocoosModel.infer(image, annotate=True)``).

The reference draws with ``supervision`` + ``cv2`` on the host (focoos/utils/vision.py:437-488).  Here the packed device results and the
bit-packed masks never leave the GPU: ``fx_annotate_labels_from_detections`` turns them into label records ("name: NN%", rectangle, colour)
and ``fx_annotate_u8`` draws outlines, half-opacity masks and the labels in one pass over the uint8 frames (csrc/annotate.hip; the contract
is in include/focoos_amd.h).  What is mirrored from the reference is the layer order (outlines, masks, labels), the palette and the class
colouring, the half-opacity masks with the smaller instance on top and the label text; pixel equality with supervision / cv2 is NOT claimed
(a bitmap font in a fixed cell, square label corners).  Keypoints are out of scope."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

LNAME = 24      # include/focoos_amd.h FX_ANN_LNAME
LMAX = 32       # FX_ANN_LMAX
GLYPHS = 95     # FX_ANN_GLYPHS: ASCII 32..126
MAX_SLOTS = 1024
FLAG_BOXES, FLAG_MASKS, FLAG_LABELS = 1, 2, 4
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


def annotate_results(fm, inputs, images: torch.Tensor, results, out: list) -> None:
    """Set ``out[i].image`` (np.uint8 [H, W, 3] at the ORIGINAL size of input i) for one batch: ``images`` is what preprocess returned,
    ``results`` the plan holding the packed device results (ignored for classification, drawn from ``out``'s detections).  When
    preprocess took the uint8 same-size fast path the batch itself is drawn on; otherwise every original goes up once (the boxes are in
    original pixels already) and each run of equal-size images is one kernel call with its ``b0``.  One pinned copy back per call."""
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
        drawn = ann.annotate_classification(fr, out[b0:b0 + n]) if cls else ann.annotate(fr, results, b0)
        host = to_host(drawn)
        for k in range(n):
            out[b0 + k].image = host[k]
