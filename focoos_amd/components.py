"""Masks split into their connected components on the device (``FocoosModel.infer(components=...)``).

The mask families return one detection per query and, in semantic mode, one per class: "class pothole, one box round all of them".
``DeviceComponents.split`` turns a packed result (``det_count``, ``det_scores``, ``det_labels``, ``det_boxes``, ``det_area``,
``mask_words``, ``mask_width``) into a packed result with one slot per connected component (csrc/mask_components.hip; the contract is in
include/focoos_amd.h), so the mask encoders, the overlay, the redaction, the tracker, the zones and the cascade work per object without
knowing of it.  ``label_components`` is the same definition in numpy: the tests' reference and the fallback for an image whose runs did
not fit the run pool."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

from .mask_pool import unpack_words
from .mask_rle import MASK_FAMILIES

MAX_COMPONENTS = 4096          # include/focoos_amd.h: M of fx_mask_components
MAX_RUN_CAPACITY = 1 << 27


@dataclass
class Components:
    """``connectivity``: 4 or 8.  ``min_area``: a component with fewer pixels is dropped silently (the speck filter).  ``max_components``:
    output slots per image; the components beyond them, in the order (source mask, first pixel), are dropped with a warning.  ``classes``:
    class ids or names whose masks are split - the masks of every other class pass through whole, one component each; None splits all."""
    connectivity: int = 8
    min_area: int = 1
    max_components: int = 64
    classes: Optional[Sequence] = None


def check(components, family: str, class_names: Sequence[str], mask_format: str, detections: bool, consumed: bool, what: str = "infer"):
    """The ``components`` keyword of the inference surface: None, True (the defaults) or a ``Components`` -> None or the validated
    ``Components``.  TypeError for anything else, NotImplementedError by name for a family without masks, ValueError for a value outside
    the contract, an unknown class, or ``mask_format="none"`` with nothing that reads the components (``consumed``: an analytics argument
    or ``annotate``).  Host only: nothing is loaded or launched."""
    if components is None:
        return None
    if components is True:
        components = Components()
    if not isinstance(components, Components):
        raise TypeError(f"{what}: components must be None, True or a components.Components, not {type(components).__name__}")
    if family not in MASK_FAMILIES:
        raise NotImplementedError(f"{what}: components= needs masks; model family {family!r} has none (supported: {', '.join(MASK_FAMILIES)})")
    c = components
    if c.connectivity not in (4, 8) or isinstance(c.connectivity, bool):
        raise ValueError(f"{what}: Components.connectivity must be 4 or 8, got {c.connectivity!r}")
    if not isinstance(c.min_area, (int, np.integer)) or c.min_area < 1:
        raise ValueError(f"{what}: Components.min_area must be an integer >= 1, got {c.min_area!r}")
    if not isinstance(c.max_components, (int, np.integer)) or not 1 <= c.max_components <= MAX_COMPONENTS:
        raise ValueError(f"{what}: Components.max_components must be in 1 .. {MAX_COMPONENTS}, got {c.max_components!r}")
    split_table(c.classes, class_names, what)
    if mask_format == "none" and detections and not consumed:
        raise ValueError(f"{what}: components= with mask_format='none' hands out boxes only: pass a mask format, or an analytics argument or "
                         "annotate= that reads the components")
    return c


def split_table(classes, class_names: Sequence[str], what: str = "infer") -> Optional[np.ndarray]:
    """``Components.classes`` -> uint8 [K], 1 for a class whose masks are split (None: every class is)."""
    if classes is None:
        return None
    names = list(class_names or ())
    table = np.zeros(max(len(names), 1), np.uint8)
    for c in classes:
        if isinstance(c, str):
            if c not in names:
                raise ValueError(f"{what}: Components.classes names {c!r}, which is no class of the model")
            table[names.index(c)] = 1
        elif isinstance(c, (int, np.integer)) and not isinstance(c, bool) and 0 <= int(c) < len(table):
            table[int(c)] = 1
        else:
            raise ValueError(f"{what}: Components.classes holds {c!r}: a class is a name or an id in 0 .. {len(table) - 1}")
    return table


def label_components(mask, connectivity: int = 8) -> np.ndarray:
    """bool [H, W] -> int32 [H, W]: 0 for an unset pixel, else the number (from 1) of the pixel's component, the components numbered by
    the raster index of their first pixel (``scipy.ndimage.label``'s order).  The device's algorithm, restated: the runs of every row, a
    union-find that links a run to the runs of the row above it touches (x range widened by one for 8-connectivity) with the smaller
    root on top, so a component's root is its first run."""
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity must be 4 or 8, got {connectivity!r}")
    m = np.asarray(mask).astype(bool)
    if m.ndim != 2:
        raise ValueError(f"label_components: a mask is [H, W], got {m.shape}")
    H, W = m.shape
    d = np.diff(np.pad(m, ((0, 0), (1, 1))).astype(np.int8), axis=1)      # [H, W + 1]: +1 where a run starts, -1 behind its end
    ys, x0 = np.nonzero(d == 1)
    x1 = np.nonzero(d == -1)[1] - 1
    n, c = len(ys), 1 if connectivity == 8 else 0
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    row = np.searchsorted(ys, np.arange(H + 1))
    for y in range(1, H):
        ps, cs, ce = row[y - 1], row[y], row[y + 1]
        if ps == cs or cs == ce:
            continue
        first = ps + np.searchsorted(x1[ps:cs], x0[cs:ce] - c)                   # the first run above that ends at or after x0 - c
        last = ps + np.searchsorted(x0[ps:cs], x1[cs:ce] + c, side="right")      # ... and the one behind the last that starts by x1 + c
        for r, a, e in zip(range(cs, ce), first.tolist(), last.tolist()):
            for p in range(a, e):
                ra, rb = find(r), find(p)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    roots = np.fromiter((find(r) for r in range(n)), np.int64, n)
    lab = (np.searchsorted(np.unique(roots), roots) + 1).astype(np.int32)         # roots are first runs: their order is the components'
    paint = np.zeros((H, W + 1), np.int32)
    np.add.at(paint, (ys, x0), lab)
    np.add.at(paint, (ys, x1 + 1), -lab)
    return np.cumsum(paint, axis=1, dtype=np.int32)[:, :W]


def split_numpy(words, count: int, scores, labels, W: int, config: Components, table: Optional[np.ndarray] = None) -> SimpleNamespace:
    """fx_mask_components for one image on the host: ``words`` int32 [Q, H, ceil(W / 32)], ``scores`` / ``labels`` [Q] -> the outputs of
    the call for that image as numpy arrays (``count``, ``dropped``, and [M] ``scores``, ``labels``, ``area``, ``source``, [M, 4]
    ``boxes``, [M, H, ceil(W / 32)] int32 ``words``)."""
    words, scores, labels = np.asarray(words), np.asarray(scores, np.float32), np.asarray(labels, np.int32)
    Q, H, W32 = words.shape
    M = int(config.max_components)
    out = SimpleNamespace(count=0, dropped=0, scores=np.zeros(M, np.float32), labels=np.zeros(M, np.int32), area=np.zeros(M, np.int32),
                          source=np.zeros(M, np.int32), boxes=np.zeros((M, 4), np.int32), words=np.zeros((M, H, W32), np.int32))
    total = 0
    for j in range(max(0, min(int(count), Q))):
        mask = unpack_words(words[j], W)
        whole = table is not None and 0 <= labels[j] < len(table) and table[labels[j]] == 0
        lab = mask.astype(np.int32) if whole else label_components(mask, config.connectivity)
        for i in range(1, int(lab.max()) + 1 if lab.size else 1):
            comp = lab == i
            area = int(comp.sum())
            if area < config.min_area:
                continue
            total += 1
            if total > M:
                continue
            k = total - 1
            yy, xx = np.nonzero(comp)
            out.scores[k], out.labels[k], out.area[k], out.source[k] = scores[j], labels[j], area, j
            out.boxes[k] = (xx.min(), yy.min(), xx.max(), yy.max())
            bits = np.zeros((H, W32 * 32), bool)
            bits[:, :W] = comp
            out.words[k] = np.packbits(bits, axis=-1, bitorder="little").view("<i4")
    out.count, out.dropped = min(total, M), total - min(total, M)
    return out


def default_run_capacity(Q: int, H: int, W: int) -> int:
    """Runs per image of the pool: 64 per row of the frame over all its masks together (the masks of a semantic result partition the
    frame, so this is 64 class changes per row), at least 4096, never more than the masks can have."""
    return int(max(1, min(max(4096, 64 * int(H)), int(Q) * int(H) * ((int(W) + 1) // 2), MAX_RUN_CAPACITY)))


class DeviceComponents:
    """Outputs, run pool and workspace of fx_mask_components for results of one shape (B images, Q slots, H x W pixels) on ``device``.
    ``split(res)`` launches on the current stream and returns the split result in the plan's field names, M = ``max_components`` slots
    per image, plus ``det_source`` (the slot a component came from) and ``status``.  The result stays valid until the next ``split``."""

    def __init__(self, B: int, Q: int, H: int, W: int, device, config: Components, table: Optional[np.ndarray] = None,
                 run_capacity: Optional[int] = None):
        import torch

        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library (the kernel is the same in both)
        self.device = torch.device(device)
        self.B, self.Q, self.H, self.W, self.M = int(B), int(Q), int(H), int(W), int(config.max_components)
        self.config = config
        self.run_capacity = default_run_capacity(Q, H, W) if run_capacity is None else int(run_capacity)
        self.table_host = None if table is None else np.ascontiguousarray(table, np.uint8)
        self.table = None if table is None else torch.from_numpy(self.table_host).to(self.device)
        nb = int(self.lib.fx_mask_components_workspace_bytes(self.B, self.Q, self.H, self.W, self.M, self.run_capacity))
        if nb == 0:
            raise ValueError(f"DeviceComponents: B = {B}, Q = {Q}, H = {H}, W = {W}, max_components = {self.M}, run_capacity = "
                             f"{self.run_capacity} is outside the kernel's limits (H W < 2^31, W <= 65535, max_components <= {MAX_COMPONENTS})")
        i32, M = dict(dtype=torch.int32, device=self.device), self.M
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self.out = SimpleNamespace(det_count=torch.zeros(self.B, **i32), det_scores=torch.zeros(self.B, M, dtype=torch.float32, device=self.device),
                                   det_labels=torch.zeros(self.B, M, **i32), det_boxes=torch.zeros(self.B, M, 4, **i32),
                                   det_area=torch.zeros(self.B, M, **i32), det_source=torch.zeros(self.B, M, **i32),
                                   mask_words=torch.zeros(self.B, M, self.H, (self.W + 31) // 32, **i32), mask_width=self.W,
                                   status=torch.zeros(self.B, 2, **i32))
        self.last_fallback = 0     # images the last split labelled on the host
        self.last_dropped = 0      # components of the last split that found no slot

    def key(self):
        c = self.config
        table = None if self.table_host is None else self.table_host.tobytes()
        return (self.B, self.Q, self.H, self.W, self.device, c.connectivity, c.min_area, c.max_components, table, self.run_capacity)

    def split(self, res) -> SimpleNamespace:
        import torch

        from ._lib import check as check_call

        shape = (self.B, self.Q, self.H, (self.W + 31) // 32)
        for name, t, shp, dt in (("mask_words", res.mask_words, shape, torch.int32), ("det_count", res.det_count, (self.B,), torch.int32),
                                 ("det_scores", res.det_scores, (self.B, self.Q), torch.float32),
                                 ("det_labels", res.det_labels, (self.B, self.Q), torch.int32),
                                 ("det_boxes", res.det_boxes, (self.B, self.Q, 4), torch.int32)):
            if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"DeviceComponents.split: {name} must be a contiguous {dt} tensor {shp} on {self.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        o, c = self.out, self.config
        check_call(self.lib.fx_mask_components(
            res.mask_words.data_ptr(), res.det_count.data_ptr(), res.det_scores.data_ptr(), res.det_labels.data_ptr(), res.det_boxes.data_ptr(),
            self.B, self.Q, self.H, self.W, int(c.connectivity), int(c.min_area), None if self.table is None else self.table.data_ptr(),
            0 if self.table is None else int(self.table.numel()), self.M, self.run_capacity, self.workspace.data_ptr(), self.workspace.numel(),
            o.det_count.data_ptr(), o.det_scores.data_ptr(), o.det_labels.data_ptr(), o.det_boxes.data_ptr(), o.det_area.data_ptr(),
            o.det_source.data_ptr(), o.mask_words.data_ptr(), o.status.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
            "fx_mask_components")
        status = o.status.cpu().numpy()      # synchronises the stream: an image whose runs did not fit is labelled here
        over = np.flatnonzero(status[:, 1])
        for b in over.tolist():
            n = int(res.det_count[b].clamp(0, self.Q).item())
            h = split_numpy(res.mask_words[b, :n].cpu().numpy(), n, res.det_scores[b, :n].cpu().numpy(), res.det_labels[b, :n].cpu().numpy(),
                            self.W, c, self.table_host)
            for dst, src in ((o.det_scores, h.scores), (o.det_labels, h.labels), (o.det_boxes, h.boxes), (o.det_area, h.area),
                             (o.det_source, h.source), (o.mask_words, h.words)):
                dst[b].copy_(torch.from_numpy(src))
            o.det_count[b] = h.count
            status[b] = (h.dropped, 1)
        self.last_fallback, self.last_dropped = len(over), int(status[:, 0].sum())
        if len(over):
            warnings.warn(f"components=: the masks of {len(over)} of {self.B} images have more than {self.run_capacity} runs and were "
                          "labelled on the host (raise the run capacity)", RuntimeWarning, stacklevel=3)
        if self.last_dropped:
            warnings.warn(f"components=: {self.last_dropped} components found no slot (max_components = {self.M}; the slots go to the first "
                          "in the order of their masks and first pixels): raise max_components", RuntimeWarning, stacklevel=3)
        return o


def splitter_for(current, res, config: Components, table: Optional[np.ndarray] = None, run_capacity: Optional[int] = None) -> DeviceComponents:
    """``current`` when it fits ``res`` (shape, device), the configuration and ``run_capacity`` (None = ``default_run_capacity``), a new
    ``DeviceComponents`` otherwise (``mask_pool.encoder_for``)."""
    B, Q, H, _ = res.mask_words.shape
    W = int(getattr(res, "mask_width", res.mask_words.shape[3] * 32))
    dev = res.mask_words.device
    cap = default_run_capacity(Q, H, W) if run_capacity is None else int(run_capacity)
    key = (B, Q, H, W, dev, config.connectivity, config.min_area, config.max_components, None if table is None else table.tobytes(), cap)
    if current is not None and current.key() == key:
        return current
    return DeviceComponents(B, Q, H, W, dev, config, table, cap)
