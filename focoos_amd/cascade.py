"""A second model on every detected object, on the device (``FocoosModel.infer_stream(classify=...)``).

The detector's packed result stays where it is; per batch, on the current stream and without a host synchronisation of its own:

  fx_roi_select              which detections of every stream are cropped this frame: at most ``max_objects``, the stalest tracks first
  fx_frames_roi_gather_f32   the crops, straight from the resident video planes -> float32 [S * K, im, im, 3] on the 0..255 scale
  classifier engine          ``ClsEngine.forward`` on that buffer (in chunks of ``batch_size`` when set)
  fx_roi_attributes          the top class of every crop, remembered per track slot, reported per detection

(csrc/roi_ops.hip, csrc/frame_ops.hip; the contracts are in include/focoos_amd.h, tests/cascade_ref.py restates the two rules.)  Three small
arrays more ride along with the packed copy; the host applies ``torch.sigmoid`` to the logits and sets ``attr_id`` / ``attr_label`` /
``attr_conf`` of the detections whose confidence exceeds the threshold.  The reference has no counterpart.  Left out on purpose:
multi-label attributes, more than one classifier per call, attribute text in the overlay, per-attribute zone counts, square or
letterboxed crops, uint8 crops, skipping classifier work for empty rows."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .tracking import BOX_FAMILIES, MAX_SLOTS, MAX_STREAMS

MAX_OBJECTS = 64       # csrc/roi_ops.hip ROI_MAX_K
MAX_CROPS = 65535      # S * K: the crops of one launch
MAX_WORDS = 256        # class_words: detector labels 0 .. 32 * 256 - 1
HOLDS = ("latest", "best")


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_num(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


@dataclass(frozen=True)
class Cascade:
    """What to classify and how.  ``classifier``: a ``FocoosModel`` of family fai_cls on the detector's device; ``classes``: the detector
    classes to classify, ids or names (None = all); ``max_objects``: K, crops per stream and frame; ``pad``: the box is grown by
    pad * extent on every side (quantised to 1/256); ``min_size``: boxes narrower or lower than this many pixels are not classified;
    ``min_score``: neither are detections below this score; ``interval``: frames before a tracked object is classified again; ``hold``:
    what a track remembers, the "latest" answer or the "best" (largest logit); ``threshold``: the attribute is shown when
    sigmoid(logit) > (threshold or 0.5); ``batch_size``: the classifier's batch (None = S * K in one plan).  Validated at construction:
    ValueError names the field."""
    classifier: object
    classes: Optional[Sequence[Union[int, str]]] = None
    max_objects: int = 16
    pad: float = 0.0
    min_size: int = 8
    min_score: float = 0.0
    interval: int = 1
    hold: str = "latest"
    threshold: Optional[float] = None
    batch_size: Optional[int] = None

    def __post_init__(self):
        def bad(name, why):
            raise ValueError(f"Cascade.{name} = {getattr(self, name)!r}: {why}")

        from .model import FocoosModel

        if not isinstance(self.classifier, FocoosModel) or getattr(getattr(self.classifier, "model", None), "family", None) != "fai_cls":
            raise ValueError(f"Cascade.classifier must be a FocoosModel of family 'fai_cls', got {_describe(self.classifier)}")
        if self.classes is not None:
            if isinstance(self.classes, (str, bytes)) or not hasattr(self.classes, "__iter__"):
                bad("classes", "must be None or a list of class ids or names")
            object.__setattr__(self, "classes", tuple(self.classes))
            if not self.classes:
                bad("classes", "must name at least one class (None = all)")
            for c in self.classes:
                if not (isinstance(c, str) or (_is_int(c) and 0 <= c < 32 * MAX_WORDS)):
                    bad("classes", f"every entry must be a class name or an id in 0..{32 * MAX_WORDS - 1}")
        if not _is_int(self.max_objects) or not 1 <= self.max_objects <= MAX_OBJECTS:
            bad("max_objects", f"must be an integer in 1..{MAX_OBJECTS}")
        if not _is_num(self.pad) or not 0.0 <= self.pad <= 1.0:
            bad("pad", "must be a number in [0, 1]")
        if not _is_int(self.min_size) or not 1 <= self.min_size <= 2 ** 30:
            bad("min_size", "must be an integer >= 1")
        if not _is_num(self.min_score):
            bad("min_score", "must be a finite number")
        if not _is_int(self.interval) or not 1 <= self.interval <= 2 ** 30:
            bad("interval", "must be an integer >= 1")
        if self.hold not in HOLDS:
            bad("hold", f"must be one of {list(HOLDS)}")
        if self.threshold is not None and (not _is_num(self.threshold) or not 0.0 <= self.threshold < 1.0):
            bad("threshold", "must be None or a number in [0, 1)")
        if self.batch_size is not None and (not _is_int(self.batch_size) or not 1 <= self.batch_size <= MAX_CROPS):
            bad("batch_size", f"must be None or an integer in 1..{MAX_CROPS}")

    @property
    def pad_q(self) -> int:
        """``pad`` in 1/256ths, rounded half up: what the kernel multiplies a box extent by."""
        return int(math.floor(float(self.pad) * 256.0 + 0.5))


def _describe(m) -> str:
    fam = getattr(getattr(m, "model", None), "family", None)
    return f"a {type(m).__name__}" + (f" of family {fam!r}" if fam is not None else "")


def class_ids(cascade: Cascade, names: Sequence[str], what: str = "infer_stream") -> Optional[List[int]]:
    """``Cascade.classes`` as detector class ids (None = every class); a name the detector does not have is a ValueError.  Host only."""
    if cascade.classes is None:
        return None
    names = list(names or ())
    out = []
    for c in cascade.classes:
        if isinstance(c, str):
            if c not in names:
                raise ValueError(f"{what}: Cascade.classes names {c!r}, which the detector does not have")
            c = names.index(c)
        out.append(int(c))
    return sorted(set(out))


def class_words(ids: Optional[Sequence[int]]) -> Optional[np.ndarray]:
    """The ids as the kernel's bit set: uint32 words, bit ``l & 31`` of word ``l >> 5``."""
    if ids is None:
        return None
    words = np.zeros(max(ids) // 32 + 1, dtype=np.uint32)
    for l in ids:
        words[l >> 5] |= np.uint32(1 << (l & 31))
    return words


def check_family(family: str, what: str = "infer_stream") -> None:
    """NotImplementedError, by name, for a family without boxes.  Host only: nothing is loaded or launched."""
    if family not in BOX_FAMILIES:
        raise NotImplementedError(f"{what}: classify needs boxes; model family {family!r} has none (supported: {', '.join(BOX_FAMILIES)})")


def _needs_tracker(c: Cascade) -> Optional[str]:
    if c.interval > 1:
        return f"interval = {c.interval}"
    if c.hold == "best":
        return "hold = 'best'"
    return None


def check(fm, classify, detections: bool, what: str, device_only: bool = False) -> None:
    """Everything ``classify=`` can be refused for without knowing the tracker or the batch: the detector's family, the type, the
    classifier's device, ``detections=False``, class names the detector does not have.  Host only."""
    check_family(fm.model.family, what)
    if not isinstance(classify, DeviceCascade if device_only else (Cascade, DeviceCascade)):
        raise TypeError(f"{what}: classify must be a {'DeviceCascade' if device_only else 'Cascade or a DeviceCascade'}, not "
                        f"{type(classify).__name__}")
    c = classify.cascade if isinstance(classify, DeviceCascade) else classify
    dev, mine = torch.device(c.classifier.model.device), torch.device(fm.model.device)
    if dev != mine:
        raise ValueError(f"{what}: Cascade.classifier lives on {dev}, the detector on {mine}")
    if not detections:
        raise ValueError(f"{what}: detections=False leaves nothing for classify to set its attributes on")
    class_ids(c, fm.model_info.classes, what)


def bind_tracker(classify, track, what: str):
    """The tracker a cascade runs with: (classify, track).  ``interval > 1`` and ``hold="best"`` need one (ValueError); a DeviceCascade built
    on a tracker runs that tracker (``track`` must be None or that one), one built without runs without.  Host only."""
    if isinstance(classify, DeviceCascade):
        if classify.tracker is not None and track is None:
            track = classify.tracker
        if track is not classify.tracker:
            raise ValueError(f"{what}: the DeviceCascade was built on {'another' if classify.tracker is not None else 'no'} tracker: pass the "
                             "DeviceTracker it was built on (or none, to run that one)")
        return classify, track
    why = _needs_tracker(classify)
    if why is not None and track is None:
        raise ValueError(f"{what}: Cascade with {why} remembers attributes per track: it needs track= / tracker=")
    return classify, track


def check_budget(classify, S: int, what: str) -> None:
    """S streams of K crops must fit one launch.  Host only."""
    c = classify.cascade if isinstance(classify, DeviceCascade) else classify
    if S * c.max_objects > MAX_CROPS:
        raise ValueError(f"{what}: {S} streams x Cascade.max_objects = {c.max_objects} crops exceed the {MAX_CROPS} crops of one launch")


def stream_frames(inputs, what: str):
    """One batch of ``classify=`` inputs as a FrameBatch (sizes may differ per stream): a FrameBatch, a Frame, or a list of Frames and / or
    uint8 RGB arrays or tensors [H, W, 3], which are wrapped as RGB24 frames - the detector's preprocess and the crops then read the same
    resident planes.  ValueError for anything else; host only."""
    from .frames import wrap_frames

    return wrap_frames(inputs, f"{what}(classify=)")


def for_batch(classify, S: int, track, device, what: str = "infer_stream") -> "DeviceCascade":
    """The device state of a batch of S streams: created from the ``Cascade`` with the first batch, which fixes S; another size is a
    ValueError."""
    if isinstance(classify, Cascade):
        return DeviceCascade(classify, S, track, device)
    if classify.streams != S:
        raise ValueError(f"{what}: a batch of {S} images for a DeviceCascade of {classify.streams} streams (the first batch fixes the batch "
                         "size; batch index b is stream b)")
    return classify


class DeviceCascade:
    """The state of ``streams`` cascades on ``device`` - per track slot the attribute it remembers - and the four steps of a batch on the
    current stream.  ``tracker``: the ``DeviceTracker`` whose slots the records follow (None: every detection is untracked and nothing is
    remembered).  The state belongs to this object and outlives a call, like ``DeviceTracker`` and ``DeviceZones``."""

    def __init__(self, cascade: Cascade, streams: int, tracker=None, device="cuda"):
        from ._lib import load
        from .tracking import DeviceTracker

        if not isinstance(cascade, Cascade):
            raise TypeError(f"DeviceCascade: cascade must be a Cascade, not {type(cascade).__name__}")
        if not _is_int(streams) or not 1 <= streams <= MAX_STREAMS:
            raise ValueError(f"DeviceCascade: streams = {streams!r} must be in 1..{MAX_STREAMS}")
        check_budget(cascade, int(streams), "DeviceCascade")
        if tracker is not None and not isinstance(tracker, DeviceTracker):
            raise TypeError(f"DeviceCascade: tracker must be a DeviceTracker, not {type(tracker).__name__}")
        if tracker is not None and tracker.streams != streams:
            raise ValueError(f"DeviceCascade: {streams} streams on a tracker of {tracker.streams}")
        why = _needs_tracker(cascade)
        if why is not None and tracker is None:
            raise ValueError(f"DeviceCascade: Cascade with {why} remembers attributes per track: it needs a tracker")
        self.cascade, self.streams, self.tracker = cascade, int(streams), tracker
        self.device = torch.device(device)
        if torch.device(cascade.classifier.model.device) != self.device:
            raise ValueError(f"DeviceCascade: Cascade.classifier lives on {cascade.classifier.model.device}, the cascade on {self.device}")
        self.lib = load("bf16")   # inference surface: the bf16 product library whatever a training step pinned (the kernels are the same in both)
        S, K = self.streams, cascade.max_objects
        self.M = tracker.config.max_tracks if tracker is not None else 1
        i32 = dict(dtype=torch.int32, device=self.device)
        self.at_id, self.at_label, self.at_frame = (torch.zeros(S, self.M, **i32) for _ in range(3))
        self.at_logit = torch.zeros(S, self.M, dtype=torch.float32, device=self.device)
        self.frame = torch.zeros(S, **i32)
        self.roi_win, self.roi_det = torch.zeros(S, K, 4, **i32), torch.zeros(S, K, **i32)
        self.roi_count, self.roi_left = torch.zeros(S, **i32), torch.zeros(S, **i32)
        im = cascade.classifier.model_info.im_size
        self.im = (int(im), int(im)) if _is_int(im) else (int(im[0]), int(im[1]))
        self.bs = S * K if cascade.batch_size is None else min(int(cascade.batch_size), S * K)
        self.Npad = -(-S * K // self.bs) * self.bs
        # zeroed once: a crop without an extent is left untouched by the gather, and the classifier's answer for such a row is never read
        self.crops = torch.zeros(self.Npad, self.im[0], self.im[1], 3, dtype=torch.float32, device=self.device)
        self.C = int(cascade.classifier.model.num_classes)
        self.logits = torch.zeros(self.Npad, self.C, dtype=torch.float32, device=self.device) if self.bs != S * K else None
        self._words_key, self._words = None, None
        self._out = None           # (attr_label, attr_logit, attr_age) of the last run, [S, T]
        self.left_seen = 0         # crops that did not fit the budget since the last warning

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _class_words(self, names) -> Tuple[int, int]:
        key = tuple(names or ())
        if self._words_key != key:
            w = class_words(class_ids(self.cascade, key))
            self._words = None if w is None else torch.from_numpy(w.view(np.int32)).to(self.device)
            self._words_key = key
        return (0, 0) if self._words is None else (self._words.data_ptr(), int(self._words.numel()))

    def select(self, pl, fb, ids: Optional[torch.Tensor], names=()) -> None:
        """fx_roi_select on the packed result ``pl`` (det_scores, det_labels, det_boxes, det_count), this frame's ``ids`` and the frames'
        descriptors: fills roi_win / roi_det / roi_count / roi_left."""
        import ctypes

        from ._lib import check

        S, T = int(pl.det_scores.shape[0]), int(pl.det_scores.shape[1])
        if S != self.streams or len(fb) != S:
            raise ValueError(f"DeviceCascade: a batch of {S} results and {len(fb)} frames for a cascade of {self.streams} streams")
        if not 1 <= T <= MAX_SLOTS:
            raise ValueError(f"DeviceCascade: T = {T} detections per stream, must be in 1..{MAX_SLOTS}")
        if (ids is None) != (self.tracker is None):
            raise ValueError("DeviceCascade: track ids come with the tracker the cascade was built on, and only with it")
        c = self.cascade
        descs, host = fb._descriptors(self.device)
        words, n_words = self._class_words(names)
        check(self.lib.fx_roi_select(pl.det_scores.data_ptr(), pl.det_labels.data_ptr(), pl.det_boxes.data_ptr(), pl.det_count.data_ptr(), S, T,
                                     ids.data_ptr() if ids is not None else None, self.tracker.id.data_ptr() if ids is not None else None, self.M,
                                     self.at_id.data_ptr(), self.at_frame.data_ptr(), self.frame.data_ptr(), descs.data_ptr(),
                                     ctypes.addressof(host), words or None, n_words, c.max_objects, c.pad_q, int(c.min_size), float(c.min_score),
                                     int(c.interval), self.roi_win.data_ptr(), self.roi_det.data_ptr(), self.roi_count.data_ptr(),
                                     self.roi_left.data_ptr(), self._stream()), "fx_roi_select")

    def gather(self, fb) -> torch.Tensor:
        """fx_frames_roi_gather_f32: the crops of roi_win into the float32 crop buffer [>= S * K, im, im, 3]."""
        import ctypes

        from ._lib import check

        descs, host = fb._descriptors(self.device)
        check(self.lib.fx_frames_roi_gather_f32(descs.data_ptr(), ctypes.addressof(host), self.streams, self.roi_win.data_ptr(),
                                                self.cascade.max_objects, self.crops.data_ptr(), self.im[0], self.im[1], self._stream()),
              "fx_frames_roi_gather_f32")
        return self.crops

    def forward(self) -> torch.Tensor:
        """The classifier engine on the crop buffer: f32 logits [>= S * K, C], valid until the next call."""
        eng = self.cascade.classifier.model.engine
        if self.logits is None:
            return eng.forward(self.crops).logits
        for c0 in range(0, self.Npad, self.bs):
            self.logits[c0:c0 + self.bs].copy_(eng.forward(self.crops[c0:c0 + self.bs]).logits, non_blocking=True)
        return self.logits

    def attributes(self, logits: torch.Tensor, pl, ids: Optional[torch.Tensor]):
        """fx_roi_attributes: updates the records and returns (attr_label i32, attr_logit f32, attr_age i32), each [S, T] on the device."""
        from ._lib import check

        S, T = int(pl.det_scores.shape[0]), int(pl.det_scores.shape[1])
        assert logits.is_contiguous() and logits.dtype == torch.float32 and logits.shape[0] >= S * self.cascade.max_objects
        out = (torch.empty(S, T, dtype=torch.int32, device=self.device), torch.empty(S, T, dtype=torch.float32, device=self.device),
               torch.empty(S, T, dtype=torch.int32, device=self.device))
        check(self.lib.fx_roi_attributes(logits.data_ptr(), int(logits.shape[1]), self.roi_det.data_ptr(), self.roi_count.data_ptr(),
                                         self.cascade.max_objects, pl.det_count.data_ptr(), S, T, ids.data_ptr() if ids is not None else None,
                                         self.tracker.id.data_ptr() if ids is not None else None, self.M, self.at_id.data_ptr(),
                                         self.at_label.data_ptr(), self.at_logit.data_ptr(), self.at_frame.data_ptr(), self.frame.data_ptr(),
                                         HOLDS.index(self.cascade.hold), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), self._stream()),
              "fx_roi_attributes")
        return out

    def update(self, pl, fb, ids: Optional[torch.Tensor], names=()) -> None:
        """One frame of every stream: select, gather, classify, attribute; ``fetch`` then reads what the detections report."""
        self.select(pl, fb, ids, names)
        self.gather(fb)
        self._out = self.attributes(self.forward(), pl, ids)

    def fetch(self):
        """Host copies of the last update: (attr_label [S][T], attr_logit f32 tensor [S, T], attr_age [S][T]); the crops that did not fit
        the budget are added to ``left_seen``."""
        label, logit, age = self._out
        self.left_seen += int(self.roi_left.cpu().sum().item())
        return label.cpu().tolist(), logit.cpu(), age.cpu().tolist()

    def last(self):
        """Host copies of what the last update wrote: dict of attr_label / attr_logit / attr_age [S, T] and roi_win / roi_det / roi_count /
        roi_left, as numpy arrays."""
        src = dict(zip(("attr_label", "attr_logit", "attr_age"), self._out), roi_win=self.roi_win, roi_det=self.roi_det,
                   roi_count=self.roi_count, roi_left=self.roi_left)
        return {k: v.cpu().numpy().copy() for k, v in src.items()}


def attach(out: List, fetched, cascade: Cascade) -> None:
    """Set ``attr_id`` / ``attr_label`` / ``attr_conf`` of the detections of one packed batch: ``attr_conf`` is ``torch.sigmoid`` of the
    device logit in fp32, as ``ClassificationProcessor.pack_detections`` computes it, and the three are set only when it exceeds
    ``threshold or 0.5``."""
    labels, logits, _ = fetched
    names = cascade.classifier.model_info.classes
    conf = torch.sigmoid(logits.to(torch.float32)).tolist()
    thr = cascade.threshold or 0.5
    for dets, lrow, crow in zip(out, labels, conf):
        for d, l, p in zip(dets.detections, lrow, crow):
            if l >= 0 and p > thr:
                d.attr_id, d.attr_conf = int(l), p
                d.attr_label = names[l] if names and l < len(names) else None


def warn_left(classify, what: str = "infer_stream") -> None:
    """One warning when eligible objects were left unclassified for want of crop budget (clears the counter)."""
    if isinstance(classify, DeviceCascade) and classify.left_seen:
        n, classify.left_seen = classify.left_seen, 0
        warnings.warn(f"{what}(classify=): {n} eligible objects were not classified in their frame: every one of Cascade.max_objects = "
                      f"{classify.cascade.max_objects} crops of their stream was taken (raise max_objects or interval)", RuntimeWarning, stacklevel=4)
