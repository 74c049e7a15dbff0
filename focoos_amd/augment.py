"""Training augmentation on the device: the reference's ``DatasetAugmentations`` (focoos/data/default_aug.py:14-201)
as one HIP resample per batch instead of per-sample cv2 / PIL transforms on CPU workers.

  DatasetAugmentations, get_default_by_task   default_aug.py:14-99, 204-313   (fields, defaults, the per-task presets)
  sample_params                               the random draws of get_augmentations' pipeline (default_aug.py:101-201), in its order:
                                              colour (ColorAugSSDTransform's coin flips and operation order, transform.py:362-440), RandomFlip
                                              (augmentation.py:433-464), ResizeShortestEdge "range" (:492-566) or Resize for a non-square
                                              resolution (:470-486), RandomCrop "absolute" (:818-878)
  transform_boxes / transform_points          the mapper's box handling: apply_box, clip to the image, drop empty (data/utils.py:93-97, 242-266)
  DeviceAugmenter                             uploads the batch's sources once and runs fx_augment_images_u8 / fx_augment_labels (csrc/augment.hip)
  AugmentedDataset                            what ``FocoosModel.train`` takes as ``data_train`` to switch the augmenter on

Fields this engine does not build are refused at construction of the augmenter, by name (``check_supported``): rotation, zoom_out,
aspect_ratio, square, a non-default color_base_hue.  Nothing here falls back to a host pipeline."""
from __future__ import annotations

import copy
import ctypes
import sys
from dataclasses import dataclass, fields
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

IGNORE_LABEL = 255          # seg_pad_value of the semantic mappers
ORDER_NONE, ORDER_BCS, ORDER_BSC = 0, 1, 2
_DRAWS = 12                 # uniform draws consumed per image, whatever the configuration (records of one seed do not shift with the options)


@dataclass
class DatasetAugmentations:
    """default_aug.py:60-86: the same field names and defaults."""
    resolution: Union[int, Tuple[int, int]] = 640
    color_augmentation: float = 0.0
    color_base_brightness: int = 32
    color_base_saturation: float = 0.5
    color_base_contrast: float = 0.5
    color_base_hue: float = 18
    horizontal_flip: float = 0.0
    vertical_flip: float = 0.0
    zoom_out: float = 0.0
    zoom_out_side: float = 4.0
    rotation: float = 0.0
    aspect_ratio: float = 0.0
    square: float = 0.0
    scale_ratio: float = 0.0
    max_size: int = 4096
    crop: bool = False
    crop_size: Optional[int] = None

    def override(self, args):
        if not isinstance(args, dict):
            args = vars(args)
        for key, value in args.items():
            if hasattr(self, key) and value is not None:
                setattr(self, key, value)
        return self


_PRESETS = {   # default_aug.py:204-272
    "fai_instance_train": dict(resolution=1024, crop=True, scale_ratio=1.0, max_size=2048, horizontal_flip=0.5, color_augmentation=1.0),
    "fai_segmentation_train": dict(resolution=640, crop=True, scale_ratio=1.0, max_size=2048, color_augmentation=1.0, horizontal_flip=0.5),
    "fai_detection_train": dict(resolution=640, color_augmentation=1.0, horizontal_flip=0.5, aspect_ratio=0.5, zoom_out=0.5, zoom_out_side=4.0,
                                square=1.0, scale_ratio=0.5),
    "detection_train": dict(resolution=640, square=1.0, max_size=int(640 * 1.25), crop=True, scale_ratio=0.5, color_augmentation=1.0,
                            horizontal_flip=0.5),
    "segmentation_train": dict(resolution=640, crop=True, scale_ratio=0.5, color_augmentation=1.0, horizontal_flip=0.5),
    "detection_val": dict(resolution=640, square=1.0),
    "segmentation_val": dict(resolution=640),
    "classification_train": dict(resolution=224, scale_ratio=0.5, crop=True, color_augmentation=1.0, horizontal_flip=0.5),
    "classification_val": dict(resolution=224),
    "keypoints_train": dict(resolution=640, crop=True, scale_ratio=0.5, color_augmentation=1.0, horizontal_flip=0.0, aspect_ratio=0.0, rotation=0.0),
    "keypoints_val": dict(resolution=640),
}
_BY_TASK = {   # default_aug.py:275-310: task -> ((train, val), (advanced train, advanced val))
    "detection": (("detection_train", "detection_val"), ("fai_detection_train", "detection_val")),
    "semseg": (("segmentation_train", "segmentation_val"), ("fai_segmentation_train", "segmentation_val")),
    "instseg": (("segmentation_train", "segmentation_val"), ("fai_instance_train", "segmentation_val")),
    "classification": (("classification_train", "classification_val"),) * 2,
    "keypoint": (("keypoints_train", "keypoints_val"),) * 2,
}


def _task_value(task) -> str:
    return str(getattr(task, "value", task))


def get_default_by_task(task, resolution: Union[int, Tuple[int, int]] = 640, advanced: bool = False):
    """default_aug.py:275-313: (train, val) presets of a task at ``resolution``."""
    key = _task_value(task)
    if key not in _BY_TASK:
        raise ValueError(f"no default augmentations for task {task!r}")
    train, val = _BY_TASK[key][1 if advanced else 0]
    out = []
    for name in (train, val):
        a = DatasetAugmentations(**copy.deepcopy(_PRESETS[name]))
        a.resolution = resolution
        out.append(a)
    return out[0], out[1]


_REFUSED = ("rotation", "zoom_out", "aspect_ratio", "square", "color_base_hue")


def check_supported(augs: DatasetAugmentations) -> None:
    """The fields this engine does not build, refused by name when they differ from the dataclass default (never ignored)."""
    defaults = DatasetAugmentations()
    for name in _REFUSED:
        if getattr(augs, name) != getattr(defaults, name):
            raise NotImplementedError(f"DatasetAugmentations.{name}={getattr(augs, name)!r} is not built by the device augmenter "
                                      f"(only the default {getattr(defaults, name)!r}); built: resolution, flips, scale_ratio, crop / crop_size, "
                                      "max_size, color_augmentation with brightness / contrast / saturation")
    for name in ("horizontal_flip", "vertical_flip", "color_augmentation"):
        if not 0.0 <= float(getattr(augs, name)) <= 1.0:
            raise ValueError(f"DatasetAugmentations.{name} must lie in [0, 1], got {getattr(augs, name)!r}")


def _resolution(augs) -> Tuple[int, int]:
    r = augs.resolution
    return (int(r), int(r)) if isinstance(r, int) else (int(r[0]), int(r[1]))


def short_edge_range(augs: DatasetAugmentations) -> Tuple[int, int]:
    """default_aug.py:170-178: the [min, max] of ResizeShortestEdge's sampled short edge."""
    res = min(_resolution(augs))
    return int(2 ** (-augs.scale_ratio) * res), int(2 ** augs.scale_ratio * res)


def _shortest_edge_shape(h: int, w: int, size: int, max_size: int) -> Tuple[int, int]:
    """ResizeShortestEdge.get_output_shape, augmentation.py:548-565."""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size * 1.0, scale * w) if h < w else (scale * h, size * 1.0)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return max(1, int(newh + 0.5)), max(1, int(neww + 0.5))


@dataclass
class AugRecord:
    """Everything that happens to one image; geometry is a pure function of it.  Integer fields are pixels: the source (src_h, src_w) is
    resized to (res_h, res_w) after the flips, columns [crop_x, crop_x + crop_w) x rows [crop_y, crop_y + crop_h) of that are placed at
    (pad_x, pad_y) of the (out_h, out_w) output."""
    src_h: int
    src_w: int
    out_h: int
    out_w: int
    res_h: int
    res_w: int
    crop_x: int
    crop_y: int
    crop_w: int
    crop_h: int
    pad_x: int = 0
    pad_y: int = 0
    hflip: bool = False
    vflip: bool = False
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    order: int = ORDER_NONE
    short_edge: int = 0

    # the source window in source pixels, axis-aligned: (x0, y0) its top-left corner in the UNFLIPPED source, (sx, sy) source pixels per output pixel
    @property
    def sx(self) -> float:
        return self.src_w / self.res_w

    @property
    def sy(self) -> float:
        return self.src_h / self.res_h

    @property
    def x0(self) -> float:
        c = self.res_w - self.crop_x - self.crop_w if self.hflip else self.crop_x
        return c * self.sx

    @property
    def y0(self) -> float:
        c = self.res_h - self.crop_y - self.crop_h if self.vflip else self.crop_y
        return c * self.sy

    def to_struct(self):
        from ._lib import FxAugRecord

        return FxAugRecord(crop_w=self.crop_w, crop_h=self.crop_h, pad_x=self.pad_x, pad_y=self.pad_y, res_w=self.res_w, res_h=self.res_h,
                           crop_x=self.crop_x, crop_y=self.crop_y, flags=int(self.hflip) | (int(self.vflip) << 1) | (int(self.order) << 4),
                           brightness=self.brightness, contrast=self.contrast, saturation=self.saturation)


def identity_record(h: int, w: int) -> AugRecord:
    return AugRecord(src_h=h, src_w=w, out_h=h, out_w=w, res_h=h, res_w=w, crop_x=0, crop_y=0, crop_w=w, crop_h=h)


def sample_params(augs: DatasetAugmentations, sizes: Sequence[Sequence[int]], generator: torch.Generator) -> List[AugRecord]:
    """One record per image of original size ``sizes[i] = (H, W)``, drawn from the seeded CPU ``generator``: pure host code, the same seed
    gives the same records.  With ``crop`` the output is the crop size (smaller images are placed top-left and padded); without it the
    output is the largest resized size of the batch, every image top-left (ImageList.from_tensors)."""
    check_supported(augs)
    res_h, res_w = _resolution(augs)
    lo, hi = short_edge_range(augs)
    max_size = augs.max_size if augs.max_size else sys.maxsize
    crop_h, crop_w = (int(augs.crop_size),) * 2 if augs.crop_size else (res_h, res_w)
    strength = float(augs.color_augmentation)
    b_delta = int(augs.color_base_brightness * strength) / 255.0   # ColorAugSSD's +-delta counts, as a share of full scale
    c_delta, s_delta = augs.color_base_contrast * strength, augs.color_base_saturation * strength
    recs = []
    for H, W in sizes:
        H, W = int(H), int(W)
        if H <= 0 or W <= 0:
            raise ValueError(f"image size {(H, W)} is empty")
        u = torch.rand(_DRAWS, generator=generator, dtype=torch.float64).tolist()
        hflip, vflip = u[0] < augs.horizontal_flip, u[1] < augs.vertical_flip
        if res_h != res_w:                       # Resize(shape): the exact (height, width), scale_ratio ignored (default_aug.py:165-168)
            short, (rh, rw) = min(res_h, res_w), (res_h, res_w)
        else:
            short = min(hi, lo + int(u[2] * (hi - lo + 1)))       # np.random.randint(lo, hi + 1)
            rh, rw = _shortest_edge_shape(H, W, short, max_size)
        if augs.crop:
            ch, cw = min(crop_h, rh), min(crop_w, rw)
            cy, cx = min(rh - ch, int(u[3] * (rh - ch + 1))), min(rw - cw, int(u[4] * (rw - cw + 1)))
        else:
            ch, cw, cy, cx = rh, rw, 0, 0
        rec = AugRecord(src_h=H, src_w=W, out_h=crop_h if augs.crop else 0, out_w=crop_w if augs.crop else 0, res_h=rh, res_w=rw, crop_x=cx,
                        crop_y=cy, crop_w=cw, crop_h=ch, hflip=hflip, vflip=vflip, short_edge=short)
        if strength > 0:
            rec.order = ORDER_BCS if u[7] < 0.5 else ORDER_BSC
            if u[5] < 0.5:
                rec.brightness = 1.0 + (2.0 * u[6] - 1.0) * b_delta
            if u[8] < 0.5:
                rec.contrast = 1.0 + (2.0 * u[9] - 1.0) * c_delta
            if u[10] < 0.5:
                rec.saturation = 1.0 + (2.0 * u[11] - 1.0) * s_delta
        recs.append(rec)
    if not augs.crop:
        oh, ow = max(r.crop_h for r in recs), max(r.crop_w for r in recs)
        for r in recs:
            r.out_h, r.out_w = oh, ow
    return recs


def transform_points(points_xy: torch.Tensor, rec: AugRecord) -> torch.Tensor:
    """[N, 2] (x, y) in source pixels (continuous, pixel edges at integers) -> output pixels; not clipped."""
    p = torch.as_tensor(points_xy, dtype=torch.float64).reshape(-1, 2).clone()
    if rec.hflip:
        p[:, 0] = rec.src_w - p[:, 0]
    if rec.vflip:
        p[:, 1] = rec.src_h - p[:, 1]
    p[:, 0] = p[:, 0] * (rec.res_w / rec.src_w) - rec.crop_x + rec.pad_x
    p[:, 1] = p[:, 1] * (rec.res_h / rec.src_h) - rec.crop_y + rec.pad_y
    return p


def points_inside(points_xy_out: torch.Tensor, rec: AugRecord) -> torch.Tensor:
    """Which transformed points lie inside the placed window (the mapper drops keypoints outside the image)."""
    p = points_xy_out
    return (p[:, 0] >= rec.pad_x) & (p[:, 0] <= rec.pad_x + rec.crop_w) & (p[:, 1] >= rec.pad_y) & (p[:, 1] <= rec.pad_y + rec.crop_h)


def transform_boxes(boxes_xyxy: torch.Tensor, rec: AugRecord, threshold: float = 1e-5):
    """[N, 4] absolute xyxy in source pixels -> (boxes in output pixels clipped to the placed window, keep mask): apply_box on the four
    corners, clip to the image (data/utils.py:95-97), then ``Boxes.nonempty(threshold=1e-5)`` (filter_empty_instances, :242-266)."""
    b = torch.as_tensor(boxes_xyxy, dtype=torch.float64).reshape(-1, 4)
    p0, p1 = transform_points(b[:, :2], rec), transform_points(b[:, 2:], rec)
    lo, hi = torch.minimum(p0, p1), torch.maximum(p0, p1)
    wl = torch.tensor([rec.pad_x, rec.pad_y], dtype=torch.float64)
    wh = torch.tensor([rec.pad_x + rec.crop_w, rec.pad_y + rec.crop_h], dtype=torch.float64)
    lo, hi = torch.maximum(torch.minimum(lo, wh), wl), torch.maximum(torch.minimum(hi, wh), wl)
    out = torch.cat([lo, hi], dim=1)
    keep = ((out[:, 2] - out[:, 0]) > threshold) & ((out[:, 3] - out[:, 1]) > threshold)
    return out, keep


class AugmentedDataset:
    """``data`` (indexable, entries = DatasetEntry) plus the augmentations ``FocoosModel.train`` applies to it on the device."""

    def __init__(self, data, augs: DatasetAugmentations):
        check_supported(augs)
        self.data, self.augmentations = data, augs

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i]


# ------------------------------------------------------------------------------------------------------------------------ device side
def _hwc_u8(image) -> np.ndarray:
    im = image.numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if im.ndim == 3 and im.shape[0] == 3 and im.shape[-1] != 3:
        im = im.transpose(1, 2, 0)
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[-1] != 3:
        raise ValueError(f"the device augmenter takes decoded uint8 RGB images, got {im.dtype} {im.shape}")
    return np.ascontiguousarray(im)


class _Upload:
    """The per-batch tables in both memories: the device copies are what the kernels read, the host copies what the library validates."""

    def __init__(self, recs: Sequence[AugRecord], device):
        from ._lib import FxAugRecord

        self.B = len(recs)
        self.recs_host = (FxAugRecord * self.B)(*[r.to_struct() for r in recs])
        self.sizes_host = np.array([[r.src_h, r.src_w] for r in recs], dtype=np.int32)
        self.recs = torch.frombuffer(bytearray(bytes(self.recs_host)), dtype=torch.uint8).to(device)
        self.sizes = torch.from_numpy(self.sizes_host).to(device)


def augment_images(sources: Sequence[np.ndarray], recs: Sequence[AugRecord], device, pad_value: int = 0, out: Optional[torch.Tensor] = None,
                   tables: Optional[_Upload] = None) -> torch.Tensor:
    """fx_augment_images_u8 on ``sources`` (HWC uint8 arrays) with one record each -> uint8 [B, Ho, Wo, 3] on ``device`` (current stream).
    The sources go up once, as one concatenated buffer plus offsets."""
    from . import _lib

    B = len(sources)
    assert B == len(recs) and B > 0
    Ho, Wo = recs[0].out_h, recs[0].out_w
    if any((r.out_h, r.out_w) != (Ho, Wo) for r in recs):
        raise ValueError("the records of one batch must share the output size")
    for s, r in zip(sources, recs):
        if s.shape != (r.src_h, r.src_w, 3) or s.dtype != np.uint8:
            raise ValueError(f"source {s.shape} {s.dtype} does not match its record {(r.src_h, r.src_w, 3)}")
    flat = np.concatenate([s.reshape(-1) for s in sources])
    offs = np.cumsum([0] + [s.size for s in sources])[:-1].astype(np.int64)
    dev = torch.device(device)
    t = tables or _Upload(recs, dev)
    src_d = torch.from_numpy(flat).to(dev)
    off_d = torch.from_numpy(offs).to(dev)
    if out is None:
        out = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    assert out.is_contiguous() and tuple(out.shape) == (B, Ho, Wo, 3) and out.dtype == torch.uint8
    need_mean = any(r.order != ORDER_NONE and np.float32(r.contrast) != np.float32(1.0) for r in recs)
    ws = torch.empty(B * 32, dtype=torch.int64, device=dev) if need_mean else None
    lib = _lib.load("bf16")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.fx_augment_images_u8(src_d.data_ptr(), off_d.data_ptr(), t.sizes.data_ptr(), t.recs.data_ptr(), offs.ctypes.data, int(flat.size),
                                  t.sizes_host.ctypes.data, ctypes.addressof(t.recs_host), B, out.data_ptr(), Ho, Wo, int(pad_value),
                                  ws.data_ptr() if need_mean else None, ctypes.c_void_p(stream))
    _lib.check(rc, "fx_augment_images_u8")
    return out


def augment_labels(planes: Sequence[np.ndarray], plane_rec: Sequence[int], recs: Sequence[AugRecord], device, pad_value: int,
                   want_flags: bool = False, tables: Optional[_Upload] = None):
    """fx_augment_labels: ``planes[p]`` ([H, W] uint8, or all int32) mapped with record ``plane_rec[p]`` -> ([P, Ho, Wo] of the same type,
    int32 [P] non-empty flags or None)."""
    from . import _lib

    P = len(planes)
    assert P == len(plane_rec) and P > 0
    Ho, Wo = recs[0].out_h, recs[0].out_w
    i32 = any(p.dtype != np.uint8 for p in planes)
    for p, b in zip(planes, plane_rec):
        if p.shape != (recs[b].src_h, recs[b].src_w):
            raise ValueError(f"plane {p.shape} does not match the source size {(recs[b].src_h, recs[b].src_w)} of its record")
    flat = np.concatenate([np.ascontiguousarray(p).astype(np.int32 if i32 else np.uint8, copy=False).reshape(-1) for p in planes])
    offs = np.cumsum([0] + [p.size for p in planes])[:-1].astype(np.int64)
    pr = np.asarray(plane_rec, dtype=np.int32)
    dev = torch.device(device)
    t = tables or _Upload(recs, dev)
    src_d, off_d, pr_d = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(pr).to(dev)
    out = torch.empty((P, Ho, Wo), dtype=torch.int32 if i32 else torch.uint8, device=dev)
    flags = torch.zeros(P, dtype=torch.int32, device=dev) if want_flags else None
    lib = _lib.load("bf16")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.fx_augment_labels(src_d.data_ptr(), off_d.data_ptr(), pr_d.data_ptr(), t.sizes.data_ptr(), t.recs.data_ptr(), offs.ctypes.data,
                               int(flat.size), pr.ctypes.data, t.sizes_host.ctypes.data, ctypes.addressof(t.recs_host), P, t.B, out.data_ptr(),
                               Ho, Wo, int(i32), int(pad_value), flags.data_ptr() if want_flags else None, ctypes.c_void_p(stream))
    _lib.check(rc, "fx_augment_labels")
    return out, flags


_TASKS = ("detection", "instseg", "semseg")


def task_of_family(family: str) -> str:
    try:
        return {"fai_detr": "detection", "fai_mf": "instseg", "bisenetformer": "semseg"}[family]
    except KeyError:
        raise NotImplementedError(f"no device augmentation for model family {family!r}") from None


class DeviceAugmenter:
    """``augmenter(entries, generator)`` -> (uint8 NHWC batch, targets) in the forms ``TrainStep.step`` takes:
    detection: [DETRTargets] (classes, cxcywh boxes normalised by the batch size, as DETRProcessor._preprocess_entries);
    instseg:   [MaskFormerTargets] from ``instances.masks`` ([T, H, W]), instances the crop removed dropped;
    semseg:    [MaskFormerTargets] built from the augmented label map of ``entry.sem_seg`` (one binary mask per class present, the ignore
               label excluded, as the semantic mapper does) - or from ``instances.masks`` like instseg when the entry carries no label map.
    Unsupported fields raise here, before anything touches the GPU."""

    def __init__(self, augs: DatasetAugmentations, task, device):
        check_supported(augs)
        task = _task_value(task)
        if task not in _TASKS:
            raise NotImplementedError(f"no device augmentation for task {task!r} (built: {', '.join(_TASKS)})")
        self.augs, self.task, self.device = copy.deepcopy(augs), task, torch.device(device)
        self.last_records: List[AugRecord] = []
        self.last_labels: Optional[torch.Tensor] = None

    def __call__(self, entries, generator: torch.Generator):
        from .ports import DETRTargets, MaskFormerTargets

        sources = [_hwc_u8(e.image) for e in entries]
        recs = sample_params(self.augs, [s.shape[:2] for s in sources], generator)
        self.last_records = recs
        dev = self.device
        tables = _Upload(recs, dev)
        images = augment_images(sources, recs, dev, pad_value=0, tables=tables)
        Ho, Wo = recs[0].out_h, recs[0].out_w
        targets = []
        if self.task == "detection":
            scale = torch.tensor([Wo, Ho, Wo, Ho], dtype=torch.float64)
            for e, r in zip(entries, recs):
                inst = e.instances
                assert inst is not None and inst.has("boxes") and inst.has("classes"), "boxes and classes are required for training"
                bx, keep = transform_boxes(inst.boxes.tensor.detach().cpu(), r)
                bx = bx[keep] / scale
                cxcywh = torch.stack([(bx[:, 0] + bx[:, 2]) / 2, (bx[:, 1] + bx[:, 3]) / 2, bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], -1)
                targets.append(DETRTargets(labels=torch.as_tensor(inst.classes)[keep].to(dev), boxes=cxcywh.to(dev, torch.float32)))
            return images, targets
        if self.task == "semseg" and all(getattr(e, "sem_seg", None) is not None for e in entries):
            maps = [np.asarray(e.sem_seg) for e in entries]
            labels, _ = augment_labels(maps, list(range(len(maps))), recs, dev, IGNORE_LABEL, tables=tables)
            self.last_labels = labels
            for lab in labels:
                classes = torch.unique(lab)
                classes = classes[classes != IGNORE_LABEL]
                targets.append(MaskFormerTargets(labels=classes.long(), masks=lab[None] == classes[:, None, None]))
            return images, targets
        planes, plane_rec, counts = [], [], []
        for b, e in enumerate(entries):
            inst = e.instances
            assert inst is not None and inst.has("masks") and inst.has("classes"), "masks and classes are required for training"
            gm = inst.masks.tensor if hasattr(inst.masks, "tensor") else inst.masks
            gm = torch.as_tensor(gm).detach().cpu()
            gm = (gm != 0).to(torch.uint8).numpy()
            counts.append(len(gm))
            planes += list(gm)
            plane_rec += [b] * len(gm)
        if planes:
            masks, flags = augment_labels(planes, plane_rec, recs, dev, 0, want_flags=True, tables=tables)
            keep = flags > 0
        start = 0
        for e, n in zip(entries, counts):
            cls = torch.as_tensor(e.instances.classes).to(dev)
            if n == 0:
                targets.append(MaskFormerTargets(labels=cls, masks=torch.zeros((0, Ho, Wo), dtype=torch.uint8, device=dev)))
                continue
            k = keep[start:start + n]
            targets.append(MaskFormerTargets(labels=cls[k], masks=masks[start:start + n][k]))
            start += n
        return images, targets
