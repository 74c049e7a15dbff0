"""COCO bbox AP for the RT-DETR family: FocoosModel.eval_detection and DetectionEvaluator (trainer/evaluation/detection_evaluation.py:35-290,
task "bbox") without pycocotools.

The algorithm is COCOeval's (computeIoU, evaluateImg, accumulate, summarize) for iouType "bbox", useCats = 1, maxDets = 100 (the only maxDets
row the reference's result dict reads), the ten IoU thresholds linspace(.5, .95, 10), the 101 recall points and the four COCO area ranges.
It is split in two:

* matching (computeIoU + evaluateImg) produces one record per scored detection - image id, category, rank in the image's score order,
  score, a 40-bit ``matched`` and a 40-bit ``ignored`` mask (bit 10 a + t = area range a, threshold t) - and the [K, 4] count of
  non-ignored ground-truth boxes (``npig``).  The driver runs it on the device (fx_detr_eval_boxes_f32 + fx_coco_match_bbox,
  csrc/coco_eval.hip) on the engine's buffers; ``DetectionEvaluator.process / evaluate`` run the same decisions vectorised in numpy on the host.
* accumulation (accumulate + summarize) runs on the records in numpy float64, with the reference's own formulas.

Reference behaviour that is kept on purpose:
* only images with at least one prediction enter the evaluation; the ground truth of every other image is dropped
  (DetectionEvaluator.evaluate :137-147 builds the image list from the predictions);
* ``image_id`` is the dataset index (the driver) / ``DatasetEntry.image_id`` (``process``);
* images are taken in ascending ``image_id`` order (COCOeval sorts imgIds; the order decides score ties);
* a ground-truth box is ignored when it is a crowd, carries ``ignore`` or has an area outside the range (evaluateImg; note that
  pycocotools' ``_prepare`` overwrites ``ignore`` with ``iscrowd``, so an annotation with ``ignore`` = 1 and ``iscrowd`` = 0 counts there);
* values are x 100, a value that cannot be computed is None, per-category rows exist only with more than one class.

Segm AP (iouType "segm") shares everything after the IoU: ``InstanceSegmentationEvaluator`` is the host form, focoos_amd/segm_eval.py the
device path behind ``FocoosModel.eval_instance_segmentation``.  Mask IoU is maskApi's rleIou on integers: 0 when the masks share no pixel,
else inter / (crowd ? |d| : |d| + |g| - inter) as one fp64 division; a detection's area is its mask's pixel count.  Ground-truth masks are
dense arrays, uncompressed RLE or ``instances.masks``; polygons and compressed RLE strings are refused (ground_truth_masks).

Keypoints, maxDets 1 / 10 and the AR rows are not built.  ``FocoosModel.eval`` keeps refusing detection and instance segmentation;
this module is reached through ``FocoosModel.eval_detection`` / ``eval_instance_segmentation``."""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from typing import List, Optional, Sequence

import numpy as np
import torch

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
MAX_DETS = 100
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
_NT, _NA = len(IOU_THRS), len(AREA_RNG)
_LANES = _NT * _NA
_LANE_AREA = np.repeat(np.arange(_NA), _NT)
_LANE_THR = np.minimum(np.tile(IOU_THRS, _NA), 1 - 1e-10)
_BITS = np.arange(_LANES, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- records
class MatchRecords:
    """Per scored detection: image_id int64, category int32, rank int32, score float64, matched / ignored uint64; ``npig`` int64 [K, 4]."""

    FIELDS = (("image_id", np.int64), ("category", np.int32), ("rank", np.int32), ("score", np.float64), ("matched", np.uint64),
              ("ignored", np.uint64))

    def __init__(self, K: int, **arrays):
        self.K = int(K)
        for name, dt in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays.get(name, np.zeros(0, dt)), dtype=dt))
        self.npig = np.asarray(arrays.get("npig", np.zeros((self.K, _NA), np.int64)), dtype=np.int64).reshape(self.K, _NA)
        self.images = np.asarray(arrays.get("images", np.zeros(0, np.int64)), dtype=np.int64)   # ids of the images that were evaluated

    def __len__(self):
        return self.image_id.size

    def state(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self.FIELDS}
        d.update(npig=self.npig, images=self.images)
        return d

    @classmethod
    def merge(cls, parts: Sequence["MatchRecords"]) -> "MatchRecords":
        """Shards of one evaluation -> one record set ordered by image id (npig is an integer sum)."""
        K = parts[0].K
        arrays = {name: np.concatenate([getattr(p, name) for p in parts]) for name, _ in cls.FIELDS}
        images = np.concatenate([p.images for p in parts])
        if np.unique(images).size != images.size:
            raise ValueError("an image id was evaluated more than once")
        order = np.lexsort((arrays["rank"], arrays["category"], arrays["image_id"]))
        arrays = {k: v[order] for k, v in arrays.items()}
        return cls(K, npig=sum(p.npig for p in parts), images=np.sort(images), **arrays)


def gather_records(rec: MatchRecords, dst: int = 0) -> Optional[MatchRecords]:
    """All ranks' records on rank ``dst`` (gather_object of the numpy arrays), merged in image order; None on the other ranks."""
    import torch.distributed as dist

    world, rank = dist.get_world_size(), dist.get_rank()
    box = [None] * world if rank == dst else None
    dist.gather_object(rec.state(), box, dst=dst)
    if rank != dst:
        return None
    return MatchRecords.merge([MatchRecords(rec.K, **s) for s in box])


# ---------------------------------------------------------------------------------------------------------------- ground truth
def ground_truth(entry):
    """(box XYWH float64 [G, 4], category int32 [G], flag int32 [G] (bit 0 crowd, bit 1 ignore), area float64 [G]) of a dataset entry:
    ``annotations`` (dicts with ``bbox`` XYWH absolute and ``category_id``; ``area`` defaults to w * h and ``iscrowd`` to 0, create_coco
    :386-392) when present, else ``instances.boxes`` (absolute XYXY, converted in float64) and ``instances.classes``."""
    anns = entry.get("annotations") if isinstance(entry, dict) else getattr(entry, "annotations", None)
    if anns is not None:
        G = len(anns)
        box, cat = np.zeros((G, 4), np.float64), np.zeros(G, np.int32)
        flag, area = np.zeros(G, np.int32), np.zeros(G, np.float64)
        for i, a in enumerate(anns):
            bb = [float(v) for v in a["bbox"]]
            box[i], cat[i] = bb, int(a["category_id"])
            area[i] = float(a["area"]) if "area" in a else bb[2] * bb[3]
            flag[i] = (1 if a.get("iscrowd", 0) else 0) | (2 if a.get("ignore", 0) else 0)
        return box, cat, flag, area
    inst = entry.get("instances") if isinstance(entry, dict) else getattr(entry, "instances", None)
    if inst is None or not inst.has("boxes"):
        z = np.zeros(0)
        return np.zeros((0, 4)), z.astype(np.int32), z.astype(np.int32), z
    b = inst.boxes.tensor if hasattr(inst.boxes, "tensor") else inst.boxes
    b = np.asarray(torch.as_tensor(b).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4)
    box = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1) if len(b) else np.zeros((0, 4))
    cat = np.asarray(torch.as_tensor(inst.classes).cpu().numpy(), dtype=np.int32).reshape(-1)
    return box, cat, np.zeros(len(cat), np.int32), box[:, 2] * box[:, 3]


def _rle_to_mask(seg: dict) -> np.ndarray:
    """uncompressed COCO RLE {"size": [H, W], "counts": [run of 0s, run of 1s, ...]} (column-major) -> bool [H, W]"""
    counts = seg["counts"]
    if isinstance(counts, (str, bytes)):
        raise NotImplementedError("ground-truth segmentation as a compressed RLE string is not decoded (maskApi's string codec cannot be "
                                  "checked against pycocotools here); give a dense mask or an uncompressed RLE")
    H, W = (int(v) for v in seg["size"])
    runs = np.asarray(counts, np.int64)
    if (runs < 0).any() or int(runs.sum()) != H * W:
        raise ValueError(f"uncompressed RLE counts sum to {int(runs.sum())}, the size is {H} x {W}")
    flat = np.repeat(np.arange(len(runs)) % 2 == 1, runs)
    return flat.reshape(W, H).T


def ground_truth_masks(entry):
    """(mask bool [G, H, W], category int32 [G], flag int32 [G] (bit 0 crowd, bit 1 ignore), area float64 [G]) of a dataset entry, H x W its
    ``height`` x ``width``.  ``annotations[i]["segmentation"]`` as a 2-D array or an uncompressed RLE dict when annotations are present
    (``area`` defaults to the mask's pixel count, create_coco :412), else ``instances.masks`` (BitMasks or a [G, H, W] tensor) with
    ``instances.classes``.  Polygon lists and compressed RLE raise NotImplementedError; a mask of another shape raises ValueError."""
    get = (lambda k: entry.get(k)) if isinstance(entry, dict) else (lambda k: getattr(entry, k, None))
    H, W = int(get("height") or 0), int(get("width") or 0)
    anns = get("annotations")
    masks = []
    if anns is not None:
        G = len(anns)
        cat, flag, area = np.zeros(G, np.int32), np.zeros(G, np.int32), np.zeros(G, np.float64)
        for i, a in enumerate(anns):
            seg = a.get("segmentation")
            if seg is None:
                raise ValueError("segm evaluation needs a segmentation on every annotation")
            if isinstance(seg, dict):
                m = _rle_to_mask(seg)
            elif isinstance(seg, (list, tuple)):                      # COCO polygons: a list of [x0, y0, x1, y1, ...] lists
                raise NotImplementedError("ground-truth segmentation as polygon lists is not rasterised (maskApi's polygon rasteriser cannot be "
                                          "checked against pycocotools here); give a dense mask or an uncompressed RLE")
            else:
                m = np.asarray(seg.cpu() if isinstance(seg, torch.Tensor) else seg)
                if m.ndim != 2:
                    raise ValueError(f"a dense ground-truth mask must be 2-D, got shape {m.shape}")
                m = m != 0
            if m.shape != (H, W):
                raise ValueError(f"ground-truth mask {m.shape} does not match the entry's (height, width) {(H, W)}")
            masks.append(m)
            cat[i] = int(a["category_id"])
            area[i] = float(a["area"]) if "area" in a else float(m.sum())
            flag[i] = (1 if a.get("iscrowd", 0) else 0) | (2 if a.get("ignore", 0) else 0)
        return (np.stack(masks) if masks else np.zeros((0, H, W), bool)), cat, flag, area
    inst = get("instances")
    if inst is None or not inst.has("masks"):
        z = np.zeros(0)
        return np.zeros((0, H, W), bool), z.astype(np.int32), z.astype(np.int32), z
    m = inst.masks.tensor if hasattr(inst.masks, "tensor") else inst.masks
    m = np.asarray(torch.as_tensor(m).detach().cpu().numpy()) != 0
    m = m.reshape((-1,) + m.shape[-2:])
    if len(m) and m.shape[1:] != (H, W):
        raise ValueError(f"ground-truth mask {m.shape[1:]} does not match the entry's (height, width) {(H, W)}")
    cat = np.asarray(torch.as_tensor(inst.classes).cpu().numpy(), dtype=np.int32).reshape(-1)
    return m.reshape(len(cat), H, W), cat, np.zeros(len(cat), np.int32), m.reshape(len(cat), -1).sum(1).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- host matching
def bbox_iou(d: np.ndarray, g: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """maskApi bbIou on XYWH float64 boxes: [D, G]; the union of a crowd box is the detection's own area."""
    w = np.minimum(d[:, None, 2] + d[:, None, 0], g[None, :, 2] + g[None, :, 0]) - np.maximum(d[:, None, 0], g[None, :, 0])
    h = np.minimum(d[:, None, 3] + d[:, None, 1], g[None, :, 3] + g[None, :, 1]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = w * h
    da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None, :]
    u = np.where(crowd[None, :], da, (da + ga) - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = inter / u
    return np.where((w <= 0) | (h <= 0), 0.0, o)


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def pack_rows(masks: np.ndarray) -> np.ndarray:
    """bool [N, H, W] -> uint8 [N, H, 8 ceil(W / 64)]: the kernels' layout (64 consecutive x of a row are one little-endian 64-bit word,
    tail bits zero); ``.view(np.int32)`` is what MaskFormerProcessor.unpack_masks reads."""
    m = np.asarray(masks, dtype=bool)
    N, H, W = m.shape
    out = np.zeros((N, H, 8 * ((W + 63) // 64)), np.uint8)
    if N and H and W:
        out[:, :, : (W + 7) // 8] = np.packbits(m, axis=-1, bitorder="little")
    return out


def popcount(packed: np.ndarray) -> np.ndarray:
    """set bits of every plane of pack_rows' output: int64 [N]"""
    return _POP8[packed].reshape(packed.shape[0], -1).sum(1) if packed.shape[0] else np.zeros(0, np.int64)


def mask_iou(dp: np.ndarray, dn: np.ndarray, gp: np.ndarray, gn: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """maskApi rleIou on packed masks and their pixel counts: [D, G] float64; integers until the one division."""
    D, G = len(dp), len(gp)
    inter = np.zeros((D, G), np.int64)
    if G:
        for d in range(D):
            inter[d] = _POP8[dp[d][None] & gp].reshape(G, -1).sum(1)
    u = np.where(crowd[None, :], dn[:, None], dn[:, None] + gn[None, :] - inter)
    return np.where(inter == 0, 0.0, inter / np.where(inter == 0, 1, u))


def _pack(bits: np.ndarray) -> np.ndarray:
    """bool [n, 40] -> uint64 [n]"""
    return np.bitwise_or.reduce(bits.astype(np.uint64) << _BITS[None, :], axis=1) if bits.shape[0] else np.zeros(0, np.uint64)


def _unpack(words: np.ndarray) -> np.ndarray:
    return ((words[:, None] >> _BITS[None, :]) & np.uint64(1)).astype(bool)


def match_image_category(dbox: np.ndarray, gbox: np.ndarray, gflag: np.ndarray, garea: np.ndarray):
    """evaluateImg for one (image, category) of boxes: ``dbox`` the detections already in descending score order and cut to MAX_DETS.
    Returns (matched bool [D, 40], ignored bool [D, 40], npig [4])."""
    iou = bbox_iou(dbox, gbox, (gflag & 1).astype(bool)) if len(dbox) and len(gbox) else np.zeros((len(dbox), len(gbox)))
    return match_from_iou(iou, dbox[:, 2] * dbox[:, 3], gflag, garea)


def match_from_iou(iou: np.ndarray, darea: np.ndarray, gflag: np.ndarray, garea: np.ndarray):
    """evaluateImg from the [D, G] IoU matrix (bbox_iou or mask_iou; detections in descending score order, cut to MAX_DETS) and the
    detections' areas.  The 40 (area range, threshold) pairs advance together, one detection per step.  Returns (matched bool [D, 40],
    ignored bool [D, 40], npig [4])."""
    D, G = iou.shape
    d_out = (darea[:, None] < AREA_RNG[None, :, 0]) | (darea[:, None] > AREA_RNG[None, :, 1])        # [D, 4]
    if G == 0 or D == 0:
        gig = (gflag[None, :] != 0) | (garea[None, :] < AREA_RNG[:, :1]) | (garea[None, :] > AREA_RNG[:, 1:])
        return np.zeros((D, _LANES), bool), d_out[:, _LANE_AREA], (~gig).sum(1).astype(np.int64)
    crowd = (gflag & 1).astype(bool)
    gig = (gflag[None, :] != 0) | (garea[None, :] < AREA_RNG[:, :1]) | (garea[None, :] > AREA_RNG[:, 1:])    # [4, G]
    order = np.argsort(gig, axis=1, kind="mergesort")                                                      # non-ignored first, stable
    nn = (~gig).sum(1)
    tile = iou[:, order][:, _LANE_AREA, :]                      # [D, 40, G] in each lane's gt order
    ig_l = np.take_along_axis(gig, order, 1)[_LANE_AREA]        # [40, G]
    crowd_l = crowd[order][_LANE_AREA]
    first = np.arange(G)[None, :] < nn[_LANE_AREA][:, None]     # the non-ignored section
    taken = np.zeros((_LANES, G), bool)
    matched, ignored = np.zeros((D, _LANES), bool), np.zeros((D, _LANES), bool)
    lanes = np.arange(_LANES)
    for d in range(D):
        row = tile[d]
        ok = (row >= _LANE_THR[:, None]) & (~taken | crowd_l)
        ok_first = ok & first
        use = np.where(ok_first.any(1)[:, None], ok_first, ok & ~first)   # a non-ignored match stops the pass before the ignored section
        found = use.any(1)
        v = np.where(use, row, -1.0)
        best = (v == v.max(1)[:, None]) & use
        m = G - 1 - np.argmax(best[:, ::-1], axis=1)                      # the last gt of the best IoU wins
        matched[d] = found
        ignored[d] = np.where(found, ig_l[lanes, m], d_out[d, _LANE_AREA])
        taken[lanes[found], m[found]] = True
    return matched, ignored, nn.astype(np.int64)


def match_image(image_id: int, dbox: np.ndarray, dscore: np.ndarray, dcls: np.ndarray, gt, K: int) -> MatchRecords:
    """computeIoU + evaluateImg of one image on the host.  ``dbox`` XYWH float64 [N, 4] (every row a prediction), ``gt`` of ground_truth()."""
    gbox, gcat, gflag, garea = gt
    return _match_image(image_id, dscore, dcls, gcat, K, lambda di, gi: match_image_category(dbox[di], gbox[gi], gflag[gi], garea[gi]))


def match_image_masks(image_id: int, dmask: np.ndarray, dscore: np.ndarray, dcls: np.ndarray, gt, K: int) -> MatchRecords:
    """The segm form: ``dmask`` bool [N, H, W] (every plane a prediction, empty ones included), ``gt`` of ground_truth_masks()."""
    gmask, gcat, gflag, garea = gt
    dp, gp = pack_rows(dmask), pack_rows(gmask)
    dn, gn = popcount(dp), popcount(gp)

    def one(di, gi):
        iou = mask_iou(dp[di], dn[di], gp[gi], gn[gi], (gflag[gi] & 1).astype(bool))
        return match_from_iou(iou, dn[di].astype(np.float64), gflag[gi], garea[gi])

    return _match_image(image_id, dscore, dcls, gcat, K, one)


def _match_image(image_id: int, dscore: np.ndarray, dcls: np.ndarray, gcat: np.ndarray, K: int, match) -> MatchRecords:
    """Per category present in the image: detections in stable descending score order cut to MAX_DETS, ``match(det indices, gt indices)``."""
    parts = {name: [] for name, _ in MatchRecords.FIELDS}
    npig = np.zeros((K, _NA), np.int64)
    cats = np.union1d(dcls, gcat)
    for c in cats[(cats >= 0) & (cats < K)]:
        di = np.flatnonzero(dcls == c)
        di = di[np.argsort(-dscore[di], kind="mergesort")][:MAX_DETS]
        gi = np.flatnonzero(gcat == c)
        m, ig, nn = match(di, gi)
        npig[c] += nn
        parts["image_id"].append(np.full(len(di), image_id, np.int64))
        parts["category"].append(np.full(len(di), c, np.int32))
        parts["rank"].append(np.arange(len(di), dtype=np.int32))
        parts["score"].append(dscore[di])
        parts["matched"].append(_pack(m))
        parts["ignored"].append(_pack(ig))
    arrays = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in parts.items()}
    return MatchRecords(K, npig=npig, images=[image_id], **arrays)


# ---------------------------------------------------------------------------------------------------------------- accumulate / summarize
def accumulate(rec: MatchRecords) -> np.ndarray:
    """COCOeval.accumulate at maxDets = 100: precision [T = 10, R = 101, K, A = 4], -1 where no non-ignored ground truth exists."""
    K = rec.K
    precision = -np.ones((_NT, len(REC_THRS), K, _NA))
    order = np.lexsort((rec.rank, rec.image_id, rec.category))      # per category: images ascending, detections in score order
    bounds = np.searchsorted(rec.category[order], np.arange(K + 1))
    for k in range(K):
        if not rec.npig[k].any():
            continue
        sl = order[bounds[k]:bounds[k + 1]]
        o = np.argsort(-rec.score[sl], kind="mergesort")
        dtm, dtig = _unpack(rec.matched[sl][o]), _unpack(rec.ignored[sl][o])
        tp_sum = np.cumsum(dtm & ~dtig, axis=0).astype(dtype=float)
        fp_sum = np.cumsum(~dtm & ~dtig, axis=0).astype(dtype=float)
        nd = len(sl)
        for a in range(_NA):
            npig = int(rec.npig[k, a])
            if npig == 0:
                continue
            for t in range(_NT):
                tp, fp = tp_sum[:, a * _NT + t], fp_sum[:, a * _NT + t]
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[::-1])[::-1]          # for i in range(nd - 1, 0, -1): pr[i - 1] = max(pr[i - 1], pr[i])
                inds = np.searchsorted(rc, REC_THRS, side="left")
                q = np.zeros(len(REC_THRS))
                ok = inds < nd
                q[ok] = pr[inds[ok]]
                precision[t, :, k, a] = q
    return precision


def summarize(precision: np.ndarray, class_names: Sequence[str]) -> "OrderedDict[str, Optional[float]]":
    """COCOeval.summarize's six AP rows + _derive_coco_results (:222-290): x 100, None where a value cannot be computed."""

    def ap(t, a):
        s = precision[:, :, :, a] if t is None else precision[t:t + 1, :, :, a]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else np.mean(s)

    stats = [ap(None, 0), ap(0, 0), ap(5, 0), ap(None, 1), ap(None, 2), ap(None, 3)]
    res = OrderedDict((m, float(s * 100 if s >= 0 else "nan")) for m, s in zip(METRICS, stats))
    if class_names is not None and len(class_names) > 1:
        assert len(class_names) == precision.shape[2], f"Found {len(class_names)} classes, but precision has dimension {precision.shape[2]}"
        for idx, name in enumerate(class_names):
            p = precision[:, :, idx, 0]
            p = p[p > -1]
            res["AP-" + str(name)] = float((np.mean(p) if p.size else float("nan")) * 100)
    return OrderedDict((k, (v if np.isfinite(v) else None)) for k, v in res.items())


def results_from(rec: MatchRecords, class_names: Sequence[str], key: str = "bbox") -> "OrderedDict":
    return OrderedDict({key: summarize(accumulate(rec), class_names)})


# ---------------------------------------------------------------------------------------------------------------- evaluator
class DetectionEvaluator:
    """The reference's DetectionEvaluator for task "bbox" on the host.  ``process(inputs, outputs)``: ``inputs`` dataset entries with
    ``image_id`` and their ground truth (ground_truth()), ``outputs`` either DETRProcessor.eval_postprocess's ``[{"instances": Instances}]``
    or raw arrays ``[{"boxes": XYXY absolute float32 [N, 4], "scores": [N], "classes": [N]}]``.  The XYXY -> XYWH subtraction is done in
    float32 (BoxMode.convert on the float32 array), everything after it in float64.  ``evaluate()`` -> ``{"bbox": {...}}`` ({} without a
    prediction).  See the module docstring for the reference behaviour that is kept."""

    def __init__(self, class_names: Sequence[str]):
        self.class_names = list(class_names)
        self.reset()

    def reset(self):
        self._images = {}

    @staticmethod
    def _arrays(output):
        if "instances" in output:
            inst = output["instances"]
            if len(inst) == 0:
                return np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
            boxes, scores, classes = inst.boxes.tensor, inst.scores, inst.classes
        elif "boxes" in output:
            boxes, scores, classes = output["boxes"], output["scores"], output["classes"]
        else:
            raise Exception("No instances in output?!")
        to_np = lambda t, dt: np.array(torch.as_tensor(t).detach().cpu().numpy(), dtype=dt)   # noqa: E731
        return to_np(boxes, np.float32).reshape(-1, 4), to_np(scores, np.float32).reshape(-1), to_np(classes, np.int64).reshape(-1)

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            image_id = inp.get("image_id") if isinstance(inp, dict) else getattr(inp, "image_id", None)
            assert image_id is not None, "Image ID must be present in the input!"
            if int(image_id) in self._images:
                raise ValueError(f"image id {image_id} was processed twice")
            boxes, scores, classes = self._arrays(out)
            if len(boxes) == 0:
                continue                                     # an image without predictions contributes nothing, its ground truth included
            boxes[:, 2] -= boxes[:, 0]                        # BoxMode.convert XYXY_ABS -> XYWH_ABS on the float32 array
            boxes[:, 3] -= boxes[:, 1]
            self._images[int(image_id)] = (boxes.astype(np.float64), scores.astype(np.float64), classes, ground_truth(inp))

    def records(self) -> Optional[MatchRecords]:
        K = len(self.class_names)
        parts = [match_image(i, *self._images[i], K) for i in sorted(self._images)]
        return MatchRecords.merge(parts) if parts else None

    def evaluate(self):
        rec = self.records()
        if rec is None:
            return {}
        return results_from(rec, self.class_names)


class InstanceSegmentationEvaluator:
    """The reference's InstanceSegmentationEvaluator (DetectionEvaluator with task "segm") on the host.  ``process(inputs, outputs)``:
    ``inputs`` dataset entries with ``image_id``, ``height``, ``width`` and their ground truth (ground_truth_masks()), ``outputs`` either
    MaskFormerProcessor.eval_postprocess's ``[{"instances": Instances}]`` (masks, scores, classes) or raw arrays ``[{"masks": bool [N, H, W],
    "scores": [N], "classes": [N]}]``.  Every prediction is scored, an empty mask included (instance_inference filters nothing).
    ``evaluate()`` -> ``{"segm": {...}}`` ({} without a prediction)."""

    def __init__(self, class_names: Sequence[str]):
        self.class_names = list(class_names)
        self.reset()

    def reset(self):
        self._images = {}

    @staticmethod
    def _arrays(output):
        if "instances" in output:
            inst = output["instances"]
            masks, scores, classes = (inst.masks.tensor if hasattr(inst.masks, "tensor") else inst.masks), inst.scores, inst.classes
        elif "masks" in output:
            masks, scores, classes = output["masks"], output["scores"], output["classes"]
        else:
            raise Exception("No instances in output?!")
        to_np = lambda t, dt: np.array(torch.as_tensor(t).detach().cpu().numpy(), dtype=dt)   # noqa: E731
        m = to_np(masks, bool)
        return m.reshape((-1,) + m.shape[-2:]), to_np(scores, np.float32).reshape(-1), to_np(classes, np.int64).reshape(-1)

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            image_id = inp.get("image_id") if isinstance(inp, dict) else getattr(inp, "image_id", None)
            assert image_id is not None, "Image ID must be present in the input!"
            if int(image_id) in self._images:
                raise ValueError(f"image id {image_id} was processed twice")
            masks, scores, classes = self._arrays(out)
            if len(scores) == 0:
                continue                                     # an image without predictions contributes nothing, its ground truth included
            gt = ground_truth_masks(inp)
            if masks.shape[1:] != gt[0].shape[1:]:
                raise ValueError(f"predicted masks {masks.shape[1:]} do not match the entry's (height, width) {gt[0].shape[1:]}")
            self._images[int(image_id)] = (masks, scores.astype(np.float64), classes, gt)

    def records(self) -> Optional[MatchRecords]:
        K = len(self.class_names)
        parts = [match_image_masks(i, *self._images[i], K) for i in sorted(self._images)]
        return MatchRecords.merge(parts) if parts else None

    def evaluate(self):
        rec = self.records()
        if rec is None:
            return {}
        return results_from(rec, self.class_names, "segm")


# ---------------------------------------------------------------------------------------------------------------- device side
def eval_boxes(probs: torch.Tensor, boxes: torch.Tensor, sizes: Sequence[Sequence[int]], top_k: int):
    """The batched eval_postprocess: top-k over [Q * K] (fx_topk_rows_ws_f32) + fx_detr_eval_boxes_f32.  Returns device tensors
    (score f32 [B, T], label i32 [B, T], keep i32 [B, T], xyxy f32 [B, T, 4], xywh f32 [B, T, 4])."""
    from . import _lib

    lib = _lib.load("bf16")
    probs, boxes = probs.contiguous().float(), boxes.contiguous().float()      # as eval_postprocess does
    dev = probs.device
    B, Q, K = probs.shape
    assert boxes.shape == (B, Q, 4) and len(sizes) == B, (tuple(boxes.shape), len(sizes))
    T = min(int(top_k), Q * K)
    stream = torch.cuda.current_stream(dev).cuda_stream
    val = torch.empty(B, T, dtype=torch.float32, device=dev)
    idx = torch.empty(B, T, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.fx_topk_rows_workspace_bytes(B, Q * K, T)), 8), dtype=torch.uint8, device=dev)
    _lib.check(lib.fx_topk_rows_ws_f32(probs.data_ptr(), Q * K, B, Q * K, T, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), stream),
               "fx_topk_rows_ws_f32")
    sz = torch.tensor([[int(h), int(w)] for h, w in sizes], dtype=torch.int32, device=dev)
    label = torch.empty(B, T, dtype=torch.int32, device=dev)
    keep = torch.empty(B, T, dtype=torch.int32, device=dev)
    xyxy = torch.empty(B, T, 4, dtype=torch.float32, device=dev)
    xywh = torch.empty(B, T, 4, dtype=torch.float32, device=dev)
    _lib.check(lib.fx_detr_eval_boxes_f32(idx.data_ptr(), boxes.data_ptr(), sz.data_ptr(), B, Q, K, T, label.data_ptr(),
                                          xyxy.data_ptr(), keep.data_ptr(), xywh.data_ptr(), ctypes.c_void_p(stream)), "fx_detr_eval_boxes_f32")
    return val, label, keep, xyxy, xywh


def device_match(label: torch.Tensor, score: torch.Tensor, keep: torch.Tensor, xywh: torch.Tensor, gts: List[tuple], K: int,
                 npig: torch.Tensor, status: torch.Tensor):
    """One fx_coco_match_bbox call on a batch: label / score / keep [B, T], xywh [B, T, 4] on the device, ``gts`` the per-image ground_truth()
    tuples (uploaded as one buffer + offsets), ``npig`` int64 [K, 4] and ``status`` int32 [1] on the device (accumulated).  Returns the device
    tensors (rank int32 [B, T] with -1 = not scored, matched int64 [B, T], ignored int64 [B, T]: the uint64 masks' bit patterns)."""
    from . import _lib

    lib = _lib.load("bf16")
    dev = label.device
    B, T = label.shape
    assert len(gts) == B
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum([len(g[1]) for g in gts])
    n_gt = int(offs[-1])
    max_gt = 0
    for g in gts:
        if len(g[1]):
            max_gt = max(max_gt, int(np.unique(g[1], return_counts=True)[1].max()))
    up = lambda arrs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(arrs), dtype=dt)).to(dev)   # noqa: E731
    if n_gt:
        box_d, cat_d = up([g[0].reshape(-1, 4) for g in gts], np.float64), up([g[1] for g in gts], np.int32)
        flag_d, area_d = up([g[2] for g in gts], np.int32), up([g[3] for g in gts], np.float64)
    off_d = torch.from_numpy(offs).to(dev)
    rank = torch.full((B, T), -1, dtype=torch.int32, device=dev)
    matched = torch.zeros(B, T, dtype=torch.int64, device=dev)
    ignored = torch.zeros(B, T, dtype=torch.int64, device=dev)
    need = int(lib.fx_coco_match_workspace_bytes(max_gt))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.fx_coco_match_bbox(label.data_ptr(), score.data_ptr(), keep.data_ptr(), xywh.data_ptr(), B, T, int(K),
                                ptr(box_d) if n_gt else None, ptr(cat_d) if n_gt else None, ptr(flag_d) if n_gt else None,
                                ptr(area_d) if n_gt else None, off_d.data_ptr(), offs.ctypes.data, n_gt, max_gt, rank.data_ptr(),
                                matched.data_ptr(), ignored.data_ptr(), npig.data_ptr(), status.data_ptr(), ptr(ws), need,
                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "fx_coco_match_bbox")
    return rank, matched, ignored


def records_from_device(image_ids: Sequence[int], label, score, keep, rank, matched, ignored, npig, K: int) -> MatchRecords:
    """Device outputs of one or more batches ([N, T] tensors, ``image_ids`` [N]) -> MatchRecords (one D2H copy per tensor)."""
    ids = np.asarray(image_ids, np.int64)
    r = rank.cpu().numpy()
    sel = r >= 0
    img = np.broadcast_to(ids[:, None], r.shape)[sel]
    evaluated = ids[(keep.cpu().numpy() != 0).any(1)]
    return MatchRecords(K, image_id=img, category=label.cpu().numpy()[sel], rank=r[sel], score=score.cpu().numpy()[sel].astype(np.float64),
                        matched=matched.cpu().numpy().view(np.uint64)[sel], ignored=ignored.cpu().numpy().view(np.uint64)[sel],
                        npig=npig.cpu().numpy(), images=evaluated)


# ---------------------------------------------------------------------------------------------------------------- driver
def check_supported(focoos_model) -> None:
    fam = focoos_model.model.family
    if fam != "fai_detr":
        raise NotImplementedError(f"FocoosModel.eval_detection: COCO bbox AP is evaluated for the fai_detr family only, not {fam!r} "
                                  "(instance segmentation is scored by FocoosModel.eval_instance_segmentation)")


def resolve(focoos_model, data_test):
    """(class names, dataset name) from the dataset metadata with evaluation.resolve's checks: task mismatch, thing_classes count."""
    from .evaluation import _metadata

    check_supported(focoos_model)
    info = focoos_model.model_info
    meta = _metadata(data_test)
    names, dname = list(info.classes), None
    if meta is not None:
        mt = getattr(meta, "task", None)
        mt = getattr(mt, "value", mt)
        if mt is not None and mt != "detection":
            raise ValueError(f"Task mismatch: model task detection != dataset task {mt}")
        cls = getattr(meta, "thing_classes", None)
        if cls is None:
            cls = getattr(meta, "classes", None)
        if cls is not None:
            if len(cls) != focoos_model.model.num_classes:
                raise ValueError(f"dataset has {len(cls)} classes, the model {focoos_model.model.num_classes}: num_classes must match")
            names = list(cls)
        dname = getattr(meta, "name", None)
    return names, dname


def collect(focoos_model, data_test, indices: Sequence[int], batch_size: int) -> MatchRecords:
    """Run the engine over ``indices`` (image id = dataset index) and match every batch on the device; nothing is read back before the last
    batch.  Plans created on the way are released afterwards."""
    from .evaluation import _batches

    model = focoos_model.model
    eng, dev, K = model.engine, model.device, model.num_classes
    top_k = focoos_model.processor.top_k
    indices = list(indices)
    npig = torch.zeros(K, _NA, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    outs, pos = [], 0
    with eng.scoped_plans():
        for batch in _batches(data_test, indices, batch_size):
            x = torch.stack([img for _, img in batch]).to(dev).contiguous()
            pl = eng.forward(x)
            sizes = [(int(getattr(e, "height", None) or 1), int(getattr(e, "width", None) or 1)) for e, _ in batch]
            score, label, keep, _, xywh = eval_boxes(pl.probs, pl.boxes, sizes, top_k)
            rank, matched, ignored = device_match(label, score, keep, xywh, [ground_truth(e) for e, _ in batch], K, npig, status)
            outs.append((label, score, keep, rank, matched, ignored))
            pos += len(batch)
        if int(status.item()):
            raise RuntimeError("fx_coco_match_bbox: a ground-truth group exceeded the workspace it was sized for")
        cat = [torch.cat([o[i] for o in outs]) for i in range(6)] if outs else None
        if cat is None:
            return MatchRecords(K)
        return records_from_device(indices[:pos], *cat, npig, K)


def _dist_worker(model_info, cfg, state, device_seed, args, data_test, out_path):
    """One rank of a multi-GPU run: its InferenceSampler shard -> match records, gathered (the records, not sums) to rank 0."""
    import torch.distributed as dist

    from .evaluation import _per_rank_batch
    from .model import ModelManager
    from .train_data import InferenceSampler

    dev = f"cuda:{torch.cuda.current_device()}"
    fm = ModelManager.get(model_info.name, model_info=model_info, device=dev, seed=device_seed)
    fm.model.load_state_dict(state, strict=False)
    rec = collect(fm, data_test, list(InferenceSampler(len(data_test))), _per_rank_batch(args))
    merged = gather_records(rec, dst=0)
    if dist.get_rank() == 0:
        torch.save(merged.state(), out_path)


def run_eval_detection(focoos_model, args, data_test, save_json: bool = True) -> dict:
    """FocoosModel.eval_detection: ``{"bbox": {...}}`` and the artifacts of FocoosModel.eval (model_info.json / metrics.json, ``bbox/...`` keys)."""
    from .evaluation import _per_rank_batch, write_artifacts

    names, dname = resolve(focoos_model, data_test)
    if len(data_test) == 0:
        raise ValueError("FocoosModel.eval_detection: empty dataset")
    world = max(1, int(getattr(args, "num_gpus", 1)))
    K = focoos_model.model.num_classes
    if world > 1:
        import copy
        import tempfile

        from .launch import launch

        info = copy.deepcopy(focoos_model.model_info)
        info.weights_uri = None
        with tempfile.TemporaryDirectory() as tmp:
            out_path = os.path.join(tmp, "records.pt")
            launch(_dist_worker, world, args=(info, info.config, focoos_model.model.state_dict(), 0, args, data_test, out_path))
            rec = MatchRecords(K, **torch.load(out_path, weights_only=False))
    else:
        rec = collect(focoos_model, data_test, range(len(data_test)), _per_rank_batch(args))
    if rec.images.size == 0:
        raise ValueError("FocoosModel.eval_detection: the model made no prediction on this dataset")
    results = results_from(rec, names)
    write_artifacts(focoos_model, args, "detection", results, dname, save_json)
    return results
