"""Instance masks as COCO run-length encoding, produced on the device (``FocoosModel.infer(mask_format="rle")``).

The mask families leave their kept masks on the device as bit-packed words.  ``MaskRleEncoder`` turns them into uncompressed COCO RLE there
(csrc/mask_rle.hip; the contract is in include/focoos_amd.h) and copies back the lengths, the offsets and the used part of each image's
pool of counts: no dense mask crosses to the host and nothing is compressed on it.  A slot whose counts did not fit the pool is encoded on
the host from its bit words (``encode_words_numpy``), with one warning per call, so the result is always complete.  The compressed RLE
*string* of maskApi is out of scope (``check_mask_format``), like tiled inference; polygons are mask_polygon.py, and what the two
encoders share (buffers, checks, copy back, fallback, ``encoder_for``) is mask_pool.py."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .mask_pool import PooledMaskEncoder, unpack_words

MASK_FORMATS = ("png", "rle", "polygon", "none")
MASK_FAMILIES = ("fai_mf", "bisenetformer")


def check_mask_format(mask_format, family: Optional[str] = None, what: str = "infer") -> str:
    """The ``mask_format`` keyword of the inference surface: "png" (the reference's base64 PNG, the default), "rle" (``FocoosDet.rle``),
    "polygon" (``FocoosDet.polygons``, mask_polygon.py) or "none" (boxes, scores and labels only).  ValueError for anything else, the
    compressed "coco_string" by name; NotImplementedError, by name, for "rle" or "polygon" on a family without masks.  Host only: nothing is loaded or launched."""
    if mask_format == "coco_string":
        raise ValueError(f"{what}: mask_format='coco_string' (maskApi's compressed RLE string) is not built: its codec cannot be checked "
                         "against pycocotools here, which is why detection_eval does not decode it either; use 'rle' (uncompressed counts)")
    if not isinstance(mask_format, str) or mask_format not in MASK_FORMATS:
        raise ValueError(f"{what}: mask_format = {mask_format!r} must be one of {', '.join(repr(f) for f in MASK_FORMATS)}")
    if mask_format in ("rle", "polygon") and family is not None and family not in MASK_FAMILIES:
        raise NotImplementedError(f"{what}: mask_format={mask_format!r} needs masks; model family {family!r} has none "
                                  f"(supported: {', '.join(MASK_FAMILIES)})")
    return mask_format


def encode_mask_numpy(mask) -> dict:
    """bool [H, W] -> {"size": [H, W], "counts": [...]}: the runs of the mask read column by column, zeros-run first."""
    m = np.asarray(mask).astype(bool)
    if m.ndim != 2:
        raise ValueError(f"encode_mask_numpy: a mask is [H, W], got {m.shape}")
    H, W = m.shape
    s = np.ascontiguousarray(m.T).ravel()
    t = np.flatnonzero(s != np.concatenate(([False], s[:-1])))
    return {"size": [H, W], "counts": np.diff(np.concatenate(([0], t, [H * W]))).tolist()}


def encode_words_numpy(words, W: int) -> dict:
    """int32 [H, ceil(W / 32)] bit-packed rows (pixel x = bit x % 32 of word x / 32) -> the RLE dict of the mask."""
    return encode_mask_numpy(unpack_words(words, W))


def _runs(rle: dict):
    counts = rle["counts"]
    if isinstance(counts, (str, bytes)):
        raise NotImplementedError("a compressed RLE string is not decoded (see check_mask_format); give the uncompressed counts")
    H, W = (int(v) for v in rle["size"])
    runs = np.asarray(counts, np.int64).reshape(-1)
    if (runs < 0).any() or int(runs.sum()) != H * W:
        raise ValueError(f"uncompressed RLE counts sum to {int(runs.sum())}, the size is {H} x {W}")
    return H, W, runs


def rle_decode(rle: dict) -> np.ndarray:
    """{"size": [H, W], "counts": [...]} -> bool [H, W]."""
    H, W, runs = _runs(rle)
    return np.repeat(np.arange(len(runs)) % 2 == 1, runs).reshape(W, H).T


def rle_area(rle: dict) -> int:
    """The number of set pixels: the sum of the ones-runs."""
    return int(_runs(rle)[2][1::2].sum())


def to_coco_results(detections, image_id, category_ids: Optional[Sequence[int]] = None) -> List[dict]:
    """The entries of a COCO results file for one image: ``detections`` (a FocoosDetections or a list of FocoosDet) -> [{"image_id",
    "category_id", "bbox" (x, y, w, h), "score", "segmentation" (the uncompressed RLE dict when the detection has one; else, when it has polygons, its outer rings as COCO's list of
    flat [x0, y0, x1, y1, ...]: a COCO polygon cannot carry a hole, so the hole rings are left out and the holes read as filled)}].
    ``category_ids[cls_id]`` maps the model's class index to the dataset's category id (identity when None).  The box of a detection with
    an RLE or polygons is the inclusive extent of its pixels, so its width is x1 - x0 + 1."""
    out = []
    for d in getattr(detections, "detections", detections):
        x0, y0, x1, y1 = (d.bbox if d.bbox is not None else (0, 0, 0, 0))
        polygons = getattr(d, "polygons", None)
        inc = 1 if (d.rle is not None or polygons is not None) else 0
        e = {"image_id": image_id, "category_id": int(category_ids[d.cls_id]) if category_ids is not None else int(d.cls_id),
             "bbox": [x0, y0, x1 - x0 + inc, y1 - y0 + inc], "score": float(d.conf)}
        if d.rle is not None:
            e["segmentation"] = {"size": list(d.rle["size"]), "counts": list(d.rle["counts"])}
        elif polygons is not None:
            from .mask_polygon import outer_rings

            e["segmentation"] = outer_rings(polygons)
        out.append(e)
    return out


def default_capacity(Q: int, W: int) -> int:
    """Counts per image of the pool: Q (2 W + 2).  A mask with at most one vertical segment per column has at most 2 W transitions, that is
    2 W + 1 counts, so the pool holds Q such masks; anything more ragged may fall back to the host."""
    return int(Q) * (2 * int(W) + 2)


class MaskRleEncoder(PooledMaskEncoder):
    """The pooled encoder (mask_pool.py) of fx_mask_rle_encode: a slot's stream is its counts, ``fetch()`` returns per image the RLE dicts
    {"size": [H, W], "counts": [...]} of its detections, in slot order."""

    CALL, LIMITS = "fx_mask_rle", "Q (H W + 1) < 2^31"

    def __init__(self, B: int, Q: int, H: int, W: int, device, capacity: Optional[int] = None):
        super().__init__(B, Q, H, W, device, capacity)
        self.rle_len, self.rle_off, self.rle_counts = self.meta[0], self.meta[1], self.pool

    @staticmethod
    def sizes(Q, H, W, capacity=None):
        return (default_capacity(Q, W) if capacity is None else int(capacity),)

    def _det_counts(self, ln):
        return (ln > 0).sum(axis=1), 0      # every mask has at least one count, and nothing more is copied

    def _decode(self, counts):
        return {"size": [self.H, self.W], "counts": counts.tolist()}

    def _encode_words(self, words):
        return encode_words_numpy(words, self.W)

    def _warning(self, fell, masks):
        return (f"mask_format='rle': {fell} of {masks} masks did not fit the pool of {self.capacity} counts per image and "
                f"were encoded on the host (raise the capacity)")
