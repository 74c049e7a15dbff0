"""Instance masks as COCO run-length encoding, produced on the device (``FocoosModel.infer(mask_format="rle")``).

The mask families leave their kept masks on the device as bit-packed words.  ``MaskRleEncoder`` turns them into uncompressed COCO RLE there
(csrc/mask_rle.hip; the contract is in include/focoos_amd.h) and copies back the lengths, the offsets and the used part of each image's
pool of counts: no dense mask crosses to the host and nothing is compressed on it.  A slot whose counts did not fit the pool is encoded on
the host from its bit words (``encode_words_numpy``), with one warning per call, so the result is always complete.  The compressed RLE
*string* of maskApi is out of scope (``check_mask_format``), like tiled inference; polygons are mask_polygon.py."""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence

import numpy as np

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
    w = np.ascontiguousarray(np.asarray(words)).astype("<i4", copy=False)
    if w.ndim != 2 or w.shape[1] != (int(W) + 31) // 32:
        raise ValueError(f"encode_words_numpy: words must be [H, {(int(W) + 31) // 32}] for W = {W}, got {w.shape}")
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[:, :int(W)]
    return encode_mask_numpy(bits)


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


class MaskRleEncoder:
    """Output buffers and workspace of fx_mask_rle_encode for results of one shape (B images, Q slots, H x W pixels) on ``device``.
    ``encode(res)`` launches on the current stream; ``fetch()`` copies the lengths, the offsets and the used prefix of each image's pool
    on that stream and returns, per image, the RLE dicts of its detections.  One encoder serves every lane of ``infer_stream``: launch
    and copy of a batch run in order on one stream before the next batch is encoded."""

    def __init__(self, B: int, Q: int, H: int, W: int, device, capacity: Optional[int] = None):
        import torch

        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library (the kernel is the same in both)
        self.device = torch.device(device)
        self.B, self.Q, self.H, self.W = int(B), int(Q), int(H), int(W)
        self.capacity = default_capacity(Q, W) if capacity is None else int(capacity)
        if self.capacity < 1:
            raise ValueError(f"MaskRleEncoder: capacity = {capacity!r} must be >= 1")
        nb = int(self.lib.fx_mask_rle_workspace_bytes(self.B, self.Q, self.H, self.W))
        if nb == 0:
            raise ValueError(f"MaskRleEncoder: B = {B}, Q = {Q}, H = {H}, W = {W} is outside the kernel's limits (Q (H W + 1) < 2^31)")
        i32 = dict(dtype=torch.int32, device=self.device)
        self.meta = torch.zeros(2, self.B, self.Q, **i32)      # rle_len, rle_off: one copy back
        self.rle_len, self.rle_off = self.meta[0], self.meta[1]
        self.rle_counts = torch.zeros(self.B, self.capacity, **i32)
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._host = None          # pinned [B, capacity], made with the first fetch
        self._res = None
        self.last_d2h_bytes = 0    # of the last fetch, fallback words included
        self.last_fallback = 0     # slots the last fetch encoded on the host
        self.total_fallback = 0    # ... and every fetch of this encoder, out of total_masks
        self.total_masks = 0

    def key(self):
        return (self.B, self.Q, self.H, self.W, self.device, self.capacity)

    def encode(self, res) -> None:
        """``res``: an engine plan or the processor's device results (``mask_words`` [B, Q, H, ceil(W / 32)], ``det_count``, ``det_boxes``)."""
        import torch

        from ._lib import check

        words = res.mask_words
        shape = (self.B, self.Q, self.H, (self.W + 31) // 32)
        if tuple(words.shape) != shape or words.dtype != torch.int32 or not words.is_contiguous() or words.device != self.device:
            raise ValueError(f"MaskRleEncoder.encode: mask_words must be a contiguous int32 tensor {shape} on {self.device}, got "
                             f"{words.dtype} {tuple(words.shape)} on {words.device}")
        for name, t, shp in (("det_count", res.det_count, (self.B,)), ("det_boxes", res.det_boxes, (self.B, self.Q, 4))):
            if tuple(t.shape) != shp or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"MaskRleEncoder.encode: {name} must be a contiguous int32 tensor {shp} on {self.device}")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.fx_mask_rle_encode(words.data_ptr(), res.det_count.data_ptr(), res.det_boxes.data_ptr(), self.B, self.Q, self.H, self.W,
                                          self.capacity, self.rle_len.data_ptr(), self.rle_off.data_ptr(), self.rle_counts.data_ptr(),
                                          self.workspace.data_ptr(), self.workspace.numel(), stream), "fx_mask_rle_encode")
        self._res = res

    def fetch(self) -> List[List[dict]]:
        """Per image the list of {"size": [H, W], "counts": [...]} of its detections, in slot order."""
        import torch

        if self._res is None:
            raise RuntimeError("MaskRleEncoder.fetch: nothing was encoded")
        meta = self.meta.cpu().numpy().astype(np.int64)      # synchronises the stream
        ln, off = meta[0], meta[1]
        stored = (ln > 0) & (off + ln <= self.capacity)
        used = np.where(stored, off + ln, 0).max(axis=1)
        if self._host is None:
            self._host = torch.empty(self.B, self.capacity, dtype=torch.int32, pin_memory=True)
        for b in range(self.B):
            if used[b]:
                self._host[b, :used[b]].copy_(self.rle_counts[b, :used[b]], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        pool = self._host.numpy()
        self.last_d2h_bytes = int(meta.size * 4 + used.sum() * 4)
        size, out, fell = [self.H, self.W], [], 0
        for b in range(self.B):
            n = int((ln[b] > 0).sum())      # detections are the leading slots
            lost = np.flatnonzero(~stored[b, :n])
            words = {}
            if len(lost):      # did not fit the pool: the same counts from the slots' bit words, on the host (one copy per image)
                w = self._res.mask_words[b, :n][torch.from_numpy(lost).to(self.device)].cpu().numpy()
                self.last_d2h_bytes += w.nbytes
                words = dict(zip(lost.tolist(), w))
                fell += len(lost)
            out.append([{"size": list(size), "counts": pool[b, off[b, j]:off[b, j] + ln[b, j]].tolist()} if stored[b, j]
                        else encode_words_numpy(words[j], self.W) for j in range(n)])
        self.last_fallback = fell
        self.total_fallback += fell
        self.total_masks += int((ln > 0).sum())
        if fell:
            warnings.warn(f"mask_format='rle': {fell} of {int((ln > 0).sum())} masks did not fit the pool of {self.capacity} counts per image and "
                          f"were encoded on the host (raise the capacity)", RuntimeWarning, stacklevel=3)
        return out


def encoder_for(current: Optional[MaskRleEncoder], res, capacity: Optional[int] = None) -> MaskRleEncoder:
    """``current`` when it fits ``res`` (shape, device, capacity), a new encoder otherwise."""
    B, Q, H, _ = res.mask_words.shape
    W = int(getattr(res, "mask_width", res.mask_words.shape[3] * 32))
    dev = res.mask_words.device
    cap = default_capacity(Q, W) if capacity is None else int(capacity)
    if current is not None and current.key() == (B, Q, H, W, dev, cap):
        return current
    return MaskRleEncoder(B, Q, H, W, dev, cap)
