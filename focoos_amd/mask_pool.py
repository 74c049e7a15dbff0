"""What the device mask encoders share on the host (``mask_format="rle"``, mask_rle.py; ``mask_format="polygon"``,
mask_polygon.py, section 19): the bit words of a mask as a bool array, and ``PooledMaskEncoder``, the buffers, checks and copy back of an
encoder that leaves per slot a stream of int32 in a pool per image.  What a stream means is the subclass's."""
from __future__ import annotations

import warnings
from typing import List

import numpy as np


def unpack_words(words, W: int) -> np.ndarray:
    """int32 [..., H, ceil(W / 32)] bit-packed rows (pixel x = bit x % 32 of word x / 32) -> bool [..., H, W]."""
    w = np.ascontiguousarray(np.asarray(words)).astype("<i4", copy=False)
    if w.ndim < 2 or w.shape[-1] != (int(W) + 31) // 32:
        raise ValueError(f"words must be [H, {(int(W) + 31) // 32}] for W = {W}, got {w.shape}")
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :int(W)].astype(bool)


class PooledMaskEncoder:
    """Outputs and workspace of a pooled mask encoder for results of one shape (B images, Q slots, H x W pixels) on ``device``: ``meta``
    [2, B, Q] (per slot the length and the offset of its stream), the pool [B, capacity] and the library's workspace.  ``encode(res)``
    launches on the current stream; ``fetch()`` copies the lengths, the offsets and the used prefix of each image's pool on that stream
    and returns, per image, what the streams of its detections decode to; a slot whose stream was not stored is encoded on the host from
    its bit words, with one warning per call.  One encoder serves every lane of ``infer_stream``: launch and copy of a batch run in order
    on one stream before the next batch is encoded.

    A subclass gives ``CALL`` (the library pair ``CALL_workspace_bytes(B, Q, H, W, *sizes[1:])`` / ``CALL_encode(words, det_count,
    det_boxes, B, Q, H, W, *sizes, len, off, pool, workspace, bytes, stream)``), ``SIZES`` (the names of what its constructor takes after
    ``device``; they become attributes), ``sizes`` (their values, defaults filled in), ``LIMITS`` (the kernel's shape limits, for the
    error), ``_det_counts``, ``_decode`` (a stored stream), ``_encode_words`` (the host fallback) and ``_warning``."""

    CALL, SIZES, LIMITS = "", ("capacity",), ""

    def __init__(self, B: int, Q: int, H: int, W: int, device, *sizes):
        import torch

        from ._lib import load

        self.lib = load("bf16")   # inference surface: the bf16 product library (the kernel is the same in both)
        self.device = torch.device(device)
        self.B, self.Q, self.H, self.W = int(B), int(Q), int(H), int(W)
        self._sizes = self.sizes(Q, H, W, *sizes)
        if min(self._sizes) < 1:
            raise ValueError(f"{type(self).__name__}: {' and '.join(f'{n} = {v!r}' for n, v in zip(self.SIZES, self._sizes))} must be >= 1")
        for n, v in zip(self.SIZES, self._sizes):
            setattr(self, n, v)
        nb = int(getattr(self.lib, self.CALL + "_workspace_bytes")(self.B, self.Q, self.H, self.W, *self._sizes[1:]))
        if nb == 0:
            raise ValueError(f"{type(self).__name__}: B = {B}, Q = {Q}, H = {H}, W = {W} is outside the kernel's limits ({self.LIMITS})")
        i32 = dict(dtype=torch.int32, device=self.device)
        self.meta = torch.zeros(2, self.B, self.Q, **i32)      # lengths, offsets: one copy back
        self.pool = torch.zeros(self.B, self.capacity, **i32)
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._host = None          # pinned [B, capacity], made with the first fetch
        self._res = None
        self.last_d2h_bytes = 0    # of the last fetch, fallback words included
        self.last_fallback = 0     # slots the last fetch encoded on the host
        self.total_fallback = 0    # ... and every fetch of this encoder, out of total_masks
        self.total_masks = 0

    def key(self):
        return (self.B, self.Q, self.H, self.W, self.device) + self._sizes

    def encode(self, res) -> None:
        """``res``: an engine plan or the processor's device results (``mask_words`` [B, Q, H, ceil(W / 32)], ``det_count``, ``det_boxes``)."""
        import torch

        from ._lib import check

        who = f"{type(self).__name__}.encode"
        words = res.mask_words
        shape = (self.B, self.Q, self.H, (self.W + 31) // 32)
        if tuple(words.shape) != shape or words.dtype != torch.int32 or not words.is_contiguous() or words.device != self.device:
            raise ValueError(f"{who}: mask_words must be a contiguous int32 tensor {shape} on {self.device}, got "
                             f"{words.dtype} {tuple(words.shape)} on {words.device}")
        for name, t, shp in (("det_count", res.det_count, (self.B,)), ("det_boxes", res.det_boxes, (self.B, self.Q, 4))):
            if tuple(t.shape) != shp or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{who}: {name} must be a contiguous int32 tensor {shp} on {self.device}")
        check(getattr(self.lib, self.CALL + "_encode")(
            words.data_ptr(), res.det_count.data_ptr(), res.det_boxes.data_ptr(), self.B, self.Q, self.H, self.W, *self._sizes,
            self.meta[0].data_ptr(), self.meta[1].data_ptr(), self.pool.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            torch.cuda.current_stream(self.device).cuda_stream), self.CALL + "_encode")
        self._res = res

    def fetch(self) -> List[list]:
        """Per image the list, in slot order, of what its detections' streams decode to."""
        import torch

        if self._res is None:
            raise RuntimeError(f"{type(self).__name__}.fetch: nothing was encoded")
        meta = self.meta.cpu().numpy().astype(np.int64)      # synchronises the stream
        ln, off = meta[0], meta[1]
        count, count_bytes = self._det_counts(ln)
        stored = (ln > 0) & (off + ln <= self.capacity)
        used = np.where(stored, off + ln, 0).max(axis=1)
        if self._host is None:
            self._host = torch.empty(self.B, self.capacity, dtype=torch.int32, pin_memory=True)
        for b in range(self.B):
            if used[b]:
                self._host[b, :used[b]].copy_(self.pool[b, :used[b]], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        pool = self._host.numpy()
        self.last_d2h_bytes = int(meta.size * 4 + count_bytes + used.sum() * 4)
        out, fell, masks = [], 0, int(count.sum())
        for b in range(self.B):
            n = int(count[b])      # detections are the leading slots
            lost = np.flatnonzero(~stored[b, :n] & (ln[b, :n] != 0))      # did not fit (the pool, or length -1: the encoder's own workspace)
            words = {}
            if len(lost):      # the same result from the slots' bit words, on the host (one copy per image)
                w = self._res.mask_words[b, :n][torch.from_numpy(lost).to(self.device)].cpu().numpy()
                self.last_d2h_bytes += w.nbytes
                words = dict(zip(lost.tolist(), w))
                fell += len(lost)
            # a slot that is neither stored nor lost has length 0: the empty stream
            out.append([self._encode_words(words[j]) if j in words else self._decode(pool[b, off[b, j]:off[b, j] + max(ln[b, j], 0)])
                        for j in range(n)])
        self.last_fallback = fell
        self.total_fallback += fell
        self.total_masks += masks
        if fell:
            warnings.warn(self._warning(fell, masks), RuntimeWarning, stacklevel=3)
        return out


def encoder_for(cls, current, res, *sizes):
    """``current`` when it fits ``res`` (shape, device) and ``sizes`` (capacity, ...: None = ``cls``'s default), a new ``cls`` otherwise."""
    B, Q, H, _ = res.mask_words.shape
    W = int(getattr(res, "mask_width", res.mask_words.shape[3] * 32))
    dev = res.mask_words.device
    sizes = cls.sizes(Q, H, W, *sizes)
    if current is not None and current.key() == (B, Q, H, W, dev) + sizes:
        return current
    return cls(B, Q, H, W, dev, *sizes)
