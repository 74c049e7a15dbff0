"""Video frames as an input type: ``Frame`` is one picture as a decoder or a camera library hands it out (packed RGB /
BGR, or NV12 / I420 with a row pitch, on the host or already on the device), ``FrameBatch`` is B of them.  One launch of
``fx_frames_ingest`` (csrc/frame_ops.hip) takes the whole batch to the engine's input:

  host planes  -> one packed staging buffer -> one upload \\
                                                           fx_frames_ingest -> uint8 [B,H,W,3] (all frames at the target size)
  device planes -> read in place on the current stream    /                   or float32 [B,Ht,Wt,3] (bilinearly resized, 0..255)

The result is defined to be, bit for bit, what ``processor.preprocess`` returns for the same frames converted to RGB arrays by the integer
conversion of include/focoos_amd.h (tests/frames_ref.py restates it), so everything downstream can be compared by equality.
Construction validates on the host and never touches the GPU."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

FORMATS = {"rgb24": 0, "bgr24": 1, "nv12": 2, "i420": 3}          # FX_FRAME_*
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
MAX_DIM = 16384
MAX_BATCH = 65535


def matrix_code(matrix: str, range: str) -> int:
    """FX_FRAME_BT601_LIMITED .. FX_FRAME_BT709_FULL."""
    return 2 * MATRICES.index(matrix) + RANGES.index(range)


def plane_shapes(format: str, height: int, width: int) -> List[Tuple[int, ...]]:
    """The planes of one frame as the table of DESIGN 21 lists them."""
    ch, cw = (height + 1) // 2, (width + 1) // 2
    if format in ("rgb24", "bgr24"):
        return [(height, width, 3)]
    if format == "nv12":
        return [(height, width), (ch, cw, 2)]
    return [(height, width), (ch, cw), (ch, cw)]


def _is_torch(p) -> bool:
    return isinstance(p, torch.Tensor)


def _strides(p) -> Tuple[int, ...]:
    return tuple(int(s) for s in (p.stride() if _is_torch(p) else p.strides))     # uint8: bytes either way


class Frame:
    """One picture: ``format`` in rgb24 / bgr24 / nv12 / i420, its ``planes`` (uint8 numpy arrays or torch tensors; innermost stride 1, any
    row pitch >= the row's bytes, so a view into a pitched decoder surface is a plane), ``height`` and ``width``, and for the YUV formats
    ``matrix`` (bt601 / bt709) and ``range`` (limited / full).  Every check happens here; a ValueError names the field."""

    def __init__(self, format: str, planes: Sequence, height: int, width: int, matrix: str = "bt601", range: str = "limited"):
        if format not in FORMATS:
            raise ValueError(f"Frame: unknown format {format!r} (one of {sorted(FORMATS)})")
        if matrix not in MATRICES:
            raise ValueError(f"Frame: unknown matrix {matrix!r} (one of {list(MATRICES)})")
        if range not in RANGES:
            raise ValueError(f"Frame: unknown range {range!r} (one of {list(RANGES)})")
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= MAX_DIM:
                raise ValueError(f"Frame: {name} must be an integer in 1..{MAX_DIM}, got {v!r}")
        height, width = int(height), int(width)
        want = plane_shapes(format, height, width)
        planes = list(planes)
        if len(planes) != len(want):
            raise ValueError(f"Frame: planes: format {format!r} has {len(want)} plane(s), got {len(planes)}")
        for i, (p, shape) in enumerate(zip(planes, want)):
            if not (_is_torch(p) or isinstance(p, np.ndarray)):
                raise ValueError(f"Frame: planes[{i}] must be a numpy array or a torch tensor, not {type(p).__name__}")
            if p.dtype not in (np.uint8, torch.uint8):
                raise ValueError(f"Frame: planes[{i}] dtype must be uint8, got {p.dtype}")
            if tuple(p.shape) != shape:
                raise ValueError(f"Frame: planes[{i}] of a {height} x {width} {format} frame must have shape {shape}, got {tuple(p.shape)}")
            st = _strides(p)
            if st[-1] != 1:
                raise ValueError(f"Frame: planes[{i}] inner stride must be 1, got {st[-1]}")
            if len(shape) == 3 and st[1] != shape[2]:
                raise ValueError(f"Frame: planes[{i}] pixel stride must be {shape[2]}, got {st[1]}")
            row = shape[1] * (shape[2] if len(shape) == 3 else 1)
            if st[0] < row and shape[0] > 1:
                raise ValueError(f"Frame: planes[{i}] pitch {st[0]} is below the row's {row} bytes")
            if st[0] >= 2 ** 31:
                raise ValueError(f"Frame: planes[{i}] pitch {st[0]} does not fit 31 bits")
        self.format, self.planes, self.height, self.width, self.matrix, self.range = format, planes, height, width, matrix, range

    @property
    def size(self) -> Tuple[int, int]:
        return (self.height, self.width)

    def pitches(self) -> List[int]:
        """Row pitch in bytes of every plane (a one-row plane has whatever pitch >= its row: the row's bytes)."""
        out = []
        for p in self.planes:
            row = int(np.prod(p.shape[1:]))
            out.append(max(_strides(p)[0], row))
        return out

    @classmethod
    def from_rgb(cls, array) -> "Frame":
        return cls._packed("rgb24", array)

    @classmethod
    def from_bgr(cls, array) -> "Frame":
        return cls._packed("bgr24", array)

    @classmethod
    def _packed(cls, format: str, array) -> "Frame":
        if not hasattr(array, "shape") or len(array.shape) != 3 or array.shape[2] != 3:
            raise ValueError(f"Frame: planes[0] of a {format} frame must be [H][W][3], got {tuple(getattr(array, 'shape', ()))}")
        return cls(format, [array], int(array.shape[0]), int(array.shape[1]))

    @classmethod
    def from_nv12(cls, buffer, height: int, width: int, pitch: Optional[int] = None, matrix: str = "bt601", range: str = "limited") -> "Frame":
        """The common single-allocation layout: ``buffer`` (1-D uint8, host or device) holds ``height`` rows of Y at ``pitch`` bytes each and,
        from byte ``pitch * height``, (height + 1) // 2 rows of interleaved UV at the same pitch.  ``pitch`` defaults to the width rounded
        up to even."""
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= MAX_DIM:
                raise ValueError(f"Frame: {name} must be an integer in 1..{MAX_DIM}, got {v!r}")
        height, width = int(height), int(width)
        ch, cw = (height + 1) // 2, (width + 1) // 2
        pitch = 2 * cw if pitch is None else int(pitch)
        if pitch < 2 * cw:
            raise ValueError(f"Frame: pitch {pitch} is below the {2 * cw} bytes of a chroma row of width {width}")
        if not (_is_torch(buffer) or isinstance(buffer, np.ndarray)) or len(buffer.shape) != 1:
            raise ValueError("Frame: buffer must be a 1-D numpy array or torch tensor")
        if buffer.dtype not in (np.uint8, torch.uint8):
            raise ValueError(f"Frame: buffer dtype must be uint8, got {buffer.dtype}")
        if _strides(buffer)[0] != 1:
            raise ValueError(f"Frame: buffer inner stride must be 1, got {_strides(buffer)[0]}")
        need = pitch * height + pitch * (ch - 1) + 2 * cw
        if int(buffer.shape[0]) < need:
            raise ValueError(f"Frame: buffer holds {int(buffer.shape[0])} bytes, a {height} x {width} NV12 frame at pitch {pitch} needs {need}")
        if _is_torch(buffer):
            y = buffer.as_strided((height, width), (pitch, 1))
            uv = buffer[pitch * height:].as_strided((ch, cw, 2), (pitch, 2, 1))
        else:
            y = np.lib.stride_tricks.as_strided(buffer, (height, width), (pitch, 1), writeable=False)
            uv = np.lib.stride_tricks.as_strided(buffer[pitch * height:], (ch, cw, 2), (pitch, 2, 1), writeable=False)
        return cls("nv12", [y, uv], height, width, matrix, range)


class _Staging:
    """One reusable host buffer (pinned when the runtime gives one) for the packed host planes and the descriptors of a batch.  The event
    marks the last upload that read it: the next batch waits for it before overwriting."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.event = None

    def get(self, nbytes: int) -> torch.Tensor:
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        if self.buf is None or self.buf.numel() < nbytes:
            cap = max(nbytes, 1 << 16)
            try:
                self.buf = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            except RuntimeError:      # no pinned memory to be had: a pageable buffer, the copy is then synchronous
                self.buf = torch.empty(cap, dtype=torch.uint8)
        return self.buf[:nbytes]

    def uploaded(self, device) -> None:
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(device))


_STAGING = _Staging()


_PACKERS = []      # the thread pool of _pack, created on first use


def _pack(copies) -> None:
    """The (destination view, source plane) copies of one batch into the staging buffer.  A batch of camera frames is ~100 MB, which one
    thread copies more slowly than the link takes it up; numpy releases the interpreter lock while it copies, so 8 threads share the work."""
    if len(copies) < 2 or sum(dst.size for dst, _ in copies) < (4 << 20):
        for dst, src in copies:
            np.copyto(dst, src)
        return
    if not _PACKERS:
        from concurrent.futures import ThreadPoolExecutor

        _PACKERS.append(ThreadPoolExecutor(max_workers=8, thread_name_prefix="frames-pack"))
    list(_PACKERS[0].map(lambda c: np.copyto(c[0], c[1]), copies))


def _align(n: int, a: int = 256) -> int:
    return -(-n // a) * a


class FrameBatch:
    """B frames; sizes, formats and matrices may differ per frame.  ``len()``, iteration, ``.sizes``."""

    def __init__(self, frames: Sequence[Frame]):
        frames = list(frames)
        if not 1 <= len(frames) <= MAX_BATCH:
            raise ValueError(f"FrameBatch: frames must hold 1..{MAX_BATCH} frames, got {len(frames)}")
        for i, f in enumerate(frames):
            if not isinstance(f, Frame):
                raise ValueError(f"FrameBatch: frames[{i}] is a {type(f).__name__}, not a Frame")
        self.frames = frames
        self._resident = None      # (device, descriptors on the device, descriptors on the host, what they point into)

    def __len__(self) -> int:
        return len(self.frames)

    def __iter__(self):
        return iter(self.frames)

    def __getitem__(self, i) -> Frame:
        return self.frames[i]

    @property
    def sizes(self) -> List[Tuple[int, int]]:
        return [f.size for f in self.frames]

    # ---- device side
    def _descriptors(self, device):
        """Upload once per device: host planes packed (rows compacted, every plane at a 256-byte offset) behind the descriptor table in one
        staging buffer, one copy; device planes are pointed at where they are.  Returns (device table, host table)."""
        from ._lib import FxFrameDesc

        device = torch.device(device)
        if self._resident is not None and self._resident[0] == device:
            return self._resident[1], self._resident[2]
        B = len(self.frames)
        off, places = _align(64 * B), []
        for bi, f in enumerate(self.frames):
            for pi, p in enumerate(f.planes):
                if _is_torch(p) and p.device.type != "cpu":
                    if p.device != device:
                        raise ValueError(f"FrameBatch: planes[{pi}] of frame {bi} lives on {p.device}, the model on {device}")
                    continue
                places.append((bi, pi, off))
                off = _align(off + int(np.prod(p.shape)))
        stage = _STAGING.get(off)
        stage_np = stage.numpy()
        dev = torch.empty(off, dtype=torch.uint8, device=device)
        host = (FxFrameDesc * B)()
        where = {(bi, pi): o for bi, pi, o in places}
        copies = []
        for bi, f in enumerate(self.frames):
            d = host[bi]
            d.height, d.width, d.format, d.matrix = f.height, f.width, FORMATS[f.format], matrix_code(f.matrix, f.range)
            for pi, (p, pitch) in enumerate(zip(f.planes, f.pitches())):
                if (bi, pi) in where:
                    o, n = where[(bi, pi)], int(np.prod(p.shape))
                    copies.append((stage_np[o:o + n].reshape(p.shape), p.numpy() if _is_torch(p) else p))
                    d.plane[pi], d.pitch[pi] = dev.data_ptr() + o, int(np.prod(p.shape[1:]))
                else:
                    d.plane[pi], d.pitch[pi] = p.data_ptr(), pitch
        _pack(copies)
        stage_np[:64 * B] = np.frombuffer(bytes(host), dtype=np.uint8)
        dev.copy_(stage, non_blocking=True)
        _STAGING.uploaded(device)
        self._resident = (device, dev, host, [p for f in self.frames for p in f.planes])
        return dev, host

    def _ingest(self, device, b0: int, n: int, out: torch.Tensor, out_f32: bool) -> torch.Tensor:
        from . import _lib

        dev, host = self._descriptors(device)
        lib = _lib.load("bf16")   # inference surface: the bf16 product library whatever a training step pinned
        stream = torch.cuda.current_stream(torch.device(device)).cuda_stream
        _lib.check(lib.fx_frames_ingest(dev.data_ptr() + 64 * b0, ctypes.addressof(host) + 64 * b0, n, out.data_ptr(), int(out_f32),
                                        int(out.shape[1]), int(out.shape[2]), ctypes.c_void_p(stream)), "fx_frames_ingest")
        return out

    def to_engine_input(self, target: Optional[Tuple[int, int]], device) -> torch.Tensor:
        """What ``preprocess`` returns for the frames as RGB arrays: uint8 [B,H,W,3] when ``target`` is None or every frame already has the
        target size, float32 [B,Ht,Wt,3] on the 0..255 scale otherwise.  One launch."""
        sizes = self.sizes
        if target is None and any(s != sizes[0] for s in sizes):
            raise ValueError("images of different sizes need an image_size to resize to (the reference fails in torch.stack here)")
        tgt = tuple(int(v) for v in target) if target is not None else sizes[0]
        same = all(s == tgt for s in sizes)
        out = torch.empty(len(sizes), tgt[0], tgt[1], 3, dtype=torch.uint8 if same else torch.float32, device=device)
        return self._ingest(device, 0, len(sizes), out, not same)

    def rgb_frames(self, device) -> List[torch.Tensor]:
        """The frames as uint8 RGB device tensors [H,W,3] at their own sizes (what ``annotate=True`` draws on): each run of equal-size
        frames is one launch."""
        sizes, res, i = self.sizes, [], 0
        while i < len(sizes):
            j = i + 1
            while j < len(sizes) and sizes[j] == sizes[i]:
                j += 1
            out = torch.empty(j - i, sizes[i][0], sizes[i][1], 3, dtype=torch.uint8, device=device)
            res.extend(self._ingest(device, i, j - i, out, False).unbind(0))
            i = j
        return res


def as_frame_batch(inputs) -> Optional[FrameBatch]:
    """``inputs`` as a FrameBatch when it is one (or a single Frame), None for everything else the entry points take."""
    if isinstance(inputs, FrameBatch):
        return inputs
    if isinstance(inputs, Frame):
        return FrameBatch([inputs])
    return None


def wrap_frames(inputs, what: str) -> FrameBatch:
    """One batch of uint8 frames as a FrameBatch: a FrameBatch, a Frame, or a list of Frames and / or uint8 RGB arrays or tensors [H, W, 3],
    which are wrapped as RGB24 frames.  ValueError, with ``what`` (entry point and argument) in front, for anything else; host only."""
    fb = as_frame_batch(inputs)
    if fb is not None:
        return fb
    if not isinstance(inputs, (list, tuple)) or not inputs:
        raise ValueError(f"{what} takes a FrameBatch or a non-empty list of Frames / uint8 RGB arrays, got {type(inputs).__name__}")
    frames = []
    for i, im in enumerate(inputs):
        if not isinstance(im, Frame):
            dt = getattr(im, "dtype", None)
            if dt not in (np.uint8, torch.uint8):
                raise ValueError(f"{what} takes uint8 frames: input {i} is {dt if dt is not None else type(im).__name__}")
            im = Frame.from_rgb(im)
        frames.append(im)
    return FrameBatch(frames)


def refuse_frames(inputs, what: str) -> None:
    """ValueError naming ``what`` for an entry point that does not take frames.  Host only."""
    if isinstance(inputs, (Frame, FrameBatch)):
        raise ValueError(f"{what} does not take a {type(inputs).__name__}: pass the picture as an RGB array")


def drawable(inputs, images: torch.Tensor, device):
    """What ``annotate_results`` draws on: the inputs themselves, or for a FrameBatch its RGB frames on the device (not needed when
    preprocess already produced the uint8 batch, which is then drawn on)."""
    if not isinstance(inputs, FrameBatch):
        return inputs
    return [] if images.dtype == torch.uint8 else inputs.rgb_frames(device)
