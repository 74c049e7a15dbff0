"""fp64 restatement of the device augmentation (csrc/augment.hip), shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py.  Written
from the definition, not from the kernel: PIL's BILINEAR resample (ImagingResample precompute_coeffs: triangle filter of half-width
max(1, in/out) around (x + 0.5) in/out, taps [int(c - s + 0.5), int(c + s + 0.5)) clipped, weights normalised), PIL's NEAREST index
int((x + 0.5) in/out), the flips applied to the source first, the crop taken from the resized image, then the colour blends of
RandomBrightness / RandomContrast / RandomSaturation.  Tap ranges use exact integers (the centre is rational), weights and sums fp64."""
import numpy as np


def axis_matrix(S: int, R: int) -> np.ndarray:
    """[R, S] fp64: row xr holds the normalised triangle weights of resized index xr over the S source samples."""
    M = np.zeros((R, S), dtype=np.float64)
    scale = S / R
    sup = max(1.0, scale)
    for xr in range(R):
        c2 = (2 * xr + 1) * S                       # centre in units of 1 / (2R)
        s2 = 2 * max(R, S)
        k0 = max(0, (c2 - s2 + R) // (2 * R))       # int(centre - support + 0.5), clipped at 0
        k1 = min(S, (c2 + s2 + R) // (2 * R))
        c = (xr + 0.5) * scale
        k = np.arange(k0, k1)
        w = np.clip(1.0 - np.abs(k + 0.5 - c) / sup, 0.0, None)
        M[xr, k0:k1] = w / w.sum()
    return M


def nearest_index(S: int, R: int) -> np.ndarray:
    return np.minimum(((2 * np.arange(R, dtype=np.int64) + 1) * S) // (2 * R), S - 1)


def _window(rec):
    """Resized row / column indices shown by the placed window, after un-mirroring: (rows [crop_h], cols [crop_w])."""
    rows = rec.crop_y + np.arange(rec.crop_h)
    cols = rec.crop_x + np.arange(rec.crop_w)
    if rec.vflip:
        rows = rec.res_h - 1 - rows
    if rec.hflip:
        cols = rec.res_w - 1 - cols
    return rows, cols


def image_f64(src: np.ndarray, rec, pad_value: float = 0.0) -> np.ndarray:
    """[out_h, out_w, 3] fp64 before the final rounding (pad pixels hold pad_value exactly)."""
    assert src.shape == (rec.src_h, rec.src_w, 3)
    rows, cols = _window(rec)
    My, Mx = axis_matrix(rec.src_h, rec.res_h)[rows], axis_matrix(rec.src_w, rec.res_w)[cols]
    x = np.einsum("yh,hwc,xw->yxc", My, src.astype(np.float64), Mx)
    if rec.order:
        mean = src.astype(np.float64).mean()

        def contrast(v):
            return mean * (1.0 - np.float64(np.float32(rec.contrast))) + np.float64(np.float32(rec.contrast)) * v

        def saturation(v):
            grey = v @ np.array([0.299, 0.587, 0.114])
            s = np.float64(np.float32(rec.saturation))
            return grey[..., None] * (1.0 - s) + s * v

        x = x * np.float64(np.float32(rec.brightness))
        x = saturation(contrast(x)) if rec.order == 1 else contrast(saturation(x))
    out = np.full((rec.out_h, rec.out_w, 3), float(pad_value), dtype=np.float64)
    out[rec.pad_y:rec.pad_y + rec.crop_h, rec.pad_x:rec.pad_x + rec.crop_w] = x
    return out


def round_u8(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def boundary_distance(v: np.ndarray) -> np.ndarray:
    """Distance of every value to the nearest rounding boundary k + 0.5."""
    f = v - np.floor(v)
    return np.abs(f - 0.5)


def max_taps(rec) -> int:
    tx = 2 * int(np.ceil(max(1.0, rec.src_w / rec.res_w))) + 1
    ty = 2 * int(np.ceil(max(1.0, rec.src_h / rec.res_h))) + 1
    return tx * ty


def near_tie_margin(rec) -> float:
    """delta: how far the kernel's fp32 value may lie from the fp64 one, from the operation count (u = 2^-24 per rounding, values <= 255).
    Resample: a weight carries 3 roundings (inverse, product, subtraction), so a normalised weight is off by <= 3u relative to a weight sum
    >= 1 -> 3u * 255 per tap over T = tx * ty taps... bounded together with the T fused accumulations (gamma_T) and the normalisation
    (3 roundings) by (2T + 6) u * 255.  Colour: brightness <= 1.126, contrast and saturation <= 1.5 each amplify that by <= 2.54, and add
    <= 12 roundings on values <= 2.54 * 255 (the mean's and the blend weights' own roundings included)."""
    u = 2.0 ** -24
    T = max_taps(rec)
    d = (2 * T + 6) * u * 255.0
    if rec.order:
        d = 2.54 * d + 12 * u * 2.54 * 255.0
    return d


def labels_ref(plane: np.ndarray, rec, pad_value: int) -> np.ndarray:
    rows, cols = _window(rec)
    iy, ix = nearest_index(rec.src_h, rec.res_h)[rows], nearest_index(rec.src_w, rec.res_w)[cols]
    out = np.full((rec.out_h, rec.out_w), pad_value, dtype=plane.dtype)
    out[rec.pad_y:rec.pad_y + rec.crop_h, rec.pad_x:rec.pad_x + rec.crop_w] = plane[np.ix_(iy, ix)]
    return out


# ---- the resample / colour cases of tests/test_gpu_augment.py (tests/test_augment_cpu.py checks on the CPU that the restatement alone keeps
# its near-boundary share under the cap for these inputs) ------------------------------------------------------------------------------
def _source(index: int, h: int, w: int, noise: bool) -> np.ndarray:
    from focoos_amd.synth import synth_image_structured

    if noise:
        return np.random.RandomState(1000 + index).randint(0, 256, (h, w, 3)).astype(np.uint8)
    return synth_image_structured(300 + index, h, w)


def case_batches():
    """[(name, sources, records)]: B >= 3 images of different sizes per batch; odd sizes, up- and down-scaling, windows that touch the left /
    right / top / bottom border of the resized image, pad on each side, both flips, both colour orders.  Batch "vec" has Wo % 16 == 0 (16-byte
    stores), batch "odd" an odd Wo (byte stores)."""
    from focoos_amd.augment import ORDER_BCS, ORDER_BSC, AugRecord

    def rec(src, oh, ow, rh, rw, cx, cy, cw, ch, px=0, py=0, **kw):
        return AugRecord(src_h=src[0], src_w=src[1], out_h=oh, out_w=ow, res_h=rh, res_w=rw, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, pad_x=px,
                         pad_y=py, **kw)

    out = []
    for name, (oh, ow) in (("vec", (96, 112)), ("odd", (75, 101))):
        sizes = [(67, 91), (200, 301), (120, 75), (50, 50), (231, 173), (64, 64)]
        srcs = [_source(i, h, w, noise=i in (3, 4)) for i, (h, w) in enumerate(sizes)]
        recs = [
            # up-scaling 1.7x, window in the top-left corner of the resized image, fills the output
            rec(sizes[0], oh, ow, 114, 155, 0, 0, ow, oh),
            # down-scaling 2.3x, whole height (touches top and bottom), touches the right border, pad above and below, horizontal flip + colour
            rec(sizes[1], oh, ow, 70, 131, 131 - ow, 0, ow, 70, 0, (oh - 70) // 2, hflip=True, brightness=1.09, contrast=0.62, saturation=1.4,
                order=ORDER_BCS),
            # up-scaling 1.33x, whole width (touches left and right), touches the bottom border, pad left and right, vertical flip
            rec(sizes[2], oh, ow, 160, 100, 0, 160 - oh, 100, oh, (ow - 100) // 2, 0, vflip=True, saturation=0.55, order=ORDER_BSC),
            # scale 1 on noise, both flips, a small window in the middle of the pad, every colour operation
            rec(sizes[3], oh, ow, 50, 50, 0, 0, 50, 50, 31, 23, hflip=True, vflip=True, brightness=0.9, contrast=1.45, saturation=0.7,
                order=ORDER_BSC),
            # down-scaling 3x on noise (49 taps), interior window
            rec(sizes[4], oh, ow, 77, 58, 3, 5, 50, 70, ow - 50, oh - 70, contrast=1.3, order=ORDER_BCS),
            # anisotropic: 64x64 -> 96 rows x 40 columns (a non-square resolution's Resize)
            rec(sizes[5], oh, ow, 96, 40, 0, 10, 40, min(oh, 80), 7, 0),
        ]
        out.append((name, srcs, recs))
    return out


def near_boundary_share(src, rec):
    v = image_f64(src, rec)
    return float((boundary_distance(v) < near_tie_margin(rec)).mean())
