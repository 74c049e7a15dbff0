"""numpy restatement of the video-frame conversion (include/focoos_amd.h fx_frames_ingest), written from the definition
and not from csrc/frame_ops.hip: per format the frame's planes (any row pitch: numpy strides) -> uint8 RGB [H][W][3].  Integer arithmetic
only, so the device result is compared with it for equality."""
import numpy as np

# (cy, crv, cgu, cgv, cbu, luma offset): the standard matrices times 256, rounded
COEF = {
    ("bt601", "limited"): (298, 409, 100, 208, 516, 16),
    ("bt601", "full"): (256, 359, 88, 183, 454, 0),
    ("bt709", "limited"): (298, 459, 55, 136, 541, 16),
    ("bt709", "full"): (256, 403, 48, 120, 475, 0),
}
# Kr, Kb of the two standards: the float64 matrices the tables are rounded from
LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def yuv_to_rgb(Y, U, V, matrix="bt601", range="limited"):
    """Element-wise on integer arrays of one shape -> uint8 [..., 3]."""
    cy, crv, cgu, cgv, cbu, off = COEF[(matrix, range)]
    c = cy * (np.asarray(Y, dtype=np.int32) - off)
    d = np.asarray(U, dtype=np.int32) - 128
    e = np.asarray(V, dtype=np.int32) - 128
    r = (c + crv * e + 128) >> 8           # numpy's >> on int32 is arithmetic
    g = (c - cgu * d - cgv * e + 128) >> 8
    b = (c + cbu * d + 128) >> 8
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def yuv_to_rgb_f64(Y, U, V, matrix="bt601", range="limited"):
    """clip(rint(float64 matrix)): what the integer tables approximate."""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    Y, U, V = (np.asarray(a, dtype=np.float64) for a in (Y, U, V))
    if range == "limited":
        y, cb, cr = (Y - 16.0) / 219.0, (U - 128.0) / 224.0, (V - 128.0) / 224.0
    else:
        y, cb, cr = Y / 255.0, (U - 128.0) / 255.0, (V - 128.0) / 255.0
    r = y + 2.0 * (1.0 - kr) * cr
    b = y + 2.0 * (1.0 - kb) * cb
    g = y - (2.0 * kr * (1.0 - kr) / kg) * cr - (2.0 * kb * (1.0 - kb) / kg) * cb
    return np.clip(np.rint(np.stack([r, g, b], -1) * 255.0), 0, 255).astype(np.uint8)


def to_rgb(format, planes, height, width, matrix="bt601", range="limited"):
    """One frame -> contiguous uint8 RGB [H][W][3].  ``planes`` are numpy arrays shaped as the table of DESIGN 21 says (strided views
    allowed).  Chroma is replicated: pixel (y, x) uses the sample (y >> 1, x >> 1)."""
    if format == "rgb24":
        return np.ascontiguousarray(planes[0])
    if format == "bgr24":
        return np.ascontiguousarray(planes[0][:, :, ::-1])
    yy, xx = np.mgrid[0:height, 0:width]
    Y = planes[0]
    if format == "nv12":
        U, V = planes[1][yy >> 1, xx >> 1, 0], planes[1][yy >> 1, xx >> 1, 1]
    elif format == "i420":
        U, V = planes[1][yy >> 1, xx >> 1], planes[2][yy >> 1, xx >> 1]
    else:
        raise ValueError(format)
    return np.ascontiguousarray(yuv_to_rgb(Y, U, V, matrix, range))


def frame_to_rgb(frame):
    """A focoos_amd.frames.Frame with host planes -> RGB."""
    planes = [p.cpu().numpy() if hasattr(p, "cpu") else p for p in frame.planes]
    return to_rgb(frame.format, planes, frame.height, frame.width, frame.matrix, frame.range)


def rgb_to_yuv_planes(rgb, noise_seed):
    """Test material: Y, U, V planes (U, V at half resolution, rounded up) from an RGB picture by a plain full-range 601 forward map plus
    seeded noise, so flat areas, edges and out-of-gamut triples that clip all occur.  Nothing depends on this map being exact."""
    rs = np.random.RandomState(noise_seed)
    f = rgb.astype(np.float64)
    H, W = rgb.shape[:2]
    y = 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]
    u = 128.0 + 0.564 * (f[..., 2] - y)
    v = 128.0 + 0.713 * (f[..., 0] - y)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    q = lambda a: np.clip(np.rint(a + rs.randint(-40, 41, a.shape)), 0, 255).astype(np.uint8)      # noqa: E731
    return q(y), q(u[::2, ::2][:ch, :cw]), q(v[::2, ::2][:ch, :cw])
