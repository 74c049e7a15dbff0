"""A plain numpy / Python restatement of the baseline JPEG that ``image_format="jpeg"`` writes, from DESIGN.md section 32 (not from the
kernel): ``encode(rgb, quality, subsampling, restart_mcus) -> bytes``.  The header comes from the package's host builder and is read back
the way a decoder reads it (DQT, SOF0, DHT, DRI); the scan is encoded here.  ``stats`` (a dict) collects what the symbol stream contained."""
import numpy as np

from focoos_amd.jpeg import Jpeg, header_bytes

# position in the zigzag order -> natural index: the anti-diagonals in turn, odd ones downwards, even ones upwards
ZZ = sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8))
_k = np.arange(8)
A = np.round(8192 * np.where(_k == 0, 2 ** -0.5, 1.0)[:, None] * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)).astype(np.int64)


def parse_header(hdr: bytes):
    """(quantisers {id: int64 [64] natural order}, codes {Tc << 4 | Th: {value: (code, length)}}, restart interval, 4:2:0?)"""
    quant, codes, ri, s420, at = {}, {}, 0, False, 2
    while True:
        marker, n = hdr[at + 1], int.from_bytes(hdr[at + 2:at + 4], "big")
        body = hdr[at + 4:at + 2 + n]
        if marker == 0xDB:
            quant[body[0] & 15] = np.zeros(64, np.int64)
            quant[body[0] & 15][ZZ] = list(body[1:65])
        elif marker == 0xC0:
            s420 = body[7] == 0x22
        elif marker == 0xC4:
            tab, code, k = {}, 0, 17
            for length in range(1, 17):
                for _ in range(body[length]):
                    tab[body[k]] = (code, length)
                    code, k = code + 1, k + 1
                code <<= 1
            codes[body[0]] = tab
        elif marker == 0xDD:
            ri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            return quant, codes, ri, s420
        at += 2 + n


def coefficients(rgb: np.ndarray, quant, s420: bool):
    """The quantised blocks of the three components in zigzag order, int64 [rows of blocks, blocks per row, 64] each."""
    mcu = 16 if s420 else 8
    H, W, _ = rgb.shape
    p = np.pad(rgb.astype(np.int64), ((0, -H % mcu), (0, -W % mcu), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
              (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16]
    if s420:
        planes[1:] = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in planes[1:]]
    out = []
    for i, c in enumerate(planes):
        s = (c - 128).reshape(c.shape[0] // 8, 8, c.shape[1] // 8, 8).transpose(0, 2, 1, 3)      # [by, bx, y, x]
        t = (s @ A.T + 1024) >> 11                                                                # [.., y, u]
        F = (A @ t + 65536) >> 17                                                                 # [.., v, u]
        q = quant[min(i, 1)].reshape(8, 8)
        c = np.sign(F) * ((np.abs(F) + (q >> 1)) // q)
        c = c.reshape(*c.shape[:2], 64)
        c[..., 1:] = np.clip(c[..., 1:], -1023, 1023)
        out.append(c[..., ZZ])
    return out


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, code: int, n: int):
        self.v, self.n = self.v << n | code, self.n + n

    def value(self, v: int, size: int):
        self.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)

    def flush(self) -> bytes:
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.v.to_bytes(self.n // 8, "big")


def encode(rgb: np.ndarray, quality: int = 85, subsampling: str = "420", restart_mcus: int = 32, stats: dict = None) -> bytes:
    H, W, _ = rgb.shape
    hdr = header_bytes(H, W, Jpeg(quality, subsampling, restart_mcus))
    quant, codes, ri, s420 = parse_header(hdr)
    Y, Cb, Cr = coefficients(rgb, quant, s420)
    st = stats if stats is not None else {}
    for k in ("zrl", "eob", "c63", "stuffed", "rst7_rst0"):
        st.setdefault(k, 0)
    st.setdefault("dc_cats", set())
    mh, mw = Cb.shape[:2]
    out, pred, bits, last_rst = bytearray(hdr), [0, 0, 0], _Bits(), -1
    for m in range(mh * mw):
        my, mx = divmod(m, mw)
        if m and m % ri == 0:
            data = bits.flush()
            st["stuffed"] += data.count(b"\xff")
            rst = (m // ri - 1) % 8
            st["rst7_rst0"] += last_rst == 7 and rst == 0
            out += data.replace(b"\xff", b"\xff\x00") + bytes([0xFF, 0xD0 + rst])
            pred, bits, last_rst = [0, 0, 0], _Bits(), rst
        blocks = [(0, Y[2 * my + dy, 2 * mx + dx]) for dy in (0, 1) for dx in (0, 1)] if s420 else [(0, Y[my, mx])]
        for comp, z in blocks + [(1, Cb[my, mx]), (2, Cr[my, mx])]:
            dc, ac = codes[min(comp, 1)], codes[0x10 | min(comp, 1)]
            diff, pred[comp] = int(z[0]) - pred[comp], int(z[0])
            size = abs(diff).bit_length()
            st["dc_cats"].add(size)
            bits.put(*dc[size])
            bits.value(diff, size)
            run = 0
            for k in range(1, 64):
                v = int(z[k])
                if v == 0:
                    run += 1
                    continue
                for _ in range(run >> 4):
                    bits.put(*ac[0xF0])
                    st["zrl"] += 1
                size = abs(v).bit_length()
                bits.put(*ac[(run & 15) << 4 | size])
                bits.value(v, size)
                run = 0
            st["c63"] += int(z[63]) != 0
            if run:
                bits.put(*ac[0x00])
                st["eob"] += 1
    data = bits.flush()
    st["stuffed"] += data.count(b"\xff")
    return bytes(out + data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9")


# (H, W, subsampling, restart_mcus) of the GPU test: one MCU; both edges replicated; nine intervals of one MCU; intervals that straddle MCU
# rows with a short last one (fifteen of them in 4:4:4: the RST index wraps); 192 blocks per interval, more than the waves of a workgroup
SHAPES = [(8, 8, "444", 32), (16, 16, "420", 32), (9, 17, "420", 32), (9, 17, "444", 32), (48, 48, "420", 1), (40, 48, "420", 2),
          (40, 48, "444", 2), (64, 128, "420", 32), (64, 128, "444", 64)]
QUALITIES = (1, 50, 100)
KINDS = ("noise", "grey", "checker", "gradient")
_DONE: dict = {}


def reference(kind: str, shape, quality: int):
    """(the image, its file, the stream's stats) of one case: computed once, shared by the tests, never changed."""
    key = (kind, shape, quality)
    if key not in _DONE:
        H, W, ss, rm = shape
        img, st = image(kind, H, W, 1), {}
        img.setflags(write=False)
        _DONE[key] = (img, encode(img, quality, ss, rm, st), st)
    return _DONE[key]


def image(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """The contents the tests encode: uint8 [H, W, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "grey":
        return np.full((H, W, 3), 128, np.uint8)
    if kind == "checker":
        return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    if kind == "gradient":
        base = (x * 200 // max(W - 1, 1) + y * 40 // max(H - 1, 1))[..., None] + np.array([0, 8, 16])
        return np.clip(base + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    raise ValueError(kind)
