"""Device PNG encoding on a real MI355X (csrc/mask_png.hip through focoos_amd/mask_png.py), exact throughout: every file fx_mask_png_encode
stores decodes (every CRC-32 and the Adler-32 checked, and again through PIL) to the trimmed mask; lengths, offsets, capacity rule,
sentinel, determinism, refusals; mask_format="png_device" end to end against the default "png".  Size gates, from
the restated tokenisation on the CPU: device IDAT payloads are 1.107 x the host encoder's over the blob cases and the 200 x 300 ellipse, 1.40 x
at worst (a 4 x 6 crop: the constant 21-byte block header); gated at 1.25 x those.  Shorter than Z_FIXED holds from 210 scanline bytes on."""
import base64
import io
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from focoos_amd import _lib
from focoos_amd import mask_png as M
from focoos_amd.processor import binary_mask_to_base64
from focoos_amd.synth import synth_image_structured

from . import mask_png_ref as R
from .mask_rle_ref import pack_words

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
SENTINEL = -777
B, Q, COUNT = 2, 3, [3, 1]
SLOTS = [(b, j) for b in range(B) for j in range(COUNT[b])]
GARBAGE_BOX = [-5, 7, 10 ** 9, -3]
RATIO_ALL, RATIO_ONE = 1.25 * 1.107, 1.25 * 1.40


def run(H, W, slots, capacity, sentinel=SENTINEL):
    """One call on B = 2, Q = 3, det_count = [3, 1]: ``slots`` = (mask, box) of the four detections, garbage in the other two slots."""
    lib = _lib.load()
    rs = np.random.RandomState(H + W)
    words = rs.randint(-2 ** 31, 2 ** 31 - 1, (B, Q, H, (W + 31) // 32), dtype=np.int64).astype(np.int32)
    boxes = np.tile(np.array(GARBAGE_BOX, np.int32), (B, Q, 1))
    for (b, j), (m, box) in zip(SLOTS, slots):
        words[b, j], boxes[b, j] = pack_words(m), box
    d_words, d_boxes = torch.from_numpy(words).to(DEV), torch.from_numpy(boxes).to(DEV)
    d_count = torch.tensor(COUNT, dtype=torch.int32, device=DEV)
    ln = torch.full((B, Q), SENTINEL, dtype=torch.int32, device=DEV)
    off = torch.full((B, Q), SENTINEL, dtype=torch.int32, device=DEV)
    pool = torch.full((B, capacity), sentinel, dtype=torch.int32, device=DEV)
    nb = lib.fx_mask_png_workspace_bytes(B, Q, H, W)
    assert nb == 8 * B * Q * (H + 1) + 4 * B * Q
    ws = torch.randint(0, 255, (nb,), dtype=torch.uint8, device=DEV)      # contents irrelevant
    rc = lib.fx_mask_png_encode(d_words.data_ptr(), d_count.data_ptr(), d_boxes.data_ptr(), B, Q, H, W, capacity, ln.data_ptr(), off.data_ptr(),
                                pool.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return ln.cpu().numpy(), off.cpu().numpy(), pool.cpu().numpy()


def check(H, W, slots, capacity, lengths=None):
    """Checks everything the contract states; ``lengths``: the true png_len (from a call with room for all) when some slots may not fit.
    Returns ({(b, j): base64 text of a stored slot}, png_len of the four detections)."""
    ln, off, pool = run(H, W, slots, capacity)
    want = [R.crop(m, box) for m, box in slots]
    untouched, texts, run_off = np.ones_like(pool, bool), {}, {b: 0 for b in range(B)}
    for b in range(B):
        assert (ln[b, COUNT[b]:] == 0).all()      # the garbage slots
    for k, ((b, j), img) in enumerate(zip(SLOTS, want)):
        assert off[b, j] == run_off[b], (H, W, b, j)      # the exclusive prefix sum of the positive lengths
        if img is None:
            assert ln[b, j] == -1
            continue
        assert ln[b, j] > 0 and (lengths is None or ln[b, j] == lengths[k])
        run_off[b] += ln[b, j]
        if off[b, j] + ln[b, j] > capacity:
            continue
        quads = pool[b, off[b, j]:off[b, j] + ln[b, j]]
        untouched[b, off[b, j]:off[b, j] + ln[b, j]] = False
        text = quads.tobytes().decode("ascii")
        png = base64.b64decode(text, validate=True)
        assert ln[b, j] == (len(png) + 2) // 3
        assert np.array_equal(M.decode_png(text), img), (H, W, b, j)
        pil = np.array(Image.open(io.BytesIO(png)))
        assert pil.dtype == np.uint8 and np.array_equal(pil, img.astype(np.uint8) * 255), (H, W, b, j)
        texts[(b, j)] = text
    for b in range(B):
        assert (off[b, COUNT[b]:] == run_off[b]).all()
    assert (pool[untouched] == SENTINEL).all()      # nothing is written outside the stored ranges
    return texts, [int(ln[b, j]) for b, j in SLOTS]


@pytest.mark.parametrize("H,W", R.FRAMES)
def test_every_stored_file_decodes_to_the_trimmed_mask(H, W):
    cs = R.cases(H, W)
    empty = 0
    for i in range(0, len(cs), 4):
        chunk = (cs[i:i + 4] + cs[:4])[:4]
        slots = [(c[1], c[2]) for c in chunk]
        texts, _ = check(H, W, slots, M.default_capacity(Q, H, W) * 8)      # room for the checkerboard: far from one segment per row
        empty += len(slots) - len(texts)
    assert empty >= 2      # the stripes' tight boxes: a crop with no pixel has length -1


def test_capacity_rule_and_sentinel():
    H, W = 33, 65
    cs = {c[0]: c for c in R.cases(H, W)}
    slots = [(cs[n][1], cs[n][2]) for n in ("blob1", "checker/frame", "corners", "blob2")]
    texts, ln = check(H, W, slots, 8192)
    assert len(texts) == 4
    # room for slot 0 only: exactly the later slots of image 0 are not stored (slot 2's offset lies behind slot 1's true length)
    texts0, _ = check(H, W, slots, ln[0], lengths=ln)
    assert set(texts0) == {(0, 0)} and ln[3] > ln[0] and texts0[(0, 0)] == texts[(0, 0)]
    # one quad short of image 0's total: its last slot is not stored; one more and everything is
    total = ln[0] + ln[1] + ln[2]
    assert set(check(H, W, slots, total - 1, lengths=ln)[0]) == {(0, 0), (0, 1), (1, 0)}
    assert check(H, W, slots, total, lengths=ln)[0] == texts


def test_a_file_longer_than_one_window():
    """Checkerboard rows take 2.5 bits a pixel: the file spans three 12288-byte windows of the emit kernel, rows straddle their borders and
    the CRC-32 register is carried across them.  Two calls give byte-equal pools, and the pool is not filled."""
    H, W = 300, 330
    yy, xx = np.indices((H, W))
    noisy = ((yy + xx) % 2 == 0) | (yy % 7 == 0)
    slots = [(noisy, [0, 0, W, H]), (R.blob(H, W, 3), [0, 0, W - 1, H - 1]), (noisy, [3, 2, W - 40, H - 1]), (R.blob(H, W, 4), [0, 0, W, H])]
    texts, ln = check(H, W, slots, 60000)
    assert len(texts) == 4 and ln[0] * 3 > 2 * 12288
    a, b = run(H, W, slots, 60000), run(H, W, slots, 60000)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and not np.array_equal(a[2], run(H, W, slots, 60000, sentinel=SENTINEL - 1)[2])


def test_arguments_outside_the_contract_are_refused():
    lib = _lib.load()
    H, W, cap = 5, 7, 64
    t = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device=DEV)      # noqa: E731
    words, count, boxes, ln, off, pool = t(B, Q, H, 1), t(B), t(B, Q, 4), t(B, Q), t(B, Q), t(B, cap)
    nb = lib.fx_mask_png_workspace_bytes(B, Q, H, W)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    base = [words.data_ptr(), count.data_ptr(), boxes.data_ptr(), B, Q, H, W, cap, ln.data_ptr(), off.data_ptr(), pool.data_ptr(), ws.data_ptr(), nb,
            torch.cuda.current_stream().cuda_stream]
    for pos, val in ((0, None), (1, None), (2, None), (8, None), (9, None), (10, None), (11, None), (0, words.data_ptr() + 2),
                     (11, ws.data_ptr() + 4), (3, 0), (4, 0), (4, 65536), (3, 65536), (5, 0), (6, 0), (7, 0), (12, nb - 1), (5, 1 << 16)):
        args = list(base)
        args[pos] = val
        if (pos, val) == (5, 1 << 16):
            args[6] = 1 << 15      # H W = 2^31
        assert lib.fx_mask_png_encode(*args) == INVALID, (pos, val)
    assert lib.fx_mask_png_workspace_bytes(B, Q, 1 << 16, 1 << 15) == 0 and lib.fx_mask_png_workspace_bytes(0, Q, H, W) == 0
    assert lib.fx_mask_png_workspace_bytes(B, 65535, 4096, 4096) == 0      # Q x the longest file of the frame passes 2^31 quads
    torch.cuda.synchronize()
    for x in (ln, off, pool):
        assert (x == SENTINEL).all()      # nothing was launched or written
    assert lib.fx_mask_png_encode(*base) == 0      # det_count = -777: no detections
    torch.cuda.synchronize()
    assert (ln == 0).all() and (off == 0).all() and (pool == SENTINEL).all()


def test_payload_sizes():
    groups = [(H, W, [c for c in R.cases(H, W) if c[0].startswith("blob")]) for H, W in R.FRAMES] + [(200, 300, [("ellipse", R.ellipse(), [0, 0, 300, 200])])]
    dev, host, fixed, raw, residues = {}, {}, {}, {}, set()
    for H, W, cs in groups:
        for i in range(0, len(cs), 4):
            four = (cs[i:i + 4] + cs * 4)[:4]      # a call has four detections: the cases of the frame, repeated where they run out
            texts, _ = check(H, W, [(c[1], c[2]) for c in four], 8192)
            for (b, j), (name, m, box) in zip(SLOTS, four):
                n, img = f"{H}x{W} {name}", R.crop(m, box)
                dev[n], host[n] = R.idat_bytes(texts[(b, j)]), R.idat_bytes(binary_mask_to_base64(img))
                fixed[n], raw[n] = R.zfixed_bytes(img), len(R.scanlines(img))
                residues.add(len(base64.b64decode(texts[(b, j)])) % 3)
    for n in dev:
        print(f"{n}: scanlines {raw[n]}, device {dev[n]}, host {host[n]} ({dev[n] / host[n]:.3f} x), Z_FIXED {fixed[n]}")
    print(f"all: device {sum(dev.values())}, host {sum(host.values())} ({sum(dev.values()) / sum(host.values()):.3f} x)")
    assert len(dev) == 26 and residues == {0, 1, 2}      # the PNG byte lengths took every residue: no, two and one '='
    for n in dev:
        assert dev[n] <= RATIO_ONE * host[n], n
        assert dev[n] < fixed[n] or raw[n] < 210, n
    assert raw["200x300 ellipse"] >= 210 and sum(dev.values()) <= RATIO_ALL * sum(host.values())


# ---------------------------------------------------------------- end to end
_MODELS = {}


@pytest.fixture(params=["fai-mf-l-coco-ins", "bisenetformer-l-ade"], ids=["threshold-branch", "all-pixels-branch"])
def fm(request):
    from focoos_amd.model import ModelManager

    if request.param not in _MODELS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
            _MODELS[request.param] = ModelManager.get(request.param, device=DEV, seed=3)
    return _MODELS[request.param]


def _plain(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label) for d in res.detections]


def _decoded(results):
    """everything of the results but the PNG's bytes: the fields, and what each mask decodes to"""
    return [[(tuple(d.bbox), d.conf, d.cls_id, d.label, d.rle, d.track_id, M.decode_png(d.mask).tobytes(), M.decode_png(d.mask).shape)
             for d in r.detections] for r in results]


def _batches(n, h=192, w=256):
    return [[synth_image_structured(500 + 10 * j + i, h, w) for i in range(2)] for j in range(n)]


def test_png_device_equals_the_default_path(fm):
    batches = _batches(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # masks of random weights are noise: some may already overflow the default pool
        png = [fm.infer_batch(b, threshold=0.05) for b in batches]
        dev = [fm.infer_batch(b, threshold=0.05, mask_format="png_device") for b in batches]
        stream = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="png_device"))
        enc = fm.processor._png_encoder
        one = fm.infer(batches[0][0], threshold=0.05, mask_format="png_device")
    n = sum(len(r.detections) for p in png for r in p)
    print(f"{fm.model.family}: {n} detections in 6 images, {enc.total_fallback} of {enc.total_masks} masks fell back at the default capacity")
    assert n > 0 and enc.total_masks > enc.total_fallback      # the device path was taken
    for p, d, s in zip(png, dev, stream):
        assert [_plain(r) for r in p] == [_plain(r) for r in d]
        assert _decoded(p) == _decoded(d) == _decoded(s)
    assert len(one.detections) > 0 and _decoded([one]) == _decoded([fm.infer(batches[0][0], threshold=0.05)])      # the single-picture entry point
    # a pool too small for any mask: the host fallback gives decode-equal results, and warns
    fm.processor.png_capacity = 8
    try:
        with pytest.warns(RuntimeWarning, match="encoded on the host"):
            small = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="png_device"))
        assert fm.processor._png_encoder.capacity == 8 and fm.processor._png_encoder.last_fallback > 0
    finally:
        fm.processor.png_capacity = None
    assert [_decoded(s) for s in small] == [_decoded(p) for p in png]
    # annotate reads the packed device results, not FocoosDet.mask
    a_png = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a_dev = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True, mask_format="png_device"))[0]
    for img, p, r in zip(batches[0], a_png, a_dev):
        assert _plain(p) == _plain(r) and np.array_equal(p.image, r.image) and (p.image != img).any()
