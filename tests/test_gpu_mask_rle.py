"""Device RLE encoding on a real MI355X (csrc/mask_rle.hip through focoos_amd/mask_rle.py): fx_mask_rle_encode bit-exact against the
restatement of tests/mask_rle_ref.py on masks written straight into a mask_words tensor (tight and full-frame boxes, the capacity rule, a
sentinel over the pool, determinism, the refusals), and mask_format="rle" end to end on the two mask families with seeded synthetic
weights against the default PNG path.  All values are integers: no tolerance anywhere.  Nothing here reads the reference tree."""
import base64
import io
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import mask_rle as M
from focoos_amd.processor import trim_mask
from focoos_amd.synth import synth_image_structured

from . import mask_rle_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
SENTINEL = -777
SHAPES = [(5, 7), (33, 65), (64, 64), (70, 100), (6, 300)]      # 300 columns: the scan kernel carries its sum and its max across a chunk of 256
B, Q, COUNT = 2, 3, [3, 1]
GARBAGE_BOX = [-5, 7, 10 ** 9, -3]


def _slots(count):
    return [(b, j) for b in range(B) for j in range(count[b])]      # the detections in (image, slot) order


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _blob(H, W, seed):
    """a seeded blob: a noisy disc with holes, ragged in every column"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    cy, cx, r = rs.uniform(0.3, 0.7) * H, rs.uniform(0.3, 0.7) * W, 0.35 * min(H, W) + 1
    return (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r) & (rs.rand(H, W) < 0.8)


def _masks(H, W):
    z = lambda: np.zeros((H, W), bool)      # noqa: E731
    full = np.ones((H, W), bool)
    first, last, stripe, lastcol = z(), z(), z(), z()
    first[0, 0] = True
    last[H - 1, W - 1] = True
    x = W // 2
    stripe[H // 2:, x], stripe[:H // 2 + 1, x + 1] = True, True      # the bottom of column x runs on into the top of column x + 1
    lastcol[:, W - 1] = True
    yy, xx = np.indices((H, W))
    checker = (yy + xx) % 2 == 0
    # every element of the column-major sequence differs from the one before it, s[0] set: the most counts a mask can have, H W + 1.  For an
    # odd H this is the checkerboard itself; for an even H the checkerboard's columns meet in runs of two and this mask is its own case
    alternate = (xx * H + yy) % 2 == 0
    return {"full": full, "first": first, "last": last, "stripe": stripe, "lastcol": lastcol, "checker": checker, "alternate": alternate,
            "blob1": _blob(H, W, 1), "blob2": _blob(H, W, 2)}


_CASES = {}


def cases(H, W):
    """[(name, mask, box, reference counts)] of a shape, computed once: every mask with its tight box and with the full frame, and one
    all-zero slot with box [0, 0, 0, 0]."""
    if (H, W) not in _CASES:
        out = []
        for name, m in _masks(H, W).items():
            ref = R.encode_mask(m)
            out.append((name, m, R.tight_box(m), ref))
            out.append((name + "/frame", m, [0, 0, W - 1, H - 1], ref))
        out.append(("empty", np.zeros((H, W), bool), [0, 0, 0, 0], [H * W]))
        _CASES[(H, W)] = out
    return _CASES[(H, W)]


def run(H, W, slots, capacity, sentinel=SENTINEL, Q=Q, count=COUNT):
    """One fx_mask_rle_encode call on B = 2, Q = 3, det_count = [3, 1] unless given: ``slots`` = the (mask, box) of the detections, by default
    four for (0, 0), (0, 1), (0, 2), (1, 0); the other slots (1 and 2 of image 1) hold garbage words and boxes.  Returns (words, rle_len,
    rle_off, pool) as numpy arrays."""
    lib = _lib.load()
    rs = np.random.RandomState(H + W)
    W32 = (W + 31) // 32
    words = rs.randint(-2 ** 31, 2 ** 31 - 1, (B, Q, H, W32), dtype=np.int64).astype(np.int32)
    boxes = np.tile(np.array(GARBAGE_BOX, np.int32), (B, Q, 1))
    assert len(slots) == sum(count)
    for (b, j), (m, box) in zip(_slots(count), slots):
        words[b, j], boxes[b, j] = R.pack_words(m), box
    d_words, d_boxes = torch.from_numpy(words).to(DEV), torch.from_numpy(boxes).to(DEV)
    d_count = torch.tensor(count, dtype=torch.int32, device=DEV)
    ln = torch.full((B, Q), SENTINEL, dtype=torch.int32, device=DEV)
    off = torch.full((B, Q), SENTINEL, dtype=torch.int32, device=DEV)
    pool = torch.full((B, capacity), sentinel, dtype=torch.int32, device=DEV)
    nb = lib.fx_mask_rle_workspace_bytes(B, Q, H, W)
    assert nb == (2 * B * Q * W + B * Q) * 4
    ws = torch.randint(0, 255, (nb,), dtype=torch.uint8, device=DEV)      # contents irrelevant
    rc = lib.fx_mask_rle_encode(d_words.data_ptr(), d_count.data_ptr(), d_boxes.data_ptr(), B, Q, H, W, capacity, ln.data_ptr(), off.data_ptr(),
                                pool.data_ptr(), ws.data_ptr(), nb, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return words, ln.cpu().numpy(), off.cpu().numpy(), pool.cpu().numpy()


def check(H, W, slots, refs, capacity, unstored, Q=Q, count=COUNT):
    """Runs the call and checks everything the contract states; ``unstored`` = the exact set of (b, j) that must not be stored."""
    words, ln, off, pool = run(H, W, slots, capacity, Q=Q, count=count)
    lengths = np.full((B, Q), 99)      # of the garbage slots: ignored by the rule
    for (b, j), ref in zip(_slots(count), refs):
        lengths[b, j] = len(ref)
    want_ln, want_off, want_st = R.capacity_rule(lengths.tolist(), count, capacity)
    assert np.array_equal(ln, want_ln) and np.array_equal(off, want_off)      # true lengths, stored or not; 0 for the garbage slots
    assert {(b, j) for (b, j) in _slots(count) if not want_st[b, j]} == set(unstored)
    untouched = np.ones_like(pool, bool)
    for (b, j), ref in zip(_slots(count), refs):
        if not want_st[b, j]:
            continue
        got = pool[b, off[b, j]:off[b, j] + ln[b, j]]
        assert got.tolist() == ref, (H, W, b, j)
        assert int(got.sum()) == H * W and int(got[1::2].sum()) == R.popcount_words(words[b, j])
        untouched[b, off[b, j]:off[b, j] + ln[b, j]] = False
    assert (pool[untouched] == SENTINEL).all()      # nothing is written outside the stored ranges
    return pool


@pytest.mark.parametrize("H,W", SHAPES)
def test_encode_is_bit_exact(H, W):
    cs = cases(H, W)
    assert len(cs) == 19 and max(len(c[3]) for c in cs) == H * W + 1      # the most counts a mask can have
    cap = 3 * (H * W + 1) + 5
    for i in range(0, len(cs), 4):
        chunk = (cs[i:i + 4] + cs[:4])[:4]
        check(H, W, [(c[1], c[2]) for c in chunk], [c[3] for c in chunk], cap, unstored=())


def test_capacity_rule_and_sentinel():
    H, W = 33, 65
    cs = {c[0]: c for c in cases(H, W)}
    blob, checker, first, stripe = cs["blob1"], cs["checker"], cs["first"], cs["stripe"]
    assert len(checker[3]) == H * W + 1      # H is odd: the checkerboard is the mask with the most counts
    # the checkerboard in slot 1 of 3: slot 0 fits, slot 1 does not - and slot 2, whose offset lies behind slot 1's true length, cannot either
    cap = len(blob[3]) + 10
    order = [blob, checker, first, stripe]
    check(H, W, [(c[1], c[2]) for c in order], [c[3] for c in order], cap, unstored={(0, 1), (0, 2)})
    # the checkerboard last: exactly one slot is not stored, the two before it are
    order = [blob, first, checker, stripe]
    cap = len(blob[3]) + len(first[3]) + len(checker[3]) - 1
    check(H, W, [(c[1], c[2]) for c in order], [c[3] for c in order], cap, unstored={(0, 2)})
    # one count more and everything is stored
    check(H, W, [(c[1], c[2]) for c in order], [c[3] for c in order], cap + 1, unstored=())


def test_slot_offsets_over_260_slots():
    """rle_off of slot j sums j lengths: from slot 257 on the 256 threads of the emit kernel take a second length each, and all four wavefronts
    contribute.  The masks are the shape's cases, cyclically; the pool holds the most 260 masks of this frame can have."""
    H, W, Qn = 5, 7, 260
    count = [Qn, 1]
    cs = cases(H, W)
    chosen = [cs[i % len(cs)] for i in range(sum(count))]
    check(H, W, [(c[1], c[2]) for c in chosen], [c[3] for c in chosen], Qn * (H * W + 1), unstored=(), Q=Qn, count=count)


def test_two_calls_give_byte_equal_pools():
    H, W = 70, 100
    cs = {c[0]: c for c in cases(H, W)}
    slots = [(cs[n][1], cs[n][2]) for n in ("blob1", "checker", "blob2", "stripe")]
    cap = 3 * (H * W + 1)
    a, b = run(H, W, slots, cap), run(H, W, slots, cap)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(a[3], run(H, W, slots, cap, sentinel=SENTINEL - 1)[3])      # the sentinel shows: the pool is not filled


def test_arguments_outside_the_contract_are_refused():
    lib = _lib.load()
    H, W, cap = 5, 7, 64
    t = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)      # noqa: E731
    words, count, boxes, ln, off, pool = t(B, Q, H, 1), t(B), t(B, Q, 4), t(B, Q), t(B, Q), t(B, cap)
    nb = lib.fx_mask_rle_workspace_bytes(B, Q, H, W)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    base = [words.data_ptr(), count.data_ptr(), boxes.data_ptr(), B, Q, H, W, cap, ln.data_ptr(), off.data_ptr(), pool.data_ptr(), ws.data_ptr(), nb,
            _stream()]
    assert lib.fx_mask_rle_encode(*base) == 0
    for pos, val in ((0, None), (1, None), (2, None), (8, None), (9, None), (10, None), (11, None), (0, words.data_ptr() + 2), (3, 0), (4, 0),
                     (4, 65536), (5, 0), (6, 0), (7, 0), (12, nb - 1), (5, 1 << 16)):
        args = list(base)
        args[pos] = val
        if (pos, val) == (5, 1 << 16):
            args[6] = 1 << 15      # H W = 2^31
        assert lib.fx_mask_rle_encode(*args) == INVALID, (pos, val)
    assert lib.fx_mask_rle_workspace_bytes(B, Q, 1 << 16, 1 << 15) == 0 and lib.fx_mask_rle_workspace_bytes(0, Q, H, W) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- end to end
def _get(name, seed):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get(name, device=DEV, seed=seed)


_MODELS = {}


@pytest.fixture(params=["fai-mf-l-coco-ins", "bisenetformer-l-ade"], ids=["threshold-branch", "all-pixels-branch"])
def fm(request):
    if request.param not in _MODELS:
        _MODELS[request.param] = _get(request.param, 3)
    return _MODELS[request.param]


def _png_mask(b64):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(base64.b64decode(b64)))) > 0


def _plain(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label) for d in res.detections]


def _full(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask, None if d.rle is None else (tuple(d.rle["size"]), tuple(d.rle["counts"])), d.track_id)
            for d in res.detections]


def _batches(n, h=192, w=256):
    return [[synth_image_structured(500 + 10 * j + i, h, w) for i in range(2)] for j in range(n)]


def test_rle_equals_the_default_path(fm):
    h, w = 192, 256
    imgs = _batches(1)[0]
    png = fm.infer_batch(imgs, threshold=0.05)
    rle = fm.infer_batch(imgs, threshold=0.05, mask_format="rle")
    none = fm.infer_batch(imgs, threshold=0.05, mask_format="none")
    n = sum(len(r.detections) for r in png)
    print(f"{fm.model.family} {h} x {w}: {n} detections in 2 images")
    assert n > 0 and len(png) == len(rle) == len(none) == 2
    for p, r, o in zip(png, rle, none):
        assert _plain(p) == _plain(r) == _plain(o)
        assert all(d.mask is None and d.rle is None for d in o.detections)
        for dp, dr in zip(p.detections, r.detections):
            assert dr.mask is None and dp.rle is None and dr.rle["size"] == [h, w]
            full = M.rle_decode(dr.rle)
            x0, y0, x1, y1 = dr.bbox
            want = _png_mask(dp.mask) if (x1 > x0 and y1 > y0) else np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), bool)
            assert np.array_equal(trim_mask(full, dr.bbox), want)
            outside = full.copy()
            outside[y0:y1 + 1, x0:x1 + 1] = False
            assert not outside.any() and full.any()
            assert full[y0].any() and full[y1].any() and full[:, x0].any() and full[:, x1].any()      # the box is the mask's extent
    # the single-picture entry point takes the keyword too
    one, one_png = fm.infer(imgs[0], threshold=0.05, mask_format="rle"), fm.infer(imgs[0], threshold=0.05)
    assert len(one.detections) > 0 and _plain(one) == _plain(one_png)
    assert all(d.mask is None and M.rle_area(d.rle) > 1 for d in one.detections)


def test_stream_fallback_and_annotate(fm):
    batches = _batches(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # masks of random weights are noise: some may already overflow the default pool
        want = [fm.infer_batch(b, threshold=0.05, mask_format="rle") for b in batches]
        got = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="rle"))
    assert sum(len(d.detections) for w_ in want for d in w_) > 0
    print(f"{fm.model.family}: {fm.processor._rle_encoder.last_fallback} slots of the last batch fell back at the default capacity")
    assert [[_full(d) for d in g] for g in got] == [[_full(d) for d in w_] for w_ in want]
    # a pool too small for most masks: the host fallback gives identical results, and warns
    fm.processor.rle_capacity = 8
    try:
        with pytest.warns(RuntimeWarning, match="encoded on the host"):
            small = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="rle"))
        assert fm.processor._rle_encoder.capacity == 8 and fm.processor._rle_encoder.last_fallback > 0
    finally:
        fm.processor.rle_capacity = None
    assert [[_full(d) for d in g] for g in small] == [[_full(d) for d in w_] for w_ in want]
    # annotate reads the packed device results, not FocoosDet.mask
    a_png = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a_rle = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True, mask_format="rle"))[0]
    for img, p, r in zip(batches[0], a_png, a_rle):
        assert _plain(p) == _plain(r) and np.array_equal(p.image, r.image) and (p.image != img).any()
