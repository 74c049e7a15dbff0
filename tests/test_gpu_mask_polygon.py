"""Device polygon tracing on a real MI355X (csrc/mask_polygon.hip through focoos_amd/mask_polygon.py): fx_mask_polygon_encode bit-exact against
the restatement of tests/mask_polygon_ref.py on masks written straight into a mask_words tensor (tight and full-frame boxes, the rules of the
pool and of the edge workspace, a sentinel over the pool, determinism, the refusals), and mask_format="polygon" end to end on the two mask
families with seeded synthetic weights against the default PNG path.  All values are integers: no tolerance anywhere.  Nothing here reads
the reference tree."""
import base64
import io
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import mask_polygon as P
from focoos_amd.processor import trim_mask
from focoos_amd.synth import synth_image_structured

from . import mask_polygon_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
SENTINEL = -777
SHAPES = [(5, 7), (33, 65), (64, 64), (70, 100), (6, 300)]
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
    corners, stripe, lastcol, island = z(), z(), z(), full.copy()
    corners[0, 0] = corners[H - 1, W - 1] = True      # the two opposite corner pixels
    for x in (31, 32, 63, 64):                        # a column on either side of every word boundary the frame has, joined by one row
        if x < W:
            stripe[:, x] = True
    stripe[:, W // 2] = True
    stripe[H // 2, :] = True
    lastcol[:, W - 1] = True
    yy, xx = np.indices((H, W))
    checker = (yy + xx) % 2 == 0
    island[1:-1, 1:-1] = False                        # the frame ring ...
    island[2:-2, 2:-2] = True                         # ... plus an island in its hole
    diag = full.copy()
    diag[1, 1] = diag[2, 2] = False                   # a hole of two diagonal pixels: one ring through their shared point twice
    return {"full": full, "corners": corners, "stripe": stripe, "lastcol": lastcol, "checker": checker, "island": island, "diag": diag,
            "blob1": _blob(H, W, 1), "blob2": _blob(H, W, 2), "noise": np.random.RandomState(0).rand(H, W) < 0.5}


_CASES = {}


def cases(H, W):
    """[(name, mask, box, reference stream, boundary edges)] of a shape, computed once: every mask with its tight box and with the full
    frame, and one all-zero slot with box [0, 0, 0, 0]."""
    if (H, W) not in _CASES:
        out = []
        for name, m in _masks(H, W).items():
            ref, n = R.stream(R.trace(m)), R.edge_count(m)
            out.append((name, m, R.tight_box(m), ref, n))
            out.append((name + "/frame", m, [0, 0, W - 1, H - 1], ref, n))
        out.append(("empty", np.zeros((H, W), bool), [0, 0, 0, 0], [], 0))
        _CASES[(H, W)] = out
    return _CASES[(H, W)]


def run(H, W, slots, capacity, max_edges, sentinel=SENTINEL, Q=Q, count=COUNT):
    """One fx_mask_polygon_encode call on B = 2, Q = 3, det_count = [3, 1] unless given: ``slots`` = the (mask, box) of the detections, by
    default four for (0, 0), (0, 1), (0, 2), (1, 0); the other slots (1 and 2 of image 1) hold garbage words and boxes.  Returns (words,
    poly_len, poly_off, pool) as numpy arrays."""
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
    nb = lib.fx_mask_polygon_workspace_bytes(B, Q, H, W, max_edges)
    assert nb == (B * Q * H * W32 + B * Q + 7 * B * max_edges) * 4
    ws = torch.randint(0, 255, (nb,), dtype=torch.uint8, device=DEV)      # contents irrelevant
    rc = lib.fx_mask_polygon_encode(d_words.data_ptr(), d_count.data_ptr(), d_boxes.data_ptr(), B, Q, H, W, capacity, max_edges, ln.data_ptr(),
                                    off.data_ptr(), pool.data_ptr(), ws.data_ptr(), nb, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return words, ln.cpu().numpy(), off.cpu().numpy(), pool.cpu().numpy()


def check(H, W, chosen, capacity, max_edges, unstored, unfit=(), Q=Q, count=COUNT):
    """Runs the call on the cases (four by default) and checks everything the contract states; ``unstored`` = the exact set of (b, j) among
    the detections that must not be stored, ``unfit`` = those of them whose poly_len must be -1."""
    refs = [c[3] for c in chosen]
    words, ln, off, pool = run(H, W, [(c[1], c[2]) for c in chosen], capacity, max_edges, Q=Q, count=count)
    lengths, edges = np.full((B, Q), 99), np.full((B, Q), 9)      # of the garbage slots: ignored by the rule
    for (b, j), c in zip(_slots(count), chosen):
        lengths[b, j], edges[b, j] = len(c[3]), c[4]
    want_ln, want_off, want_st = R.capacity_rule(lengths.tolist(), edges.tolist(), count, capacity, max_edges)
    assert np.array_equal(ln, want_ln) and np.array_equal(off, want_off)      # true lengths, stored or not; 0 for the garbage slots
    assert {(b, j) for (b, j) in _slots(count) if not want_st[b, j] and lengths[b, j]} == set(unstored)
    assert {(b, j) for b in range(B) for j in range(Q) if ln[b, j] < 0} == set(unfit)
    untouched = np.ones_like(pool, bool)
    for (b, j), ref in zip(_slots(count), refs):
        if not want_st[b, j]:
            continue
        got = pool[b, off[b, j]:off[b, j] + ln[b, j]]
        assert got.tolist() == ref, (H, W, b, j)      # bit for bit
        rings = P.decode_stream(got)
        assert np.array_equal(P.polygons_to_mask(rings, H, W), R.unpack_words(words[b, j], W))      # the round trip gives the words back
        assert P.polygons_area(rings) == R.popcount_words(words[b, j])
        untouched[b, off[b, j]:off[b, j] + ln[b, j]] = False
    assert (pool[untouched] == SENTINEL).all()      # nothing is written outside the stored ranges
    return pool


@pytest.mark.parametrize("H,W", SHAPES)
def test_encode_is_bit_exact(H, W):
    cs = cases(H, W)
    assert len(cs) == 21
    cap = 3 * max(len(c[3]) for c in cs) + 5
    me = 3 * max(c[4] for c in cs)
    for i in range(0, len(cs), 4):
        check(H, W, (cs[i:i + 4] + cs[:4])[:4], cap, me, unstored=())


def test_capacity_rule_and_sentinel():
    H, W = 33, 65
    cs = {c[0]: c for c in cases(H, W)}
    blob, checker, corners, stripe = cs["blob1"], cs["checker"], cs["corners"], cs["stripe"]
    assert len(checker[3]) == 5 * ((H * W + 1) // 2) and checker[4] == 4 * ((H * W + 1) // 2)
    me = blob[4] + checker[4] + stripe[4]
    # the checkerboard in slot 1 of 3 with room for slot 0 only: slot 1 does not fit - and slot 2, whose offset lies behind slot 1's true
    # length, cannot either
    order = [blob, checker, stripe, corners]
    check(H, W, order, len(blob[3]), me, unstored={(0, 1), (0, 2)})
    # one word short of everything: exactly the last slot is not stored
    total = len(blob[3]) + len(checker[3]) + len(stripe[3])
    check(H, W, order, total - 1, me, unstored={(0, 2)})
    # exactly one word more stores everything
    check(H, W, order, total, me, unstored=())


def test_a_slot_over_max_edges_is_minus_one_and_shifts_nothing():
    H, W = 33, 65
    cs = {c[0]: c for c in cases(H, W)}
    blob, checker, corners, stripe = cs["blob1/frame"], cs["checker"], cs["corners"], cs["stripe/frame"]
    order = [blob, checker, stripe, corners]
    cap = len(blob[3]) + len(checker[3]) + len(stripe[3])
    me = blob[4] + checker[4] - 1      # slot 1 is one edge over the limit; slot 2 fits behind slot 0
    assert stripe[4] < checker[4]
    pool = check(H, W, order, cap, me, unstored={(0, 1)}, unfit={(0, 1)})
    assert pool[0, len(blob[3]):len(blob[3]) + len(stripe[3])].tolist() == stripe[3]      # slot 2 follows slot 0 directly
    # one edge more: slot 1 fits, and now slot 2 finds no room behind it
    check(H, W, order, cap, me + 1, unstored={(0, 2)}, unfit={(0, 2)})
    check(H, W, order, cap, me + 1 + stripe[4], unstored=())      # room for all three


def test_slot_offsets_over_260_slots():
    """poly_off of slot j sums j lengths: from slot 257 on the 256 threads of the emit kernel take a second length each, and all four
    wavefronts contribute.  The masks are the shape's cases, cyclically.  The edge workspace has room for 260 slots at the frame's limit of
    L = 2 H W + H + W = 82 edges, and the pool of 260 x 89 words is four times what these masks take together (the largest, the
    checkerboard, takes 90): everything is stored, which ``unstored=()`` asserts."""
    H, W, Qn = 5, 7, 260
    count = [Qn, 1]
    cs = cases(H, W)
    check(H, W, [cs[i % len(cs)] for i in range(sum(count))], Qn * 89, Qn * 82, unstored=(), Q=Qn, count=count)


def test_two_calls_give_byte_equal_pools():
    H, W = 70, 100
    cs = {c[0]: c for c in cases(H, W)}
    chosen = [cs[n] for n in ("blob1", "checker", "noise", "stripe")]
    slots = [(c[1], c[2]) for c in chosen]
    cap, me = sum(len(c[3]) for c in chosen), sum(c[4] for c in chosen)
    assert len(cs["checker"][3]) == 3500 + 14000
    a, b = run(H, W, slots, cap, me), run(H, W, slots, cap, me)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(a[3], run(H, W, slots, cap, me, sentinel=SENTINEL - 1)[3])      # the sentinel shows: the pool is not filled


def test_arguments_outside_the_contract_are_refused():
    lib = _lib.load()
    H, W, cap, me = 5, 7, 64, 128
    t = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)      # noqa: E731
    words, count, boxes, ln, off, pool = t(B, Q, H, 1), t(B), t(B, Q, 4), t(B, Q), t(B, Q), t(B, cap)
    nb = lib.fx_mask_polygon_workspace_bytes(B, Q, H, W, me)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    base = [words.data_ptr(), count.data_ptr(), boxes.data_ptr(), B, Q, H, W, cap, me, ln.data_ptr(), off.data_ptr(), pool.data_ptr(), ws.data_ptr(),
            nb, _stream()]
    assert lib.fx_mask_polygon_encode(*base) == 0
    for pos, val in ((0, None), (1, None), (2, None), (9, None), (10, None), (11, None), (12, None), (0, words.data_ptr() + 2), (3, 0), (4, 0),
                     (4, 65536), (5, 0), (6, 0), (7, 0), (8, 0), (13, nb - 1), (5, 32768), (6, 32768), (5, 32767)):
        args = list(base)
        args[pos] = val
        if (pos, val) == (5, 32767):
            args[6] = 32767      # Q (L + L / 4) = 3 * 2.68e9 >= 2^31
        assert lib.fx_mask_polygon_encode(*args) == INVALID, (pos, val)
    assert lib.fx_mask_polygon_workspace_bytes(B, Q, 32768, 8, me) == 0 and lib.fx_mask_polygon_workspace_bytes(0, Q, H, W, me) == 0
    assert lib.fx_mask_polygon_workspace_bytes(B, Q, H, W, 0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- end to end
def _get(name, seed):
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get(name, device=DEV, seed=seed)


_MODELS = {}
ROOMY = 4_000_000      # words and edges per image that hold every mask of the 192 x 256 test pictures: no fallback


@pytest.fixture(params=["fai-mf-l-coco-ins", "bisenetformer-l-ade"], ids=["threshold-branch", "all-pixels-branch"])
def fm(request):
    if request.param not in _MODELS:
        _MODELS[request.param] = _get(request.param, 3)
    return _MODELS[request.param]


@pytest.fixture
def roomy(fm):
    fm.processor.polygon_capacity = fm.processor.polygon_max_edges = ROOMY
    try:
        yield fm
    finally:
        fm.processor.polygon_capacity = fm.processor.polygon_max_edges = None


def _png_mask(b64):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(base64.b64decode(b64)))) > 0


def _plain(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label) for d in res.detections]


def _full(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask, d.rle, d.polygons, d.track_id) for d in res.detections]


def _batches(n, h=192, w=256):
    return [[synth_image_structured(500 + 10 * j + i, h, w) for i in range(2)] for j in range(n)]


def test_polygons_equal_the_default_path(roomy):
    fm = roomy
    h, w = 192, 256
    imgs = _batches(1)[0]
    png = fm.infer_batch(imgs, threshold=0.05)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # no fallback with the roomy pool
        pol = fm.infer_batch(imgs, threshold=0.05, mask_format="polygon")
    enc = fm.processor._polygon_encoder
    n = sum(len(r.detections) for r in png)
    print(f"{fm.model.family} {h} x {w}: {n} detections in 2 images, {enc.last_d2h_bytes} bytes copied back")
    assert n > 0 and len(png) == len(pol) == 2 and enc.last_fallback == 0 and enc.capacity == enc.max_edges == ROOMY
    words = 0
    for p, r in zip(png, pol):
        assert _plain(p) == _plain(r)
        for dp, dr in zip(p.detections, r.detections):
            assert dr.mask is None and dr.rle is None and dp.polygons is None and len(dr.polygons) > 0
            words += sum(1 + len(ring) // 2 for ring in dr.polygons)
            full = P.polygons_to_mask(dr.polygons, h, w)
            x0, y0, x1, y1 = dr.bbox
            want = _png_mask(dp.mask) if (x1 > x0 and y1 > y0) else np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), bool)
            assert np.array_equal(trim_mask(full, dr.bbox), want)
            outside = full.copy()
            outside[y0:y1 + 1, x0:x1 + 1] = False
            assert not outside.any() and full.any()
            assert full[y0].any() and full[y1].any() and full[:, x0].any() and full[:, x1].any()      # the box is the mask's extent
    # lengths, offsets and det_count, plus the used prefix of each image's pool: no mask word is copied
    assert enc.last_d2h_bytes == (2 * enc.B * enc.Q + enc.B) * 4 + words * 4
    one, one_png = fm.infer(imgs[0], threshold=0.05, mask_format="polygon"), fm.infer(imgs[0], threshold=0.05)
    assert len(one.detections) > 0 and _plain(one) == _plain(one_png)
    for dp, dr in zip(one_png.detections, one.detections):      # a batch of one is another plan: compared with its own PNG path
        x0, y0, x1, y1 = dr.bbox
        if x1 > x0 and y1 > y0:
            assert np.array_equal(trim_mask(P.polygons_to_mask(dr.polygons, h, w), dr.bbox), _png_mask(dp.mask))
    assert [d.polygons for d in fm(imgs[0], threshold=0.05, mask_format="polygon").detections] == [d.polygons for d in one.detections]


def test_stream_fallback_and_annotate(roomy):
    fm = roomy
    batches = _batches(3)
    want = [fm.infer_batch(b, threshold=0.05, mask_format="polygon") for b in batches]
    got = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="polygon"))
    assert sum(len(d.detections) for w_ in want for d in w_) > 0 and fm.processor._polygon_encoder.total_fallback == 0
    assert [[_full(d) for d in g] for g in got] == [[_full(d) for d in w_] for w_ in want]
    # a pool too small for any mask: the host fallback gives identical polygons, and warns
    fm.processor.polygon_capacity = 8
    with pytest.warns(RuntimeWarning, match="traced on the host"):
        small = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="polygon"))
    assert fm.processor._polygon_encoder.capacity == 8 and fm.processor._polygon_encoder.last_fallback > 0
    assert [[_full(d) for d in g] for g in small] == [[_full(d) for d in w_] for w_ in want]
    # the default pool and workspace: whatever falls back, the result is the same
    fm.processor.polygon_capacity = fm.processor.polygon_max_edges = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # masks of random weights are noise: some may overflow the defaults
        dflt = list(fm.infer_stream(iter(batches), threshold=0.05, mask_format="polygon"))
    print(f"{fm.model.family}: {fm.processor._polygon_encoder.last_fallback} slots of the last batch fell back at the default sizes")
    assert [[_full(d) for d in g] for g in dflt] == [[_full(d) for d in w_] for w_ in want]
    # annotate reads the packed device results, not FocoosDet.mask
    a_png = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a_pol = list(fm.infer_stream(iter(batches[:1]), threshold=0.05, annotate=True, mask_format="polygon"))[0]
    for img, p, r in zip(batches[0], a_png, a_pol):
        assert _plain(p) == _plain(r) and np.array_equal(p.image, r.image) and (p.image != img).any()
