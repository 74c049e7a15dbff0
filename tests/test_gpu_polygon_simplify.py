"""Device polygon simplification on a real MI355X (csrc/mask_polygon.hip): fx_mask_polygon_simplify word for word against
``ref_ring``, a recursive restatement of the definition in Python integers that shares nothing with ``simplify_ring`` (which must equal it
too), then ``polygon_tolerance=`` end to end.  Integers only: no tolerance anywhere.  The equal-ends branch (p_i == p_j) cannot be reached
from a ring with two distinct points: a vertex that coincides with an end of its chain has c = 0, a winner is kept only with c > 0, and
the anchors differ; ``test_revisited_point`` asserts what the reference did on its ring - no such chain - not the opposite."""
import sys
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import mask_polygon as P

from .test_gpu_mask_polygon import _batches, _blob, _full, _plain, fm, roomy  # noqa: F401  (the roomy recipe and its models)

pytestmark = pytest.mark.gpu
DEV, INVALID, SENTINEL = "cuda:0", -1, -777
B, Q, COUNT, SLOTS = 2, 3, [3, 1], [(0, 0), (0, 1), (0, 2), (1, 0)]
LDS_WORDS = 5120      # POLY_SIMP_LDS_WORDS: a longer stream runs on the workspace in global memory
_REF, _TRACED = {}, {}


def ref_ring(pts, T, equal_ends=None):
    """[(x, y)] of one ring, T sixteenths -> the kept vertices.  ``equal_ends`` collects the chains evaluated with p_i == p_j."""
    V, p, equal_ends = len(pts), list(pts) + [pts[0]], [] if equal_ends is None else equal_ends
    d2 = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2      # noqa: E731
    b = min(range(V), key=lambda k: (-d2(p[k], p[0]), k))
    keep = {0, b}

    def top(i, j):      # (c, k*, kept) of the chain (i, j)
        if j - i < 2:
            return None
        if p[i] == p[j]:
            equal_ends.append((i, j))
            c = [d2(p[k], p[i]) for k in range(i + 1, j)]
            return max(c), i + 1 + c.index(max(c)), 256 * max(c) > T * T
        c = [abs((p[j][0] - p[i][0]) * (p[k][1] - p[i][1]) - (p[j][1] - p[i][1]) * (p[k][0] - p[i][0])) for k in range(i + 1, j)]
        return max(c), i + 1 + c.index(max(c)), max(c) ** 2 > T * T * d2(p[i], p[j]) // 256

    def rec(i, j):
        t = top(i, j)
        if t and t[2]:
            keep.add(t[1])
            rec(i, t[1])
            rec(t[1], j)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 2 * V + 100))      # the staircase recurses nearly as deep as the ring is long
    rec(0, b)
    rec(b, V)
    sys.setrecursionlimit(limit)
    if len(keep) == 2:
        keep.add(min((t for t in (top(0, b), top(b, V)) if t), key=lambda t: (-t[0], t[1]))[1])
    return [pts[k] for k in sorted(keep)]


def ref_stream(rings, T):
    """the rings of a mask (flat) -> the simplified stream, with every invariant of the definition checked on the way; computed once"""
    out = _REF.setdefault((tuple(map(tuple, rings)), T), [])
    for ring in rings if not out else ():
        pts = list(zip(ring[0::2], ring[1::2]))
        got, it = ref_ring(pts, T), iter(pts)
        assert got[0] == pts[0] and len(got) >= 3 and all(q in it for q in got)      # p_0 first, V' >= 3, a subsequence
        assert P.simplify_ring(ring, T / 16) == [v for q in got for v in q]
        out += [len(got) - (P.ring_area2(ring) < 0) * 2 ** 31] + [x | y << 16 for x, y in got]      # the hole bit of the ORIGINAL ring
    return out


def stream_of(rings):
    return [w for r in rings for w in [len(r) // 2] + [x | y << 16 for x, y in zip(r[0::2], r[1::2])]]


def traced(H, W):
    if (H, W) not in _TRACED:
        yy, xx = np.mgrid[:H, :W]
        diag = np.ones((H, W), bool)
        diag[1, 1] = diag[2, 2] = False
        m = {"disc": (yy - H / 2 + 0.5) ** 2 + (xx - W / 2 + 0.5) ** 2 < (0.45 * min(H, W) + 0.5) ** 2, "blob": _blob(H, W, 1), "diag": diag,
             "checker": (yy + xx) % 2 == 0, "stairs": xx <= yy * W // H}
        _TRACED[(H, W)] = {k: P.trace_mask_numpy(v) for k, v in m.items()}
    return _TRACED[(H, W)]


def check(ring_lists, T, lengths=(None,) * 4, capacity=None):
    """One call on B = 2, Q = 3, det_count = [3, 1]: the rings of slots (0, 0), (0, 1), (0, 2), (1, 0) laid out as fx_mask_polygon_encode
    lays them out (``lengths`` overrides a poly_len, a small ``capacity`` leaves slots out), garbage in the other slots, random bytes in
    the workspace, a sentinel over the outputs.  Lengths, offsets and every stored word equal the reference; nothing else is written."""
    lib, streams = _lib.load(), [stream_of(r) for r in ring_lists]
    capacity = capacity or max(sum(len(s) for s in streams[:3]), len(streams[3]), 1) + 7
    ln, off = np.full((B, Q), 99, np.int32), np.full((B, Q), 12345, np.int32)
    pool = np.random.RandomState(T).randint(0, 2 ** 31 - 1, (B, capacity)).astype(np.int32)
    want = []
    for (b, j), s, rings, n in zip(SLOTS, streams, ring_lists, lengths):
        o = sum(len(t) for t in streams[:j]) if b == 0 else 0
        ln[b, j], off[b, j] = len(s) if n is None else n, o
        if o + len(s) <= capacity:
            pool[b, o:o + len(s)] = s
        want.append(ref_stream(rings, T) if n is None and o + len(s) <= capacity else None)
    dev = [torch.from_numpy(a).to(DEV) for a in (ln, off, pool, np.array(COUNT, np.int32))]
    outs = [torch.full(s, SENTINEL, dtype=torch.int32, device=DEV) for s in ((B, Q), (B, Q), (B, capacity))]
    nb = lib.fx_mask_polygon_simplify_workspace_bytes(B, Q, capacity)
    ws = torch.randint(0, 255, (nb,), dtype=torch.uint8, device=DEV)
    assert nb == 28 * B * capacity + 8 and lib.fx_mask_polygon_simplify(
        *[t.data_ptr() for t in dev], B, Q, capacity, T, *[t.data_ptr() for t in outs], ws.data_ptr(), nb,
        torch.cuda.current_stream(torch.device(DEV)).cuda_stream) == 0
    oln, ooff, opool = [t.cpu().numpy() for t in outs]
    untouched = np.ones_like(opool, bool)
    for (b, j), w, rings in zip(SLOTS, want, ring_lists):
        assert oln[b, j] == (-1 if w is None else len(w)) and ooff[b, j] == (sum(len(x or []) for x in want[:j]) if b == 0 else 0), (b, j)
        if w:
            assert opool[b, ooff[b, j]:ooff[b, j] + oln[b, j]].tolist() == w, (b, j)      # word for word
            got, holes = P.decode_simplified_stream(w)
            assert len(got) == len(rings) and holes == [P.is_hole(r) for r in rings]      # ring count and order, the original's hole bit
            untouched[b, ooff[b, j]:ooff[b, j] + oln[b, j]] = False
    assert (oln[1, 1:] == -1).all() and (ooff[1, 1:] == max(oln[1, 0], 0)).all()      # the slots beyond det_count
    assert (opool[untouched] == SENTINEL).all()      # nothing is written outside the stored ranges
    return oln, ooff, opool


@pytest.mark.parametrize("T", [8, 16, 40])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 65), (70, 100), (6, 300)])
def test_simplify_is_word_exact(H, W, T):
    t = traced(H, W)
    if (H, W) == (70, 100):      # the checkerboard runs in global memory, the blob's many rings in LDS
        assert len(t["checker"]) == 3500 and len(stream_of(t["checker"])) == 17500 > LDS_WORDS > len(stream_of(t["blob"])) and len(t["blob"]) > 100
    check([t["disc"], t["blob"], t["diag"], t["checker"]], T)
    check([t["stairs"], t["checker"], t["blob"], t["disc"]], T)


def test_deep_staircase_and_an_empty_slot():
    yy, xx = np.mgrid[:400, :400]
    rings = P.trace_mask_numpy(xx <= yy)
    assert [len(r) // 2 for r in rings] == [802]
    check([rings, [], rings, rings], 8)      # the empty slot between: out_len 0, nothing shifted


def test_unstored_slots_and_two_calls():
    t = traced(33, 65)
    rings = [t[k] for k in ("disc", "blob", "diag", "stairs")]
    check(rings, 16, lengths=[None, -1, None, None])      # a slot the encoder refused stays -1
    cap = len(stream_of(rings[0])) + len(stream_of(rings[1])) + 3      # slot (0, 2) does not fit the pool: not stored, -1
    for x, y in zip(check(rings, 16, capacity=cap), check(rings, 16, capacity=cap)):
        assert x.tobytes() == y.tobytes()      # two calls give byte-equal pools


def test_revisited_point():
    """A ring through (200, 100) twice with a loop of one pixel between the visits, at a tolerance of two pixels: the loop shrinks to its
    far corner, both visits go, and - see the module docstring - the reference meets no chain whose ends are one point."""
    ring = [(0, 0), (200, 0), (200, 100), (201, 100), (201, 101), (200, 101), (200, 100), (150, 100), (150, 300), (0, 300)]
    log = []
    assert ref_ring(ring, 32, log) == [(0, 0), (200, 0), (201, 101), (150, 100), (150, 300), (0, 300)] and log == []
    flat = [v for q in ring for v in q]
    check([[flat], [flat, flat], [flat], [flat]], 32)


def test_largest_magnitudes():
    """Vertices at 0 and 32767 on both axes and two vertices one unit off the long diagonal: c = 32767 against floor(T^2 2 M^2 / 256) decides
    between T = 11 and T = 12, and the corner (0, M) compares c^2 = M^4 with the right side at T = 1024, the largest either side gets."""
    M = 32767
    ring = [0, 0, 16384, 16383, M, M, 16383, 16384, 0, M]
    for T in (1, 11, 12, 1024):
        check([[ring], [ring, ring], [ring], [ring]], T)
    assert len(ref_stream([ring], 11)) == 6 and len(ref_stream([ring], 12)) == 5


def test_arguments_outside_the_contract_are_refused():
    lib, cap = _lib.load(), 64
    ins = [torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((B, Q), (B, Q), (B, cap))] + [torch.tensor(COUNT, dtype=torch.int32, device=DEV)]
    outs = [torch.full(s, SENTINEL, dtype=torch.int32, device=DEV) for s in ((B, Q), (B, Q), (B, cap))]
    nb = lib.fx_mask_polygon_simplify_workspace_bytes(B, Q, cap)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    base = [t.data_ptr() for t in ins] + [B, Q, cap, 16] + [t.data_ptr() for t in outs] + [ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream]
    for pos, val in ((0, None), (1, None), (2, None), (3, None), (8, None), (9, None), (10, None), (11, None), (2, ins[2].data_ptr() + 2),
                     (4, 0), (4, 65536), (5, 0), (5, 65536), (6, 0), (7, 0), (7, 1025), (7, -3), (12, nb - 1)):
        assert lib.fx_mask_polygon_simplify(*base[:pos], val, *base[pos + 1:]) == INVALID, (pos, val)
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in outs)      # nothing written
    assert lib.fx_mask_polygon_simplify_workspace_bytes(0, Q, cap) == 0 and lib.fx_mask_polygon_simplify_workspace_bytes(B, Q, 0) == 0
    assert lib.fx_mask_polygon_simplify(*base) == 0      # the same arguments unbroken: four empty slots, two beyond det_count
    assert outs[0].tolist() == [[0, 0, 0], [0, -1, -1]] and (outs[1] == 0).all() and (outs[2] == SENTINEL).all()


def _polys(res):
    return [[(d.polygons, d.polygon_holes) for d in r.detections] for r in res]


def test_tolerance_end_to_end(roomy):  # noqa: F811
    fm, imgs = roomy, _batches(1)[0]  # noqa: F811
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # no fallback with the roomy pool
        plain = fm.infer_batch(imgs, threshold=0.05, mask_format="polygon")
        simple = fm.infer_batch(imgs, threshold=0.05, mask_format="polygon", polygon_tolerance=1.0)
        copied = fm.processor._polygon_encoder.last_d2h_bytes
        again = fm.infer_batch(imgs, threshold=0.05, mask_format="polygon")
    assert sum(len(r.detections) for r in plain) > 0 and [_full(r) for r in again] == [_full(r) for r in plain]
    assert all(d.polygon_holes is None for r in plain for d in r.detections)      # None gives today's output
    want = [[P.simplify_rings(d.polygons, 1.0) for d in r.detections] for r in plain]
    assert _polys(simple) == want and [_plain(r) for r in simple] == [_plain(r) for r in plain]
    enc, words = fm.processor._polygon_encoder, sum(1 + len(ring) // 2 for img in want for rings, _ in img for ring in rings)
    assert copied == (2 * enc.B * enc.Q + enc.B) * 4 + words * 4      # only the simplified streams were copied
    assert _polys([fm.infer(imgs[0], threshold=0.05, mask_format="polygon", polygon_tolerance=1.0)])[0] == \
        [P.simplify_rings(d.polygons, 1.0) for d in fm.infer(imgs[0], threshold=0.05, mask_format="polygon").detections]
    fm.processor.polygon_tolerance = 1.0      # the processor's field is the default of the keyword
    try:
        assert _polys(list(fm.infer_stream(iter([imgs]), threshold=0.05, mask_format="polygon"))[0]) == want
        # room for the smaller of the two images' first streams: later slots are traced and simplified on the host, under the warning
        fm.processor.polygon_capacity = min(sum(1 + len(r) // 2 for r in p.detections[0].polygons) for p in plain)
        with pytest.warns(RuntimeWarning, match="traced on the host"):
            small = fm.infer_batch(imgs, threshold=0.05, mask_format="polygon")
        assert fm.processor._polygon_encoder.last_fallback > 0 and _polys(small) == want
    finally:
        fm.processor.polygon_tolerance = None
