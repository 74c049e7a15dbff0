"""The overlay on a real MI355X (csrc/overlay.hip through focoos_amd/annotate.py): the geometry pass, the trace ring
behind the real DeviceTracker, the two record kernels and the refusals of all five entry points against the restatement of
tests/overlay_ref.py, for equality; then infer_stream / infer_batch(annotate=Overlay(...)) with seeded synthetic weights against the
restatement drawn from a tracker, zones and traces stepped by hand.  Nothing here reads the reference tree."""
import math
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import annotate as AN
from focoos_amd.annotate import DeviceAnnotator, DeviceTraces, Overlay
from focoos_amd.synth import synth_image_structured
from focoos_amd.tracking import DeviceTracker, TrackerConfig
from focoos_amd.zones import DeviceZones, Line, Zone, build_tables

from . import annotate_ref as A
from . import overlay_ref as O
from . import zones_ref as Z
from .test_gpu_tracking import sequence

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
ALL = O.FILL | O.STROKE | O.TRACES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def overlay_call(lib, src, dst, B, H, W, b0, zon, tr, s, flags):
    """fx_annotate_overlay_u8 with the tables of a DeviceZones and a dict of trace tensors (either may be None)."""
    z = [None] * 6 + [0, 0] if zon is None else [zon._d_records.data_ptr(), zon._d_reg_first.data_ptr(), zon._d_verts.data_ptr(), zon.records.ctypes.data,
                                                 zon.reg_first.ctypes.data, zon.verts.ctypes.data, zon.R, int(zon.verts.shape[0])]
    t = [None] * 6 + [1, 1] if tr is None else [tr[k].data_ptr() for k in ("trk", "id", "label", "len", "head", "xy")] + [tr["xy"].shape[1], tr["xy"].shape[2]]
    streams = zon.streams if zon is not None else (tr["id"].shape[0] if tr is not None else b0 + B)
    return lib.fx_annotate_overlay_u8(src.data_ptr(), dst.data_ptr(), B, H, W, b0, streams, *z, *t, s, flags, _stream())


# ---------------------------------------------------------------- (a) the geometry pass
def scene(H, W):
    """Regions of 4 streams for an H x W frame, b0 = 1: stream 1 has the shared region only (1), stream 2 five, stream 3 thirty-two;
    polygons of 3, 4, 7 (concave) and 64 vertices, lines, vertices outside the frame on every side and one at the coordinate limit."""
    fx, fy = lambda v: int(round(v * W)), lambda v: int(round(v * H))      # noqa: E731
    concave7 = [(fx(-0.2), fy(0.1)), (fx(0.5), fy(-0.3)), (fx(1.2), fy(0.2)), (fx(0.6), fy(0.45)), (fx(1.1), fy(1.25)), (fx(0.3), fy(0.7)), (fx(-0.1), fy(1.1))]
    ring = [(fx(0.5) + int(round(0.42 * W * math.cos(2 * math.pi * i / 64))), fy(0.5) + int(round(0.42 * H * math.sin(2 * math.pi * i / 64)))) for i in range(64)]
    regs = [Zone("shared7", concave7),
            Zone("tri", [(-32768, 32768), (fx(0.7), fy(0.2)), (fx(0.9), fy(0.9))], stream=2),
            Line("line", (fx(-0.3), fy(0.8)), (fx(1.3), fy(0.1)), stream=2),
            Zone("ring", ring, stream=2),
            Zone("quad", [(fx(0.1), fy(0.1)), (fx(0.4), fy(0.1)), (fx(0.4), fy(0.6)), (fx(0.1), fy(0.6))], stream=2)]
    rs = np.random.RandomState(H * 1000 + W)
    for i in range(31):
        p = [(int(rs.randint(-W // 2, W + W // 2 + 1)), int(rs.randint(-H // 2, H + H // 2 + 1))) for _ in range(4)]
        if i % 3 == 2:
            regs.append(Line(f"l{i}", p[0], p[1] if p[1] != p[0] else (p[0][0] + 1, p[0][1]), stream=3))
        else:
            regs.append(Zone(f"z{i}", p[:3 + i % 2], stream=3))
    return regs


def fake_traces(S, M, L, H, W, seed):
    """A hand-made trace state: live and stale slots, rings of every fill level, heads anywhere, points inside and outside the frame."""
    rs = np.random.RandomState(seed)
    trk = rs.randint(0, 4, (S, M)).astype(np.int32) * rs.randint(1, 50, (S, M)).astype(np.int32)
    tid = np.where(rs.rand(S, M) < 0.7, trk, trk + 1).astype(np.int32)
    st = dict(trk=trk, id=tid, label=rs.randint(0, 7, (S, M)).astype(np.int32), len=rs.randint(0, L + 1, (S, M)).astype(np.int32),
              head=rs.randint(0, L, (S, M)).astype(np.int32))
    st["xy"] = np.stack([rs.randint(-W // 2, 2 * W + W // 2, (S, M, L)), rs.randint(-H // 2, 2 * H + H // 2, (S, M, L))], -1).astype(np.int32)
    st["xy"][:, 0, 1] = st["xy"][:, 0, 0]                      # a track that stood still: a segment of length 0
    st["len"][:, 0], st["head"][:, 0], st["id"][:, 0], st["trk"][:, 0] = 2, 2 % L, 5, 5
    return st


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("H,W", [(70, 301), (64, 512), (9, 5)])
def test_geometry_pass_equals_the_restatement(H, W, s):
    lib = _lib.load("bf16")
    S, b0, B, M, L = 4, 1, 3, 6, 5
    regions = scene(H, W)
    trk = DeviceTracker(S, TrackerConfig(max_tracks=M), DEV)
    zon = DeviceZones(S, regions, trk)
    assert np.diff(zon.reg_first).tolist() == [1, 1, 5, 32]
    st = fake_traces(S, M, L, H, W, 7)
    tr = {k: _dev(v) for k, v in st.items()}
    assert any(len(O.live_slots(st, st["trk"], b)) >= 2 for b in range(1, S))
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    drawn = 0
    for flags in (O.FILL, O.STROKE, O.TRACES, ALL):
        want = O.draw_geometry(frames, s, flags, b0, zon.per_stream, st, st["trk"])
        drawn += int((want != frames).any(-1).sum())
        d = _dev(frames)
        assert overlay_call(lib, d, d, B, H, W, b0, zon, tr, s, flags) == 0      # in place
        assert np.array_equal(d.cpu().numpy(), want), flags
        if flags in (O.STROKE, ALL):                                              # into a buffer between canary frames
            buf = torch.full((B + 2, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)
            src = _dev(frames)
            assert overlay_call(lib, src, buf[1:], B, H, W, b0, zon, tr, s, flags) == 0
            got = buf.cpu().numpy()
            assert np.array_equal(got[1:-1], want) and (got[0] == 0xA5).all() and (got[-1] == 0xA5).all() and np.array_equal(src.cpu().numpy(), frames)
    assert drawn > 0
    # the fill of the far-vertex triangle of stream 2 is the counter's inside predicate on every pixel centre
    tri = Z.region(regions[1])
    only = DeviceZones(S, [Zone("tri", regions[1].polygon)], trk)
    d = _dev(np.zeros((1, H, W, 3), np.uint8))
    assert overlay_call(lib, d, d, 1, H, W, 2, only, None, s, O.FILL) == 0
    tinted = d.cpu().numpy()[0].any(-1)
    assert np.array_equal(tinted, np.array([[Z.in_polygon((2 * x + 1, 2 * y + 1), tri["verts"]) for x in range(W)] for y in range(H)]))


def test_a_stream_without_regions_and_traces_keeps_its_bytes():
    lib = _lib.load("bf16")
    H, W, S, M, L = 70, 301, 3, 4, 3
    trk = DeviceTracker(S, TrackerConfig(max_tracks=M), DEV)
    zon = DeviceZones(S, [Zone("a", [(10, 10), (200, 20), (100, 60)], stream=1), Line("l", (0, 0), (300, 69), stream=0)], trk)
    assert np.diff(zon.reg_first).tolist() == [1, 1, 0]
    st = fake_traces(S, M, L, H, W, 9)
    st["id"][2] = st["trk"][2] + 1                               # stream 2: every trace is stale
    st["len"][1] = 1                                            # stream 1: live slots, but no ring holds a segment
    tr = {k: _dev(v) for k, v in st.items()}
    frames = np.random.RandomState(4).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    want = O.draw_geometry(frames, 2, ALL, 1, zon.per_stream, st, st["trk"])
    assert np.array_equal(want[1], frames[1]) and (want[0] != frames[0]).any()
    d = _dev(frames)
    assert overlay_call(lib, d, d, 2, H, W, 1, zon, tr, 2, ALL) == 0
    assert np.array_equal(d.cpu().numpy(), want)
    buf = torch.full((2, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)      # out of place the untouched stream is a copy
    assert overlay_call(lib, _dev(frames), buf, 2, H, W, 1, zon, tr, 2, ALL) == 0 and np.array_equal(buf.cpu().numpy(), want)
    assert overlay_call(lib, d, d, 2, H, W, 1, None, None, 2, 0) == 0 and np.array_equal(d.cpu().numpy(), want)      # no flag: nothing


# ---------------------------------------------------------------- (b) traces behind the real tracker
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,M,L", [(8, 4, 2), (64, 64, 8), (70, 130, 64)])
def test_traces_equal_the_restatement_after_every_frame(B, T, M, L):
    lib = _lib.load("bf16")
    trk = DeviceTracker(B, TrackerConfig(track_buffer=2, max_tracks=M), DEV)
    tr, ref = DeviceTraces(trk, L), O.RefTraces(B, M, L)
    if L > 12:              # 12 frames cannot fill a ring of 64: the heads start 3 before its end, so that every ring still turns over
        tr.head.fill_(L - 3)
        ref.head[:] = L - 3
    H, W = 288, 352
    frames = np.zeros((B, H, W, 3), np.uint8)
    for f, (s, l, bx, c) in enumerate(sequence(1000 * T + B, B, T)):
        dl, dbx, dc = _dev(l), _dev(bx), _dev(c)
        ids = trk.update(_dev(s), dl, dbx, dc)
        tr.update(dl, dbx, dc, ids)
        slots = trk.state()["id"]
        ref.update(l, bx, c, ids.cpu().numpy(), slots)                          # stepped on the tracker's own ids and slot table
        got, want = tr.state(), ref.state()
        for k in DeviceTraces.STATE:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (f, k)
        if f in (5, 11):
            d = _dev(frames)
            dt = dict(trk=trk.id, id=tr.id, label=tr.label, len=tr.len, head=tr.head, xy=tr.xy)
            assert overlay_call(lib, d, d, B, H, W, 0, None, dt, 1, O.TRACES) == 0
            img = O.draw_geometry(frames, 1, O.TRACES, 0, None, want, slots)
            assert img.any() and np.array_equal(d.cpu().numpy(), img), f
    print(f"B={B} T={T} M={M} L={L}: {ref.stats}")
    st = ref.stats
    assert st["turned"] > 0 and st["reused_slot"] > 0 and (L > 12 or st["wrapped"] > 0), st
    tr.reset(B - 1), ref.reset(B - 1)
    got, want = tr.state(), ref.state()
    assert all(np.array_equal(got[k], want[k]) for k in ("id", "label", "len", "head")) and (B == 1 or got["id"][0].any())
    tr.reset()
    assert not any(tr.state()[k].any() for k in ("id", "label", "len", "head"))


# ---------------------------------------------------------------- (c) the record kernels
NAMES = ["person", "a-very-long-class-name-of-30-ch", "x"]


def test_tracked_label_records_equal_the_restatement():
    B, T, H, W = 2, 8, 70, 301
    ann = DeviceAnnotator(NAMES, "detection", DEV)
    rs = np.random.RandomState(5)
    scores = np.array([0.0, 0.004, 0.0951, 0.5, 0.87, 0.995, 1.0, 0.31], np.float32)[None].repeat(B, 0)
    labels = rs.randint(-1, 4, (B, T)).astype(np.int32)
    labels[0, :3] = (0, 1, 1)
    boxes = rs.randint(-20, 320, (B, T, 4)).astype(np.int32)
    ids = np.array([[17, 2147483647, -1, 0, 9, 10, 99, 100], [-1, -5, 1000, 99999, 100000, 123456789, 1, 42]], np.int32)
    count = np.array([8, 6], np.int32)
    res = SimpleNamespaceResults(scores, labels, boxes, count)
    tab, ln = A.name_table(NAMES)
    for s in (1, 3):
        got = ann.records_tracked(res, _dev(ids), 0, B, H, W, s).cpu().numpy().view(A.REC).reshape(B, T)
        want = O.tracked_records(scores, labels, boxes, count, ids, tab, ln, len(NAMES), H, W, s, ann.gw, ann.gh)
        assert got.tobytes() == want.tobytes(), s
        # without an id the record is the one annotate=True has always made, byte for byte
        today = ann.records(res, 0, B, H, W, s).cpu().numpy().view(A.REC).reshape(B, T)
        none = ann.records_tracked(res, _dev(np.full((B, T), -1, np.int32)), 0, B, H, W, s).cpu().numpy().view(A.REC).reshape(B, T)
        assert none.tobytes() == today.tobytes() and got[0, 2].tobytes() == today[0, 2].tobytes()
    assert bytes(got[0, 1]["glyph"]) == bytes(A.glyphs_of("#2147483647 a-very-long-cl: 0%") + [0, 0]) and got[0, 1]["nchar"] == 30


class SimpleNamespaceResults:
    """The packed device results DeviceAnnotator reads."""

    def __init__(self, scores, labels, boxes, count):
        self.det_scores, self.det_labels, self.det_boxes, self.det_count = _dev(scores), _dev(labels), _dev(boxes), _dev(count)


def test_zone_records_equal_the_restatement_for_32_regions():
    S, H, W = 3, 70, 301
    regions = [Zone("shared-door", [(5, 60), (50, 60), (30, 69)])] + scene(H, W)[5:] + \
              [Line("a-name-of-more-than-16", (290, 3), (10, 40), stream=1), Zone("gate", [(-4, -4), (20, 5), (5, 20)], stream=1)]
    regions = [r if r.stream != 3 else (Zone(r.name, r.polygon, stream=2) if isinstance(r, Zone) else Line(r.name, r.start, r.end, stream=2)) for r in regions]
    trk = DeviceTracker(S, TrackerConfig(max_tracks=4), DEV)
    zon = DeviceZones(S, regions, trk)
    assert np.diff(zon.reg_first).tolist() == [1, 3, 32]
    R = zon.R
    rs = np.random.RandomState(6)
    counts = rs.randint(0, 2000, 3 * R).astype(np.int32)
    counts[[1, R + 1, 2 * R + 2]] = (999999, 1000000, 1024)
    counts[[2, R + 2]] = (-3, 2 ** 31 - 1)
    counts[R + 5:R + 9] = (9, 10, 99999, 100000)
    zon._io[:3 * R] = _dev(counts)
    ann = DeviceAnnotator(NAMES, "detection", DEV)
    for s in (1, 3):
        got = ann.zone_records(zon, H, W, s).cpu().numpy().view(A.REC).reshape(S, 32)
        want = O.zone_records(zon.per_stream, counts[:R], counts[R:2 * R], counts[2 * R:], H, W, s, ann.gw, ann.gh)
        assert got.tobytes() == want.tobytes(), s
    assert not got[0, 1:].view(np.uint8).any() and got[2, 31]["nchar"] > 0
    # drawn by fx_annotate_u8 with the labels flag alone, the streams' region counts as det_count
    atlas, gw, gh = AN.glyph_atlas()
    frames = np.random.RandomState(8).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    tab = ann._zone_tables(zon)
    d = _dev(frames)
    assert ann.lib.fx_annotate_u8(d.data_ptr(), d.data_ptr(), 2, H, W, 1, 32, tab["count"].data_ptr(), tab["zeros"].data_ptr(), tab["zeros"].data_ptr(), None,
                                  None, 0, 0, tab["rec"].data_ptr(), ann.atlas.data_ptr(), gw, gh, 3, A.LABELS, _stream()) == 0
    zero = np.zeros((S, 32, 4), np.int32)
    img = A.draw(frames, np.diff(zon.reg_first), zero[..., 0], zero, A.LABELS, 3, b0=1, rec=want, atlas=atlas, gw=gw, gh=gh)
    assert (img != frames).any() and np.array_equal(d.cpu().numpy(), img)


# ---------------------------------------------------------------- (d) refusals
def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, M, L, H, W, S = 2, 8, 4, 3, 20, 24, 2
    s, l, bx, c = sequence(3, B, T, 1)[0]
    regions = [Zone("z", [(2, 2), (20, 4), (9, 18)]), Line("mid", (0, 10), (24, 10), stream=1)]
    rec, first, verts, _ = build_tables(regions, S)
    Rt, Vt = int(first[-1]), int(verts.shape[0])
    keep = []

    def host(a):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data

    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)      # noqa: E731
    d_rec, d_first, d_verts = _dev(rec), _dev(first), _dev(np.concatenate([verts.reshape(-1), np.zeros(2, np.int32)]))
    dl, dbx, dc = _dev(l), _dev(np.concatenate([bx.reshape(-1), np.zeros(4, np.int32)])), _dev(c)
    ds = _dev(s)
    ids = _dev(np.arange(B * T, dtype=np.int32).reshape(B, T) % 5)
    trk = _dev(np.array([[1, 2, 3, 0], [4, 0, 2, 1]], np.int32))
    tables = dict(rec=d_rec.data_ptr(), first=d_first.data_ptr(), verts=d_verts.data_ptr(), hrec=host(rec), hfirst=host(first), hverts=host(verts), R=Rt, V=Vt)
    bad_tables = [dict(rec=None), dict(first=None), dict(verts=None), dict(hrec=None), dict(hfirst=None), dict(hverts=None), dict(verts=tables["verts"] + 4),
                  dict(R=0), dict(R=Rt + 1), dict(V=1), dict(V=Vt - 1), dict(hfirst=host(np.array([0, 3, 2], np.int32)))]
    frame_bad = [dict(H=0), dict(W=0), dict(H=16385), dict(s=0), dict(s=9)]

    def run(fn, order, base, bad, outs):
        """Every bad set is refused and writes nothing; then the unbroken call runs and stays inside its buffers (last element = canary)."""
        call = lambda **k: fn(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731
        for k in bad:
            assert call(**k) == INVALID, (fn.__name__, k)
        torch.cuda.synchronize()
        for name, t in outs.items():
            assert bool((t == t.flatten()[-1]).all()), (fn.__name__, name)
        assert call() == 0, fn.__name__
        torch.cuda.synchronize()
        for name, t in outs.items():
            assert int(t.flatten()[-1]) in (-7, 0xA5), (fn.__name__, name)
            assert bool((t.flatten()[:-1] != t.flatten()[-1]).any()), (fn.__name__, name)

    # fx_annotate_labels_tracked
    names, name_len = _dev(A.name_table(NAMES)[0]), _dev(A.name_table(NAMES)[1])
    out = torch.full((B * T * 56 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    order = ["s", "l", "bx", "c", "ids", "B", "T", "names", "name_len", "K", "H", "W", "s_", "gw", "gh", "out"]
    base = dict(s=ds.data_ptr(), l=dl.data_ptr(), bx=dbx.data_ptr(), c=dc.data_ptr(), ids=ids.data_ptr(), B=B, T=T, names=names.data_ptr(),
                name_len=name_len.data_ptr(), K=3, H=H, W=W, s_=1, gw=7, gh=11, out=out.data_ptr())
    bad = [{p: None} for p in ("s", "l", "bx", "c", "ids", "names", "name_len", "out")] + [dict(ids=base["ids"] + 2), dict(out=base["out"] + 1), dict(B=0),
           dict(T=0), dict(K=-1), dict(gw=0), dict(gh=33)] + [{("s_" if k == "s" else k): v for k, v in d.items()} for d in frame_bad]
    run(lib.fx_annotate_labels_tracked, order, base, bad, dict(rec=out))

    # fx_annotate_zone_records
    rnames, rlen = _dev(AN.region_name_table(["z", "z", "mid"])[0]), _dev(AN.region_name_table(["z", "z", "mid"])[1])
    cnt = _dev(np.arange(3 * Rt, dtype=np.int32))
    out = torch.full((S * 32 * 56 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    order = ["rec", "first", "verts", "hrec", "hfirst", "hverts", "R", "V", "names", "name_len", "in", "out_t", "now", "B", "H", "W", "s", "gw", "gh", "out"]
    base = dict(tables, names=rnames.data_ptr(), name_len=rlen.data_ptr(), **{"in": cnt.data_ptr()}, out_t=cnt.data_ptr() + 4 * Rt, now=cnt.data_ptr() + 8 * Rt,
                B=S, H=H, W=W, s=1, gw=7, gh=11, out=out.data_ptr())
    bad = bad_tables + [{p: None} for p in ("names", "name_len", "in", "out_t", "now", "out")] + [dict(B=0), dict(B=1), dict(B=65536), dict(now=base["now"] + 2),
                                                                                              dict(gw=33)] + frame_bad
    run(lib.fx_annotate_zone_records, order, base, bad, dict(rec=out))

    # fx_annotate_overlay_u8
    st = {k: _dev(v) for k, v in fake_traces(S, M, L, H, W, 2).items()}
    src = _dev(np.random.RandomState(1).randint(0, 250, (B, H, W, 3)).astype(np.uint8))
    out = torch.full((B * H * W * 3 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    order = ["src", "dst", "B", "H", "W", "b0", "S", "rec", "first", "verts", "hrec", "hfirst", "hverts", "R", "V", "trk", "tid", "tlabel", "tlen", "thead", "txy",
             "M", "L", "s", "flags"]
    base = dict(tables, src=src.data_ptr(), dst=out.data_ptr(), B=B, H=H, W=W, b0=0, S=S, trk=st["trk"].data_ptr(), tid=st["id"].data_ptr(),
                tlabel=st["label"].data_ptr(), tlen=st["len"].data_ptr(), thead=st["head"].data_ptr(), txy=st["xy"].data_ptr(), M=M, L=L, s=1, flags=ALL)
    bad = bad_tables + [{p: None} for p in ("src", "dst", "trk", "tid", "tlabel", "tlen", "thead", "txy")] + frame_bad + [
        dict(B=0), dict(b0=-1), dict(b0=1), dict(S=1), dict(S=0), dict(S=65536), dict(M=0), dict(M=1025), dict(L=0), dict(L=65), dict(flags=8), dict(flags=-1),
        dict(txy=base["txy"] + 4), dict(tlen=base["tlen"] + 2), dict(dst=base["src"] + 3), dict(dst=base["src"] + B * H * W * 3 - 1)]
    run(lib.fx_annotate_overlay_u8, order, base, bad, dict(dst=out))

    # fx_trace_update / fx_trace_reset
    state = dict(tid=i32(B * M + 1), tlabel=i32(B * M + 1), tlen=i32(B * M + 1), thead=i32(B * M + 1), txy=i32(B * M * L * 2 + 2))
    rorder = ["tid", "tlabel", "tlen", "thead", "B", "M", "b"]
    rbase = dict({k: v.data_ptr() for k, v in state.items()}, B=B, M=M, b=-1)
    rbad = [{p: None} for p in rorder[:4]] + [dict(b=B), dict(b=-2), dict(B=0), dict(M=0), dict(M=1025), dict(tid=rbase["tid"] + 2)]
    run(lib.fx_trace_reset, rorder, rbase, rbad, {k: state[k] for k in rorder[:4]})
    order = ["l", "bx", "c", "B", "T", "ids", "trk", "M", "L", "tid", "tlabel", "tlen", "thead", "txy"]
    base = dict(rbase, l=dl.data_ptr(), bx=dbx.data_ptr(), c=dc.data_ptr(), T=T, ids=ids.data_ptr(), trk=trk.data_ptr(), L=L)
    bad = [{p: None} for p in order if p not in ("B", "T", "M", "L")] + [dict(bx=base["bx"] + 8), dict(txy=base["txy"] + 4), dict(ids=base["ids"] + 1), dict(B=0),
                                                                        dict(B=65536), dict(T=0), dict(T=1025), dict(M=0), dict(M=1025), dict(L=0), dict(L=65)]
    before = {k: v.clone() for k, v in state.items()}
    call = lambda **k: lib.fx_trace_update(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731
    for k in bad:
        assert call(**k) == INVALID, k
    torch.cuda.synchronize()
    assert all(torch.equal(state[k], before[k]) for k in state)
    assert call() == 0
    torch.cuda.synchronize()
    ref = O.RefTraces(B, M, L)
    ref.update(l, bx, c, ids.cpu().numpy(), trk.cpu().numpy())
    for k, name in (("tid", "id"), ("tlabel", "label"), ("tlen", "len"), ("thead", "head")):
        assert int(state[k][-1]) == -7 and np.array_equal(state[k][:-1].cpu().numpy().reshape(B, M), getattr(ref, name)), k
    assert (state["txy"][-2:] == -7).all() and ref.stats["appended"] > 0
    xy = state["txy"][:-2].cpu().numpy().reshape(B, M, L, 2)
    assert all(np.array_equal(xy[b, t, 0], ref.xy[b, t, 0]) for b in range(B) for t in range(M) if ref.len[b, t])


# ---------------------------------------------------------------- (e) the public interface
SIZE = 128
LOW = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)
PUBLIC = [Zone("door", [(32, 16), (112, 40), (96, 120), (16, 88)], anchor="bottom_center"), Line("gate", (0, 64), (128, 64), anchor="center")]


@pytest.fixture(scope="module")
def detr():
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        fm = ModelManager.get("fai-detr-m-coco", device=DEV, seed=3)
    fm.processor.image_size = SIZE
    return fm


def _dets(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask, d.track_id) for d in res.detections]


def _packed(batch, T=300):
    B = len(batch)
    s, l, bx = np.zeros((B, T), np.float32), np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
    c = np.array([len(r.detections) for r in batch], np.int32)
    for b, r in enumerate(batch):
        for j, d in enumerate(r.detections):
            s[b, j], l[b, j], bx[b, j] = d.conf, d.cls_id, d.bbox
    return s, l, bx, c


def test_infer_stream_and_infer_batch_draw_like_state_stepped_by_hand(detr):
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) if j % 3 else synth_image_structured(40 + b + 10 * j, SIZE, SIZE) for b in range(2)]
               for j in range(6)]
    classes = detr.model_info.classes
    atlas, gw, gh = AN.glyph_atlas()
    tab, ln = A.name_table(classes)
    s1 = AN.scale_for(SIZE, SIZE)
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    counted = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC))
    # by hand: tracker, zones, traces on the plain run's packed results, then the restatement's picture
    trk = DeviceTracker(2, LOW, DEV)
    zref, tref, want = Z.RefZones(2, PUBLIC, LOW.max_tracks), O.RefTraces(2, LOW.max_tracks, 4), []
    for batch, imgs in zip(plain, batches):
        s, l, bx, c = _packed(batch)
        ids = trk.update(_dev(s), _dev(l), _dev(bx), _dev(c)).cpu().numpy()
        slots = trk.state()["id"]
        now = zref.update(l, bx, c, ids, slots)["now"]
        tref.update(l, bx, c, ids, slots)
        img = O.draw_geometry(np.stack(imgs), s1, ALL, 0, zref.per_stream, tref.state(), slots)
        rec = O.tracked_records(s, l, bx, c, ids, tab, ln, len(classes), SIZE, SIZE, s1, gw, gh)
        img = A.draw(img, c, l, bx, A.BOXES | A.LABELS, s1, rec=rec, atlas=atlas, gw=gw, gh=gh)
        zrec = O.zone_records(zref.per_stream, zref.in_total, zref.out_total, now, SIZE, SIZE, s1, gw, gh)
        zero = np.zeros((2, 32, 4), np.int32)
        want.append(A.draw(img, np.diff(zref.reg_first), zero[..., 0], zero, A.LABELS, s1, rec=zrec, atlas=atlas, gw=gw, gh=gh))
    print(f"{sum(len(r.detections) for b in plain for r in b)} detections in 12 frames, traces {tref.stats}, in {zref.in_total.tolist()} out {zref.out_total.tolist()}")
    assert tref.stats["appended"] > 0 and any((w != np.stack(i)).any() for w, i in zip(want, batches))
    got = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, annotate=Overlay(traces=4)))
    for f, (batch, w) in enumerate(zip(got, want)):
        for b, r in enumerate(batch):
            assert r.image.dtype == np.uint8 and np.array_equal(r.image, w[b]), (f, b)
    # the detections, ids and zone dicts are those of annotate=False
    assert [[_dets(r) for r in b] for b in got] == [[_dets(r) for r in b] for b in counted]
    assert [[r.zones for r in b] for b in got] == [[r.zones for r in b] for b in counted]
    # infer_batch, one call per batch, with state objects of its own
    trk2 = DeviceTracker(2, LOW, DEV)
    dz, dt = DeviceZones(2, PUBLIC, trk2), DeviceTraces(trk2, 4)
    one = [detr.infer_batch(b, threshold=0.05, tracker=trk2, zones=dz, annotate=Overlay(traces=dt)) for b in batches]
    assert all(np.array_equal(r.image, w[b]) for batch, w in zip(one, want) for b, r in enumerate(batch))
    assert [[_dets(r) for r in b] for b in one] == [[_dets(r) for r in b] for b in counted]
    assert all(np.array_equal(dt.state()[k], tref.state()[k]) for k in DeviceTraces.STATE)
    # annotate=True beside the same tracker and zones draws what it draws without them
    drawn = list(detr.infer_stream(iter(batches), threshold=0.05, annotate=True))
    both = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, annotate=True))
    assert all(np.array_equal(p.image, q.image) for bp, bq in zip(drawn, both) for p, q in zip(bp, bq))
    assert any((r.image != img).any() for batch, imgs in zip(drawn, batches) for r, img in zip(batch, imgs))
    assert [[_dets(r) for r in b] for b in both] == [[_dets(r) for r in b] for b in counted]
    assert [[r.zones for r in b] for b in both] == [[r.zones for r in b] for b in counted]
    trk2.reset(), dz.reset()
    same = [detr.infer_batch(b, threshold=0.05, tracker=trk2, zones=dz, annotate=True) for b in batches]
    assert all(np.array_equal(p.image, q.image) for bp, bq in zip(drawn, same) for p, q in zip(bp, bq))
