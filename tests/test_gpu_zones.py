"""Zone and line counting on a real MI355X (csrc/zone_ops.hip through focoos_amd/zones.py): fx_zone_update against the restatement of
tests/zones_ref.py after every frame of seeded moving boxes that first go through the real DeviceTracker (every output and every state
array, for equality), occupancy without ids, fx_zone_reset, the refusals, and infer_stream(zones=...) / infer_batch(zones=...) with seeded
synthetic weights against a DeviceZones stepped by hand over the same packed results.  Nothing here reads the reference tree."""
import math
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.synth import synth_image_structured
from focoos_amd.tracking import DeviceTracker, TrackerConfig
from focoos_amd.zones import ANCHORS, KEYS, DeviceZones, Line, Zone, build_tables

from . import zones_ref as R
from .test_gpu_tracking import sequence

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
SHAPES = [(8, 4), (64, 64), (70, 130)]      # (T, max_tracks): one wave partly filled; exactly one wave; two waves and more than 64 slots
# The seed of a configuration's sequence is 1000 T + B unless that sequence misses one of the events the test asks for (checked with the
# two restatements on the host): four tracks and one zone need a sequence with an exit and an anchor on an edge.
SEEDS = {(1, 8): 8006}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ---------------------------------------------------------------- the regions
# The boxes of test_gpu_tracking.sequence live on a grid of 16 inside about 256 x 256 and move by even steps, so vertices on multiples of
# 8 put anchors exactly on edges and vertices.
HEPTAGON = [(64, 48), (128, 32), (208, 64), (224, 144), (160, 208), (96, 192), (48, 128)]
RING64 = [(128 + int(round(90 * math.cos(2 * math.pi * i / 64))), 128 + int(round(90 * math.sin(2 * math.pi * i / 64)))) for i in range(64)]


def five(stream):
    """The shared heptagon plus four regions of ``stream``: a class-filtered triangle, a line, the 64-gon and a class-filtered line."""
    return [Zone("hept", HEPTAGON, anchor="center"),
            Zone("tri", [(0, 0), (256, 0), (0, 256)], stream=stream, classes=[1]),
            Line("mid", (128, 0), (128, 256), stream=stream, anchor="center"),
            Zone("ring", RING64, stream=stream, anchor="top_left"),
            Line("row", (0, 128), (256, 128), stream=stream, classes=[0], anchor="bottom_right")]


def many(stream, n, seed):
    """``n`` seeded regions of ``stream``: rectangles, triangles and lines on the grid of 8, every anchor, every class filter."""
    rs, out = np.random.RandomState(seed), []
    for i in range(n):
        kw = dict(stream=stream, anchor=ANCHORS[rs.randint(9)], classes=[None, [0], [1], [0, 1, 200]][rs.randint(4)])
        x0, y0 = (rs.randint(0, 20, 2) * 8).tolist()
        w, h = (rs.randint(4, 16, 2) * 8).tolist()
        if i % 3 == 0:
            out.append(Zone(f"rect{i}", [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)], **kw))
        elif i % 3 == 1:
            out.append(Zone(f"tri{i}", [(x0, y0), (x0 + w, y0 + h), (x0, y0 + h)], **kw))
        else:
            out.append(Line(f"line{i}", (x0, y0), (x0 + w, y0 + h), **kw))
    return out


def regions_for(B, T):
    """1, 5 and 32 regions per stream (the limit); polygons of 3, 7 and 64 vertices; both kinds; shared and stream-specific.  B = 3 has
    all three counts at once (stream 0: the shared one only), B = 1 one of them per shape."""
    if B == 3:
        return five(1) + many(2, 31, 11)
    return {8: [Zone("hept", HEPTAGON, anchor="center")], 64: five(0), 70: [Zone("hept", HEPTAGON, anchor="center")] + many(0, 31, 12)}[T]


def _same(got, want, where):
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape, (where, k)
        assert np.array_equal(g.astype(np.int64) & 0xFFFFFFFF, w.astype(np.int64) & 0xFFFFFFFF), (where, k, g.tolist(), w.tolist())


def _host(out):
    return {k: out[k].cpu().numpy() for k in ("now", "det_inside", "det_in", "det_out")}


def expected_stats(regions):
    """What a sequence must have exercised, given what its regions can produce."""
    need = ["zone_in", "zone_out", "reused_slot", "on_edge", "untracked_inside"]
    if any(isinstance(r, Line) for r in regions):
        need += ["line_in", "line_out"]
    if any(r.classes is not None for r in regions):
        need += ["class_filtered"]
    return need


# ---------------------------------------------------------------- (a) equality with the restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,M", SHAPES)
def test_update_equals_the_restatement_after_every_frame(B, T, M):
    cfg = TrackerConfig(track_buffer=2, max_tracks=M)
    regions = regions_for(B, T)
    trk = DeviceTracker(B, cfg, DEV)
    zon, ref = DeviceZones(B, regions, trk), R.RefZones(B, regions, M)
    assert zon.reg_first.tolist() == ref.reg_first.tolist()
    per = np.diff(zon.reg_first).tolist()
    assert per == ([1, 5, 32] if B == 3 else [{8: 1, 64: 5, 70: 32}[T]])
    for f, (s, l, bx, c) in enumerate(sequence(SEEDS.get((B, T), 1000 * T + B), B, T)):
        dl, dbx, dc = _dev(l), _dev(bx), _dev(c)
        ids = trk.update(_dev(s), dl, dbx, dc)
        got = _host(zon.update(dl, dbx, dc, ids))
        want = ref.update(l, bx, c, ids.cpu().numpy(), trk.state()["id"])      # stepped on the tracker's own ids and slot table
        _same(got, want, f)
        _same(zon.state(), ref.state(), f)
        if f == 3:
            assert c[B - 1] == 0 and not got["det_inside"][B - 1].any()      # the ragged counts include 0
    print(f"B={B} T={T} M={M} regions per stream {per}: {ref.stats}, events in {int(ref.in_total.sum())} out {int(ref.out_total.sum())}")
    for k in expected_stats(regions):
        assert ref.stats[k] > 0, (k, ref.stats)
    # fetch() says the same thing in the public form
    pub, st = zon.fetch(), ref.state()
    for b in range(B):
        assert list(pub[b]) == [r.name for r in zon.per_stream[b]]
        for k, reg in enumerate(zon.per_stream[b]):
            r, d = int(ref.reg_first[b]) + k, pub[b][reg.name]
            assert tuple(d) == KEYS and d["kind"] == reg.kind
            assert (d["count"], d["entered"], d["exited"]) == (int(want["now"][r]), int(st["in_total"][r]), int(st["out_total"][r]))
            for key, m in (("detections", "det_inside"), ("crossed_in", "det_in"), ("crossed_out", "det_out")):
                assert d[key] == np.nonzero((want[m][b] >> np.uint32(k)) & np.uint32(1))[0].tolist(), (b, reg.name, key)
            if reg.kind == "line":
                assert d["count"] == 0 and d["detections"] == []


# ---------------------------------------------------------------- (b) occupancy without ids, reset
def _run(B, T, M, frames, regions):
    cfg = TrackerConfig(track_buffer=2, max_tracks=M)
    trk = DeviceTracker(B, cfg, DEV)
    zon, ref = DeviceZones(B, regions, trk), R.RefZones(B, regions, M)
    seq = sequence(77, B, T, frames)

    def step(fr, with_ids=True):
        s, l, bx, c = fr
        dl, dbx, dc = _dev(l), _dev(bx), _dev(c)
        ids = trk.update(_dev(s), dl, dbx, dc)
        if with_ids:
            return _host(zon.update(dl, dbx, dc, ids)), ref.update(l, bx, c, ids.cpu().numpy(), trk.state()["id"])
        return _host(zon.update(dl, dbx, dc)), ref.update(l, bx, c)

    return trk, zon, ref, seq, step


def test_without_ids_only_the_occupancy_is_counted_and_the_state_stays():
    trk, zon, ref, seq, step = _run(3, 64, 64, 6, five(1))
    for fr in seq[:4]:
        _same(*step(fr), "warm")
    before = zon.state()
    assert before["st_id"].any() and before["in_total"].any()
    got, want = step(seq[4], with_ids=False)
    _same(got, want, "no ids")
    assert got["now"].any() and not got["det_in"].any() and not got["det_out"].any()
    _same(zon.state(), before, "no ids: state")
    # a DeviceZones without a tracker counts the same occupancy and refuses ids
    plain = DeviceZones(3, [r for r in five(1) if isinstance(r, Zone)], device=DEV)
    s, l, bx, c = seq[5]
    occ = _host(plain.update(_dev(l), _dev(bx), _dev(c)))
    _same(occ, R.RefZones(3, plain.regions).update(l, bx, c), "trackerless")
    with pytest.raises(ValueError, match="tracker"):
        plain.update(_dev(l), _dev(bx), _dev(c), torch.zeros(3, 64, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="batch"):
        plain.update(_dev(l[:2]), _dev(bx[:2]), _dev(c[:2]))
    with pytest.raises(ValueError, match="det_boxes"):
        plain.update(_dev(l), _dev(bx.astype(np.int64)), _dev(c))


def test_reset_clears_one_streams_regions_and_keeps_the_counters_on_request():
    trk, zon, ref, seq, step = _run(3, 64, 64, 10, five(1))
    for fr in seq[:5]:
        _same(*step(fr), "warm")
    lo, hi = int(ref.reg_first[1]), int(ref.reg_first[2])
    assert ref.st_id[lo:hi].any() and ref.in_total[lo:hi].any() and ref.st_id[:lo].any()
    zon.reset(1), ref.reset(1)
    _same(zon.state(), ref.state(), "reset(1)")
    st = zon.state()
    assert not st["st_id"][lo:hi].any() and not st["in_total"][lo:hi].any() and st["st_id"][:lo].any()
    for f, fr in enumerate(seq[5:8]):                 # stream 1 learns its sides again (no event in its first frame), the others go on
        got, want = step(fr)
        _same(got, want, f)
        _same(zon.state(), ref.state(), f)
        assert f > 0 or not got["det_in"][1].any()
    totals = ref.in_total.copy()
    assert totals.any()
    zon.reset(None, counters=False), ref.reset(None, counters=False)
    _same(zon.state(), ref.state(), "reset(None, counters=False)")
    st = zon.state()
    assert not st["st_id"].any() and not st["st_side"].any() and np.array_equal(st["in_total"], totals)
    for f, fr in enumerate(seq[8:]):
        _same(*step(fr), f)
        _same(zon.state(), ref.state(), f)
    zon.reset(), ref.reset()
    _same(zon.state(), ref.state(), "reset()")
    assert not zon.state()["in_total"].any() and not zon.state()["out_total"].any()
    with pytest.raises(ValueError):
        zon.reset(3)


# ---------------------------------------------------------------- (c) refusals
def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, M = 2, 8, 4
    s, l, bx, c = sequence(3, B, T, 1)[0]
    regions = [Zone("hept", HEPTAGON, anchor="center"), Line("mid", (128, 0), (128, 256), stream=1), Zone("tri", [(0, 0), (256, 0), (0, 256)], stream=0)]
    rec, first, verts, _ = build_tables(regions, B)
    Rt, Vt = int(first[-1]), int(verts.shape[0])
    assert (Rt, Vt) == (4, 12)
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)      # noqa: E731
    out = dict(st_id=i32(Rt + 1, M), st_side=i32(Rt + 1, M), in_total=i32(Rt + 1), out_total=i32(Rt + 1), now=i32(Rt + 1), det_inside=i32(B * T + 1),
               det_in=i32(B * T + 1), det_out=i32(B * T + 1))                       # one canary row / element past the end of each
    dl, dbx, dc = _dev(l), _dev(np.concatenate([bx.reshape(-1), np.zeros(4, np.int32)])), _dev(c)
    ids, trk = torch.full((B, T), -1, dtype=torch.int32, device=DEV), torch.zeros(B, M, dtype=torch.int32, device=DEV)
    d_rec, d_first, d_verts = _dev(rec), _dev(first), _dev(np.concatenate([verts.reshape(-1), np.zeros(2, np.int32)]))
    keep = []

    def host(a):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data

    base = dict(l=dl.data_ptr(), bx=dbx.data_ptr(), c=dc.data_ptr(), B=B, T=T, ids=ids.data_ptr(), trk=trk.data_ptr(), M=M, rec=d_rec.data_ptr(),
                first=d_first.data_ptr(), verts=d_verts.data_ptr(), hrec=host(rec), hfirst=host(first), hverts=host(verts), R=Rt, V=Vt,
                **{k: v.data_ptr() for k, v in out.items()})
    order = ["l", "bx", "c", "B", "T", "ids", "trk", "M", "rec", "first", "verts", "hrec", "hfirst", "hverts", "R", "V", "st_id", "st_side", "in_total",
             "out_total", "now", "det_inside", "det_in", "det_out"]
    call = lambda **k: lib.fx_zone_update(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731

    def table(row, col, value):
        t = rec.copy()
        t[row, col] = value
        return dict(hrec=host(t))

    def vert(i, xy):
        v = verts.copy()
        v[i] = xy
        return dict(hverts=host(v))

    bad = [{p: None} for p in order if p not in ("B", "T", "M", "R", "V", "ids", "trk")]
    bad += [dict(trk=None), dict(bx=base["bx"] + 4), dict(bx=base["bx"] + 8), dict(verts=base["verts"] + 4), dict(l=base["l"] + 2), dict(now=base["now"] + 1),
            dict(B=0), dict(B=65536), dict(B=1), dict(T=0), dict(T=1025), dict(M=0), dict(M=1025), dict(R=0), dict(R=Rt - 1), dict(R=Rt + 1),
            dict(V=1), dict(V=Vt - 1),
            table(0, 0, 2), table(0, 0, -1), table(0, 1, 9), table(0, 1, -1), table(0, 2, 2), table(0, 4, 2), table(0, 4, 65), table(3, 4, 3), table(3, 4, 1),
            table(0, 3, -1), table(1, 3, Vt - 2), vert(0, (32769, 0)), vert(1, (0, -32769)), vert(8, verts[7]),
            dict(hfirst=host(np.array([0, 3, 2], np.int32))), dict(hfirst=host(np.array([1, 2, 4], np.int32))), dict(hfirst=host(np.array([0, 2, 3], np.int32)))]
    # 33 regions on one stream: a table of its own, every other argument sized for it
    big_rec = np.repeat(rec[:1], 34, 0)
    bad.append(dict(hrec=host(big_rec), hfirst=host(np.array([0, 33, 34], np.int32)), R=34))
    for k in bad:
        assert call(**k) == INVALID, k
    rorder = ["st_id", "st_side", "in_total", "out_total", "hfirst", "B", "M", "b", "clear"]
    rcall = lambda **k: lib.fx_zone_reset(*[dict(dict(base, b=0, clear=1), **k)[n] for n in rorder], _stream())      # noqa: E731
    rbad = [{p: None} for p in rorder[:5]] + [dict(b=B), dict(b=-2), dict(B=0), dict(M=0), dict(M=1025), dict(st_id=base["st_id"] + 2),
                                              dict(hfirst=host(np.array([0, 3, 2], np.int32))), dict(hfirst=host(np.array([0, 33, 34], np.int32)))]
    for k in rbad:
        assert rcall(**k) == INVALID, k
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())
    # the same arguments unbroken run: reset, then one update; the canaries past the end stay
    assert rcall(b=-1) == 0 and call() == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v[-1] == -7).all()), k
        assert not bool((v[:-1] == -7).any()), k                     # every element was written
    want = R.RefZones(B, regions, M).update(l, bx, c, ids.cpu().numpy(), trk.cpu().numpy())
    _same({k: out[k][:-1].cpu().numpy().reshape(want[k].shape) for k in want}, want, "unbroken")
    assert rcall(b=1, clear=0) == 0 and rcall(b=0) == 0


# ---------------------------------------------------------------- (d) the public interface
SIZE = 128
LOW = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)
PUBLIC = [Zone("left", [(0, 0), (64, 0), (64, 128), (0, 128)], anchor="center"), Zone("blob", [(32, 16), (112, 40), (96, 120), (16, 88)], anchor="bottom_center"),
          Line("mid", (0, 64), (128, 64), anchor="center"), Zone("cam1", [(0, 64), (128, 64), (128, 128), (0, 128)], stream=1, classes=list(range(0, 80, 2)))]


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
    """One batch of FocoosDetections back as the packed arrays, in the order of the list."""
    B = len(batch)
    s, l, bx = np.zeros((B, T), np.float32), np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
    c = np.array([len(r.detections) for r in batch], np.int32)
    for b, r in enumerate(batch):
        for j, d in enumerate(r.detections):
            s[b, j], l[b, j], bx[b, j] = d.conf, d.cls_id, d.bbox
    return s, l, bx, c


def test_infer_stream_and_infer_batch_count_like_zones_stepped_by_hand(detr):
    """6 batches of 2 frames.  The zone dicts are those of a DeviceZones stepped by hand over the packed results of a plain run (so
    pack_detections kept the slot order: the indices are indices into ``detections``), and of the restatement; one DeviceZones over two
    calls, infer_batch and detections=False say the same; zones=None changes nothing."""
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) if j % 3 else synth_image_structured(40 + b + 10 * j, SIZE, SIZE) for b in range(2)]
               for j in range(6)]
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    tracked = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW))
    assert all(r.zones is None for batch in plain + tracked for r in batch)
    # by hand: tracker, then zones, then the public form; the restatement alongside
    trk = DeviceTracker(2, LOW, DEV)
    hand, ref, want = DeviceZones(2, PUBLIC, trk), R.RefZones(2, PUBLIC, LOW.max_tracks), []
    for batch in plain:
        s, l, bx, c = _packed(batch)
        ids = trk.update(_dev(s), _dev(l), _dev(bx), _dev(c))
        got = _host(hand.update(_dev(l), _dev(bx), _dev(c), ids))
        _same(got, ref.update(l, bx, c, ids.cpu().numpy(), trk.state()["id"]), "by hand")
        want.append(hand.fetch())
    inside = sum(z["count"] for fr in want for st in fr for z in st.values())
    print(f"{sum(len(r.detections) for batch in plain for r in batch)} detections in 12 frames, {inside} zone memberships, {ref.stats}, "
          f"in {ref.in_total.tolist()} out {ref.out_total.tolist()}")
    assert [list(st) for st in want[0]] == [["left", "blob", "mid"], ["left", "blob", "mid", "cam1"]]
    assert inside > 0 or not any(r.detections for batch in plain for r in batch)
    for fr, batch in zip(want, plain):               # the indices point into the detection lists
        for st, r in zip(fr, batch):
            assert all(0 <= j < len(r.detections) for z in st.values() for key in ("detections", "crossed_in", "crossed_out") for j in z[key])
    for run in range(2):
        got = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC))
        assert [[r.zones for r in batch] for batch in got] == want, run
        assert [[_dets(r) for r in batch] for batch in got] == [[_dets(r) for r in batch] for batch in tracked], run
    # one DeviceZones over two calls carries its state (and its tracker's) across them
    trk2 = DeviceTracker(2, LOW, DEV)
    dz = DeviceZones(2, PUBLIC, trk2)
    halves = list(detr.infer_stream(iter(batches[:3]), threshold=0.05, zones=dz)) + list(detr.infer_stream(iter(batches[3:]), threshold=0.05, track=trk2, zones=dz))
    assert [[r.zones for r in batch] for batch in halves] == want
    assert [[_dets(r) for r in batch] for batch in halves] == [[_dets(r) for r in batch] for batch in tracked]
    _same(dz.state(), hand.state(), "halves")
    # infer_batch(tracker=, zones=)
    trk2.reset(), dz.reset()
    one = [detr.infer_batch(b, threshold=0.05, tracker=trk2, zones=dz) for b in batches]
    assert [[r.zones for r in batch] for batch in one] == want
    assert [[_dets(r) for r in batch] for batch in one] == [[_dets(r) for r in batch] for batch in tracked]
    # the analytics-only mode: the same dicts, no detection objects
    lean = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, detections=False))
    assert [[r.zones for r in batch] for batch in lean] == want
    assert all(r.detections == [] for batch in lean for r in batch)
    # zones=None is the run without the argument; occupancy without a tracker needs no ids
    again = list(detr.infer_stream(iter(batches), threshold=0.05, zones=None))
    assert [[_dets(r) for r in batch] for batch in again] == [[_dets(r) for r in batch] for batch in plain]
    only = [z for z in PUBLIC if isinstance(z, Zone)]
    occ = list(detr.infer_stream(iter(batches), threshold=0.05, zones=only))
    assert [[_dets(r) for r in batch] for batch in occ] == [[_dets(r) for r in batch] for batch in plain]
    for fr, batch in zip(want, occ):
        for st, r in zip(fr, batch):
            assert {n: (z["count"], z["detections"]) for n, z in r.zones.items()} == {n: (st[n]["count"], st[n]["detections"]) for n in r.zones}
            assert all(z["entered"] == z["exited"] == 0 and z["crossed_in"] == [] for z in r.zones.values())
    with pytest.raises(ValueError, match="another tracker"):
        list(detr.infer_stream(iter(batches[:1]), threshold=0.05, track=True, zones=dz))
    with pytest.raises(ValueError, match="batch"):
        detr.infer_batch(batches[0][:1], threshold=0.05, zones=dz)
