"""Dwell times on a real MI355X (csrc/dwell_ops.hip through focoos_amd/zones.py DeviceDwell): fx_dwell_update against the restatement of
tests/dwell_ref.py after every frame of seeded moving boxes that first go through the real DeviceTracker and fx_zone_update (the output
and all seven state arrays, for equality), both resets and the refusals.  The public interface is exercised in tests/test_gpu_heat.py
together with the heat map.  Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.tracking import DeviceTracker, TrackerConfig
from focoos_amd.zones import DeviceDwell, DeviceZones, Line, Zone

from . import dwell_ref as R
from .test_gpu_tracking import sequence

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
SHAPES = [(8, 4), (70, 130)]      # (T, max_tracks): one wave partly filled and four slots; two waves and more than 64 slots
# The seed of a configuration's sequence is 1000 T + B unless that sequence, stepped on the host through the three restatements (tracker,
# zones, dwell) with track_buffer 2, misses one of the ways a visit ends or never resumes one after an unobserved frame.
SEEDS = {(1, 8): 8002}
TRACK_BUFFER = 2
NEED = ("closed_left", "closed_stale", "closed_reused", "resumed_after_gap", "kept_unobserved", "first_inside")
HEPTAGON = [(64, 48), (128, 32), (208, 64), (224, 144), (160, 208), (96, 192), (48, 128)]


def regions_for(B):
    """Two shared zones with a line between them (so the watched bits are 0 and 2) and, for B = 3, a class-filtered zone of the last
    stream only (so the streams have different row counts)."""
    r = [Zone("hept", HEPTAGON, anchor="center"), Line("mid", (128, 0), (128, 256), anchor="center"), Zone("left", [(0, 0), (128, 0), (128, 256), (0, 256)])]
    if B > 1:
        r.append(Zone("ones", [(0, 0), (256, 0), (0, 256)], stream=B - 1, classes=[1], anchor="top_left"))
    return r


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _same(got, want, where):
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (where, k, g.dtype, w.dtype)
        assert np.array_equal(g, w), (where, k, g.tolist(), w.tolist())


def _make(B, M):
    trk = DeviceTracker(B, TrackerConfig(track_buffer=TRACK_BUFFER, max_tracks=M), DEV)
    zon = DeviceZones(B, regions_for(B), trk)
    dw = DeviceDwell(zon)
    ref = R.RefDwell([[k for _, k in rows] for rows in dw.rows], M)
    assert dw.dw_first.tolist() == ref.dw_first.tolist() and dw.dw_bit.tolist() == [k for r in ref.rows for k in r]
    return trk, zon, dw, ref


def _step(trk, zon, dw, ref, fr):
    s, l, bx, c = fr
    dl, dbx, dc = _dev(l), _dev(bx), _dev(c)
    ids = trk.update(_dev(s), dl, dbx, dc)
    inside = zon.update(dl, dbx, dc, ids)["det_inside"]
    got = dw.update(dc, ids, inside).cpu().numpy()
    want = ref.update(c, ids.cpu().numpy(), inside.cpu().numpy(), trk.state()["id"])      # stepped on the tracker's own ids and slot table
    return got, want


# ---------------------------------------------------------------- (a) equality with the restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,M", SHAPES)
def test_update_equals_the_restatement_after_every_frame(B, T, M):
    trk, zon, dw, ref = _make(B, M)
    assert np.diff(dw.dw_first).tolist() == ([2, 2, 3] if B == 3 else [2]) and dw.dw_bit.tolist()[:2] == [0, 2]
    seen = 0
    for f, fr in enumerate(sequence(SEEDS.get((B, T), 1000 * T + B), B, T)):
        got, want = _step(trk, zon, dw, ref, fr)
        assert got.shape == want.shape == (dw.D, T) and np.array_equal(got, want), (f, got.tolist(), want.tolist())
        _same(dw.state(), ref.state(), f)
        seen += int((want > 1).sum())
        c = fr[3]
        for b in range(B):      # 0 from det_count on
            assert not got[int(dw.dw_first[b]):int(dw.dw_first[b + 1]), int(c[b]):].any()
    st = ref.state()
    print(f"B={B} T={T} M={M}: {ref.stats}, visits {st['visits'].tolist()} total {st['dwell_sum'].tolist()} longest {st['dwell_max'].tolist()}")
    for k in NEED:
        assert ref.stats[k] > 0, (k, ref.stats)
    assert seen > 0 and st["frame"].tolist() == [12] * B and st["visits"].sum() > 0
    # fetch() says the same thing in the public form
    pub = dw.fetch()
    for b in range(B):
        for i, (name, _) in enumerate(dw.rows[b]):
            d, z = int(dw.dw_first[b]) + i, pub[b][name]
            assert z["dwell"] == want[d, z["detections"]].tolist() and len(z["dwell"]) == z["count"]
            assert (z["visits"], z["dwell_total"], z["dwell_max"]) == (int(st["visits"][d]), int(st["dwell_sum"][d]), int(st["dwell_max"][d]))
            assert z["dwell_mean"] == (z["dwell_total"] / z["visits"] if z["visits"] else 0.0) and "dwell_seconds" not in z
        assert "dwell" not in pub[b]["mid"]


# ---------------------------------------------------------------- (b) both resets
def test_reset_clears_one_streams_visits_and_keeps_the_totals_on_request():
    B, T, M = 3, 70, 130
    trk, zon, dw, ref = _make(B, M)
    seq = sequence(70003, B, T)
    for f, fr in enumerate(seq[:6]):
        got, want = _step(trk, zon, dw, ref, fr)
        assert np.array_equal(got, want), f
    lo, hi = int(ref.dw_first[1]), int(ref.dw_first[2])
    assert ref.dw_id[lo:hi].any() and ref.visits[lo:hi].any() and ref.dw_id[:lo].any()
    # what must follow DeviceTracker.reset(b): the visits in progress and the frame count of that stream go, the totals stay
    trk.reset(1), zon.reset(1, counters=False), dw.reset(1, totals=False), ref.reset(1, totals=False)
    _same(dw.state(), ref.state(), "reset(1, totals=False)")
    st = dw.state()
    assert not st["dw_id"][lo:hi].any() and st["visits"][lo:hi].any() and st["frame"].tolist() == [6, 0, 6] and st["dw_id"][:lo].any()
    for f, fr in enumerate(seq[6:9]):
        got, want = _step(trk, zon, dw, ref, fr)
        assert np.array_equal(got, want), f
        _same(dw.state(), ref.state(), f)
    dw.reset(2), ref.reset(2)
    _same(dw.state(), ref.state(), "reset(2)")
    assert not dw.state()["visits"][hi:].any() and dw.state()["visits"][:hi].any()
    dw.reset(), ref.reset()
    _same(dw.state(), ref.state(), "reset()")
    assert not any(v.any() for v in dw.state().values())
    for f, fr in enumerate(seq[9:]):
        got, want = _step(trk, zon, dw, ref, fr)
        assert np.array_equal(got, want), f
        _same(dw.state(), ref.state(), f)
    with pytest.raises(ValueError):
        dw.reset(3)
    with pytest.raises(ValueError, match="batch"):
        dw.update(_dev(seq[0][3][:2]), torch.zeros(2, T, dtype=torch.int32, device=DEV), torch.zeros(2, T, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="det_inside"):
        dw.update(_dev(seq[0][3]), torch.zeros(3, T, dtype=torch.int32, device=DEV), torch.zeros(3, T, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------- (c) refusals
def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, M, D = 2, 8, 4, 3
    first, region, bit, reg_first = (np.array(a, np.int32) for a in ([0, 2, 3], [0, 2, 4], [0, 2, 1], [0, 3, 5]))
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)      # noqa: E731
    out = dict(dw_id=i32(D + 1, M), dw_enter=i32(D + 1, M), dw_last=i32(D + 1, M), visits=i32(D + 1), dwell_max=i32(D + 1), frame=i32(B + 1),
               det_dwell=i32(D + 1, T), dwell_sum=torch.full((D + 1,), -7, dtype=torch.int64, device=DEV))      # one canary row / element past the end
    cnt, ids = _dev(np.array([3, 8], np.int32)), _dev(np.array([[5, 6, 9, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 8]], np.int32))
    ins = _dev(np.array([[5, 1, 7, 0, 0, 0, 0, 0], [2, 3, 0, 1, 2, 3, 0, 1]], np.int32))
    trk = _dev(np.array([[6, 5, 0, 9], [4, 3, 2, 1]], np.int32))
    d_first, d_bit = _dev(first), _dev(bit)
    keep = []

    def host(a):
        a = np.ascontiguousarray(a, np.int32)
        keep.append(a)
        return a.ctypes.data

    base = dict(c=cnt.data_ptr(), ids=ids.data_ptr(), ins=ins.data_ptr(), B=B, T=T, trk=trk.data_ptr(), M=M, first=d_first.data_ptr(), bit=d_bit.data_ptr(),
                hfirst=host(first), hregion=host(region), hbit=host(bit), hreg=host(reg_first), D=D, **{k: v.data_ptr() for k, v in out.items()})
    order = ["c", "ids", "ins", "B", "T", "trk", "M", "first", "bit", "hfirst", "hregion", "hbit", "hreg", "D", "dw_id", "dw_enter", "dw_last", "visits",
             "dwell_sum", "dwell_max", "frame", "det_dwell"]
    call = lambda **k: lib.fx_dwell_update(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731
    bad = [{p: None} for p in order if p not in ("B", "T", "M", "D")]
    bad += [dict(c=base["c"] + 2), dict(ids=base["ids"] + 1), dict(dwell_sum=base["dwell_sum"] + 4), dict(det_dwell=base["det_dwell"] + 2),
            dict(B=0), dict(B=65536), dict(B=1), dict(T=0), dict(T=1025), dict(M=0), dict(M=1025), dict(D=0), dict(D=2), dict(D=4),
            dict(hfirst=host([1, 2, 3])), dict(hfirst=host([0, 3, 2])), dict(hfirst=host([0, 1, 2])),
            dict(hbit=host([0, 3, 1])), dict(hbit=host([0, -1, 1])), dict(hbit=host([0, 0, 1])), dict(hbit=host([0, 2, 2])),
            dict(hregion=host([0, 1, 4])), dict(hregion=host([0, 2, 3])), dict(hreg=host([0, 2, 5])), dict(hreg=host([1, 3, 5])), dict(hreg=host([0, 3, 2]))]
    # 33 rows on one stream: tables of their own
    bad.append(dict(hfirst=host([0, 33, 34]), hregion=host(list(range(34))), hbit=host(list(range(33)) + [0]), hreg=host([0, 32, 33]), D=34))
    for k in bad:
        assert call(**k) == INVALID, k
    rorder = ["dw_id", "dw_enter", "dw_last", "visits", "dwell_sum", "dwell_max", "frame", "hfirst", "B", "M", "b", "clear"]
    rcall = lambda **k: lib.fx_dwell_reset(*[dict(dict(base, b=0, clear=1), **k)[n] for n in rorder], _stream())      # noqa: E731
    rbad = [{p: None} for p in rorder[:8]] + [dict(b=B), dict(b=-2), dict(B=0), dict(M=0), dict(M=1025), dict(dw_id=base["dw_id"] + 2),
                                              dict(dwell_sum=base["dwell_sum"] + 4), dict(hfirst=host([0, 3, 2])), dict(hfirst=host([0, 33, 34]))]
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
    ref = R.RefDwell([[0, 2], [1]], M)
    want = ref.update(cnt.cpu().numpy(), ids.cpu().numpy(), ins.cpu().numpy(), trk.cpu().numpy())
    assert np.array_equal(out["det_dwell"][:-1].cpu().numpy(), want) and want.any()
    _same({k: out[k][:-1].cpu().numpy() for k in ref.state()}, ref.state(), "unbroken")
    assert rcall(b=1, clear=0) == 0 and rcall(b=0) == 0
    torch.cuda.synchronize()
    assert out["frame"].tolist() == [0, 0, -7] and not out["dw_id"][:-1].any() and bool((out["dw_id"][-1] == -7).all())
