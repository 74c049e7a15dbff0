"""Heat maps on a real MI355X (csrc/heat_ops.hip through focoos_amd/heat.py): fx_heat_update against the restatement of tests/heat_ref.py
after every frame (the grid and its maximum, for equality), fx_annotate_heat_u8 byte for byte, the refusals of both, and
infer_stream(track=, zones=, dwell=, heatmap=, annotate=Overlay(heat=True)) / infer_batch with seeded synthetic weights against objects
stepped by hand over the packed results of a plain run.  Nothing here reads the reference tree."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.annotate import Overlay, OverlayPass, annotator_of
from focoos_amd.heat import DeviceHeatmap, Heatmap
from focoos_amd.synth import synth_image_structured
from focoos_amd.tracking import DeviceTracker, TrackerConfig
from focoos_amd.zones import DWELL_KEYS, KEYS, DeviceDwell, DeviceZones, Line, Zone

from . import dwell_ref as DR
from . import heat_ref as R
from .test_gpu_tracking import sequence

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _same(got, want, where):
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == w.dtype and np.array_equal(got[k], w), (where, k)


# ---------------------------------------------------------------- (a) the update
# The boxes of test_gpu_tracking.sequence live inside about 300 x 300, so a frame of 150 x 270 has anchors on it, on its right / bottom
# edge and past it.  Tiles are 32 x 8 cells: cell 4 -> 68 x 38 cells (3 x 5 tiles, both partial), cell 32 -> 9 x 5 (one partial tile),
# cell 8 -> 34 x 19.
H, W = 150, 270
CASES = [dict(cell=4, radius=2, T=70, B=3),
         dict(cell=4, radius=16, decay_shift=3, classes=[1], T=8, B=1),
         dict(cell=32, radius=0, tracked_only=True, T=70, B=1, anchor="center"),
         dict(cell=32, radius=2, decay_shift=1, T=8, B=3, anchor="top_left"),
         dict(cell=8, radius=2, decay_shift=15, classes=[0], tracked_only=True, T=70, B=3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_update_equals_the_restatement_after_every_frame(case):
    kw = dict(case)
    T, B = kw.pop("T"), kw.pop("B")
    cfg = Heatmap(H, W, **kw)
    dh, ref = DeviceHeatmap(B, cfg, DEV), R.RefHeat(B, H, W, **kw)
    assert tuple(dh.heat.shape) == ref.heat.shape == (B,) + cfg.grid_shape
    rs = np.random.RandomState(5)
    for f, (s, l, bx, c) in enumerate(sequence(300 + T + B, B, T, 6)):
        ids = np.where(rs.rand(B, T) < 0.6, rs.randint(1, 50, (B, T)), rs.randint(-1, 1, (B, T))).astype(np.int32)
        dh.update(_dev(l), _dev(bx), _dev(c), _dev(ids) if cfg.tracked_only or f % 2 else None)
        ref.update(l, bx, c, ids)
        _same(dh.state(), ref.state(), f)
        if f == 3:
            assert c[B - 1] == 0                                         # the ragged counts include 0
    print(f"{case}: {ref.deposited} deposits, maxima {ref.heat_max.tolist()}")
    assert ref.deposited > 0 and ref.heat_max.max() > R.ONE
    assert np.array_equal(dh.grid(), (ref.heat / 256.0).astype(np.float32)) and dh.grid(B - 1).shape == cfg.grid_shape
    dh.reset(B - 1)
    st = dh.state()
    assert not st["heat"][B - 1].any() and st["heat_max"][B - 1] == 0 and (B == 1 or st["heat"][0].any())
    dh.reset()
    assert not dh.state()["heat"].any()


def test_a_preloaded_state_saturates_at_the_clamp_and_decays_from_it():
    B, T = 2, 8
    s, l, bx, c = sequence(11, B, T, 1)[0]
    for shift in (0, 2):
        dh, ref = DeviceHeatmap(B, Heatmap(H, W, cell=8, radius=16, decay_shift=shift), DEV), R.RefHeat(B, H, W, cell=8, radius=16, decay_shift=shift)
        pre = np.random.RandomState(3).randint(R.CLAMP - 600, R.CLAMP + 1, ref.heat.shape).astype(np.int32)
        ref.heat[...] = pre
        dh.heat.copy_(_dev(pre))
        for f in range(2):
            dh.update(_dev(l), _dev(bx), _dev(c))
            ref.update(l, bx, c)
            _same(dh.state(), ref.state(), (shift, f))
        assert ref.heat.max() == R.CLAMP if shift == 0 else ref.heat.max() < R.CLAMP
        assert ref.heat_max.tolist() == ref.heat.reshape(B, -1).max(1).tolist()
    with pytest.raises(ValueError, match="batch"):
        dh.update(_dev(l[:1]), _dev(bx[:1]), _dev(c[:1]))
    with pytest.raises(ValueError, match="det_boxes"):
        dh.update(_dev(l), _dev(bx.astype(np.int64)), _dev(c))
    with pytest.raises(ValueError, match="tracked_only"):
        DeviceHeatmap(B, Heatmap(H, W, tracked_only=True), DEV).update(_dev(l), _dev(bx), _dev(c))


# ---------------------------------------------------------------- (b) the drawing
def _user_lut(seed):
    rs = np.random.RandomState(seed)
    lut = rs.randint(0, 1 << 32, 256, dtype=np.int64).astype(np.uint32)
    lut[0] &= np.uint32(0x00FFFFFF)                    # nothing where nobody stood
    lut[7] |= np.uint32(0xFF000000)                    # an opaque entry and a transparent one in the middle
    lut[9] &= np.uint32(0x00FFFFFF)
    lut[255] |= np.uint32(0x80000000)                  # the hottest colour is never transparent
    return lut


# (H, W) = (37, 53) and (135, 241): the byte path and partial tiles in both directions; (64, 96): the dword path
@pytest.mark.parametrize("Hf,Wf,cell,full_scale", [(37, 53, 4, 0), (64, 96, 8, 3), (64, 96, 32, 0), (135, 241, 16, 3)])
def test_drawing_equals_the_restatement_byte_for_byte(Hf, Wf, cell, full_scale):
    S = 3
    lut = _user_lut(Hf)
    dh = DeviceHeatmap(S, Heatmap(Hf, Wf, cell=cell, full_scale=full_scale, lut=lut), DEV)
    rs = np.random.RandomState(Wf)
    heat = (rs.randint(0, 1200, dh.heat.shape) * (rs.rand(*dh.heat.shape) < 0.7)).astype(np.int32)
    heat[1] = 0                                        # stream 1 is cold
    heat[2, 0, 0] = 5000                               # above full_scale 3: the index saturates at 255
    hmax = heat.reshape(S, -1).max(1).astype(np.int32)
    dh.heat.copy_(_dev(heat)), dh.heat_max.copy_(_dev(hmax))
    for b0, B in ((0, 3), (1, 2)):
        frames = rs.randint(0, 256, (B, Hf, Wf, 3)).astype(np.uint8)
        want = np.stack([R.render_fast(frames[b], heat[b0 + b], hmax[b0 + b], cell, full_scale, lut) for b in range(B)])
        cold = 1 - b0                                  # the cold stream's frame
        assert np.array_equal(want[cold], frames[cold]) and not np.array_equal(want[B - 1], frames[B - 1])      # v = 0 -> lut[0], alpha 0
        # in place and into another buffer, each inside canary slabs
        slab = torch.full((B + 2, Hf, Wf, 3), 0x5A, dtype=torch.uint8, device=DEV)
        slab[1:B + 1] = _dev(frames)
        assert dh.render(slab[1:B + 1], b0) is not None
        got = slab.cpu().numpy()
        assert np.array_equal(got[1:B + 1], want), (b0, "in place")
        assert (got[0] == 0x5A).all() and (got[-1] == 0x5A).all()
        src, dst = _dev(frames), torch.full((B + 2, Hf, Wf, 3), 0xA5, dtype=torch.uint8, device=DEV)
        dh.render(src, b0, out=dst[1:B + 1])
        got = dst.cpu().numpy()
        assert np.array_equal(got[1:B + 1], want), (b0, "disjoint")               # a cold stream's frame is copied
        assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all() and np.array_equal(src.cpu().numpy(), frames)
    if (Hf, Wf) == (37, 53):                            # small enough for the per-pixel restatement
        assert np.array_equal(want[0], R.render(frames[0], heat[1], hmax[1], cell, full_scale, lut))
        assert np.array_equal(want[1], R.render(frames[1], heat[2], hmax[2], cell, full_scale, lut))
    with pytest.raises(ValueError, match="heat map of"):
        dh.render(torch.zeros(1, Hf, Wf + 1, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="streams"):
        dh.render(torch.zeros(2, Hf, Wf, 3, dtype=torch.uint8, device=DEV), 2)


def test_update_then_draw_with_the_current_maximum_as_the_scale():
    """The scale of full_scale = 0 is the heat_max the update kernel left on the device."""
    B, T, Hf, Wf = 2, 70, 135, 241
    cfg = Heatmap(Hf, Wf, cell=8, radius=2, anchor="center")
    dh, ref = DeviceHeatmap(B, cfg, DEV), R.RefHeat(B, Hf, Wf, cell=8, radius=2, anchor="center")
    for s, l, bx, c in sequence(9, B, T, 3):
        dh.update(_dev(l), _dev(bx), _dev(c))
        ref.update(l, bx, c)
    frames = np.random.RandomState(1).randint(0, 256, (B, Hf, Wf, 3)).astype(np.uint8)
    got = dh.render(_dev(frames)).cpu().numpy()
    want = np.stack([R.render_fast(frames[b], ref.heat[b], ref.heat_max[b], 8, 0, cfg.table) for b in range(B)])
    assert np.array_equal(got, want) and not np.array_equal(got, frames)


# ---------------------------------------------------------------- (c) refusals
def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, Hf, Wf, cell = 2, 8, 37, 53, 4
    Gh, Gw = R.cells(Hf, cell), R.cells(Wf, cell)
    tiles = lib.fx_heat_tiles(Hf, Wf, cell)
    assert tiles == 1 * 2 and lib.fx_heat_tiles(Hf, Wf, 5) == INVALID and lib.fx_heat_tiles(0, Wf, 4) == INVALID and lib.fx_heat_tiles(16384, 16384, 4) == 128 * 512
    s, l, bx, c = sequence(3, B, T, 1)[0]
    bx = bx // 6                                          # into the small frame
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)      # noqa: E731
    out = dict(heat=i32(B + 1, Gh, Gw), heat_max=i32(B + 1), part=i32(B + 1, tiles))      # one canary row / element past the end of each
    dl, dbx, dc = _dev(l), _dev(np.concatenate([bx.reshape(-1), np.zeros(4, np.int32)])), _dev(c)
    ids = _dev(np.ones((B, T), np.int32))
    words = np.zeros(8, np.uint32)
    base = dict(l=dl.data_ptr(), bx=dbx.data_ptr(), c=dc.data_ptr(), ids=ids.data_ptr(), B=B, T=T, H=Hf, W=Wf, cell=cell, radius=2, anchor=7, decay=0, flags=1,
                words=words.ctypes.data, **{k: v.data_ptr() for k, v in out.items()})
    order = ["l", "bx", "c", "ids", "B", "T", "H", "W", "cell", "radius", "anchor", "decay", "flags", "words", "heat", "heat_max", "part"]
    call = lambda **k: lib.fx_heat_update(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731
    bad = [{p: None} for p in ("l", "bx", "c", "words", "heat", "heat_max", "part")]
    bad += [dict(ids=None, flags=3), dict(ids=None, flags=2), dict(bx=base["bx"] + 4), dict(bx=base["bx"] + 8), dict(l=base["l"] + 2), dict(heat=base["heat"] + 1),
            dict(ids=base["ids"] + 2), dict(B=0), dict(B=65536), dict(T=0), dict(T=1025), dict(H=0), dict(H=16385), dict(W=0), dict(W=16385),
            dict(cell=0), dict(cell=2), dict(cell=12), dict(cell=64), dict(radius=-1), dict(radius=17), dict(anchor=-1), dict(anchor=9), dict(decay=-1),
            dict(decay=16), dict(flags=-1), dict(flags=4)]
    for k in bad:
        assert call(**k) == INVALID, k
    frames = torch.full((B + 2, Hf, Wf, 3), 0x5A, dtype=torch.uint8, device=DEV)
    lut = _dev(_user_lut(1).view(np.int32))
    heat, hmax = _dev(np.full((B, Gh, Gw), 300, np.int32)), _dev(np.full(B, 300, np.int32))
    dbase = dict(src=frames[1:].data_ptr(), dst=frames[1:].data_ptr(), B=B, H=Hf, W=Wf, b0=0, streams=B, heat=heat.data_ptr(), hmax=hmax.data_ptr(), cell=cell,
                 fs=0, lut=lut.data_ptr())
    dorder = ["src", "dst", "B", "H", "W", "b0", "streams", "heat", "hmax", "cell", "fs", "lut"]
    dcall = lambda **k: lib.fx_annotate_heat_u8(*[dict(dbase, **k)[n] for n in dorder], _stream())      # noqa: E731
    dbad = [{p: None} for p in ("src", "dst", "heat", "hmax", "lut")]
    dbad += [dict(B=0), dict(b0=-1), dict(b0=1), dict(streams=0), dict(streams=65536), dict(streams=1), dict(H=0), dict(W=16385), dict(cell=3), dict(cell=64),
             dict(fs=-1), dict(fs=(1 << 22) + 1), dict(heat=dbase["heat"] + 2), dict(lut=dbase["lut"] + 1), dict(hmax=dbase["hmax"] + 2),
             dict(dst=dbase["src"] + 3), dict(dst=dbase["src"] - Hf * Wf * 3), dict(B=1, dst=dbase["src"] + Hf * Wf * 3 - 1)]      # overlapping, not equal
    for k in dbad:
        assert dcall(**k) == INVALID, k
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values()) and bool((frames == 0x5A).all())
    # the same arguments unbroken run; the canaries past the end stay
    assert call() == 0 and dcall(B=1) == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v[-1] == -7).all()), k
    ref = R.RefHeat(B, Hf, Wf, cell=cell, radius=2)
    ref.heat[...] = -7                                    # the sentinel is a state like any other
    ref.update(l, bx, c)
    assert np.array_equal(out["heat"][:-1].cpu().numpy(), ref.heat) and np.array_equal(out["heat_max"][:-1].cpu().numpy(), ref.heat_max) and ref.deposited > 0
    assert not bool((out["part"][:-1] == -7).any())
    got = frames.cpu().numpy()
    want = R.render_fast(np.full((Hf, Wf, 3), 0x5A, np.uint8), np.full((Gh, Gw), 300, np.int32), 300, cell, 0, _user_lut(1))
    assert (got[0] == 0x5A).all() and (got[2] == 0x5A).all() and np.array_equal(got[1], want) and not (want == 0x5A).all()


# ---------------------------------------------------------------- (d) the public interface
SIZE = 128
LOW = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)
PUBLIC = [Zone("left", [(0, 0), (64, 0), (64, 128), (0, 128)], anchor="center"), Zone("blob", [(32, 16), (112, 40), (96, 120), (16, 88)], anchor="bottom_center"),
          Line("mid", (0, 64), (128, 64), anchor="center"), Zone("cam1", [(0, 64), (128, 64), (128, 128), (0, 128)], stream=1, classes=list(range(0, 80, 2)))]
HEAT = dict(cell=8, radius=2)


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


def test_infer_stream_and_infer_batch_say_what_objects_stepped_by_hand_say(detr):
    """6 batches of 2 frames.  The zone dicts (with the dwell keys) and the heat maps are those of a DeviceDwell / DeviceHeatmap stepped by
    hand over the packed results of a plain run, and of the two restatements; the picture is the hand-heated frame with the rest of the
    overlay drawn on it; one DeviceDwell / DeviceHeatmap over two calls, infer_batch and detections=False say the same; with the three
    new arguments unset nothing changes."""
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) if j % 3 else synth_image_structured(40 + b + 10 * j, SIZE, SIZE) for b in range(2)]
               for j in range(6)]
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    ov0 = Overlay()
    base = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, annotate=ov0))      # a run that never names the new arguments
    # by hand: tracker, zones, dwell, heat, then the picture; the restatements alongside
    trk = DeviceTracker(2, LOW, DEV)
    zon = DeviceZones(2, PUBLIC, trk)
    dw, hm = DeviceDwell(zon), DeviceHeatmap(2, Heatmap(SIZE, SIZE, **HEAT), DEV)
    rdw, rhm = DR.RefDwell([[k for _, k in rows] for rows in dw.rows], LOW.max_tracks), R.RefHeat(2, SIZE, SIZE, **HEAT)
    ann, want, pictures = annotator_of(detr), [], []
    for batch, frames in zip(plain, batches):
        s, l, bx, c = _packed(batch)
        ds, dl, dbx, dc = _dev(s), _dev(l), _dev(bx), _dev(c)
        ids = trk.update(ds, dl, dbx, dc)
        inside = zon.update(dl, dbx, dc, ids)["det_inside"]
        got = dw.update(dc, ids, inside).cpu().numpy()
        assert np.array_equal(got, rdw.update(c, ids.cpu().numpy(), inside.cpu().numpy(), trk.state()["id"]))
        hm.update(dl, dbx, dc, ids)
        rhm.update(l, bx, c)
        _same(hm.state(), rhm.state(), "by hand")
        want.append(dw.fetch())
        fr = np.stack(frames)
        heated = hm.render(_dev(fr))
        assert np.array_equal(heated.cpu().numpy(), np.stack([R.render_fast(fr[b], rhm.heat[b], rhm.heat_max[b], 8, 0, hm.config.table) for b in range(2)]))
        res = SimpleNamespace(det_scores=ds, det_labels=dl, det_boxes=dbx, det_count=dc)
        pictures.append(ann.annotate_overlay(heated, res, 0, OverlayPass(ov0, ids, zon, None, None)).cpu().numpy())
    _same(dw.state(), rdw.state(), "by hand")
    dwell_keys = [z for fr in want for st in fr for z in st.values() if "dwell" in z]
    print(f"{sum(len(r.detections) for batch in plain for r in batch)} detections in 12 frames, {rhm.deposited} deposits, maxima {rhm.heat_max.tolist()}, "
          f"{rdw.stats}, longest dwell now {max([max(z['dwell'], default=0) for z in dwell_keys], default=0)}")
    assert rhm.deposited > 0 and [list(st) for st in want[0]] == [["left", "blob", "mid"], ["left", "blob", "mid", "cam1"]]
    for fr in want:
        for st in fr:
            assert tuple(st["mid"]) == KEYS and all(tuple(st[n]) == KEYS + DWELL_KEYS for n in st if n != "mid")
            assert all(len(z["dwell"]) == len(z["detections"]) for n, z in st.items() if n != "mid")
    ov = Overlay(heat=True)
    for run in range(2):
        got = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, dwell=True, heatmap=Heatmap(SIZE, SIZE, **HEAT), annotate=ov))
        assert [[r.zones for r in batch] for batch in got] == want, run
        assert [[_dets(r) for r in batch] for batch in got] == [[_dets(r) for r in batch] for batch in base], run
        for j, batch in enumerate(got):
            for b, r in enumerate(batch):
                assert np.array_equal(r.image, pictures[j][b]), (run, j, b)
    assert any(not np.array_equal(r.image, q.image) for g, p in zip(got, base) for r, q in zip(g, p))      # the heat layer shows
    # a list of names keeps only those; fps adds the seconds
    some = list(detr.infer_stream(iter(batches[:2]), threshold=0.05, track=LOW, zones=PUBLIC, dwell=["blob"]))
    assert all(tuple(st["blob"]) == KEYS + DWELL_KEYS and tuple(st["left"]) == KEYS for batch in some for st in (r.zones for r in batch))
    assert [[r.zones["blob"] for r in batch] for batch in some] == [[st["blob"] for st in fr] for fr in want[:2]]
    # one DeviceDwell / DeviceHeatmap over two calls carry their state across them
    trk2 = DeviceTracker(2, LOW, DEV)
    dz = DeviceZones(2, PUBLIC, trk2)
    dd, dh = DeviceDwell(dz, fps=25.0), DeviceHeatmap(2, Heatmap(SIZE, SIZE, **HEAT), DEV)
    halves = (list(detr.infer_stream(iter(batches[:3]), threshold=0.05, zones=dz, dwell=dd, heatmap=dh)) +
              list(detr.infer_stream(iter(batches[3:]), threshold=0.05, track=trk2, zones=dz, dwell=dd, heatmap=dh)))
    strip = lambda st: {n: {k: v for k, v in z.items() if k != "dwell_seconds"} for n, z in st.items()}      # noqa: E731
    assert [[strip(r.zones) for r in batch] for batch in halves] == want
    assert all(z["dwell_seconds"] == [n / 25.0 for n in z["dwell"]] for batch in halves for r in batch for n, z in r.zones.items() if n != "mid")
    _same(dd.state(), dw.state(), "halves")
    _same(dh.state(), hm.state(), "halves")
    # infer_batch(tracker=, zones=, dwell=, heatmap=)
    trk2.reset(), dz.reset(), dd.reset(), dh.reset()
    one = [detr.infer_batch(b, threshold=0.05, tracker=trk2, zones=dz, dwell=dd, heatmap=dh, annotate=ov) for b in batches]
    assert [[strip(r.zones) for r in batch] for batch in one] == want
    assert all(np.array_equal(r.image, pictures[j][b]) for j, batch in enumerate(one) for b, r in enumerate(batch))
    _same(dh.state(), hm.state(), "infer_batch")
    # the analytics-only mode: the same dicts and the same maps, no detection objects
    dh.reset()
    lean = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, dwell=True, heatmap=dh, detections=False))
    assert [[r.zones for r in batch] for batch in lean] == want and all(r.detections == [] for batch in lean for r in batch)
    _same(dh.state(), hm.state(), "detections=False")
    # with the three new arguments unset, results and pictures are those of the run that never names them
    again = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, zones=PUBLIC, annotate=ov0, dwell=None, heatmap=None))
    assert [[r.zones for r in batch] for batch in again] == [[r.zones for r in batch] for batch in base]
    assert all(tuple(z) == KEYS for batch in again for r in batch for z in r.zones.values())
    assert [[_dets(r) for r in batch] for batch in again] == [[_dets(r) for r in batch] for batch in base]
    assert all(np.array_equal(r.image, q.image) for g, p in zip(again, base) for r, q in zip(g, p))
    with pytest.raises(ValueError, match="another DeviceZones"):
        list(detr.infer_stream(iter(batches[:1]), threshold=0.05, zones=DeviceZones(2, PUBLIC, trk2), dwell=dd))
    with pytest.raises(ValueError, match="input 0 is 128 x 128, the heat map is 64 x 128"):
        list(detr.infer_stream(iter(batches[:1]), threshold=0.05, heatmap=Heatmap(64, 128)))
    with pytest.raises(ValueError, match="batch"):
        detr.infer_batch(batches[0][:1], threshold=0.05, heatmap=dh)
