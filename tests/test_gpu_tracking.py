"""Device tracking on a real MI355X (csrc/track_ops.hip through focoos_amd/tracking.py): fx_track_update against the numpy restatement of
tests/tracking_ref.py after every frame (ids and every state array, floats by bits), fx_track_reset, the refusals, and
infer_stream(track=...) / infer_batch(tracker=...) with seeded synthetic weights against a DeviceTracker stepped by hand over the same
packed results.  Nothing here reads the reference tree."""
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.synth import synth_image_structured
from focoos_amd.tracking import DeviceTracker, TrackerConfig

from . import tracking_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
FRAMES = 12
SCORES = np.array([0.05, 0.3, 0.55, 0.9], np.float32)      # nothing / low / high but below new_thresh / high


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def sequence(seed, B, T, frames=FRAMES):
    """``frames`` packed frames [(scores, labels, boxes, count)] of B streams with T slots.  Per stream T + T / 2 objects (more than fit, so
    most frames fill all T slots and, with max_tracks > 64, more than 64 slots are live) on a coarse grid (sizes and
    positions multiples of 16 inside 256 x 256: dense overlaps and exact IoU ties), two labels, moving by small even velocities; every
    object is hidden for a stretch of 0, 3 or 5 frames (with track_buffer 2: rescue, expiry and re-entry), visible ones are detected with
    a score out of SCORES, the first two detections of a frame are duplicated (identical boxes), some boxes have no area.  Slots are
    shuffled, det_count is ragged (whatever fits, 0 for the last stream in frame 3), and the slots past it hold garbage with a
    high score."""
    rs = np.random.RandomState(seed)
    N = T + max(2, T // 2)
    pos = rs.randint(0, 12, (B, N, 2)) * 16
    size = rs.randint(0, 4, (B, N, 2)) * 16 + 16 * (rs.rand(B, N, 2) < 0.93)
    vel = rs.randint(-3, 4, (B, N, 2)) * 2
    lab = rs.randint(0, 2, (B, N))
    off0, offn = rs.randint(1, max(2, frames - 4), (B, N)), rs.choice([0, 3, 5], (B, N))
    out = []
    for f in range(frames):
        s, l, bx = np.full((B, T), 2.0, np.float32), rs.randint(0, 2, (B, T)).astype(np.int32), rs.randint(0, 256, (B, T, 4)).astype(np.int32)
        count = np.zeros(B, np.int32)
        for b in range(B):
            if b == B - 1 and f == 3:
                continue
            dets = []
            for o in range(N):
                if off0[b, o] <= f < off0[b, o] + offn[b, o] or rs.rand() < 0.1:
                    continue
                p = pos[b, o] + f * vel[b, o]
                dets.append((rs.choice(SCORES, p=[0.1, 0.3, 0.15, 0.45]), lab[b, o], p[0], p[1], p[0] + size[b, o, 0], p[1] + size[b, o, 1]))
            dets = dets[:2] + dets                      # two exact duplicates
            order = rs.permutation(len(dets))[:T]
            for j, k in enumerate(order):
                s[b, j], l[b, j], bx[b, j] = dets[k][0], dets[k][1], dets[k][2:]
            count[b] = len(order)
        out.append((s, l, bx, count))
    return out


def _same_state(got, want, where, skip=()):
    for k in DeviceTracker.STATE:
        if k in skip:
            continue
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), (where, k)      # floats by bits


# ---------------------------------------------------------------- (a) equality with the restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,M", [(8, 4), (64, 64), (65, 65), (70, 130)])
def test_update_equals_the_numpy_restatement_after_every_frame(B, T, M):
    cfg = TrackerConfig(track_buffer=2, max_tracks=M, min_hits=2 if T == 65 else 1)
    ref, trk = R.RefTracker(B, cfg), DeviceTracker(B, cfg, DEV)
    peak = 0
    for f, (s, l, bx, c) in enumerate(sequence(1000 * T + B, B, T)):
        want = ref.update(s, l, bx, c)
        got = trk.update(_dev(s), _dev(l), _dev(bx), _dev(c)).cpu().numpy()
        assert np.array_equal(got, want), (f, got.tolist(), want.tolist())
        _same_state(trk.state(), ref.state(), f)
        peak = max(peak, int((ref.id != 0).sum(1).max()))
    st = ref.stats
    print(f"B={B} T={T} M={M}: {st}, most live slots of a stream {peak}, next_id {ref.next_id.tolist()}")
    # the sequence did exercise both stages, expiry, re-entry into freed slots and (where the slots are few) the overflow
    assert st["stage1"] > 0 and st["stage2"] > 0 and st["freed"] > 0 and st["born"] > 0
    assert int(ref.next_id.max()) - 1 > peak      # more ids than slots ever live at once: freed slots were taken again
    if (T, M) == (8, 4):
        assert st["dropped"] > 0 and ref.status.sum() == st["dropped"]
    if M > 64:
        assert peak > 64                         # live slots on both sides of the 64-lane boundary
    got_status = trk.status()
    assert np.array_equal(got_status, ref.status) and not trk.status().any()      # read and cleared


# ---------------------------------------------------------------- (b) reset
def test_reset_clears_one_stream_and_leaves_the_others_bit_identical():
    B, T, M = 3, 64, 64
    cfg = TrackerConfig(track_buffer=2, max_tracks=M)
    ref, trk = R.RefTracker(B, cfg), DeviceTracker(B, cfg, DEV)
    seq = sequence(5, B, T, 8)
    for s, l, bx, c in seq[:4]:
        ref.update(s, l, bx, c)
        trk.update(_dev(s), _dev(l), _dev(bx), _dev(c))
    assert (ref.id[1] != 0).any() and ref.next_id[1] > 1
    ref.reset(1)
    trk.reset(1)
    _same_state(trk.state(), ref.state(), "reset(1)")
    assert not trk.state()["id"][1].any() and trk.state()["next_id"].tolist()[1] == 1
    for f, (s, l, bx, c) in enumerate(seq[4:]):                           # the cleared stream starts over, the others go on
        want = ref.update(s, l, bx, c)
        assert np.array_equal(trk.update(_dev(s), _dev(l), _dev(bx), _dev(c)).cpu().numpy(), want), f
        _same_state(trk.state(), ref.state(), f)
    ref.reset()
    trk.reset()
    _same_state(trk.state(), ref.state(), "reset()")
    assert not trk.state()["id"].any() and trk.state()["next_id"].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        trk.reset(3)


# ---------------------------------------------------------------- (c) refusals
def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, M = 2, 8, 4
    s, l, bx, c = [_dev(a) for a in sequence(3, B, T, 1)[0]]
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)      # noqa: E731
    f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=DEV)  # noqa: E731
    st = dict(id=i32(B, M), label=i32(B, M), tsu=i32(B, M), hits=i32(B, M), box=f32(B * M + 1, 4), vel=f32(B * M + 1, 4), next_id=i32(B), status=i32(B))
    ids = i32(B, T)
    base = dict(s=s.data_ptr(), l=l.data_ptr(), bx=bx.data_ptr(), c=c.data_ptr(), B=B, T=T, **{k: v.data_ptr() for k, v in st.items()}, M=M,
                high=0.5, low=0.1, new=0.6, iou1=0.2, iou2=0.5, buf=30, hits_min=1, alpha=0.5, ids=ids.data_ptr())
    order = ["s", "l", "bx", "c", "B", "T", "id", "label", "tsu", "hits", "box", "vel", "next_id", "status", "M", "high", "low", "new", "iou1", "iou2",
             "buf", "hits_min", "alpha", "ids"]
    call = lambda **k: lib.fx_track_update(*[dict(base, **k)[n] for n in order], _stream())      # noqa: E731
    nan = float("nan")
    bad = [{p: None} for p in ("s", "l", "bx", "c", "id", "label", "tsu", "hits", "box", "vel", "next_id", "status", "ids")]
    bad += [dict(s=base["s"] + 2), dict(bx=base["bx"] + 4), dict(box=base["box"] + 8), dict(vel=base["vel"] + 4), dict(ids=base["ids"] + 1),
            dict(B=0), dict(B=65536), dict(T=0), dict(T=1025), dict(M=0), dict(M=1025), dict(low=0.0), dict(low=0.6), dict(high=1.5, new=2.0),
            dict(new=0.4), dict(iou1=0.0), dict(iou1=1.5), dict(iou2=0.0), dict(iou2=nan), dict(buf=-1), dict(hits_min=0), dict(alpha=-0.1),
            dict(alpha=nan), dict(high=nan), dict(low=nan), dict(new=nan)]
    for k in bad:
        assert call(**k) == INVALID, k
    rorder = ["id", "label", "tsu", "hits", "box", "vel", "next_id", "status", "B", "M", "b"]
    rcall = lambda **k: lib.fx_track_reset(*[dict(dict(base, b=0), **k)[n] for n in rorder], _stream())      # noqa: E731
    for k in [{p: None} for p in rorder[:8]] + [dict(b=B), dict(b=-2), dict(B=0), dict(M=1025), dict(box=base["box"] + 4)]:
        assert rcall(**k) == INVALID, k
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and all(bool((v == -7).all()) for v in st.values())
    # the same arguments unbroken run: reset, then one update
    assert rcall(b=-1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((st["box"][-1] == -7.0).all()) and bool((st["vel"][-1] == -7.0).all())      # the canary slot past the last stream
    assert int(st["next_id"].min()) >= 1 and bool((ids >= -1).all())


def test_device_tracker_refuses_other_batch_sizes_and_layouts():
    trk = DeviceTracker(2, TrackerConfig(max_tracks=4), DEV)
    s, l, bx, c = [_dev(a) for a in sequence(3, 2, 8, 1)[0]]
    before = trk.state()
    s3, l3, bx3, c3 = [_dev(a) for a in sequence(3, 3, 8, 1)[0]]
    for args in ((s3, l3, bx3, c3), (s, l.to(torch.int64), bx, c), (s, l, bx[:, :, :2], c), (s.cpu(), l, bx, c), (s, l, bx, c[:1])):
        with pytest.raises(ValueError):
            trk.update(*args)
    _same_state(trk.state(), before, "refused")


# ---------------------------------------------------------------- (d) the public interface
SIZE = 128


@pytest.fixture(scope="module")
def detr():
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        fm = ModelManager.get("fai-detr-m-coco", device=DEV, seed=3)
    fm.processor.image_size = SIZE
    return fm


def _dets(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label, d.mask) for d in res.detections]


def _packed(batch, T=300):
    """One batch of FocoosDetections back as the packed arrays."""
    B = len(batch)
    s, l, bx = np.zeros((B, T), np.float32), np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
    c = np.array([len(r.detections) for r in batch], np.int32)
    for b, r in enumerate(batch):
        for j, d in enumerate(r.detections):
            s[b, j], l[b, j], bx[b, j] = d.conf, d.cls_id, d.bbox
    return s, l, bx, c


def _by_hand(plain, cfg):
    """The ids a DeviceTracker gives when it is stepped over the packed results of ``plain``, as [batch][image][detection] with None for -1;
    the numpy restatement must agree with it."""
    trk, ref, out = DeviceTracker(len(plain[0]), cfg, DEV), R.RefTracker(len(plain[0]), cfg), []
    for batch in plain:
        s, l, bx, c = _packed(batch)
        ids = trk.update(_dev(s), _dev(l), _dev(bx), _dev(c)).cpu().numpy()
        assert np.array_equal(ids, ref.update(s, l, bx, c))
        out.append([[None if i < 0 else int(i) for i in ids[b, :c[b]]] for b in range(len(batch))])
    return out, trk


def _ids(results):
    return [[[d.track_id for d in r.detections] for r in batch] for batch in results]


@pytest.mark.parametrize("cfg", [None, TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)], ids=["defaults", "low"])
def test_infer_stream_and_infer_batch_track_like_a_tracker_stepped_by_hand(detr, cfg):
    """6 batches of 2 frames (stream b sees a slowly changing scene); the detections are those of track=None, field by field, and the ids
    are those of a DeviceTracker stepped by hand - on a second run and through infer_batch(tracker=...) as well."""
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) if j % 3 else synth_image_structured(40 + b + 10 * j, SIZE, SIZE) for b in range(2)]
               for j in range(6)]
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    assert all(d.track_id is None for batch in plain for r in batch for d in r.detections)
    want, hand = _by_hand(plain, cfg or TrackerConfig())
    tracked = sum(i is not None for batch in want for img in batch for i in img)
    print(f"{sum(len(r.detections) for batch in plain for r in batch)} detections in 12 frames, {tracked} with an id, next_id "
          f"{hand.state()['next_id'].tolist()}")
    for run in range(2):
        got = list(detr.infer_stream(iter(batches), threshold=0.05, track=True if cfg is None else cfg))
        assert [[_dets(r) for r in batch] for batch in got] == [[_dets(r) for r in batch] for batch in plain], run
        assert _ids(got) == want, run
    # a DeviceTracker outlives the call: two halves of the sequence through one tracker give the ids of the whole
    trk = DeviceTracker(2, cfg or TrackerConfig(), DEV)
    halves = list(detr.infer_stream(iter(batches[:3]), threshold=0.05, track=trk)) + list(detr.infer_stream(iter(batches[3:]), threshold=0.05, track=trk))
    assert _ids(halves) == want
    _same_state(trk.state(), hand.state(), "halves", skip=("status",))      # infer_stream read and cleared the drop counters
    trk.reset()
    one = [detr.infer_batch(b, threshold=0.05, tracker=trk) for b in batches]
    assert [[_dets(r) for r in batch] for batch in one] == [[_dets(r) for r in batch] for batch in plain]
    assert _ids(one) == want
    if cfg is not None:      # every returned detection scores >= 0.05, so whatever reaches 0.06 with a real box is born at once
        born = any(d.conf >= np.float32(0.06) and d.bbox[2] > d.bbox[0] and d.bbox[3] > d.bbox[1] for r in plain[0] for d in r.detections)
        assert (tracked > 0) == born
    with pytest.raises(ValueError, match="batch"):
        list(detr.infer_stream(iter([batches[0], batches[1][:1]]), threshold=0.05, track=True))
    with pytest.raises(ValueError, match="batch"):
        detr.infer_batch(batches[0][:1], threshold=0.05, tracker=trk)


def test_infer_stream_warns_once_when_births_are_dropped(detr):
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) for b in range(2)] for j in range(3)]
    cfg = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, max_tracks=1)
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    ref = R.RefTracker(2, cfg)
    for batch in plain:
        ref.update(*_packed(batch))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        list(detr.infer_stream(iter(batches), threshold=0.05, track=cfg))
    drops = [x for x in w if "new tracks dropped" in str(x.message)]
    assert len(drops) == (1 if ref.status.any() else 0)
    if drops:
        assert str(int(ref.status.sum())) in str(drops[0].message)
