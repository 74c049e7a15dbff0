"""Tiled inference of video streams on a real MI355X: fx_frames_tile_gather_f32 against fx_frames_ingest followed by
fx_tile_gather_u8_f32 (bit for bit), fx_merge_detections_nms_batched against fx_merge_detections_nms per stream and the numpy restatement
of tests/tiled_ref.py (equality), and infer_stream(tiling=) / infer_batch(tiling=) against the same pieces, the tracker and the zones stepped
by hand.  Nothing here reads the reference tree."""
import ctypes
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import tiled as T
from focoos_amd.frames import Frame, FrameBatch
from focoos_amd.synth import synth_image_structured

from . import frames_ref as FR
from . import tiled_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- gather
GH, GW = 71, 91      # odd extents: the last chroma row and column are read


def _gather_frames():
    """(frames, their RGB bytes by the restatement): NV12 at pitch 96 in one device allocation, I420 on the host (bt709 full), BGR on the
    device in rows padded to 96 pixels."""
    frames, rgbs = [], []
    y, u, v = FR.rgb_to_yuv_planes(synth_image_structured(31, GH, GW), 31)
    uv = np.ascontiguousarray(np.stack([u, v], -1))
    ch, pitch = (GH + 1) // 2, 96
    buf = np.full(pitch * (GH + ch) + 64, 0xA5, np.uint8)
    rows = buf[:pitch * (GH + ch)].reshape(GH + ch, pitch)
    rows[:GH, :GW] = y
    rows[GH:, :uv.shape[1] * 2] = uv.reshape(ch, -1)
    frames.append(Frame.from_nv12(torch.from_numpy(buf).to(DEV), GH, GW, pitch)), rgbs.append(FR.to_rgb("nv12", [y, uv], GH, GW))
    y, u, v = FR.rgb_to_yuv_planes(synth_image_structured(32, GH, GW), 32)
    frames.append(Frame("i420", [y, u, v], GH, GW, matrix="bt709", range="full")), rgbs.append(FR.to_rgb("i420", [y, u, v], GH, GW, "bt709", "full"))
    bgr = synth_image_structured(33, GH, GW)
    wide = np.full((GH, 96, 3), 0x5A, np.uint8)
    wide[:, :GW] = bgr
    frames.append(Frame.from_bgr(torch.from_numpy(wide).to(DEV)[:, :GW])), rgbs.append(np.ascontiguousarray(bgr[:, :, ::-1]))
    assert frames[2].pitches() == [96 * 3]
    return frames, rgbs


def _gather_windows(Ho, Wo):
    """(x0, y0, w, h): an odd origin, exactly (Ho, Wo), touching the bottom-right corner, narrower than Wo (enlarging), the whole frame."""
    return np.array([[13, 7, 50, 40], [10, 12, Wo, Ho], [GW - 40, GH - 30, 40, 30], [21, 3, 20, 60], [0, 0, GW, GH]], dtype=np.int32)


def _tile_gather(lib, fb, wins, out, S=None, V=None, descs_off=0):
    dev, host = fb._descriptors(DEV)
    wh = torch.from_numpy(wins)
    wd = wh.to(DEV)
    return lib.fx_frames_tile_gather_f32(dev.data_ptr() + descs_off, ctypes.addressof(host), len(fb) if S is None else S, wd.data_ptr(), wh.data_ptr(),
                                         len(wins) if V is None else V, out.data_ptr(), out.shape[1], out.shape[2], _stream())


@pytest.fixture(scope="module")
def gather_frames():
    return _gather_frames()


@pytest.mark.parametrize("Ho,Wo", [(48, 64), (45, 63)], ids=["vec16", "scalar"])
def test_gather_equals_ingest_then_the_single_frame_gather(gather_frames, Ho, Wo):
    lib = _lib.load("bf16")
    frames, rgbs = gather_frames
    assert any(np.any(r == 0) and np.any(r == 255) for r in rgbs[:2])       # noisy chroma: triples that clip occur
    fb = FrameBatch(frames)
    wins = _gather_windows(Ho, Wo)
    S, V = len(fb), len(wins)
    buf = torch.full((S * V + 2, Ho, Wo, 3), -7.0, dtype=torch.float32, device=DEV)     # a canary view on either side
    out = buf[1:S * V + 1]
    assert _tile_gather(lib, fb, wins, out) == 0
    torch.cuda.synchronize()
    assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
    got = out.cpu()
    wh = torch.from_numpy(wins)
    wd = wh.to(DEV)
    dev, host = fb._descriptors(DEV)
    for s in range(S):
        rgb_d = torch.empty(1, GH, GW, 3, dtype=torch.uint8, device=DEV)
        _lib.check(lib.fx_frames_ingest(dev.data_ptr() + 64 * s, ctypes.addressof(host) + 64 * s, 1, rgb_d.data_ptr(), 0, GH, GW, _stream()),
                   "fx_frames_ingest")
        want = torch.empty(V, Ho, Wo, 3, dtype=torch.float32, device=DEV)
        T.gather_views(lib, rgb_d[0], wh, wd, want)
        torch.cuda.synchronize()
        assert np.array_equal(rgb_d[0].cpu().numpy(), rgbs[s]), s
        for v in range(V):
            assert torch.equal(got[s * V + v], want[v].cpu()), (s, frames[s].format, wins[v].tolist())
    # one frame against the restated conversion and the resize of the host crop
    for v, (x0, y0, w, h) in enumerate(wins.tolist()):
        crop = _dev(rgbs[1][y0:y0 + h, x0:x0 + w])
        want = torch.empty(Ho, Wo, 3, dtype=torch.float32, device=DEV)
        _lib.check(lib.fx_resize_bilinear_u8(crop.data_ptr(), h, w, want.data_ptr(), Ho, Wo, _stream()), "fx_resize_bilinear_u8")
        torch.cuda.synchronize()
        assert torch.equal(got[V + v], want.cpu()), (v, (x0, y0, w, h))
    # a window of exactly (Ho, Wo) holds the converted bytes as floats
    assert torch.equal(got[1], torch.from_numpy(rgbs[0][12:12 + Ho, 10:10 + Wo].astype(np.float32)))
    # the host wrapper is that call
    again = torch.empty(S * V, Ho, Wo, 3, dtype=torch.float32, device=DEV)
    T.gather_stream_views(lib, fb, DEV, wh, wd, again)
    assert torch.equal(again.cpu(), got)


def test_gather_refuses_bad_arguments_and_writes_nothing(gather_frames):
    lib = _lib.load("bf16")
    frames, _ = gather_frames
    fb = FrameBatch(frames)
    out = torch.full((6, 48, 64, 3), -7.0, dtype=torch.float32, device=DEV)
    good = [0, 0, 64, 48]
    for bad in ([GW - 63, 0, 64, 48], [0, GH - 47, 64, 48], [-1, 0, 64, 48], [0, 0, 0, 48], [0, 0, GW + 1, 48]):      # a window leaving the frame
        assert _tile_gather(lib, fb, np.array([good, bad], dtype=np.int32), out) == INVALID, bad
    two = FrameBatch([frames[0], Frame.from_rgb(synth_image_structured(1, GH, GW + 1))])                                 # frames of two sizes
    assert _tile_gather(lib, two, np.array([good], dtype=np.int32), out) == INVALID
    many = np.tile(np.array([good], dtype=np.int32), (21846, 1))                                                         # 3 x 21846 = 65538 views
    assert _tile_gather(lib, fb, many, out) == INVALID
    one = np.array([good], dtype=np.int32)
    assert _tile_gather(lib, fb, one, out, descs_off=4) == INVALID                                                       # misaligned descs
    assert _tile_gather(lib, fb, one, out, S=0) == INVALID and _tile_gather(lib, fb, one, out, V=0) == INVALID
    dev, host = fb._descriptors(DEV)
    wh = torch.from_numpy(one)
    wd = wh.to(DEV)
    args = lambda **k: [k.get("dev", dev.data_ptr()), k.get("host", ctypes.addressof(host)), 3, k.get("wd", wd.data_ptr()), k.get("wh", wh.data_ptr()),
                        1, k.get("out", out.data_ptr()), k.get("Ho", 48), k.get("Wo", 64), _stream()]
    for k in (dict(dev=None), dict(host=None), dict(wd=None), dict(wh=None), dict(out=None), dict(Ho=0), dict(Wo=16385), dict(wd=wd.data_ptr() + 2),
              dict(out=out.data_ptr() + 2)):
        assert lib.fx_frames_tile_gather_f32(*args(**k)) == INVALID, k
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.fx_frames_tile_gather_f32(*args()) == 0          # the same arguments unbroken run
    torch.cuda.synchronize()
    assert bool((out[:3] != -7.0).all()) and bool((out[3:] == -7.0).all())


# ---------------------------------------------------------------- batched merge
FRAME = 512
TOTALS = [0, 1, 5, 64, 65, 130]


def _split(rs, M, V, Tk):
    """M candidates over V views of Tk slots, raggedly: a multinomial draw, its overflow moved to the views with room."""
    assert M <= V * Tk
    c = rs.multinomial(M, np.ones(V) / V).astype(np.int64)
    for v in range(V):
        while c[v] > Tk:
            room = [u for u in range(V) if c[u] < Tk]
            c[v] -= 1
            c[room[0]] += 1
    return c.astype(np.int32)


def _stream_case(rs, M, V, Tk, pool, labels_n):
    """One stream: boxes drawn from a pool of ``pool`` (so duplicates occur), ``labels_n`` labels, few distinct scores (ties), garbage with
    high scores in the slots past the count."""
    count = _split(rs, M, V, Tk)
    xy = rs.randint(-10, 320, (pool, 2))
    boxes_pool = np.concatenate([xy, xy + rs.randint(1, 220, (pool, 2))], -1).astype(np.int32)
    boxes = boxes_pool[rs.randint(0, pool, (V, Tk))]
    labels = rs.randint(0, labels_n, (V, Tk)).astype(np.int32)
    scores = (rs.randint(1, 24, (V, Tk)) / np.float32(24)).astype(np.float32)
    for v in range(V):
        scores[v, count[v]:] = 2.0
    return scores, labels, boxes, count


def _batched_case(seed, totals, V, Tk, pool=12, labels_n=2):
    """S = len(totals) streams of V views sharing one window list: arrays [S * V][Tk] and the windows."""
    rs = np.random.RandomState(seed)
    wins = np.concatenate([rs.randint(0, 200, (V, 2)), np.full((V, 2), 320)], 1).astype(np.int32)
    parts = [_stream_case(rs, M, V, Tk, pool, labels_n) for M in totals]
    return tuple(np.concatenate([p[i] for p in parts], 0) for i in range(4)) + (wins,)


def _run_batched(lib, case, S, V, thr, metric, D):
    d = [_dev(a) for a in case]
    status = torch.zeros(S, dtype=torch.int32, device=DEV)
    res = T.merge_batched(lib, d[0], d[1], d[2], d[3], d[4], S, V, (FRAME, FRAME), T.Tiling(merge_threshold=thr, merge_metric=metric, max_detections=D),
                          status)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (res.det_scores, res.det_labels, res.det_boxes, res.det_count, status)]


def _check_batched(lib, case, S, V, thr, metric, D):
    """Stream s of the batched call == fx_merge_detections_nms on its own views == tiled_ref.merge.  Returns the reference's (kept, total)."""
    scores, labels, boxes, count, wins = case
    gs, gl, gb, gc, gst = _run_batched(lib, case, S, V, thr, metric, D)
    d = [_dev(a) for a in case]
    stats = []
    for s in range(S):
        sl = slice(s * V, (s + 1) * V)
        o_s, o_l, o_b, cs = T.merge_detections(lib, d[0][sl], d[1][sl], d[2][sl], d[3][sl], d[4], V, (FRAME, FRAME), thr, metric, D)
        torch.cuda.synchronize()
        assert np.array_equal(gs[s], o_s[0].cpu().numpy()) and np.array_equal(gl[s], o_l[0].cpu().numpy()), s
        assert np.array_equal(gb[s], o_b[0].cpu().numpy()) and [int(gc[s]), int(gst[s])] == cs.cpu().tolist(), s
        ws, wl, wb, dropped = R.merge(scores[sl], labels[sl], boxes[sl], count[sl], wins, (FRAME, FRAME), thr, metric, D)
        k = len(ws)
        assert int(gc[s]) == k and int(gst[s]) == dropped, (s, int(gc[s]), k, int(gst[s]), dropped)
        assert np.array_equal(gs[s, :k], ws) and np.array_equal(gl[s, :k], wl) and np.array_equal(gb[s, :k], wb), s
        assert not gs[s, k:].any() and not gl[s, k:].any() and not gb[s, k:].any(), s       # slots past the count are zero
        stats.append((len(R.merge(scores[sl], labels[sl], boxes[sl], count[sl], wins, (FRAME, FRAME), thr, metric, 10_000)[0]), int(count[sl].sum())))
    return stats


@pytest.mark.parametrize("V", [1, 3, 7])
@pytest.mark.parametrize("S", [1, 3])
def test_batched_merge_equals_the_single_frame_merge_per_stream(S, V):
    lib = _lib.load("bf16")
    Tk = 64
    fit = [M for M in TOTALS if M <= V * Tk]           # one view of 64 slots holds at most 64 candidates
    suppressed = 0
    for r in range(len(fit)):                          # every total is the first stream's once; every stream differs from its neighbour
        totals = [fit[(r + s) % len(fit)] for s in range(S)]
        assert all(a != b for a, b in zip(totals, totals[1:]))
        case = _batched_case(1000 * S + 100 * V + r, totals, V, Tk)
        assert len(set(case[1].ravel().tolist())) == 2                                      # both labels occur
        for metric, thr in (("iou", 0.5), ("ios", 0.8)):
            stats = _check_batched(lib, case, S, V, thr, metric, 300)
            assert [t for _, t in stats] == totals
            assert all(k < t for k, t in stats if t >= 64)                                  # 24 (box, label) pairs: 64 candidates repeat some
            suppressed += sum(k < t for k, t in stats)
    assert suppressed > 0                                                                    # by the reference's own counts


def test_batched_merge_cap_is_per_stream_and_nothing_leaks():
    """Stream 0 is full (5 x 1024 candidates, 1024 beyond the cap), stream 1 has 10."""
    lib = _lib.load("bf16")
    S, V, Tk = 2, 5, 1024
    case = _batched_case(7, [V * Tk, 10], V, Tk, pool=400, labels_n=5)
    assert case[3][:V].tolist() == [Tk] * V and int(case[3][V:].sum()) == 10
    stats = _check_batched(lib, case, S, V, 0.5, "iou", 300)
    st = _run_batched(lib, case, S, V, 0.5, "iou", 300)[4]
    assert st.tolist() == [1024, 0] and stats[1][1] == 10 and stats[1][0] <= 10


def test_batched_merge_max_detections_below_the_survivors():
    lib = _lib.load("bf16")
    case = _batched_case(11, [130, 65, 5], 3, 64, pool=60)
    full = _check_batched(lib, case, 3, 3, 0.5, "iou", 300)
    assert full[0][0] > 7 and full[1][0] > 7 and full[2][0] <= 7
    assert _run_batched(lib, case, 3, 3, 0.5, "iou", 7)[3].tolist() == [7, 7, full[2][0]]
    _check_batched(lib, case, 3, 3, 0.5, "iou", 7)
    _check_batched(lib, case, 3, 3, 0.5, "iou", 1)


def test_batched_merge_refuses_bad_arguments_and_writes_nothing():
    lib = _lib.load("bf16")
    S, V, Tk, D = 2, 2, 8, 4
    scores, labels, boxes, count, wins = [_dev(a) for a in _batched_case(1, [6, 3], V, Tk)]
    o_s = torch.full((S, D), -7.0, dtype=torch.float32, device=DEV)
    o_l = torch.full((S, D), -7, dtype=torch.int32, device=DEV)
    o_b = torch.full((S * D + 1, 4), -7, dtype=torch.int32, device=DEV)
    o_c = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    need = int(lib.fx_merge_detections_batched_workspace_bytes(S, V, Tk))
    assert need == S * int(lib.fx_merge_detections_workspace_bytes(V, Tk)) == S * 2_195_472 and need % 16 == 0
    for bad in ((0, V, Tk), (S, 0, Tk), (S, V, 0), (65536, 1, 1), (1 << 15, 1 << 8, 1 << 8), (2, 1 << 16, 1 << 15)):
        assert lib.fx_merge_detections_batched_workspace_bytes(*bad) == 0, bad
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    base = dict(scores=scores.data_ptr(), labels=labels.data_ptr(), boxes=boxes.data_ptr(), count=count.data_ptr(), wins=wins.data_ptr(), S=S, V=V,
                T=Tk, H=FRAME, W=FRAME, thr=0.5, metric=0, D=D, o_s=o_s.data_ptr(), o_l=o_l.data_ptr(), o_b=o_b.data_ptr(), o_c=o_c.data_ptr(),
                st=st.data_ptr(), ws=ws.data_ptr(), wsb=need)
    order = ["scores", "labels", "boxes", "count", "wins", "S", "V", "T", "H", "W", "thr", "metric", "D", "o_s", "o_l", "o_b", "o_c", "st", "ws", "wsb"]
    call = lambda **k: lib.fx_merge_detections_nms_batched(*[dict(base, **k)[n] for n in order], _stream())
    bad = [{p: None} for p in ("scores", "labels", "boxes", "count", "wins", "o_s", "o_l", "o_b", "o_c", "st", "ws")]
    bad += [dict(scores=base["scores"] + 2), dict(o_b=base["o_b"] + 4), dict(ws=base["ws"] + 8), dict(wsb=need - 1), dict(S=0), dict(S=65536),
            dict(V=0), dict(T=0), dict(S=1 << 15, V=1 << 8, T=1 << 8), dict(H=0), dict(W=16385), dict(thr=0.0), dict(thr=1.5), dict(metric=2),
            dict(D=0)]
    for k in bad:
        assert call(**k) == INVALID, k
    torch.cuda.synchronize()
    assert bool((o_s == -7.0).all()) and bool((o_l == -7).all()) and bool((o_b == -7).all()) and bool((o_c == -7).all()) and bool((st == -7).all())
    st.zero_()
    assert call() == 0                      # the same arguments unbroken run
    torch.cuda.synchronize()
    assert all(1 <= int(c) <= D for c in o_c.tolist()) and st.tolist() == [0, 0] and bool((o_b[S * D:] == -7).all())


# ---------------------------------------------------------------- end to end
EH, EW = 200, 260
THR = 0.01
TILING = T.Tiling(tile=128, overlap=0.25, batch_size=4)


def _regions():
    from focoos_amd.zones import Line, Zone

    return [Zone("mid", [(40, 40), (220, 40), (220, 180), (40, 180)]), Line("gate", (130, 0), (130, 200))]


def _tracker_config():
    from focoos_amd.tracking import TrackerConfig

    return TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)


def _frame_batches():
    """Three frame batches of S = 2 frames of 200 x 260, stream 0 as NV12 (host planes) and stream 1 as an RGB array; batch 1 repeats batch
    0's pictures (so tracks persist), batch 2 differs.  Returns ([inputs of a batch], [their RGB bytes])."""
    batches, rgbs = [], []
    for j in (0, 0, 1):
        y, u, v = FR.rgb_to_yuv_planes(synth_image_structured(40 + j, EH, EW), 40 + j)
        uv = np.ascontiguousarray(np.stack([u, v], -1))
        rgb = synth_image_structured(50 + j, EH, EW)
        batches.append([Frame("nv12", [y, uv], EH, EW), rgb])
        rgbs.append([FR.to_rgb("nv12", [y, uv], EH, EW), rgb])
    return batches, rgbs


def _dets(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label, d.track_id) for d in res.detections]


@pytest.fixture(scope="module")
def detr():
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get("fai-detr-m-coco", device=DEV, seed=3)


@pytest.fixture(scope="module")
def expected(detr):
    """The hand-composed reference of the three frame batches: the new gather's views through model.detect in chunks of 4, tiled_ref.merge per
    stream, then a DeviceTracker, a DeviceZones and the overlay stepped over the merged packed arrays.  Per batch: the detections and zone
    dicts of both streams and the drawn pictures."""
    from focoos_amd.annotate import Overlay, OverlayPass, annotator_of
    from focoos_amd.tracking import DeviceTracker
    from focoos_amd.zones import DeviceZones

    lib = _lib.load("bf16")
    fm = detr
    classes = fm.model_info.classes
    batches, rgbs = _frame_batches()
    wins = T.views_of(EH, EW, 128, 128, 0.25, True)
    S, V, D = 2, len(wins), 300
    assert V == 7 and wins[-1].tolist() == [0, 0, EW, EH]            # 3 x 2 windows + the whole frame: 14 views in 4 chunks of 4
    wh = torch.from_numpy(wins)
    wd = wh.to(DEV)
    sizes = np.full((16, 2), 128, dtype=np.int32)
    sizes[:14] = np.concatenate([wins[:, [3, 2]]] * 2, 0)
    trk = DeviceTracker(S, _tracker_config(), DEV)
    zon = DeviceZones(S, _regions(), tracker=trk, device=DEV)
    ann = annotator_of(fm)
    out = []
    for inputs, rgb in zip(batches, rgbs):
        views = torch.zeros(16, 128, 128, 3, dtype=torch.float32, device=DEV)
        T.gather_stream_views(lib, T.stream_frames(inputs, "test"), DEV, wh, wd, views)
        parts = []
        for c0 in range(0, 16, 4):
            pl = fm.model.detect(views[c0:c0 + 4], sizes=torch.from_numpy(sizes[c0:c0 + 4]).to(DEV), threshold=THR)
            torch.cuda.synchronize()
            parts.append([t.cpu().numpy().copy() for t in (pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)])
        s, l, b, c = (np.concatenate([p[i] for p in parts], 0)[:14] for i in range(4))
        ps, plab, pb, pc = np.zeros((S, D), np.float32), np.zeros((S, D), np.int32), np.zeros((S, D, 4), np.int32), np.zeros(S, np.int32)
        cands = []
        for st in range(S):
            sl = slice(st * V, (st + 1) * V)
            ws, wl, wb, dropped = R.merge(s[sl], l[sl], b[sl], c[sl], wins, (EH, EW), 0.5, "iou", D)
            k = len(ws)
            ps[st, :k], plab[st, :k], pb[st, :k], pc[st] = ws, wl, wb, k
            cands.append(int(c[sl].sum()))
            assert dropped == 0
        res = SimpleNamespace(det_scores=_dev(ps), det_labels=_dev(plab), det_boxes=_dev(pb), det_count=_dev(pc))
        ids = trk.update(res.det_scores, res.det_labels, res.det_boxes, res.det_count)
        zon.update(res.det_labels, res.det_boxes, res.det_count, ids)
        zd = zon.fetch()
        idl = ids.cpu().tolist()
        dets = [[(tuple(int(x) for x in pb[st, i]), float(ps[st, i]), int(plab[st, i]), classes[int(plab[st, i])],
                  None if idl[st][i] < 0 else idl[st][i]) for i in range(int(pc[st]))] for st in range(S)]
        drawn = ann.annotate_overlay(_dev(np.stack(rgb, 0)), res, 0, OverlayPass(Overlay(ids=True, zones=True), ids, zon, None, None))
        torch.cuda.synchronize()
        out.append(SimpleNamespace(dets=dets, zones=zd, images=drawn.cpu().numpy(), candidates=cands, rgb=rgb))
    return out


def test_the_hand_composed_reference_has_work_in_it(expected):
    """Otherwise the equalities below prove nothing: the merge has candidates to suppress, both streams keep several detections, and at
    least one id lives through two frames."""
    for j, e in enumerate(expected):
        print(f"batch {j}: candidates {e.candidates}, survivors {[len(d) for d in e.dets]}, "
              f"ids {[sum(t[4] is not None for t in d) for d in e.dets]}, best score {[max((t[1] for t in d), default=0) for d in e.dets]}")
    for e in expected:
        assert all(c > 7 for c in e.candidates) and all(len(d) > 1 for d in e.dets)
        assert all(len(d) < c for d, c in zip(e.dets, e.candidates))
    for s in range(2):
        first = {t[4] for t in expected[0].dets[s] if t[4] is not None}
        second = {t[4] for t in expected[1].dets[s] if t[4] is not None}
        assert first & second, (s, first, second)
    assert any(z["mid"]["count"] > 0 for e in expected for z in e.zones)
    assert any(not np.array_equal(e.images[s], e.rgb[s]) for e in expected for s in range(2))


def test_infer_stream_tiled_equals_the_pieces_composed_by_hand(detr, expected):
    batches, _ = _frame_batches()
    got = list(detr.infer_stream(iter(batches), threshold=THR, tiling=TILING, track=_tracker_config(), zones=_regions()))
    assert len(got) == 3 and all(len(g) == 2 for g in got)
    for g, e in zip(got, expected):
        assert [_dets(r) for r in g] == e.dets
        assert [r.zones for r in g] == e.zones


def test_infer_batch_tiled_equals_the_pieces_composed_by_hand(detr, expected):
    from focoos_amd.tracking import DeviceTracker
    from focoos_amd.zones import DeviceZones

    batches, _ = _frame_batches()
    trk = DeviceTracker(2, _tracker_config(), DEV)
    zon = DeviceZones(2, _regions(), tracker=trk, device=DEV)
    for inputs, e in zip(batches, expected):
        g = detr.infer_batch(inputs, threshold=THR, tiling=TILING, tracker=trk, zones=zon)
        assert [_dets(r) for r in g] == e.dets
        assert [r.zones for r in g] == e.zones
        assert g[0].latency is not None and g[0].latency.inference > 0


def test_analytics_only_mode_gives_the_same_zone_dicts(detr, expected):
    batches, _ = _frame_batches()
    got = list(detr.infer_stream(iter(batches), threshold=THR, tiling=TILING, track=_tracker_config(), zones=_regions(), detections=False))
    for g, e in zip(got, expected):
        assert all(r.detections == [] for r in g)
        assert [r.zones for r in g] == e.zones


def test_one_stream_equals_infer_tiled(detr):
    frame = synth_image_structured(50, EH, EW)
    want = detr.infer_tiled(frame, tile=128, overlap=0.25, threshold=THR, batch_size=4)
    got = detr.infer_batch([frame], threshold=THR, tiling=T.Tiling(tile=128, overlap=0.25, batch_size=4))[0]
    assert len(want.detections) > 1 and _dets(got) == _dets(want)
    streamed = list(detr.infer_stream(iter([[frame]]), threshold=THR, tiling=T.Tiling(tile=128, overlap=0.25, batch_size=4)))
    assert _dets(streamed[0][0]) == _dets(want)


def test_overlay_is_drawn_on_the_full_size_frames(detr, expected):
    from focoos_amd.annotate import Overlay

    batches, _ = _frame_batches()
    got = list(detr.infer_stream(iter(batches), threshold=THR, tiling=TILING, track=_tracker_config(), zones=_regions(),
                                 annotate=Overlay(ids=True, zones=True)))
    for g, e in zip(got, expected):
        assert [_dets(r) for r in g] == e.dets
        for s, r in enumerate(g):
            assert r.image.shape == (EH, EW, 3) and r.image.dtype == np.uint8
            assert np.array_equal(r.image, e.images[s]), s
