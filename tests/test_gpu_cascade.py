"""A second model on every detected object, on a real MI355X: fx_roi_select and fx_roi_attributes against the numpy
restatement of tests/cascade_ref.py (equality), fx_frames_roi_gather_f32 against fx_frames_tile_gather_f32 called per frame and window (bit
for bit), and infer_stream(classify=) / infer_batch(classify=) against the same pieces composed by hand.  Nothing here reads the reference
tree."""
import ctypes
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import cascade as CS
from focoos_amd import tiled as T
from focoos_amd.frames import Frame, FrameBatch
from focoos_amd.synth import synth_image_structured

from . import cascade_ref as R
from . import frames_ref as FR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------- select
SEL_SIZES = [(100, 200), (64, 48), (300, 300)]      # (H, W) per stream
SEL_M = 8
# a small pool, so equal scores and equal boxes occur: inside, at the edges, partly and wholly outside the smallest frame, too small, inverted
SEL_BOXES = np.array([[10, 10, 40, 50], [0, 0, 30, 20], [30, 40, 48, 64], [40, 50, 90, 120], [150, 70, 260, 130], [60, 70, 90, 90],
                      [5, 5, 11, 40], [20, 20, 10, 10], [12, 8, 44, 30]], dtype=np.int32)
SEL_SCORES = np.array([0.2, 0.5, 0.5, 0.9, 0.35], dtype=np.float32)
SEL_LABELS = np.array([0, 1, 2, 40, 1], dtype=np.int32)
SEL_WORDS = np.array([0b110], dtype=np.uint32)      # labels 1 and 2; 40 lies outside the words
SEL_SEED = 104      # chosen so that the reference has the work in it that test_the_select_reference_has_work_in_it asks for


def _select_frames(T_, tracked, seed):
    """Four consecutive frames of S = 3 streams: per frame (scores, labels, boxes, count, track_ids, trk_id).  The counts rotate over
    {0, 1, T} (T, 1, T, 0, shifted by one per stream, so every stream has two full frames); the slots past a count hold garbage; the
    tracker's table keeps its ids, so records age."""
    rng = np.random.default_rng(seed)
    S = len(SEL_SIZES)
    trk = np.stack([rng.permutation(np.array([1, 2, 3, 4, 5, 6, 0, 0], np.int32)) for _ in range(S)])
    frames = []
    for f in range(4):
        count = np.array([(T_, 1, T_, 0)[(s + f) % 4] for s in range(S)], np.int32)
        boxes = SEL_BOXES[rng.integers(0, len(SEL_BOXES), (S, T_))].copy()
        scores = SEL_SCORES[rng.integers(0, len(SEL_SCORES), (S, T_))].copy()
        labels = SEL_LABELS[rng.integers(0, len(SEL_LABELS), (S, T_))].copy()
        ids = rng.choice(np.array([-1, 1, 2, 3, 4, 5, 6, 9], np.int32), (S, T_)).astype(np.int32)      # duplicates, and 9 has no slot
        for s in range(S):
            ids[s, :min(T_, 4)] = rng.permutation(np.array([1, 2, 3, 4, 5, 6], np.int32))[:min(T_, 4)]     # the same few tracks lead every frame
            if T_ == 5:      # five tracks that stay, in boxes and classes that pass: what is cropped when is then a matter of staleness
                ids[s], boxes[s], labels[s] = [1, 2, 3, 4, 5], SEL_BOXES[0], 1
        for s in range(S):
            n = int(count[s])
            boxes[s, n:] = rng.integers(-2 ** 31, 2 ** 31 - 1, (T_ - n, 4))
            scores[s, n:] = np.nan
            labels[s, n:] = rng.integers(-2 ** 31, 2 ** 31 - 1, T_ - n)
            ids[s, n:] = rng.integers(-5, 12, T_ - n)
        if f == 2:
            trk[:, 0] = np.where(trk[:, 0] == 0, 7, 0)      # a slot changes hands
        frames.append((scores, labels, boxes, count, ids if tracked else None, trk.copy() if tracked else None))
    return frames


def _select_params(K, words):
    """``interval`` 2 with one crop per frame, 1 with four: both ways some records are older than others by the fourth frame."""
    return dict(K=K, pad_q=38, min_size=8, min_score=0.3, interval=2 if K == 1 else 1, words=SEL_WORDS if words else None)


def _select_reference(T_, K, tracked, words):
    """The reference over the four frames with the state carried: per frame (inputs, state before, outputs).  The state advances by the
    reference's own attribute step on fixed logits."""
    S, M = len(SEL_SIZES), SEL_M if tracked else 1
    state = R.new_state(S, M)
    rng = np.random.default_rng(7)
    out = []
    for fr in _select_frames(T_, tracked, SEL_SEED + T_):
        scores, labels, boxes, count, ids, trk = fr
        before = {k: v.copy() for k, v in state.items()}
        res = R.select(scores, labels, boxes, count, SEL_SIZES, state, track_ids=ids, trk_id=trk, **_select_params(K, words))
        out.append((fr, before, res))
        logits = rng.integers(-3, 4, (S * K, 3)).astype(np.float32)
        R.attributes(logits, res[1], res[2], count, T_, state, K, 0, ids, trk)
    return out


SEL_CASES = [(T_, K, tracked, words) for T_ in (5, 70, 300) for K in (1, 4) for tracked in (True, False) for words in (True, False)]


def test_the_select_reference_has_work_in_it():
    """Checked on the reference alone: budgets that overflow, streams without an eligible detection, and a stale track that outranks a
    fresh detection of a higher score."""
    left = empty = outranked = 0
    for T_, K, tracked, words in SEL_CASES:
        for (scores, labels, boxes, count, ids, trk), before, (win, det, cnt, lft) in _select_reference(T_, K, tracked, words):
            left += int((lft > 0).sum())
            empty += int(((cnt == 0) & (count > 0)).sum())
            # the whole ranking (K = T): a selected track with a record that stands before a track with a younger record and a higher score
            p = {**_select_params(K, words), "K": T_}
            full = R.select(scores, labels, boxes, count, SEL_SIZES, before, track_ids=ids, trk_id=trk, **p)[1]
            for s in range(len(SEL_SIZES)):
                f = int(before["frame"][s]) + 1
                slot = R.owners(None if ids is None else ids[s], None if trk is None else trk[s], int(count[s]))
                order = [int(j) for j in full[s] if j >= 0]
                assert order[:K] == [int(j) for j in det[s] if j >= 0]
                recorded = [j for j in order if j in slot and before["at_id"][s, slot[j]] == ids[s, j]]
                for a, j in enumerate(recorded):
                    for q in recorded[a + 1:]:
                        if order.index(j) < K and scores[s, j] < scores[s, q]:
                            assert f - before["at_frame"][s, slot[j]] > f - before["at_frame"][s, slot[q]]
                            outranked += 1
    print(f"select reference: {left} stream-frames left something out, {empty} had detections but none eligible, {outranked} stale-before-fresh pairs")
    assert left > 0 and empty > 0 and outranked > 0


def _call_select(lib, fb, fr, state, T_, M, K, pad_q, min_size, min_score, interval, words, out, **over):
    scores, labels, boxes, count, ids, trk = fr
    descs, host = fb._descriptors(DEV)
    keep = [_dev(scores), _dev(labels), _dev(boxes), _dev(count), None if ids is None else _dev(ids), None if trk is None else _dev(trk),
            _dev(state["at_id"]), _dev(state["at_frame"]), _dev(state["frame"]), None if words is None else _dev(words.view(np.int32))]
    a = dict(scores=_ptr(keep[0]), labels=_ptr(keep[1]), boxes=_ptr(keep[2]), count=_ptr(keep[3]), S=len(count), T=T_, ids=_ptr(keep[4]),
             trk=_ptr(keep[5]), M=M, at_id=_ptr(keep[6]), at_frame=_ptr(keep[7]), frame=_ptr(keep[8]), descs=descs.data_ptr(),
             host=ctypes.addressof(host), words=_ptr(keep[9]), n_words=0 if words is None else len(words), K=K, pad_q=pad_q, min_size=min_size,
             min_score=min_score, interval=interval, win=out[0].data_ptr(), det=out[1].data_ptr(), cnt=out[2].data_ptr(), left=out[3].data_ptr())
    a.update(over)
    rc = lib.fx_roi_select(a["scores"], a["labels"], a["boxes"], a["count"], a["S"], a["T"], a["ids"], a["trk"], a["M"], a["at_id"], a["at_frame"],
                           a["frame"], a["descs"], a["host"], a["words"], a["n_words"], a["K"], a["pad_q"], a["min_size"], a["min_score"],
                           a["interval"], a["win"], a["det"], a["cnt"], a["left"], _stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def select_frames():
    return FrameBatch([Frame.from_rgb(torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)) for h, w in SEL_SIZES])


def _select_out(S, K, fill=-7):
    i32 = dict(dtype=torch.int32, device=DEV)
    return (torch.full((S, K, 4), fill, **i32), torch.full((S, K), fill, **i32), torch.full((S,), fill, **i32), torch.full((S,), fill, **i32))


@pytest.mark.parametrize("T_,K,tracked,words", SEL_CASES)
def test_select_equals_the_reference_over_four_frames(select_frames, T_, K, tracked, words):
    lib = _lib.load("bf16")
    S, M = len(SEL_SIZES), SEL_M if tracked else 1
    p = _select_params(K, words)
    for f, (fr, before, want) in enumerate(_select_reference(T_, K, tracked, words)):
        out = _select_out(S, K)
        assert _call_select(lib, select_frames, fr, before, T_, M, out=out, **p) == 0
        for name, g, w in zip(("roi_win", "roi_det", "roi_count", "roi_left"), out, want):
            assert np.array_equal(g.cpu().numpy(), w), (f, name, g.cpu().numpy().tolist(), w.tolist())


def test_select_refuses_bad_arguments_and_writes_nothing(select_frames):
    lib = _lib.load("bf16")
    T_, K = 5, 4
    fr, before, _ = _select_reference(T_, K, True, True)[1]
    out = _select_out(3, K)
    p = _select_params(K, True)
    call = lambda **k: _call_select(lib, select_frames, fr, before, T_, out=out, **{**p, "M": SEL_M, **k})      # noqa: E731
    base = dict(boxes=_dev(fr[2]).data_ptr())
    bad = [{n: None} for n in ("scores", "labels", "boxes", "count", "at_id", "at_frame", "frame", "descs", "host", "win", "det", "cnt", "left")]
    bad += [dict(ids=None), dict(trk=None), dict(S=0), dict(S=65536), dict(T=0), dict(T=1025), dict(M=0), dict(M=1025), dict(K=0), dict(K=65),
            dict(pad_q=-1), dict(pad_q=257), dict(min_size=0), dict(interval=0), dict(min_score=float("nan")), dict(n_words=0), dict(n_words=257),
            dict(boxes=base["boxes"] + 4), dict(win=out[0].data_ptr() + 4), dict(det=out[1].data_ptr() + 2),
            dict(descs=select_frames._descriptors(DEV)[0].data_ptr() + 4)]
    for k in bad:
        assert call(**k) == INVALID, k
    broken = (_lib.FxFrameDesc * 3).from_buffer_copy(bytes(select_frames._descriptors(DEV)[1]))
    broken[1].width = 0
    assert call(host=ctypes.addressof(broken)) == INVALID
    assert all(bool((o == -7).all()) for o in out)
    assert call() == 0 and int(out[2].sum()) > 0      # the same arguments unbroken run


# ---------------------------------------------------------------- gather
GUARD = 8      # rows of known bytes above and below every device plane: a wrong clamp of a few pixels still reads allocated memory


def _guarded(plane, pitch):
    """``plane`` [h, w(, c)] as a view into a larger device allocation of rows of ``pitch`` bytes, GUARD rows of 0xA5 on either side."""
    h, row = plane.shape[0], int(np.prod(plane.shape[1:]))
    big = np.full((h + 2 * GUARD, pitch), 0xA5, np.uint8)
    big[GUARD:GUARD + h, :row] = plane.reshape(h, row)
    d = torch.from_numpy(big).to(DEV)
    view = d[GUARD:GUARD + h, :row]
    return view if plane.ndim == 2 else view.unflatten(1, plane.shape[1:])


def _roi_frames():
    """71 x 91 NV12 at pitch 96 on the device, 50 x 64 I420 bt709-full on the host, 40 x 40 BGR on the device in rows of 48 pixels; the
    device planes are sub-rectangles of guarded allocations."""
    y, u, v = FR.rgb_to_yuv_planes(synth_image_structured(61, 71, 91), 61)
    uv = np.ascontiguousarray(np.stack([u, v], -1))
    nv12 = Frame("nv12", [_guarded(y, 96), _guarded(uv, 96)], 71, 91)
    y, u, v = FR.rgb_to_yuv_planes(synth_image_structured(62, 50, 64), 62)
    i420 = Frame("i420", [y, u, v], 50, 64, matrix="bt709", range="full")
    bgr = Frame.from_bgr(_guarded(synth_image_structured(63, 40, 40), 48 * 3))
    assert nv12.pitches() == [96, 96] and bgr.pitches() == [144]
    return [nv12, i420, bgr]


@pytest.fixture(scope="module")
def roi_frames():
    return _roi_frames()


def _call_gather(lib, fb, wins_d, K, out, **over):
    descs, host = fb._descriptors(DEV)
    a = dict(descs=descs.data_ptr(), host=ctypes.addressof(host), S=len(fb), win=wins_d.data_ptr(), K=K, y=out.data_ptr(), Ho=out.shape[1],
             Wo=out.shape[2])
    a.update(over)
    rc = lib.fx_frames_roi_gather_f32(a["descs"], a["host"], a["S"], a["win"], a["K"], a["y"], a["Ho"], a["Wo"], _stream())
    torch.cuda.synchronize()
    return rc


def _single_window(lib, fb, s, win, Ho, Wo):
    """fx_frames_tile_gather_f32 for frame s alone with one window (S = 1, V = 1)."""
    descs, host = fb._descriptors(DEV)
    wh = torch.tensor([win], dtype=torch.int32)
    wd = wh.to(DEV)
    want = torch.empty(1, Ho, Wo, 3, dtype=torch.float32, device=DEV)
    _lib.check(lib.fx_frames_tile_gather_f32(descs.data_ptr() + 64 * s, ctypes.addressof(host) + 64 * s, 1, wd.data_ptr(), wh.data_ptr(), 1,
                                             want.data_ptr(), Ho, Wo, _stream()), "fx_frames_tile_gather_f32")
    torch.cuda.synchronize()
    return want[0].cpu()


def _check_crops(lib, fb, wins, clamped, Ho, Wo):
    S, K = wins.shape[:2]
    buf = torch.full((S * K + 2, Ho, Wo, 3), -7.0, dtype=torch.float32, device=DEV)      # a canary crop on either side
    assert _call_gather(lib, fb, _dev(wins), K, buf[1:S * K + 1]) == 0
    assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
    got = buf[1:S * K + 1].cpu()
    for s in range(S):
        for k in range(K):
            x0, y0, w, h = clamped[s][k]
            if w < 1 or h < 1:
                assert bool((got[s * K + k] == -7.0).all()), (s, k, "a crop without an extent is left untouched")
            else:
                assert torch.equal(got[s * K + k], _single_window(lib, fb, s, [x0, y0, w, h], Ho, Wo)), (s, fb[s].format, wins[s, k].tolist())


@pytest.mark.parametrize("Ho,Wo", [(32, 32), (45, 63)], ids=["vec16", "scalar"])
def test_gather_equals_the_tile_gather_per_frame_and_window(roi_frames, Ho, Wo):
    lib = _lib.load("bf16")
    fb = FrameBatch(roi_frames)
    # per frame: an odd origin, touching the bottom-right corner, 1 x 1, empty
    wins = np.array([[[13, 7, 50, 41], [91 - 40, 71 - 30, 40, 30], [17, 33, 1, 1], [5, 5, 0, 9]],
                     [[3, 9, 33, 20], [64 - 21, 50 - 17, 21, 17], [63, 49, 1, 1], [5, 5, 9, 0]],
                     [[1, 1, 38, 39], [40 - 16, 40 - 8, 16, 8], [0, 39, 1, 1], [7, 7, -3, -3]]], dtype=np.int32)
    _check_crops(lib, fb, wins, wins.tolist(), Ho, Wo)


@pytest.mark.parametrize("Ho,Wo", [(32, 32), (45, 63)], ids=["vec16", "scalar"])
def test_gather_clamps_a_window_to_its_own_frame(roi_frames, Ho, Wo):
    """Windows that overhang the declared frame by a few pixels equal the gather of the window clamped by hand: origin into the frame, extent
    to what is left.  Device frames only: their planes sit inside guarded allocations."""
    lib = _lib.load("bf16")
    fb = FrameBatch([roi_frames[0], roi_frames[2]])
    wins = np.array([[[-3, 5, 20, 20], [80, 60, 20, 20], [93, 74, 10, 10], [5, -2, 200, 200]],
                     [[-2, -3, 12, 12], [30, 33, 13, 9], [42, 41, 5, 5], [0, 0, 43, 44]]], dtype=np.int32)
    clamped = [[[0, 5, 20, 20], [80, 60, 11, 11], [90, 70, 1, 1], [5, 0, 86, 71]],
               [[0, 0, 12, 12], [30, 33, 10, 7], [39, 39, 1, 1], [0, 0, 40, 40]]]
    _check_crops(lib, fb, wins, clamped, Ho, Wo)


def test_gather_refuses_bad_arguments_and_writes_nothing(roi_frames):
    lib = _lib.load("bf16")
    fb = FrameBatch(roi_frames)
    K = 2
    wins = _dev(np.tile(np.array([[2, 3, 20, 10]], np.int32), (3 * K, 1)))
    out = torch.full((3 * K, 32, 32, 3), -7.0, dtype=torch.float32, device=DEV)
    call = lambda **k: _call_gather(lib, fb, wins, **{"K": K, "out": out, **k})      # noqa: E731
    descs, host = fb._descriptors(DEV)
    bad = [dict(descs=None), dict(host=None), dict(win=None), dict(y=None), dict(descs=descs.data_ptr() + 4), dict(win=wins.data_ptr() + 2),
           dict(y=out.data_ptr() + 2), dict(S=0), dict(S=65536), dict(K=0), dict(K=21846), dict(Ho=0), dict(Wo=0), dict(Ho=16385), dict(Wo=16385)]
    for k in bad:
        assert call(**k) == INVALID, k
    for field, value in (("format", 9), ("matrix", -1), ("height", 0), ("width", 16385)):
        broken = (_lib.FxFrameDesc * 3).from_buffer_copy(bytes(host))
        setattr(broken[2], field, value)
        assert call(host=ctypes.addressof(broken)) == INVALID, field
    broken = (_lib.FxFrameDesc * 3).from_buffer_copy(bytes(host))
    broken[0].pitch[1] = 91      # below the 92 bytes of an NV12 chroma row of width 91
    assert call(host=ctypes.addressof(broken)) == INVALID
    assert bool((out == -7.0).all())
    assert call() == 0 and not bool((out == -7.0).any())      # the same arguments unbroken write every crop


# ---------------------------------------------------------------- attributes
def _attr_frames(C, tracked):
    """Four frames of S = 2 streams, T = 6, K = 3, M = 4: (logits, roi_det, roi_count, count, track_ids, trk_id).  Small integer logits, so
    ties occur; a row of NaNs and a row with one; a crop of an untracked detection; garbage past the counts; slot 1 of stream 0 changes its
    id in frame 2."""
    rng = np.random.default_rng(300 + C)
    S, T_, K = 2, 6, 3
    frames = []
    trk = np.array([[3, 5, 0, 8], [1, 2, 3, 4]], np.int32)
    for f in range(4):
        logits = rng.integers(-2, 3, (S * K, C)).astype(np.float32)
        logits[2] = np.nan              # an untracked crop with nothing but NaNs: (0, -inf)
        logits[4, C // 2] = np.nan
        if f == 1:
            logits[3] = np.nan          # and a tracked one: "latest" takes (0, -inf), "best" keeps what it has
        count = np.array([6, 4 if f != 1 else 0], np.int32)
        if f == 2:
            trk[0, 1] = 6
        ids = np.array([[3, 5 if f < 2 else 6, 5, -1, 8, 3], [2, -1, 4, 4, 1, 3]], np.int32)      # a duplicate of 3, and 5 without a slot later
        # a detection is named once; slot 1's new id gets its record in frame 2; stream 1's third crop (frame 3) is past its count
        det = np.array([[(1, 2, 1, 4)[f], 0, 5], [2, 1, 5]], np.int32)
        rcnt = np.array([3, 2 if f != 3 else 3], np.int32)
        det[1, int(rcnt[1]):] = -1
        frames.append((logits, det, rcnt, count, ids if tracked else None, trk.copy() if tracked else None))
    return frames


@pytest.mark.parametrize("tracked", [True, False], ids=["tracked", "untracked"])
@pytest.mark.parametrize("hold", [0, 1], ids=["latest", "best"])
@pytest.mark.parametrize("C", [1, 5, 80])
def test_attributes_equal_the_reference_over_four_frames(C, hold, tracked):
    lib = _lib.load("bf16")
    S, T_, K, M = 2, 6, 3, 4 if tracked else 1
    state = R.new_state(S, M)
    dstate = {k: _dev(v) for k, v in state.items()}
    for f, (logits, det, rcnt, count, ids, trk) in enumerate(_attr_frames(C, tracked)):
        want = R.attributes(logits, det, rcnt, count, T_, state, K, hold, ids, trk)
        keep = [_dev(logits), _dev(det), _dev(rcnt), _dev(count), None if ids is None else _dev(ids), None if trk is None else _dev(trk)]
        out = (torch.full((S, T_), -7, dtype=torch.int32, device=DEV), torch.full((S, T_), -7.0, dtype=torch.float32, device=DEV),
               torch.full((S, T_), -7, dtype=torch.int32, device=DEV))
        args = [_ptr(keep[0]), C, _ptr(keep[1]), _ptr(keep[2]), K, _ptr(keep[3]), S, T_, _ptr(keep[4]), _ptr(keep[5]), M, dstate["at_id"].data_ptr(),
                dstate["at_label"].data_ptr(), dstate["at_logit"].data_ptr(), dstate["at_frame"].data_ptr(), dstate["frame"].data_ptr(), hold,
                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream()]
        if f == 0:      # refused argument sets first: nothing written, the state untouched
            for i, v in ((0, None), (2, None), (11, None), (17, None), (1, 0), (4, 0), (4, 65), (6, 0), (7, 1025), (10, 0), (16, 2),
                         (8, None) if tracked else (6, 65536), (19, out[2].data_ptr() + 2)):
                broken = list(args)
                broken[i] = v
                assert lib.fx_roi_attributes(*broken) == INVALID, i
            torch.cuda.synchronize()
            assert bool((out[0] == -7).all()) and bool((out[2] == -7).all()) and int(dstate["frame"].sum()) == 0
        assert lib.fx_roi_attributes(*args) == 0
        torch.cuda.synchronize()
        for name, g, w in zip(("attr_label", "attr_logit", "attr_age"), out, want):
            assert np.array_equal(g.cpu().numpy(), w), (f, name, g.cpu().numpy().tolist(), w.tolist())
        for name in state:
            assert np.array_equal(dstate[name].cpu().numpy(), state[name]), (f, name)
    if tracked:
        assert (state["at_id"] != 0).any() and state["frame"].tolist() == [4, 4]


# ---------------------------------------------------------------- end to end
EH, EW = 200, 260
THR = 0.01
K = 4
TILING = T.Tiling(tile=128, overlap=0.25, batch_size=4)


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


def _attrs(res):
    return [(d.attr_id, d.attr_label, d.attr_conf) for d in res.detections]


@pytest.fixture(scope="module")
def models():
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        return ModelManager.get("fai-detr-m-coco", device=DEV, seed=3), ModelManager.get("fai-cls-n-coco", device=DEV, seed=4)


def _cascade(cls):
    return CS.Cascade(cls, max_objects=K, pad=0.1, interval=2, threshold=0.01)


def _expected(models, tiling):
    """The by-hand procedure over the three batches: the packed results and ids of the same call without ``classify`` (and the tracker's
    slot table after each batch), cascade_ref's selection, crops by the existing tile gather, the classifier engine on the same
    [8][224][224][3] buffer, cascade_ref's attributes."""
    from focoos_amd.tracking import DeviceTracker

    lib = _lib.load("bf16")
    det, cls = models
    c = _cascade(cls)
    batches, rgbs = _frame_batches()
    trk = DeviceTracker(2, _tracker_config(), DEV)
    S, T_, M = 2, 300, 1024
    state = R.new_state(S, M)
    crops = torch.zeros(S * K, 224, 224, 3, dtype=torch.float32, device=DEV)
    out = []
    for inputs, rgb in zip(batches, rgbs):
        plain = det.infer_batch(inputs if tiling is not None else CS.stream_frames(inputs, "test"), threshold=THR, tracker=trk, tiling=tiling)
        trk_id = trk.state()["id"]
        scores, labels = np.zeros((S, T_), np.float32), np.zeros((S, T_), np.int32)
        boxes, count, ids = np.zeros((S, T_, 4), np.int32), np.zeros(S, np.int32), np.full((S, T_), -1, np.int32)
        for s, r in enumerate(plain):
            count[s] = len(r.detections)
            for j, d in enumerate(r.detections):
                scores[s, j], labels[s, j], boxes[s, j], ids[s, j] = d.conf, d.cls_id, d.bbox, -1 if d.track_id is None else d.track_id
        win, rdet, rcnt, left = R.select(scores, labels, boxes, count, [(EH, EW)] * S, state, K, c.pad_q, c.min_size, c.min_score, c.interval,
                                         ids, trk_id)
        fb = CS.stream_frames(inputs, "test")
        for s in range(S):
            for k in range(int(rcnt[s])):
                crops[s * K + k].copy_(_single_window(lib, fb, s, win[s, k].tolist(), 224, 224))
        logits = cls.model.engine.forward(crops).logits.cpu().numpy().copy()
        lab, lg, age = R.attributes(logits, rdet, rcnt, count, T_, state, K, 0, ids, trk_id)
        out.append(SimpleNamespace(dets=[_dets(r) for r in plain], count=count, win=win, det=rdet, cnt=rcnt, left=left, logits=logits, label=lab,
                                   logit=lg, age=age, rgb=rgb))
    return out


@pytest.fixture(scope="module")
def expected(models):
    return _expected(models, None)


@pytest.fixture(scope="module")
def expected_tiled(models):
    return _expected(models, TILING)


def _want_attrs(e, cls, s):
    conf = torch.sigmoid(torch.from_numpy(e.logit))[s].tolist()      # the whole [S, T] array at once, as cascade.attach does
    names = cls.model_info.classes
    return [(int(e.label[s, j]), names[int(e.label[s, j])], conf[j]) if e.label[s, j] >= 0 and conf[j] > 0.01 else (None, None, None)
            for j in range(int(e.count[s]))]


def _check(got, dc, e, cls):
    """One batch of results and the cascade's device outputs against the by-hand procedure."""
    last = dc.last()
    assert [_dets(r) for r in got] == e.dets
    for name, w in (("roi_win", e.win), ("roi_det", e.det), ("roi_count", e.cnt), ("roi_left", e.left), ("attr_label", e.label),
                    ("attr_logit", e.logit), ("attr_age", e.age)):
        assert np.array_equal(last[name], w), name
    for s, r in enumerate(got):
        assert _attrs(r) == _want_attrs(e, cls, s), s


@pytest.mark.parametrize("which", ["expected", "expected_tiled"])
def test_the_by_hand_procedure_has_work_in_it(which, request, models):
    exp = request.getfixturevalue(which)
    for j, e in enumerate(exp):
        print(f"{which} batch {j}: detections {e.count.tolist()}, crops {e.cnt.tolist()}, left {e.left.tolist()}, "
              f"ages {[sorted(set(e.age[s][:e.count[s]].tolist())) for s in range(2)]}, best logit {float(e.logit.max()):.3f}")
    assert exp[0].cnt.tolist() == [K, K]
    assert any((exp[1].age[s][:exp[1].count[s]] == 1).any() for s in range(2))      # a record carried into frame 1 without a new crop
    assert any(a[0] is not None for e in exp for s in range(2) for a in _want_attrs(e, models[1], s))


def test_infer_stream_classify_equals_the_pieces_composed_by_hand(models, expected):
    from focoos_amd.tracking import DeviceTracker

    det, cls = models
    batches, _ = _frame_batches()
    plain = list(det.infer_stream((CS.stream_frames(b, "test") for b in batches), threshold=THR, track=_tracker_config()))
    assert [[_dets(r) for r in g] for g in plain] == [e.dets for e in expected]
    assert all(a == (None, None, None) for g in plain for r in g for a in _attrs(r))
    trk = DeviceTracker(2, _tracker_config(), DEV)
    dc = CS.DeviceCascade(_cascade(cls), 2, trk, DEV)
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # the crop budget overflows on purpose
        for got, e in zip(det.infer_stream(iter(batches), threshold=THR, track=trk, classify=dc), expected):
            _check(got, dc, e, cls)
            n += 1
    assert n == 3
    # a Cascade in the place of the device object: the state is the call's own
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # the crop budget overflows on purpose
        again = list(det.infer_stream(iter(batches), threshold=THR, track=_tracker_config(), classify=_cascade(cls)))
    assert [[_attrs(r) for r in g] for g in again] == [[_want_attrs(e, cls, s) for s in range(2)] for e in expected]


def test_infer_batch_classify_equals_the_pieces_composed_by_hand(models, expected):
    from focoos_amd.tracking import DeviceTracker

    det, cls = models
    batches, _ = _frame_batches()
    trk = DeviceTracker(2, _tracker_config(), DEV)
    dc = CS.DeviceCascade(_cascade(cls), 2, trk, DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for inputs, e in zip(batches, expected):
            _check(det.infer_batch(inputs, threshold=THR, classify=dc), dc, e, cls)      # the cascade runs the tracker it was built on


def test_tiled_classify_equals_the_pieces_composed_by_hand(models, expected_tiled):
    from focoos_amd.tracking import DeviceTracker

    det, cls = models
    batches, _ = _frame_batches()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        trk = DeviceTracker(2, _tracker_config(), DEV)
        dc = CS.DeviceCascade(_cascade(cls), 2, trk, DEV)
        for got, e in zip(det.infer_stream(iter(batches), threshold=THR, tiling=TILING, track=trk, classify=dc), expected_tiled):
            _check(got, dc, e, cls)
        trk = DeviceTracker(2, _tracker_config(), DEV)
        dc = CS.DeviceCascade(_cascade(cls), 2, trk, DEV)
        for inputs, e in zip(batches, expected_tiled):
            _check(det.infer_batch(inputs, threshold=THR, tiling=TILING, tracker=trk, classify=dc), dc, e, cls)


def test_a_chunked_classifier_gives_the_same_top_classes(models, expected):
    """``batch_size`` runs the classifier on another plan (no bit equality is claimed across batch sizes): same crops, same selection, and
    the same label wherever the top-2 logit margin exceeds the classifier's own logit gate of 0.062."""
    from focoos_amd.tracking import DeviceTracker

    det, cls = models
    batches, _ = _frame_batches()
    trk = DeviceTracker(2, _tracker_config(), DEV)
    dc = CS.DeviceCascade(CS.Cascade(cls, max_objects=K, pad=0.1, interval=2, threshold=0.01, batch_size=3), 2, trk, DEV)
    assert (dc.bs, dc.Npad) == (3, 9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = det.infer_batch(batches[0], threshold=THR, classify=dc)
    e, last = expected[0], dc.last()
    assert [_dets(r) for r in got] == e.dets and np.array_equal(last["roi_win"], e.win) and np.array_equal(last["roi_det"], e.det)
    top2 = np.sort(e.logits, axis=1)[:, -2:]
    for s in range(2):
        for k in range(int(e.cnt[s])):
            if top2[s * K + k, 1] - top2[s * K + k, 0] > 0.062:
                assert last["attr_label"][s, e.det[s, k]] == e.label[s, e.det[s, k]], (s, k)


def test_the_public_classifier_on_host_crops_agrees_where_the_margin_is_clear(models, expected):
    """The loose cross-check: ``classifier.infer_batch`` on the host-cropped RGB arrays of stream 1's crops gives the cascade's top-1 labels
    wherever the top-2 logit margin exceeds 0.062, the classifier's own logit gate.  The batch size differs there,
    so no bit equality is claimed."""
    det, cls = models
    checked = 0
    for e in expected:
        arrays = [np.ascontiguousarray(e.rgb[1][y0:y0 + h, x0:x0 + w]) for x0, y0, w, h in e.win[1, :int(e.cnt[1])].tolist()]
        if not arrays:
            continue
        res = cls.infer_batch(arrays, threshold=1e-9)
        top2 = np.sort(e.logits[K:2 * K], axis=1)[:, -2:]
        for k, r in enumerate(res):
            if top2[k, 1] - top2[k, 0] > 0.062:
                best = max(r.detections, key=lambda d: d.conf)
                assert best.cls_id == R.top1(e.logits[K + k])[0], (k, best.cls_id)
                checked += 1
    print(f"host-crop cross-check: {checked} crops with a clear margin")
    assert checked > 0


def test_the_budget_warning_is_issued_once_per_call(models):
    det, cls = models
    batches, _ = _frame_batches()
    with pytest.warns(RuntimeWarning, match="max_objects") as rec:
        list(det.infer_stream(iter(batches), threshold=THR, classify=CS.Cascade(cls, max_objects=1, min_size=1)))
    assert len([w for w in rec if "max_objects" in str(w.message)]) == 1


def test_infer_stream_and_infer_batch_run_one_analytics_tail(models):
    """Everything at once (analytics.py): tracker, a zone and a line, dwell times, heat map, traces, cascade and an
    overlay with redaction.  ``infer_stream`` on one set of device objects equals three ``infer_batch`` calls on a second, fresh set
    exactly: both run the same kernels on the same inputs, so no margin is needed."""
    from focoos_amd.annotate import DeviceTraces, Overlay, Redact
    from focoos_amd.heat import DeviceHeatmap, Heatmap
    from focoos_amd.tracking import DeviceTracker
    from focoos_amd.zones import DeviceDwell, DeviceZones, Line, Zone

    det, cls = models
    batches, rgbs = _frame_batches()
    regions = [Zone("yard", [(20, 20), (240, 20), (240, 180), (20, 180)]), Line("gate", (130, 0), (130, 199))]

    def device_objects():
        trk = DeviceTracker(2, _tracker_config(), DEV)
        zon = DeviceZones(2, regions, trk, DEV)
        ov = Overlay(traces=DeviceTraces(trk, 8), heat=True, redact=Redact(hold=1))
        return trk, dict(zones=zon, dwell=DeviceDwell(zon), heatmap=DeviceHeatmap(2, Heatmap(EH, EW), DEV),
                         classify=CS.DeviceCascade(_cascade(cls), 2, trk, DEV), annotate=ov)

    def facts(results):
        return [[(_dets(r), r.zones, _attrs(r)) for r in g] for g in results], [[r.image for r in g] for g in results]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # the crop budget overflows on purpose
        trk, kw = device_objects()
        with pytest.warns(RuntimeWarning, match=r"infer_batch\(classify=\).*max_objects") as rec:      # close() warns from this entry point too
            first = det.infer_batch(batches[0], threshold=THR, tracker=trk, **kw)
        left = [w for w in rec if "max_objects" in str(w.message)]
        assert len(left) == 1 and left[0].filename == __file__      # once per call, attributed to the caller of infer_batch
        want, want_images = facts([first] + [det.infer_batch(inputs, threshold=THR, tracker=trk, **kw) for inputs in batches[1:]])
        # the infer_batch side has work in it: identity carried across frames, a count, an attribute, pixels changed
        assert any(d[4] is not None for g in want[1:] for dets, _, _ in g for d in dets)
        assert any(z["count"] > 0 for g in want for _, zd, _ in g for z in zd.values())
        assert any(a[0] is not None for g in want for _, _, attrs in g for a in attrs)
        assert all(im.shape == (EH, EW, 3) and not np.array_equal(im, rgb) for g, r in zip(want_images, rgbs) for im, rgb in zip(g, r))
        trk, kw = device_objects()
        got, got_images = facts(list(det.infer_stream(iter(batches), threshold=THR, track=trk, **kw)))
    assert got == want
    assert all(np.array_equal(a, b) for g, w in zip(got_images, want_images) for a, b in zip(g, w)) and len(got_images) == 3
