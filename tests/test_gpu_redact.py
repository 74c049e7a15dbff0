"""Redaction on a real MI355X (csrc/redact.hip through focoos_amd/annotate.py): fx_redact_u8 and fx_redact_regions
against the restatement of tests/redact_ref.py, for equality, the refusals of both, then infer_stream / infer_batch with
annotate=Overlay(redact=Redact(...)) and seeded synthetic weights against the restatement redacted from a tracker stepped by hand and
drawn by annotate_ref / overlay_ref.  Nothing here reads the reference tree."""
import functools
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import annotate as AN
from focoos_amd.annotate import Overlay, Redact
from focoos_amd.synth import synth_image_structured
from focoos_amd.tracking import DeviceTracker, TrackerConfig

from . import annotate_ref as A
from . import overlay_ref as O
from . import redact_ref as R
from . import tracking_ref as TR
from .test_gpu_tracking import sequence

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


# ---------------------------------------------------------------- (a) fx_redact_u8
S, B0, NB, RR, TP = 4, 1, 2, 320, 8      # streams, first stream drawn, frames drawn, region slots per stream, mask planes per stream


def region_sets(H, W, rs):
    """{name: (regions [S, RR, 4], slots [S, RR], counts [S])}.  Streams 1 and 2 are drawn; streams 0 and 3 always list the whole frame, which
    must never show.  Slots run over -1 .. TP + 1: -1 and >= TP have no plane."""
    def blank():
        reg, cnt = np.zeros((S, RR, 4), np.int32), np.zeros(S, np.int32)
        reg[0, 0] = reg[3, 0] = (0, 0, W - 1, H - 1)
        cnt[0] = cnt[3] = 1
        return reg, rs.randint(-1, TP + 2, (S, RR)).astype(np.int32), cnt

    def boxes(n):
        x0, y0 = rs.randint(-W // 4, W, n), rs.randint(-H // 4, H, n)
        return np.stack([x0, y0, x0 + rs.randint(0, max(2, W // 3), n), y0 + rs.randint(0, max(2, H // 2), n)], -1)

    out = {}
    out["none"] = blank()
    reg, slot, cnt = blank()
    reg[1, 0], cnt[1] = (W // 2, H // 2, W // 2, H // 2), 1                                   # one pixel
    reg[2, :3], cnt[2] = [(W, 0, W + 9, H - 1), (-9, -9, -1, -1), (3, 3, 2, 8)], 3             # wholly outside, and an inverted one
    out["pixel+outside"] = (reg, slot, cnt)
    reg, slot, cnt = blank()
    reg[1, 0], cnt[1] = (-7, -3, W + 5, H + 40), 1                                            # covers the frame
    edges = [(-5, -5, 2, 2), (W - 3, -2, W + 4, 3), (-1, H - 2, 1, H + 7), (W - 2, H - 2, W, H), (62, 30, 65, 33), (60, 62, 131, 66), (126, 0, 129, H - 1),
             (0, 31, W - 1, 32), (W // 3, -100, W // 3 + 4, 16384), (-16385, H // 2, 32769, H // 2 + 1)]
    reg[2, :len(edges)], cnt[2] = edges, len(edges)
    out["frame+edges"] = (reg, slot, cnt)
    reg, slot, cnt = blank()
    reg[1, :300], cnt[1] = boxes(300), 300
    reg[2], cnt[2] = boxes(RR), RR + 5                                                        # above R: clamped
    reg[2, :, 2] = reg[2, :, 0] + rs.randint(0, 6, RR)                                        # small ones: the frame stays partly uncovered
    reg[2, :, 3] = reg[2, :, 1] + rs.randint(0, 6, RR)
    out["300+clamped"] = (reg, slot, cnt)
    return out


def redact_call(lib, src, dst, B, H, W, b0, reg, slot, cnt, words, wpr, mode, shape, cell, radius, colour, R_=RR, T=TP):
    return lib.fx_redact_u8(src.data_ptr(), dst.data_ptr(), B, H, W, b0, reg.data_ptr(), slot.data_ptr(), cnt.data_ptr(), R_,
                            None if words is None else words.data_ptr(), wpr, H * wpr, T, mode, shape, cell, radius, colour, _stream())


@pytest.mark.parametrize("H,W", [(70, 301), (64, 512), (9, 5)], ids=["70x301-bytes", "64x512-aligned", "9x5-tiny"])
def test_redact_u8_equals_the_restatement(H, W):
    lib = _lib.load("bf16")
    rs = np.random.RandomState(H * 1000 + W)
    frames = rs.randint(0, 256, (NB, H, W, 3)).astype(np.uint8)
    wpr = (W + 31) // 32 + 1                                                                  # more words per row than the frame needs
    ys, xs = np.mgrid[0:H, 0:W]
    masks = ((xs[None, None] * rs.randint(1, 5, (S, TP, 1, 1)) + ys[None, None] * rs.randint(1, 5, (S, TP, 1, 1))) % 7 < 3)
    d_words = _dev(A.pack_words(masks, wpr))
    modes = [(R.PIXELATE, 4, 16), (R.PIXELATE, 64, 16), (R.BLUR, 16, 1), (R.BLUR, 16, 7), (R.BLUR, 16, 32), (R.FILL, 16, 16)]
    colour = 0x10C0FE
    value = {m: np.stack([R.pixelated(f, m[1]) if m[0] == R.PIXELATE else R.blurred(f, m[2]) if m[0] == R.BLUR else
                          np.broadcast_to(np.array([0xFE, 0xC0, 0x10], np.uint8), f.shape) for f in frames]) for m in modes}
    d_src = _dev(frames)
    changed = {}
    for name, (reg, slot, cnt) in region_sets(H, W, rs).items():
        d_reg, d_slot, d_cnt = _dev(reg), _dev(slot), _dev(cnt)
        for shape in (R.BOX, R.ELLIPSE, R.MASK):
            cov = np.stack([R.covered(H, W, reg[B0 + b], slot[B0 + b], cnt[B0 + b], shape, masks[B0 + b]) for b in range(NB)])
            changed[name, shape] = int(cov.sum())
            for m in modes:
                mode, cell, radius = m
                want = np.where(cov[..., None], value[m], frames)
                where = (name, shape, m)
                buf = torch.full((NB + 2, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)      # out of place, between canary frames
                assert redact_call(lib, d_src, buf[1:], NB, H, W, B0, d_reg, d_slot, d_cnt, d_words, wpr, mode, shape, cell, radius, colour) == 0, where
                got = buf.cpu().numpy()
                assert np.array_equal(got[1:-1], want), where
                assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), where
                buf = torch.full((NB + 2, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)
                buf[1:-1] = d_src
                rc = redact_call(lib, buf[1:], buf[1:], NB, H, W, B0, d_reg, d_slot, d_cnt, d_words, wpr, mode, shape, cell, radius, colour)
                if mode == R.BLUR:                                                            # in place: refused, nothing written
                    assert rc == INVALID, where
                    want = frames
                else:
                    assert rc == 0, where
                got = buf.cpu().numpy()
                assert np.array_equal(got[1:-1], want) and (got[0] == 0xA5).all() and (got[-1] == 0xA5).all(), where
        assert np.array_equal(d_src.cpu().numpy(), frames)                                    # src is never written
    # the sets did what their names say
    assert all(changed["none", s] == 0 for s in (R.BOX, R.ELLIPSE, R.MASK))
    assert changed["pixel+outside", R.BOX] == 1 and changed["frame+edges", R.BOX] > H * W
    assert 0 < changed["frame+edges", R.ELLIPSE] < changed["frame+edges", R.BOX] and 0 < changed["frame+edges", R.MASK] < changed["frame+edges", R.BOX]
    assert 0 < changed["300+clamped", R.BOX] < 2 * H * W or H * W < 64
    # R.redact itself composes the same pieces
    reg, slot, cnt = region_sets(H, W, np.random.RandomState(5))["frame+edges"]
    buf = torch.empty((NB, H, W, 3), dtype=torch.uint8, device=DEV)
    assert redact_call(lib, d_src, buf, NB, H, W, B0, _dev(reg), _dev(slot), _dev(cnt), d_words, wpr, R.PIXELATE, R.MASK, 8, 16, 0) == 0
    assert np.array_equal(buf.cpu().numpy(), R.redact(frames, B0, reg, slot, cnt, R.PIXELATE, R.MASK, 8, masks=masks))


# ---------------------------------------------------------------- (b) fx_redact_regions behind the real tracker
HOLD_CFG = dict(track_buffer=2)


def regions_call(lib, l, bx, c, B, T, words, K, trk, M, hold, pad256, top256, reg, slot, cnt):
    t = [None] * 4 if trk is None else [trk.id.data_ptr(), trk.label.data_ptr(), trk.tsu.data_ptr(), trk.box.data_ptr()]
    return lib.fx_redact_regions(l.data_ptr(), bx.data_ptr(), c.data_ptr(), B, T, None if words is None else words.data_ptr(), K, *t, M, hold, pad256,
                                 top256, reg.data_ptr(), slot.data_ptr(), cnt.data_ptr(), _stream())


def inverted(seq):
    """The frames of ``sequence`` with one detection per stream and frame turned inside out (x1 < x0 or y1 < y0): boxes the list skips.
    The tracker sees the same frames on both sides."""
    out = []
    for f, (s, l, bx, c) in enumerate(seq):
        bx = bx.copy()
        for b in range(len(c)):
            if c[b] > 2:
                j = (f + b) % int(c[b])
                x0, y0, x1, y1 = bx[b, j]
                bx[b, j] = (x1 + 1, y0, x0, y1) if (f + b) % 2 else (x0, y1 + 1, x1, y0)
        out.append((s, l, bx, c))
    return out


SELECT = [(None, 0), (np.array([0b10], np.uint32), 2), (np.array([0b11], np.uint32), 1)]      # all; label 1; label 0 alone, label 1 >= K


@functools.lru_cache(maxsize=None)
def tracked_frames(B, T, M):
    """The 12 frames and the restated tracker's state after each of them (computed once, left unchanged)."""
    ref, out = TR.RefTracker(B, TrackerConfig(max_tracks=M, **HOLD_CFG)), []
    for frame in inverted(sequence(1000 * T + B, B, T)):
        ref.update(*frame)
        out.append((frame, ref.state()))
    return out


def run_regions_ref(B, T, M, hold):
    """The restatement alone over the 12 frames: per frame the lists, and the counters of the whole sequence."""
    st, frames = R.new_stats(), []
    for f, ((s, l, bx, c), state) in enumerate(tracked_frames(B, T, M)):
        words, K = SELECT[f % 3]
        pad256, top256 = (0, 256) if f % 2 else (77, 128)
        frames.append(((s, l, bx, c), (words, K, pad256, top256), R.regions(l, bx, c, words, K, state, hold, pad256, top256, st), state))
    return frames, st


@pytest.mark.parametrize("hold", [0, 2])
@pytest.mark.parametrize("T,M", [(8, 4), (64, 64), (70, 130)])
@pytest.mark.parametrize("B", [1, 3])
def test_regions_equal_the_restatement_after_every_frame(B, T, M, hold):
    frames, st = run_regions_ref(B, T, M, hold)      # on the CPU first: the sequence must exercise what the assertions below name
    print(f"B={B} T={T} M={M} hold={hold}: {st}")
    assert st["selected"] > 0 and st["skipped"] > 0 and (st["coasting"] > 0) == (hold > 0)
    lib = _lib.load("bf16")
    trk = DeviceTracker(B, TrackerConfig(max_tracks=M, **HOLD_CFG), DEV)
    Rn = T + M
    reg = torch.full((B * Rn * 4 + 4,), -7, dtype=torch.int32, device=DEV)      # the last elements are canaries
    slot, cnt = torch.full((B * Rn + 1,), -7, dtype=torch.int32, device=DEV), torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    for f, ((s, l, bx, c), (words, K, pad256, top256), (wreg, wslot, wcnt), state) in enumerate(frames):
        dl, dbx, dc = _dev(l), _dev(bx), _dev(c)
        trk.update(_dev(s), dl, dbx, dc)
        got = trk.state()
        assert all(np.array_equal(got[k].view(np.int32), state[k].view(np.int32)) for k in ("id", "label", "tsu", "box")), f
        d_words = None if words is None else _dev(words.view(np.int32))
        assert regions_call(lib, dl, dbx, dc, B, T, d_words, K, trk, M, hold, pad256, top256, reg, slot, cnt) == 0
        assert np.array_equal(cnt[:-1].cpu().numpy(), wcnt), f
        assert np.array_equal(slot[:-1].cpu().numpy().reshape(B, Rn), wslot), f
        assert np.array_equal(reg[:-4].cpu().numpy().reshape(B, Rn, 4), wreg), f
        assert (reg[-4:] == -7).all() and int(slot[-1]) == -7 and int(cnt[-1]) == -7
    # without a tracker R = T and only the detections are listed
    (s, l, bx, c), (words, K, pad256, top256), _, _ = frames[-2]
    reg2, slot2, cnt2 = (torch.full(shape, -7, dtype=torch.int32, device=DEV) for shape in ((B, T, 4), (B, T), (B,)))
    d_words = None if words is None else _dev(words.view(np.int32))
    assert regions_call(lib, _dev(l), _dev(bx), _dev(c), B, T, d_words, K, None, 0, 0, pad256, top256, reg2, slot2, cnt2) == 0
    wreg, wslot, wcnt = R.regions(l, bx, c, words, K, None, 0, pad256, top256)
    assert np.array_equal(reg2.cpu().numpy(), wreg) and np.array_equal(slot2.cpu().numpy(), wslot) and np.array_equal(cnt2.cpu().numpy(), wcnt)


# ---------------------------------------------------------------- (c) refusals
def run_refusals(fn, order, base, bad, outs):
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


def test_refused_arguments_return_the_error_and_leave_everything_untouched():
    lib = _lib.load("bf16")
    B, T, M, H, W = 2, 8, 4, 20, 24
    s, l, bx, c = sequence(3, B, T, 1)[0]
    dl, dbx, dc = _dev(l), _dev(np.concatenate([bx.reshape(-1), np.zeros(4, np.int32)])), _dev(c)
    words = _dev(np.array([3, 0], np.int32))
    trk = dict(id=_dev(np.array([[1, 2, 3, 0], [4, 0, 2, 1]], np.int32)), label=_dev(np.zeros((B, M), np.int32)), tsu=_dev(np.array([[1, 0, 2, 1], [1, 1, 0, 3]], np.int32)),
               box=_dev(np.concatenate([np.tile(np.array([2, 3, 9, 12], np.float32), B * M), np.zeros(4, np.float32)])))
    Rn = T + M
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)      # noqa: E731
    reg, slot, cnt = i32(B * Rn * 4 + 4), i32(B * Rn + 1), i32(B + 1)
    order = ["l", "bx", "c", "B", "T", "words", "K", "tid", "tlabel", "ttsu", "tbox", "M", "hold", "pad", "top", "reg", "slot", "cnt"]
    base = dict(l=dl.data_ptr(), bx=dbx.data_ptr(), c=dc.data_ptr(), B=B, T=T, words=words.data_ptr(), K=2, tid=trk["id"].data_ptr(),
                tlabel=trk["label"].data_ptr(), ttsu=trk["tsu"].data_ptr(), tbox=trk["box"].data_ptr(), M=M, hold=2, pad=26, top=256, reg=reg.data_ptr(),
                slot=slot.data_ptr(), cnt=cnt.data_ptr())
    none = dict(tid=None, tlabel=None, ttsu=None, tbox=None)
    bad = [{p: None} for p in ("l", "bx", "c", "reg", "slot", "cnt", "tid", "tlabel", "ttsu", "tbox")] + [
        dict(B=0), dict(B=65536), dict(T=0), dict(T=1025), dict(K=0), dict(K=-1), dict(M=0), dict(M=1025), dict(hold=-1), dict(hold=1025), dict(pad=-1),
        dict(pad=257), dict(top=0), dict(top=257), dict(none, M=M), dict(none, M=0, hold=1), dict(bx=base["bx"] + 8), dict(tbox=base["tbox"] + 4),
        dict(reg=base["reg"] + 4), dict(l=base["l"] + 2), dict(slot=base["slot"] + 1), dict(words=base["words"] + 2), dict(ttsu=base["ttsu"] + 2)]
    run_refusals(lib.fx_redact_regions, order, base, bad, dict(reg=reg, slot=slot, cnt=cnt))
    assert cnt[:-1].min() >= 1                                                 # the unbroken call listed something to cover

    src = _dev(np.random.RandomState(1).randint(0, 250, (B, H, W, 3)).astype(np.uint8))
    out = torch.full((B * H * W * 3 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    greg = _dev(np.tile(np.array([2, 2, 15, 11], np.int32), (B, Rn, 1)))
    gslot, gcnt = _dev(np.zeros((B, Rn), np.int32)), _dev(np.full(B, 2, np.int32))
    planes = _dev(np.full((B * T * H * 1 + 1,), -1, np.int32))
    order = ["src", "dst", "B", "H", "W", "b0", "reg", "slot", "cnt", "R", "words", "wpr", "stride", "T", "mode", "shape", "cell", "radius", "colour"]
    base = dict(src=src.data_ptr(), dst=out.data_ptr(), B=B, H=H, W=W, b0=0, reg=greg.data_ptr(), slot=gslot.data_ptr(), cnt=gcnt.data_ptr(), R=Rn,
                words=planes.data_ptr(), wpr=1, stride=H, T=T, mode=R.BLUR, shape=R.MASK, cell=16, radius=3, colour=0)
    bad = [{p: None} for p in ("src", "dst", "reg", "slot", "cnt", "words")] + [
        dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(b0=-1), dict(R=0), dict(R=2049), dict(T=0), dict(T=1025),
        dict(mode=-1), dict(mode=3), dict(shape=-1), dict(shape=3), dict(cell=0), dict(cell=12), dict(cell=128), dict(radius=0), dict(radius=33),
        dict(colour=-1), dict(colour=1 << 24), dict(wpr=0), dict(stride=H - 1), dict(reg=base["reg"] + 8), dict(slot=base["slot"] + 2), dict(cnt=base["cnt"] + 1),
        dict(words=base["words"] + 2), dict(dst=base["src"]), dict(dst=base["src"] + 3), dict(dst=base["src"] + B * H * W * 3 - 1),
        dict(mode=R.PIXELATE, dst=base["src"] + 3), dict(mode=R.FILL, dst=base["src"] + B * H * W * 3 - 1)]
    run_refusals(lib.fx_redact_u8, order, base, bad, dict(dst=out))
    want = R.redact(src.cpu().numpy(), 0, greg.cpu().numpy(), gslot.cpu().numpy(), gcnt.cpu().numpy(), R.BLUR, R.MASK, radius=3,
                    masks=np.ones((B, T, H, W), bool))
    assert np.array_equal(out[:-4].cpu().numpy().reshape(B, H, W, 3), want)


# ---------------------------------------------------------------- (d) the public interface
SIZE = 128
LOW = TrackerConfig(high=0.06, low=0.05, new_thresh=0.06, track_buffer=1, max_tracks=1024)


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


def test_infer_stream_and_infer_batch_redact_like_state_stepped_by_hand(detr):
    """6 batches of 2 frames.  Overlay(zones=False, redact=...): the call has no zones, every other field is the default."""
    batches = [[synth_image_structured(40 + b, SIZE, SIZE) if j % 3 else synth_image_structured(40 + b + 10 * j, SIZE, SIZE) for b in range(2)]
               for j in range(6)]
    classes = detr.model_info.classes
    atlas, gw, gh = AN.glyph_atlas()
    tab, ln = A.name_table(classes)
    s1 = AN.scale_for(SIZE, SIZE)
    red = Redact(cell=8, hold=2)
    plain = list(detr.infer_stream(iter(batches), threshold=0.05))
    tracked = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW))
    # by hand: the tracker on the plain run's packed results, the restatement's lists and pixels, then the restatement's drawing
    trk, st = DeviceTracker(2, LOW, DEV), R.new_stats()
    alone, want, undone = [], [], []
    for batch, imgs in zip(plain, batches):
        s, l, bx, c = _packed(batch)
        ids = trk.update(_dev(s), _dev(l), _dev(bx), _dev(c)).cpu().numpy()
        reg, slot, cnt = R.regions(l, bx, c, None, 0, trk.state(), red.hold, red.pad256, red.top256, st)
        alone.append(R.redact(np.stack(imgs), 0, reg, slot, cnt, R.PIXELATE, R.BOX, red.cell))
        rec = O.tracked_records(s, l, bx, c, ids, tab, ln, len(classes), SIZE, SIZE, s1, gw, gh)
        want.append(A.draw(alone[-1], c, l, bx, A.BOXES | A.LABELS, s1, rec=rec, atlas=atlas, gw=gw, gh=gh))
        undone.append(A.draw(np.stack(imgs), c, l, bx, A.BOXES | A.LABELS, s1, rec=rec, atlas=atlas, gw=gw, gh=gh))
    print(f"{sum(len(r.detections) for b in plain for r in b)} detections in 12 frames, regions {st}")
    assert st["selected"] > 0 and any((a != np.stack(i)).any() for a, i in zip(alone, batches))
    got = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, annotate=Overlay(zones=False, redact=red)))
    for f, (batch, w) in enumerate(zip(got, want)):
        for b, r in enumerate(batch):
            assert r.image.dtype == np.uint8 and np.array_equal(r.image, w[b]), (f, b)
    # the detections and ids are those of annotate=False
    assert [[_dets(r) for r in b] for b in got] == [[_dets(r) for r in b] for b in tracked]
    # draw=False: the redaction alone
    bare = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, annotate=Overlay(ids=False, zones=False, redact=red, draw=False)))
    assert all(np.array_equal(r.image, a[b]) for batch, a in zip(bare, alone) for b, r in enumerate(batch))
    # infer_batch, one call per batch, with a tracker of its own
    trk2 = DeviceTracker(2, LOW, DEV)
    one = [detr.infer_batch(b, threshold=0.05, tracker=trk2, annotate=Overlay(zones=False, redact=red)) for b in batches]
    assert all(np.array_equal(r.image, w[b]) for batch, w in zip(one, want) for b, r in enumerate(batch))
    assert [[_dets(r) for r in b] for b in one] == [[_dets(r) for r in b] for b in tracked]
    # an Overlay without the new fields draws what it drew
    old = list(detr.infer_stream(iter(batches), threshold=0.05, track=LOW, annotate=Overlay(zones=False)))
    assert all(np.array_equal(r.image, w[b]) for batch, w in zip(old, undone) for b, r in enumerate(batch))
    # blur goes through the scratch frame: the same lists, the other pixels
    blur = Redact(mode="blur", radius=5, shape="ellipse", pad=0.1, top=0.5)
    soft = list(detr.infer_stream(iter(batches[:2]), threshold=0.05, annotate=Overlay(ids=False, zones=False, redact=blur, draw=False)))
    for batch, res, imgs in zip(plain, soft, batches):
        s, l, bx, c = _packed(batch)
        reg, slot, cnt = R.regions(l, bx, c, None, 0, None, 0, blur.pad256, blur.top256)
        w = R.redact(np.stack(imgs), 0, reg, slot, cnt, R.BLUR, R.ELLIPSE, radius=5)
        assert all(np.array_equal(r.image, w[b]) for b, r in enumerate(res))


def test_infer_batch_redacts_an_instance_by_its_own_mask():
    from .test_gpu_annotate import _get, _mask_inputs

    fm = _get("fai-mf-l-coco-ins", 3)
    img = synth_image_structured(9, 128, 160)
    red = Redact(shape="mask", cell=8)
    res = fm.infer_batch([img], threshold=0.05, annotate=Overlay(ids=False, zones=False, redact=red))[0]
    masks, area = _mask_inputs(fm, res, 128, 160)
    plain = fm.infer(img, threshold=0.05)
    n = len(res.detections)
    assert n > 0 and [(tuple(d.bbox), d.conf, d.cls_id, d.mask) for d in res.detections] == [(tuple(d.bbox), d.conf, d.cls_id, d.mask) for d in plain.detections]
    s, l, bx, c = _packed([res], max(n, 1))
    reg, slot, cnt = R.regions(l, bx, c)
    hidden = R.redact(img[None], 0, reg, slot, cnt, R.PIXELATE, R.MASK, 8, masks=masks)
    assert (hidden != img[None]).any() and not np.array_equal(hidden, R.redact(img[None], 0, reg, slot, cnt, R.PIXELATE, R.BOX, 8))
    atlas, gw, gh = AN.glyph_atlas()
    tab, ln = A.name_table(fm.model_info.classes)
    s1 = AN.scale_for(128, 160)
    rec = A.records(s, l, bx, c, tab, ln, len(fm.model_info.classes), 128, 160, s1, gw, gh)
    want = A.draw(hidden, c, l, bx, A.BOXES | A.MASKS | A.LABELS, s1, area=area, masks=masks, rec=rec, atlas=atlas, gw=gw, gh=gh)[0]
    assert np.array_equal(res.image, want)
    bare = fm.infer_batch([img], threshold=0.05, annotate=Overlay(ids=False, zones=False, redact=red, draw=False))[0]
    assert np.array_equal(bare.image, hidden[0])
