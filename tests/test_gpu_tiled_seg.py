"""Tiled segmentation on a real MI355X (csrc/seg_merge.hip through focoos_amd/tiled_seg.py): fx_seg_merge_views on
seeded random views against the float64 restatement of tests/tiled_seg_ref.py, and FocoosModel.segment_tiled against the same pieces
composed by hand.  Nothing here reads the reference tree.

Margin.  eps = 2^-24, h = 8 map rows.  A tap's source index is three fp32 operations on values up to h: its weight is off by at most
3 h eps.  One lerp is off by that (its two values differ by at most 1) plus eps for 1 - w1 plus three roundings: (3 h + 4) eps; x then y:
2 (3 h + 4) eps on P; times the score and one rounding: (6 h + 9) eps on S.  A sums `cover` of them with cover - 1 roundings of partial
sums of at most cover: A is off by at most cover (6 h + 9) eps + cover^2 eps = E.  Two competing classes: MARGIN = 2 E.  conf = A / cover
adds one rounding: TOL_CONF = E / cover + eps.  A class's score is a mean of conf, each pixel quantised to 2^-24 (half a unit) and, inside
the margin, taken for a class whose A is at most MARGIN below: TOL_SCORE = TOL_CONF + MARGIN + eps."""
import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import tiled_seg as TS
from focoos_amd.tiled import tile_grid

from . import tiled_seg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
EPS, HL = 2.0 ** -24, 8
GUARD = 256


def _tolerances(cover):
    e = cover * (6 * HL + 9) * EPS + cover * cover * EPS
    return 2 * e, e / cover + EPS, e / cover + EPS + 2 * e + EPS      # MARGIN, TOL_CONF, TOL_SCORE


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class _Out:
    """Every output of fx_seg_merge_views inside a buffer with GUARD sentinel elements on either side."""

    SPEC = (("label_map", torch.uint8), ("conf", torch.float32), ("det_count", torch.int32), ("det_label", torch.int32),
            ("det_score", torch.float32), ("det_box", torch.int32), ("det_area", torch.int32), ("mask_words", torch.int32), ("status", torch.int32))

    def __init__(self, Hf, Wf, M):
        n = {"label_map": Hf * Wf, "conf": Hf * Wf, "det_count": 1, "det_label": M, "det_score": M, "det_box": 4 * M, "det_area": M,
             "mask_words": M * Hf * ((Wf + 31) // 32), "status": 1}
        self.bufs = {k: torch.full((n[k] + 2 * GUARD,), 77, dtype=dt, device=DEV) for k, dt in self.SPEC}
        self.n = n

    def ptr(self, k):
        return self.bufs[k].data_ptr() + GUARD * self.bufs[k].element_size()

    def get(self, k):
        return self.bufs[k][GUARD:GUARD + self.n[k]].cpu().numpy()

    def guards_intact(self):
        return all(bool((b[:GUARD] == 77).all()) and bool((b[-GUARD:] == 77).all()) for b in self.bufs.values())

    def untouched(self):
        return all(bool((b == 77).all()) for b in self.bufs.values())


def _call(lib, dev_in, wins, Hf, Wf, K, thr, M, out, **over):
    """fx_seg_merge_views on device inputs (probs, score, label); ``over`` breaks single arguments for the refusal test."""
    probs, score, label = dev_in
    _, Q, h, w = (int(v) for v in probs.shape)
    wh = torch.from_numpy(np.ascontiguousarray(over.get("wins_host", wins), dtype=np.int32))
    wd = torch.from_numpy(np.ascontiguousarray(wins, dtype=np.int32)).to(DEV)
    ws = torch.empty(max(int(lib.fx_seg_merge_workspace_bytes(len(wh), Q, h, w, Hf, Wf, K, M)), 16), dtype=torch.uint8, device=DEV)
    N, Q, K = len(wh), over.get("bad_Q", Q), over.get("bad_K", K)
    rc = lib.fx_seg_merge_views(probs.data_ptr(), score.data_ptr(), label.data_ptr(), wd.data_ptr(), wh.data_ptr(), N, Q, h, w, Hf, Wf, K,
                                float(thr), M, ws.data_ptr(), over.get("ws_bytes", ws.numel()), over.get("label_map", out.ptr("label_map")),
                                out.ptr("conf"), out.ptr("det_count"), out.ptr("det_label"), out.ptr("det_score"), out.ptr("det_box"),
                                out.ptr("det_area"), out.ptr("mask_words"), out.ptr("status"), _stream())
    torch.cuda.synchronize()
    return rc


def _inputs(seed, N, Q, K):
    rs = np.random.RandomState(seed)
    probs = rs.rand(N, Q, HL, HL).astype(np.float32)
    score = (0.2 + 0.8 * rs.rand(N, Q)).astype(np.float32)
    label = rs.randint(0, K, (N, Q)).astype(np.int32)
    if N > 1 and Q >= 3 and K >= 3:
        label[0, :2] = 0                     # two queries of one class in a view
        label[1][label[1] == 1] = 2          # class 1 lives in view 0 only, and view 0 overlaps view 1
        label[0, 2] = 1
    return probs, score, label


# name: (Hf, Wf, overlap, Q, K, seed, tile).  multi_block: x edges 0, 144, 256, 400 and y edges 0, 44, 256, 300 - rectangles of 2 x 4 workgroup
# blocks (128 x 64) with ragged last ones, blocks that start at x = 128, 144, 256, 384 with Wf % 16 == 0 (16-byte label stores off the origin)
CASES = {"one_view_q128_k255": (64, 64, 0.2, 128, 255, 1, 64), "snapped_2x2": (90, 100, 0.2, 12, 5, 2, 64), "short_axis_q1_k2": (50, 150, 0.0, 1, 2, 3, 64),
         "three_cover": (64, 200, 0.5, 20, 7, 4, 64), "wide_taps": (64, 12, 0.2, 6, 3, 5, 64), "multi_block": (300, 400, 0.2, 16, 6, 6, 256)}


@pytest.mark.parametrize("name", list(CASES))
def test_merge_against_the_float64_restatement(name):
    lib = _lib.load("bf16")
    Hf, Wf, overlap, Q, K, seed, tile = CASES[name]
    wins = tile_grid(Hf, Wf, tile, tile, overlap)
    N = len(wins)
    probs, score, label = _inputs(seed, N, Q, K)
    A, cover = R.class_sums(probs, score, label, wins, Hf, Wf, K)
    margin, tol_conf, tol_score = _tolerances(int(cover.max()))
    top = np.sort(A, axis=0)
    near = (top[-1] - top[-2]) <= margin if K > 1 else np.zeros((Hf, Wf), bool)
    assert near.mean() < 0.01, "the seed leaves too many near-ties in the reference itself"
    dev_in = tuple(torch.from_numpy(a).to(DEV) for a in (probs, score, label))
    out, again = _Out(Hf, Wf, K), _Out(Hf, Wf, K)
    assert _call(lib, dev_in, wins, Hf, Wf, K, 0.0, K, out) == 0 and _call(lib, dev_in, wins, Hf, Wf, K, 0.0, K, again) == 0
    assert out.guards_intact() and all(torch.equal(out.bufs[k], again.bufs[k]) for k in out.bufs)      # two runs: equal bytes
    got = out.get("label_map").reshape(Hf, Wf)
    want = A.argmax(0)
    assert np.array_equal(got[~near], want[~near])
    assert (A.max(0) - np.take_along_axis(A, got[None].astype(np.int64), 0)[0] <= margin)[near].all()
    want = np.where(near, got, want)
    conf = A.max(0) / cover
    err = np.abs(out.get("conf").reshape(Hf, Wf) - conf).max()
    print(f"MEASURED {name}: near-tie pixels {int(near.sum())}, max |conf - ref| {err:.3g} (tolerance {tol_conf:.3g})")
    assert err <= tol_conf + margin * near.any()
    stored, dropped = R.class_stats(want, conf, K, 0.0, K)
    assert len(stored) < K or name != "one_view_q128_k255"       # a class that wins no pixel
    _check_packed(out, stored, dropped, Hf, Wf, tol_score)
    if N == 1 and (Hf, Wf) == (64, 64):      # one tile-sized view: the per-query winner of fx_seg_postprocess names the same classes
        pp = _Out(Hf, Wf, Q)
        winner = torch.zeros(Hf, Wf, dtype=torch.uint8, device=DEV)
        nb = lib.fx_seg_postprocess_workspace_bytes(1, Q, HL, HL, Hf, Wf)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        q_idx = torch.zeros(Q, dtype=torch.int32, device=DEV)
        _lib.check(lib.fx_seg_postprocess(dev_in[0].data_ptr(), HL, HL, Hf, Wf, dev_in[1].data_ptr(), dev_in[2].data_ptr(), 1, Q, 0.0, 0,
                                          ws.data_ptr(), ws.numel(), pp.ptr("det_count"), q_idx.data_ptr(), pp.ptr("det_score"), pp.ptr("det_label"),
                                          pp.ptr("det_box"), pp.ptr("det_area"), None, winner.data_ptr(), _stream()), "fx_seg_postprocess")
        torch.cuda.synchronize()
        assert np.array_equal(label[0][winner.cpu().numpy()][~near], got[~near])
    if name == "snapped_2x2":      # a threshold between two classes' scores drops the lower ones; one plane too few drops the last class
        scores = sorted(s for *_, s in stored)
        assert len(scores) >= 3 and scores[1] - scores[0] > 4 * tol_score
        thr = (scores[0] + scores[1]) / 2
        kept, _ = R.class_stats(want, conf, K, thr, K)
        assert len(kept) == len(stored) - 1
        few = _Out(Hf, Wf, len(kept) - 1)
        assert _call(lib, dev_in, wins, Hf, Wf, K, thr, len(kept) - 1, few) == 0 and few.guards_intact()
        _check_packed(few, kept[:-1], 1, Hf, Wf, tol_score)


def _check_packed(out, stored, dropped, Hf, Wf, tol_score):
    n, label_map = len(stored), out.get("label_map").reshape(Hf, Wf)
    assert int(out.get("det_count")[0]) == n and int(out.get("status")[0]) == dropped
    assert out.get("det_label")[:n].tolist() == [c for c, *_ in stored] and out.get("det_area")[:n].tolist() == [a for _, a, *_ in stored]
    assert out.get("det_box").reshape(-1, 4)[:n].tolist() == [b for _, _, b, _ in stored]
    assert np.abs(out.get("det_score")[:n] - np.array([s for *_, s in stored])).max(initial=0) <= tol_score
    assert not out.get("det_label")[n:].any() and not out.get("det_score")[n:].any() and not out.get("det_box")[4 * n:].any()
    words = out.get("mask_words").reshape(-1, Hf, (Wf + 31) // 32)
    bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")      # the planes are the kernel's OWN label map, pad bits zero
    for j, (c, *_) in enumerate(stored):
        assert np.array_equal(bits[j, :, :Wf], label_map == c) and not bits[j, :, Wf:].any(), c


def test_refused_arguments_leave_the_outputs_untouched():
    lib = _lib.load("bf16")
    Hf, Wf, Q, K = 64, 100, 4, 3
    wins = tile_grid(Hf, Wf, 64, 64, 0.2)
    probs, score, label = _inputs(7, 10, Q, K)      # ten views of data, so that no refused call could read past a buffer
    dev_in = tuple(torch.from_numpy(a).to(DEV) for a in (probs, score, label))
    two = tuple(t[:2] for t in dev_in)
    out = _Out(Hf, Wf, K)
    outside, gap = wins.copy(), wins.copy()
    outside[1, 0] += 1          # the second window leaves the frame
    gap[1, 0] += 1              # ... or, one pixel narrower as well, stays inside and leaves a column uncovered
    gap[1, 2] -= 2
    for over in (dict(wins_host=outside), dict(wins_host=gap), dict(wins_host=wins[:1]), dict(bad_Q=129), dict(bad_K=256), dict(label_map=None),
                 dict(ws_bytes=1024), dict(wins_host=np.tile([[0, 0, Wf, Hf]], (10, 1)))):
        src = dev_in if len(over.get("wins_host", wins)) == 10 else two
        assert _call(lib, src, wins, Hf, Wf, K, 0.0, K, out, **over) == INVALID, list(over)
    assert out.untouched()
    assert _call(lib, two, wins, Hf, Wf, K, 0.0, K, out) == 0 and out.guards_intact() and not out.untouched()


def test_segment_tiled_equals_the_pieces_composed_by_hand():
    from focoos_amd.mask_png import decode_png
    from focoos_amd.mask_rle import rle_decode
    from focoos_amd.processor import trim_mask
    from focoos_amd.model import ModelManager
    from focoos_amd.synth import synth_image_structured
    from focoos_amd.tiled import gather_views

    fm = ModelManager.get("bisenetformer-s-ade", device=DEV, seed=3)
    lib = _lib.load("bf16")
    frame = synth_image_structured(5, 150, 200)
    kw = dict(tile=64, overlap=0.2, batch_size=5, threshold=0.0, return_label_map=True, mask_format="rle")
    res, res_map = fm.segment_tiled(frame, **kw)
    # by hand: gather, the engine chunk by chunk, the merge
    wins = tile_grid(150, 200, 64, 64, 0.2)
    N = len(wins)
    assert N > 5 and N % 5      # several chunks, the last one padded
    wh = torch.from_numpy(wins)
    wd = wh.to(DEV)
    views = torch.zeros(-(-N // 5) * 5, 64, 64, 3, dtype=torch.float32, device=DEV)
    gather_views(lib, torch.from_numpy(frame).to(DEV), wh, wd, views)
    chunks = []
    for c0 in range(0, views.shape[0], 5):
        pl = fm.model.detect(views[c0:c0 + 5])
        chunks.append([t.clone() for t in (pl.mask_probs, pl.cls_score, pl.cls_label)])
    probs, score, label = (torch.cat([c[i] for c in chunks]) for i in range(3))
    K = fm.model.num_classes
    hand = TS.merge_views(lib, probs, score, label, wh, wd, (150, 200), K, 0.0, K)
    torch.cuda.synchronize()
    lm = hand.label_map.cpu().numpy()
    n = int(hand.det_count.item())
    assert n >= 1 and np.array_equal(res_map, lm) and res_map.dtype == np.uint8
    assert [d.cls_id for d in res.detections] == hand.det_labels[0, :n].tolist() == sorted(set(lm.ravel().tolist()) & set(hand.det_labels[0, :n].tolist()))
    assert [d.bbox for d in res.detections] == hand.det_boxes[0, :n].tolist() and [d.conf for d in res.detections] == hand.det_scores[0, :n].tolist()
    for d in res.detections:
        assert d.label == fm.model_info.classes[d.cls_id] and np.array_equal(rle_decode(d.rle), lm == d.cls_id)
    again, again_map = fm.segment_tiled(frame, **kw)
    assert np.array_equal(again_map, res_map) and again.detections == res.detections
    # the other readers of the packed result: the host PNG path, the device PNG encoder and the annotator
    kw.update(return_label_map=False)
    plain, drawn = fm.segment_tiled(frame, **dict(kw, mask_format="png")), fm.segment_tiled(frame, **dict(kw, mask_format="png_device", annotate=True))
    assert drawn.image.shape == frame.shape and drawn.image.dtype == np.uint8 and (drawn.image != frame).any()
    assert len(plain.detections) == len(drawn.detections) == n
    for r, p, d in zip(res.detections, plain.detections, drawn.detections):
        crop = trim_mask(lm == r.cls_id, r.bbox)
        assert crop.size == 0 or (np.array_equal(decode_png(p.mask), crop) and np.array_equal(decode_png(d.mask), crop))
