"""Connected components on a real MI355X (csrc/mask_components.hip): fx_mask_components against the host restatement
(``components.split_numpy``, built on ``label_components``), then ``components=`` end to end on the two mask families with seeded
synthetic weights.  Integers only: everything is compared for equality, the scores as bit patterns."""
import types
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import components as CC
from focoos_amd.mask_rle import rle_decode

from .test_gpu_mask_polygon import _batches, _full, fm  # noqa: F401  (the synthetic models of the mask tests)

pytestmark = pytest.mark.gpu
DEV, INVALID = "cuda:0", -1
OUT = ("count", "scores", "labels", "boxes", "area", "source", "words", "status")


def _pack(mask):
    H, W = mask.shape
    bits = np.zeros((H, (W + 31) // 32 * 32), bool)
    bits[:, :W] = mask
    return np.packbits(bits, axis=-1, bitorder="little").view("<i4")


def _noise(H, W, density, seed=0):
    return np.random.RandomState(seed).rand(H, W) < density


def _inputs(slots, count, labels=None):
    """slots[b][j]: a bool mask, or None for a slot of poison (all-ones words, a wild box).  Boxes alternate between the tight one and the
    full frame.  -> H, W and the five input arrays."""
    B, Q = len(slots), len(slots[0])
    H, W = next(m for row in slots for m in row if m is not None).shape
    words, boxes = np.full((B, Q, H, (W + 31) // 32), -1, np.int32), np.full((B, Q, 4), [-9, -9, 10 ** 6, 10 ** 6], np.int32)
    for b, j in np.ndindex(B, Q):
        m = slots[b][j]
        if m is not None:
            yy, xx = np.nonzero(m)
            words[b, j] = _pack(m)
            boxes[b, j] = (xx.min(), yy.min(), xx.max(), yy.max()) if (b + j) % 2 == 0 and m.any() else (0, 0, W - 1, H - 1)
    scores = np.random.RandomState(1).rand(B, Q).astype(np.float32)
    labels = np.zeros((B, Q), np.int32) if labels is None else np.asarray(labels, np.int32)
    return H, W, words, np.asarray(count, np.int32), scores, labels, boxes


def run(slots, count, conn, min_area=1, M=256, cap=1024, labels=None, table=None):
    """One fx_mask_components call -> (its outputs per image as numpy arrays, the reference's)."""
    H, W, words, count, scores, labels, boxes = _inputs(slots, count, labels)
    B, Q = words.shape[:2]
    lib = _lib.load()
    dev = [torch.from_numpy(a).to(DEV) for a in (words, count, scores, labels, boxes)]
    tab = None if table is None else torch.tensor(table, dtype=torch.uint8, device=DEV)
    nb = lib.fx_mask_components_workspace_bytes(B, Q, H, W, M, cap)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    o = dict(count=torch.full((B,), -7, **i32), scores=torch.zeros(B, M, device=DEV), labels=torch.zeros(B, M, **i32),
             boxes=torch.zeros(B, M, 4, **i32), area=torch.zeros(B, M, **i32), source=torch.zeros(B, M, **i32),
             words=torch.full((B, M, H, (W + 31) // 32), -1, **i32), status=torch.full((B, 2), -7, **i32))
    assert nb > 0 and lib.fx_mask_components(
        *[t.data_ptr() for t in dev], B, Q, H, W, conn, min_area, None if tab is None else tab.data_ptr(), 0 if tab is None else len(table), M, cap,
        ws.data_ptr(), nb, *[o[k].data_ptr() for k in OUT], torch.cuda.current_stream().cuda_stream) == 0
    got = {k: v.cpu().numpy() for k, v in o.items()}
    cfg = CC.Components(conn, min_area, M)
    ref = [CC.split_numpy(words[b], count[b], scores[b], labels[b], W, cfg, None if table is None else np.asarray(table, np.uint8)) for b in range(B)]
    return got, ref


def same(got, ref, b):
    """Image b of a call equals the reference: the records and planes of its components, zero planes behind them."""
    r, n = ref[b], ref[b].count
    assert got["count"][b] == n and got["status"][b].tolist() == [r.dropped, 0]
    for k in ("labels", "source", "area", "boxes", "words"):
        assert np.array_equal(got[k][b, :n], getattr(r, k)[:n]), k
    assert np.array_equal(got["scores"][b, :n].view(np.int32), r.scores[:n].view(np.int32))
    assert not got["words"][b, n:].any()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("min_area,M", [(1, 512), (4, 512), (1, 8)])
def test_noise_two_slots_poison_and_an_empty_image(conn, min_area, M):
    """W = 70: three words per row, the last one partial.  The same pattern in two slots (tight box, full frame), poison in slot 2 and in
    every slot of image 1, whose det_count is 0.  The two slots have 2 x 179 components in 2 x 642 runs at 4-connectivity: M = 512 and a
    run pool of 2048 hold them."""
    m = _noise(37, 70, 0.5)
    got, ref = run([[m, m, None], [None, None, None]], [2, 0], conn, min_area, M, cap=2048)
    total = ref[0].count + ref[0].dropped
    print(f"conn {conn} min_area {min_area} M {M}: {total} components, {ref[0].count} kept")
    assert total % 2 == 0 and total > 8 and ref[1].count == 0
    assert (ref[0].dropped == 0) == (M == 512) and (M == 512 or (ref[0].count == 8 and ref[0].dropped == total - 8))
    same(got, ref, 0), same(got, ref, 1)
    h = ref[0].count // 2 if M == 512 else 0      # the two slots give the same components, one after the other
    assert np.array_equal(got["words"][0, :h], got["words"][0, h:2 * h]) and got["source"][0, :2 * h].tolist() == [0] * h + [1] * h


def _shapes():
    H, W = 33, 70
    seams = np.zeros((7, W), bool)
    seams[0, 0:32] = seams[1, 31:33] = seams[3, :] = seams[5, W - 1] = seams[6, 32:64] = True
    snake = np.zeros((H, W), bool)      # a one-pixel serpentine: one component whose chain of unions spans every row
    snake[0::2, :] = True
    snake[1::4, W - 1] = snake[3::4, 0] = True
    comb = np.zeros((H, W), bool)       # teeth that join only in the last row
    comb[:, 0::2] = comb[H - 1, :] = True
    checker = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)      # at 4-connectivity every pixel is a component
    return {"seams": seams, "snake": snake, "comb": comb, "checker": checker}


@pytest.mark.parametrize("lds", [None, "0"], ids=["lds", "workspace"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["seams", "snake", "comb", "checker"])
def test_word_seams_and_long_chains(monkeypatch, name, conn, lds):
    if lds is not None:
        monkeypatch.setenv("FX_COMPONENTS_LDS_RUNS", lds)
    m = _shapes()[name]
    got, ref = run([[m]], [1], conn, M=2048, cap=4096)
    want = {"seams": {4: 4, 8: 4}, "snake": {4: 1, 8: 1}, "comb": {4: 1, 8: 1}, "checker": {4: int(m.sum()), 8: 1}}[name][conn]
    assert ref[0].count == want and ref[0].dropped == 0
    same(got, ref, 0)


@pytest.mark.parametrize("conn", [4, 8])
def test_workspace_path_equals_lds_path(monkeypatch, conn):
    m = _noise(150, 97, 0.55)
    got, ref = run([[m]], [1], conn, M=1024, cap=8192)
    monkeypatch.setenv("FX_COMPONENTS_LDS_RUNS", "100")      # the slot has thousands of runs: the state goes to the workspace
    again, _ = run([[m]], [1], conn, M=1024, cap=8192)
    print(f"conn {conn}: {ref[0].count} components")
    assert 20 < ref[0].count < 1024 and ref[0].dropped == 0
    same(got, ref, 0), same(again, ref, 0)
    assert all(np.array_equal(got[k], again[k]) for k in OUT)


@pytest.mark.parametrize("conn", [4, 8])
def test_a_class_that_is_not_split_comes_back_whole(conn):
    m, other = _noise(37, 70, 0.5), _noise(37, 70, 0.5, seed=3)
    got, ref = run([[m, other, m]], [3], conn, labels=[[1, 0, 1]], table=[0, 1], M=512, cap=4096)
    same(got, ref, 0)
    whole = np.flatnonzero(got["source"][0, :ref[0].count] == 1)
    assert len(whole) == 1 and got["area"][0, whole[0]] == other.sum() and np.array_equal(got["words"][0, whole[0]], _pack(other))
    assert ref[0].count > 20 and got["source"][0, :ref[0].count].tolist() == sorted(got["source"][0, :ref[0].count].tolist())


@pytest.mark.parametrize("conn", [4, 8])
def test_run_pool_overflow_and_the_host_fallback(conn):
    m, small = _noise(37, 70, 0.5), _shapes()["seams"]
    small = np.pad(small, ((0, 30), (0, 0)))
    got, ref = run([[m, m], [small, None]], [2, 1], conn, M=1024, cap=256)
    assert got["count"][0] == 0 and got["status"][0].tolist() == [0, 1]      # more than 256 runs: nothing of image 0 is defined
    same(got, ref, 1)
    H, W, words, count, scores, labels, boxes = _inputs([[m, m], [small, None]], [2, 1])
    res = types.SimpleNamespace(mask_words=torch.from_numpy(words).to(DEV), det_count=torch.from_numpy(count).to(DEV), mask_width=W,
                             det_scores=torch.from_numpy(scores).to(DEV), det_labels=torch.from_numpy(labels).to(DEV),
                             det_boxes=torch.from_numpy(boxes).to(DEV))
    dc = CC.DeviceComponents(2, 2, H, W, DEV, CC.Components(conn, 1, 1024), run_capacity=256)
    with pytest.warns(RuntimeWarning, match="labelled on the host"):
        o = dc.split(res)
    host = dict(count=o.det_count, scores=o.det_scores, labels=o.det_labels, boxes=o.det_boxes, area=o.det_area, source=o.det_source,
                words=o.mask_words)
    host = {k: v.cpu().numpy() for k, v in host.items()}
    host["status"] = np.zeros((2, 2), np.int32)
    assert dc.last_fallback == 1 and ref[0].count > 20
    same(host, ref, 0), same(host, ref, 1)


def test_arguments_outside_the_contract_are_refused():
    lib, (B, Q, H, W, M, cap) = _lib.load(), (2, 3, 5, 70, 4, 64)
    i32 = dict(dtype=torch.int32, device=DEV)
    ins = [torch.zeros(s, **i32) for s in ((B, Q, H, 3), (B,))] + [torch.zeros(B, Q, device=DEV), torch.zeros(B, Q, **i32), torch.zeros(B, Q, 4, **i32)]
    outs = [torch.full(s, -7, **i32) for s in ((B,), (B, M), (B, M), (B, M, 4), (B, M), (B, M), (B, M, H, 3), (B, 2))]
    nb = lib.fx_mask_components_workspace_bytes(B, Q, H, W, M, cap)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    base = [t.data_ptr() for t in ins] + [B, Q, H, W, 8, 1, None, 0, M, cap, ws.data_ptr(), nb] + [t.data_ptr() for t in outs] + \
        [torch.cuda.current_stream().cuda_stream]
    for pos, val in [(p, None) for p in (0, 1, 2, 3, 4, 15, 17, 18, 19, 20, 21, 22, 23, 24)] + [
            (0, ins[0].data_ptr() + 2), (5, 0), (6, 65536), (7, 0), (8, 65536), (9, 6), (9, 0), (10, 0), (12, -1), (13, 0), (13, 4097), (14, 0),
            (16, nb - 1)]:
        assert lib.fx_mask_components(*base[:pos], val, *base[pos + 1:]) == INVALID, (pos, val)
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in outs)      # nothing written
    assert lib.fx_mask_components_workspace_bytes(B, Q, H, 65536, M, cap) == 0 and lib.fx_mask_components_workspace_bytes(B, Q, 1 << 16, 1 << 15, M, cap) == 0
    assert lib.fx_mask_components(*base) == 0      # the same arguments unbroken: no detections
    assert outs[0].tolist() == [0, 0] and not outs[7].any() and not outs[6].any()


def test_components_end_to_end(fm, monkeypatch):  # noqa: F811
    from focoos_amd.tracking import DeviceTracker, TrackerConfig

    imgs, cfg = _batches(1)[0], CC.Components(min_area=2, max_components=1024)
    monkeypatch.setattr(fm.processor, "components_run_capacity", 1 << 20)      # seeded weights give ragged masks: room for every run
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # neither the run pool nor the slots overflow
        plain = fm.infer_batch(imgs, threshold=0.05, mask_format="rle")
        split = fm.infer_batch(imgs, threshold=0.05, mask_format="rle", components=cfg)
        tracker = DeviceTracker(2, TrackerConfig(high=0.02, low=0.01, new_thresh=0.02, max_tracks=1024), DEV)
        tracked = fm.infer_batch(imgs, threshold=0.05, mask_format="rle", components=cfg, tracker=tracker)
        none = fm.infer_batch(imgs, threshold=0.05, mask_format="rle", components=None)
    assert [_full(r) for r in none] == [_full(r) for r in plain]
    assert [[(d.bbox, d.rle) for d in r.detections] for r in tracked] == [[(d.bbox, d.rle) for d in r.detections] for r in split]
    # the tracker gives an id to every detection it can start a track from: a box of positive extent (track_ops.hip; x1 > x0 and y1 > y0
    # in the inclusive convention) - so every component does but those one pixel wide or high
    ids = [(d.track_id is not None, d.bbox[2] > d.bbox[0] and d.bbox[3] > d.bbox[1]) for r in tracked for d in r.detections]
    assert all(has == wide for has, wide in ids) and sum(has for has, _ in ids) > 0
    for p, s in zip(plain, split):
        print(f"{fm.model.family}: {len(p.detections)} masks, {len(s.detections)} components")
        assert len(s.detections) >= len(p.detections) > 0
        parts = iter(s.detections)
        for d in p.detections:      # the components come in the order of their masks
            mask = rle_decode(d.rle)
            lab = CC.label_components(mask, 8)
            areas = np.bincount(lab.ravel())[1:]
            want = np.isin(lab, 1 + np.flatnonzero(areas >= 2))      # the mask less its specks
            union = np.zeros_like(mask)
            for _ in range(int((areas >= 2).sum())):
                c = next(parts)
                m = rle_decode(c.rle)
                yy, xx = np.nonzero(m)
                assert (c.cls_id, c.conf) == (d.cls_id, d.conf) and list(c.bbox) == [xx.min(), yy.min(), xx.max(), yy.max()]
                assert CC.label_components(m, 8).max() == 1 and not (union & m).any()
                union |= m
            assert np.array_equal(union, want)
        assert next(parts, None) is None
