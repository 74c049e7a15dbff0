"""Tiled inference on a real MI355X (csrc/tile_ops.hip through focoos_amd/tiled.py): the gather against fx_resize_bilinear_u8 on host crops
(bit for bit), the merge against the numpy restatement of tests/tiled_ref.py (equality), and FocoosModel.infer_tiled against the same
pieces composed by hand.  Nothing here reads the reference tree."""
import warnings

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import tiled as T
from focoos_amd.synth import synth_image_structured

from . import tiled_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # FX_ERR_INVALID_ARGUMENT
FH, FW = 157, 203


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _windows(Ho, Wo):
    """8 windows (x0, y0, w, h) of the 157 x 203 frame: identity size, snapped to each of the four borders, the whole frame (a 3.2x
    downscale at these sizes), a 1.5x upscale of a small window, one pixel wide."""
    return np.array([[30, 20, Wo, Ho], [0, 40, 100, 80], [FW - 90, 30, 90, 70], [50, 0, 77, 31], [20, FH - 60, 120, 60], [0, 0, FW, FH],
                     [60, 50, round(Wo / 1.5), round(Ho / 1.5)], [100, 10, 1, 90]], dtype=np.int32)


def _gather(lib, frame_d, wins, out):
    wh = torch.from_numpy(wins)
    wd = wh.to(DEV)
    return lib.fx_tile_gather_u8_f32(frame_d.data_ptr(), frame_d.shape[0], frame_d.shape[1], wd.data_ptr(), wh.data_ptr(), len(wins), out.data_ptr(),
                                     out.shape[1], out.shape[2], _stream())


@pytest.mark.parametrize("Ho,Wo", [(48, 64), (45, 63)], ids=["vec16", "scalar"])
def test_gather_equals_resize_of_the_host_crop(Ho, Wo):
    lib = _lib.load("bf16")
    frame = synth_image_structured(3, FH, FW)
    frame_d = torch.from_numpy(frame).to(DEV)
    wins = _windows(Ho, Wo)
    N = len(wins)
    buf = torch.full((N + 2, Ho, Wo, 3), -7.0, dtype=torch.float32, device=DEV)     # a canary view on either side
    out = buf[1:N + 1]
    assert _gather(lib, frame_d, wins, out) == 0
    torch.cuda.synchronize()
    assert bool((buf[0] == -7.0).all()) and bool((buf[-1] == -7.0).all())
    got = out.cpu()
    for n, (x0, y0, w, h) in enumerate(wins.tolist()):
        crop = torch.from_numpy(np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w])).to(DEV)
        want = torch.empty(Ho, Wo, 3, dtype=torch.float32, device=DEV)
        _lib.check(lib.fx_resize_bilinear_u8(crop.data_ptr(), h, w, want.data_ptr(), Ho, Wo, _stream()), "fx_resize_bilinear_u8")
        torch.cuda.synchronize()
        assert torch.equal(got[n], want.cpu()), (n, (x0, y0, w, h))
    # a window of exactly (Ho, Wo) holds the frame's bytes as floats
    assert torch.equal(got[0], torch.from_numpy(frame[20:20 + Ho, 30:30 + Wo].astype(np.float32)))


def test_gather_refuses_bad_windows_and_launches_nothing():
    lib = _lib.load("bf16")
    frame_d = torch.from_numpy(synth_image_structured(3, FH, FW)).to(DEV)
    out = torch.full((2, 48, 64, 3), -7.0, dtype=torch.float32, device=DEV)
    good = [0, 0, 64, 48]
    for bad in ([FW - 63, 0, 64, 48], [0, FH - 47, 64, 48], [-1, 0, 64, 48], [0, -1, 64, 48], [0, 0, 0, 48], [0, 0, 64, 0], [0, 0, FW + 1, 48]):
        assert _gather(lib, frame_d, np.array([good, bad], dtype=np.int32), out) == INVALID, bad
    wh = torch.tensor([good], dtype=torch.int32)
    wd = wh.to(DEV)
    args = lambda **k: [k.get("frame", frame_d.data_ptr()), FH, FW, k.get("wd", wd.data_ptr()), k.get("wh", wh.data_ptr()), k.get("N", 1),
                        k.get("out", out.data_ptr()), k.get("Ho", 48), k.get("Wo", 64), _stream()]
    for k in (dict(frame=None), dict(wd=None), dict(wh=None), dict(out=None), dict(N=0), dict(N=65536), dict(Ho=0), dict(Wo=16385)):
        assert lib.fx_tile_gather_u8_f32(*args(**k)) == INVALID, k
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---------------------------------------------------------------- merge
FRAME = 512


def _merge_case(seed, M, N, Tk, labels_n=3):
    """M candidates spread raggedly over N views of Tk slots: integer boxes in window pixels, window origins that keep most boxes inside a
    512 x 512 frame (some are clamped), few labels and few distinct scores (ties), garbage with high scores in the slots past the count."""
    rs = np.random.RandomState(seed)
    count = rs.multinomial(M, np.ones(N) / N).astype(np.int32)
    assert count.sum() == M and count.max(initial=0) <= Tk
    wins = np.concatenate([rs.randint(0, 200, (N, 2)), np.full((N, 2), 320)], 1).astype(np.int32)
    xy = rs.randint(-10, 320, (N, Tk, 2))
    boxes = np.concatenate([xy, xy + rs.randint(0, 220, (N, Tk, 2))], -1).astype(np.int32)
    labels = rs.randint(0, labels_n, (N, Tk)).astype(np.int32)
    scores = (rs.randint(1, 24, (N, Tk)) / np.float32(24)).astype(np.float32)
    for n in range(N):
        scores[n, count[n]:] = 2.0
    return scores, labels, boxes, count, wins


def _run_merge(lib, scores, labels, boxes, count, wins, thr, metric, max_det):
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (scores, labels, boxes, count, wins)]
    o_s, o_l, o_b, cs = T.merge_detections(lib, d[0], d[1], d[2], d[3], d[4], scores.shape[0], (FRAME, FRAME), thr, metric, max_det)
    torch.cuda.synchronize()
    return o_s[0].cpu().numpy(), o_l[0].cpu().numpy(), o_b[0].cpu().numpy(), cs.cpu().numpy()


def _check_merge(lib, case, thr, metric, max_det):
    scores, labels, boxes, count, wins = case
    ws, wl, wb, dropped = R.merge(scores, labels, boxes, count, wins, (FRAME, FRAME), thr, metric, max_det)
    gs, gl, gb, cs = _run_merge(lib, scores, labels, boxes, count, wins, thr, metric, max_det)
    k = len(ws)
    assert int(cs[0]) == k and int(cs[1]) == dropped, (cs.tolist(), k, dropped)
    assert np.array_equal(gs[:k], ws) and np.array_equal(gl[:k], wl) and np.array_equal(gb[:k], wb)
    assert not gs[k:].any() and not gl[k:].any() and not gb[k:].any()       # slots past the count are zero
    return k


@pytest.mark.parametrize("N", [1, 3, 7])
@pytest.mark.parametrize("M", [0, 1, 5, 64, 65, 130])
def test_merge_equals_the_numpy_restatement(M, N):
    lib = _lib.load("bf16")
    case = _merge_case(100 * M + N, M, N, 160)
    kept = [_check_merge(lib, case, thr, metric, 300) for metric, thr in (("iou", 0.5), ("ios", 0.5), ("iou", 0.3), ("ios", 0.8))]
    if M >= 64:
        assert min(kept) < M          # something was suppressed: the case is not vacuous


def test_merge_cap_drops_the_rest_and_counts_them():
    lib = _lib.load("bf16")
    case = _merge_case(7, R.NMS_CAP + 40, 7, 700, labels_n=5)
    for metric in ("iou", "ios"):
        scores, labels, boxes, count, wins = case
        _check_merge(lib, case, 0.5, metric, 300)
        assert int(_run_merge(lib, scores, labels, boxes, count, wins, 0.5, metric, 300)[3][1]) == 40


def test_merge_max_detections_below_the_survivors():
    lib = _lib.load("bf16")
    case = _merge_case(11, 130, 3, 160)
    assert len(R.merge(*case, (FRAME, FRAME), 0.5, "iou", 10_000)[0]) > 7
    assert _check_merge(lib, case, 0.5, "iou", 7) == 7
    assert _check_merge(lib, case, 0.5, "iou", 1) == 1


def test_merge_refuses_bad_arguments_and_launches_nothing():
    lib = _lib.load("bf16")
    N, Tk, D = 2, 8, 4
    scores, labels, boxes, count, wins = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in _merge_case(1, 6, N, Tk)]
    o_s = torch.full((D,), -7.0, dtype=torch.float32, device=DEV)
    o_l = torch.full((D,), -7, dtype=torch.int32, device=DEV)
    o_b = torch.full((D + 1, 4), -7, dtype=torch.int32, device=DEV)
    cs = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    need = int(lib.fx_merge_detections_workspace_bytes(N, Tk))
    assert need > 0 and lib.fx_merge_detections_workspace_bytes(0, Tk) == 0 and lib.fx_merge_detections_workspace_bytes(1 << 16, 1 << 15) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    base = dict(scores=scores.data_ptr(), labels=labels.data_ptr(), boxes=boxes.data_ptr(), count=count.data_ptr(), wins=wins.data_ptr(), N=N, T=Tk,
                H=FRAME, W=FRAME, thr=0.5, metric=0, D=D, o_s=o_s.data_ptr(), o_l=o_l.data_ptr(), o_b=o_b.data_ptr(), o_c=cs.data_ptr(),
                st=cs.data_ptr() + 4, ws=ws.data_ptr(), wsb=need)
    order = ["scores", "labels", "boxes", "count", "wins", "N", "T", "H", "W", "thr", "metric", "D", "o_s", "o_l", "o_b", "o_c", "st", "ws", "wsb"]
    call = lambda **k: lib.fx_merge_detections_nms(*[dict(base, **k)[n] for n in order], _stream())
    bad = [{p: None} for p in ("scores", "labels", "boxes", "count", "wins", "o_s", "o_l", "o_b", "o_c", "st", "ws")]
    bad += [dict(scores=base["scores"] + 2), dict(o_b=base["o_b"] + 4), dict(ws=base["ws"] + 8), dict(wsb=need - 1), dict(N=0), dict(T=0),
            dict(N=1 << 16, T=1 << 15), dict(H=0), dict(W=16385), dict(thr=0.0), dict(thr=1.5), dict(metric=2), dict(D=0)]
    for k in bad:
        assert call(**k) == INVALID, k
    torch.cuda.synchronize()
    assert bool((o_s == -7.0).all()) and bool((o_l == -7).all()) and bool((o_b == -7).all()) and bool((cs == -7).all())
    cs.zero_()
    assert call() == 0                      # the same arguments unbroken run
    torch.cuda.synchronize()
    assert 1 <= int(cs[0]) <= D and int(cs[1]) == 0


# ---------------------------------------------------------------- end to end
def _dets(res):
    return [(tuple(d.bbox), d.conf, d.cls_id, d.label) for d in res.detections]


def test_infer_tiled_equals_the_pieces_composed_by_hand():
    """700 x 900 frame, tile 320, overlap 0.25: 4 x 3 windows + the whole frame = 13 views in chunks of 4, so the last chunk carries 3
    zero views.  Expected = the gather's own output through model.detect in the same chunks, origins added on the host, tiled_ref NMS."""
    from focoos_amd.model import ModelManager

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "no pretrained weights: seeded synthetic weights"
        fm = ModelManager.get("fai-detr-m-coco", seed=3)
    lib = _lib.load("bf16")
    frame = synth_image_structured(21, 700, 900)
    kw = dict(tile=320, overlap=0.25, threshold=0.01, batch_size=4)
    res = fm.infer_tiled(frame, **kw)
    again = fm.infer_tiled(torch.from_numpy(frame).permute(2, 0, 1), **kw)      # CHW tensor input, second call on the same plan

    wins = T.views_of(700, 900, 320, 320, 0.25, True)
    assert len(wins) == 13 and wins[-1].tolist() == [0, 0, 900, 700]
    views = torch.zeros(16, 320, 320, 3, dtype=torch.float32, device=DEV)
    wh = torch.from_numpy(wins)
    T.gather_views(lib, torch.from_numpy(frame).to(DEV), wh, wh.to(DEV), views)
    sizes = np.full((16, 2), 320, dtype=np.int32)
    sizes[:13] = wins[:, [3, 2]]
    parts = []
    for c0 in range(0, 16, 4):
        pl = fm.model.detect(views[c0:c0 + 4], sizes=torch.from_numpy(sizes[c0:c0 + 4]).to(DEV), threshold=0.01)
        torch.cuda.synchronize()
        parts.append([t.cpu().numpy().copy() for t in (pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)])
    s, l, b, c = (np.concatenate([p[i] for p in parts], 0)[:13] for i in range(4))
    ws, wl, wb, dropped = R.merge(s, l, b, c, wins, (700, 900), 0.5, "iou", 300)
    print(f"candidates {int(c.sum())} of {13 * s.shape[1]} slots, survivors {len(ws)}, dropped by the cap {dropped}")
    assert int(c.sum()) > 13 and len(ws) > 1                # random weights at threshold 0.01: the merge has work to do
    classes = fm.model_info.classes
    want = [(tuple(int(v) for v in wb[i]), float(ws[i]), int(wl[i]), classes[int(wl[i])]) for i in range(len(ws))]
    assert _dets(res) == want
    assert _dets(again) == want
    assert all(0 <= x0 <= x1 <= 900 and 0 <= y0 <= y1 <= 700 for (x0, y0, x1, y1), *_ in want)
    assert res.latency is not None and res.latency.inference > 0
