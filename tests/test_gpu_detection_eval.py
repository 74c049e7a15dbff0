"""COCO bbox AP on the MI355X: fx_detr_eval_boxes_f32 against DETRProcessor.eval_postprocess bit for bit, fx_coco_match_bbox
(csrc/coco_eval.hip) against the naive restatement tests/cocoeval_ref.py with zero exceptions (LDS and workspace paths), the refusals,
and FocoosModel.eval_detection end to end against DetectionEvaluator fed from eval_postprocess.  Gates: DESIGN.md section 12; measured
values are printed (``MEASURED``)."""
import ctypes
import json
import time

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import detection_eval as D
from focoos_amd.ports import DETRModelOutput, DetectionDatasetEntry, TrainerArgs
from focoos_amd.synth import synth_image_structured
from tests import cocoeval_ref as R
from tests import detection_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = time.perf_counter()


@pytest.mark.parametrize("B", [1, 5])
def test_eval_boxes_equal_eval_postprocess(B):
    from focoos_amd.processor import DETRProcessor

    g = torch.Generator().manual_seed(B)
    Q, K, T = 300, 80, 300
    probs = torch.rand(B, Q, K, generator=g)
    cxcywh = torch.rand(B, Q, 4, generator=g) * torch.tensor([1.2, 1.2, 0.5, 0.5]) - torch.tensor([0.1, 0.1, 0.0, 0.0])
    boxes = torch.cat([cxcywh[..., :2] - cxcywh[..., 2:] / 2, cxcywh[..., :2] + cxcywh[..., 2:] / 2], -1)
    boxes[0, :7, 2] = boxes[0, :7, 0]            # empty boxes ...
    boxes[0, 7:12] = boxes[0, 7:12].abs() + 1.0  # ... and boxes outside the image: degenerate after clipping
    probs[0, :12] += 1.0                         # that the top-k selects
    sizes = [(480, 640), (333, 500), (1, 1), (720, 1280), (97, 31)][:B]
    ents = [{"height": h, "width": w} for h, w in sizes]
    probs_d, boxes_d = probs.to(DEV), boxes.to(DEV)
    want = DETRProcessor({"top_k": T, "threshold": 0.5}, 640).eval_postprocess(DETRModelOutput(logits=probs_d, boxes=boxes_d, loss=None), ents)
    score, label, keep, xyxy, xywh = (t.cpu() for t in D.eval_boxes(probs_d, boxes_d, sizes, T))
    dropped = 0
    for i in range(B):
        inst = want[i]["instances"]
        k = keep[i] != 0
        dropped += int((~k).sum())
        assert int(k.sum()) == len(inst)
        assert torch.equal(label[i][k].long(), inst.classes.cpu().long()) and torch.equal(score[i][k], inst.scores.cpu())
        wb = inst.boxes.tensor.cpu()
        assert torch.equal(xyxy[i][k], wb)
        ref = wb.numpy().copy()                   # BoxMode.convert XYXY_ABS -> XYWH_ABS on the float32 array
        ref[:, 2] -= ref[:, 0]
        ref[:, 3] -= ref[:, 1]
        assert np.array_equal(xywh[i][k].numpy(), ref)
    assert dropped >= 12 or B > 1
    print(f"MEASURED eval_boxes B={B}: {dropped} of {B * T} slots dropped by nonempty(), everything else equal bit for bit")


def _device_scene(scene):
    """a scene as the kernel's inputs: [B, T] slots, detections first, the padding with keep = 0"""
    ims = scene["images"]
    B, T = len(ims), max(1, max(len(im["score"]) for im in ims))
    label, score = np.zeros((B, T), np.int32), np.zeros((B, T), np.float32)
    keep, xywh = np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.float32)
    for b, im in enumerate(ims):
        n = len(im["score"])
        bx = im["xyxy"].astype(np.float32)
        label[b, :n], score[b, :n], keep[b, :n] = im["cls"], im["score"], 1
        xywh[b, :n] = np.stack([bx[:, 0], bx[:, 1], bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], 1) if n else 0
    gts = [D.ground_truth(DetectionDatasetEntry(annotations=im["gts"])) for im in ims]
    return [torch.from_numpy(a).to(DEV) for a in (label, score, keep, xywh)], gts


def _check_scene(scene, tag, expect_ws=None):
    K = len(scene["class_names"])
    (label, score, keep, xywh), gts = _device_scene(scene)
    npig = torch.zeros(K, 4, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rank, matched, ignored = D.device_match(label, score, keep, xywh, gts, K, npig, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    rank, matched, ignored = rank.cpu().numpy(), matched.cpu().numpy().view(np.uint64), ignored.cpu().numpy().view(np.uint64)
    ref = R.evaluate_images(S.ref_images(scene), K)
    want_rank = np.full(rank.shape, -1, np.int32)
    want_m, want_i = np.zeros(rank.shape, np.uint64), np.zeros(rank.shape, np.uint64)
    want_npig = np.zeros((K, 4), np.int64)
    for (img, c), e in ref.items():
        b = [im["image_id"] for im in scene["images"]].index(img)
        slots = np.flatnonzero(scene["images"][b]["cls"] == c)
        for a in range(4):
            want_npig[c, a] += e["npig"][a]
        for r, j in enumerate(e["order"]):
            s = slots[j]
            want_rank[b, s] = r
            for a in range(4):
                for t in range(10):
                    want_m[b, s] |= np.uint64(int(e["matched"][a][t][r]) << (10 * a + t))
                    want_i[b, s] |= np.uint64(int(e["ignored"][a][t][r]) << (10 * a + t))
    n_scored = int((want_rank >= 0).sum())
    bad = int((rank != want_rank).sum()) + int((matched != want_m).sum()) + int((ignored != want_i).sum())
    assert bad == 0, f"{tag}: {bad} rank / matched / ignored words differ"
    assert np.array_equal(npig.cpu().numpy(), want_npig), tag
    max_gt = max([0] + [int(np.unique(g[1], return_counts=True)[1].max()) for g in gts if len(g[1])])
    used_ws = int(_lib.load("bf16").fx_coco_match_workspace_bytes(max_gt)) > 0
    assert expect_ws is None or used_ws == expect_ws, (tag, max_gt)
    D.device_match(label, score, keep, xywh, gts, K, npig, status)      # a second call accumulates
    torch.cuda.synchronize()
    assert np.array_equal(npig.cpu().numpy(), 2 * want_npig) and int(status.item()) == 0
    return n_scored, int(want_npig.sum()), used_ws


def test_match_kernel_equals_restatement_on_random_scenes():
    scored = gt = nws = 0
    for seed in range(200):
        s, g, w = _check_scene(S.make_scene(seed), f"scene {seed}")
        scored, gt, nws = scored + s, gt + g, nws + int(w)
    print(f"MEASURED match kernel, 200 random scenes ({nws} with a workspace): {scored} scored detections x 40 decisions, {gt} non-ignored "
          "gt counts, 0 differences")


def test_match_kernel_on_hand_derived_cases():
    """the cases of tests/golden/coco_bbox_cases.json (crowd, ``ignore`` without crowd, equal IoUs, the 101st detection, ...) on the device"""
    import os

    with open(os.path.join(os.path.dirname(__file__), "golden", "coco_bbox_cases.json")) as f:
        cases = json.load(f)["cases"]
    assert any("ignore" in g for c in cases for im in c["images"] for g in im["gts"])
    for c in cases:
        _check_scene(S.golden_scene(c), c["name"], expect_ws=False)
    print(f"MEASURED match kernel, {len(cases)} hand-derived cases: 0 differences")


def test_match_kernel_workspace_path_and_one_sided_categories():
    big = S.make_scene(1000, n_images=1, n_classes=1, max_gt=0, max_det=150)
    rs = np.random.RandomState(5)
    x0, y0 = rs.randint(0, 900, size=700) / 4.0, rs.randint(0, 900, size=700) / 4.0
    wh = rs.randint(4, 120, size=(700, 2)) / 4.0
    big["images"][0]["gts"] = [{"bbox": [float(a), float(b), float(c), float(d)], "category_id": 0, "iscrowd": int(rs.rand() < 0.1)}
                               for a, b, (c, d) in zip(x0, y0, wh)]
    if len(big["images"][0]["score"]) == 0:
        big = None
    assert big is not None
    s, g, _ = _check_scene(big, "G = 700", expect_ws=True)
    print(f"MEASURED match kernel, workspace path: G = 700, {s} scored detections, {g} non-ignored gt counts, 0 differences")
    one = S.make_scene(1001, n_images=2, n_classes=2, max_gt=20, max_det=60)
    for im in one["images"]:
        im["cls"][:] = 0                      # detections of class 0 only ...
        for gg in im["gts"]:
            gg["category_id"] = 1             # ... ground truth of class 1 only
    one["images"][0]["gts"] = one["images"][0]["gts"] or [{"bbox": [1.0, 1.0, 8.0, 8.0], "category_id": 1, "iscrowd": 0}]
    s, g, _ = _check_scene(one, "one-sided categories", expect_ws=False)
    assert s > 0 and g > 0
    empty = S.make_scene(1002, n_images=2, n_classes=3)
    empty["images"][1]["xyxy"], empty["images"][1]["score"] = np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    empty["images"][1]["cls"] = np.zeros(0, np.int64)     # an image without predictions: its ground truth must not be counted
    _check_scene(empty, "image without predictions")


def test_invalid_arguments_leave_outputs_untouched():
    lib = _lib.load("bf16")
    B, T, K, Q = 2, 8, 3, 4
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)   # noqa: E731
    label, keep, score, xywh = i32(B, T), i32(B, T) + 1, torch.rand(B, T, device=DEV), torch.rand(B, T, 4, device=DEV)
    gbox, gcat, gflag = torch.rand(4, 4, dtype=torch.float64, device=DEV), i32(4), i32(4)
    garea = torch.rand(4, dtype=torch.float64, device=DEV)
    offs = np.array([0, 2, 4], np.int64)
    off_d = torch.from_numpy(offs).to(DEV)
    rank = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    m, ig = torch.full((B, T), -7, dtype=torch.int64, device=DEV), torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    npig, status = torch.full((K, 4), -7, dtype=torch.int64, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(max(16, int(lib.fx_coco_match_workspace_bytes(700))), dtype=torch.uint8, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(label_p=label.data_ptr(), Kx=K, Tx=T, off_host=offs, n_gt=4, max_gt=2, gbox_p=gbox.data_ptr(), rank_p=rank.data_ptr(),
             m_p=m.data_ptr(), ws_p=None, ws_n=0, npig_p=npig.data_ptr()):
        return lib.fx_coco_match_bbox(label_p, score.data_ptr(), keep.data_ptr(), xywh.data_ptr(), B, Tx, Kx, gbox_p, gcat.data_ptr(),
                                      gflag.data_ptr(), garea.data_ptr(), off_d.data_ptr(), off_host.ctypes.data, n_gt, max_gt, rank_p, m_p,
                                      ig.data_ptr(), npig_p, status.data_ptr(), ws_p, ws_n, s)

    rcs = [call(label_p=None), call(Kx=0), call(Kx=-3), call(Tx=0), call(off_host=np.array([-1, 2, 4], np.int64)),
           call(off_host=np.array([0, 3, 2], np.int64)), call(off_host=np.array([0, 2, 5], np.int64)), call(n_gt=-1), call(max_gt=-1),
           call(gbox_p=None), call(gbox_p=gbox.data_ptr() + 4), call(rank_p=rank.data_ptr() + 2), call(m_p=m.data_ptr() + 4),
           call(npig_p=None), call(max_gt=700), call(max_gt=700, ws_p=ws.data_ptr(), ws_n=ws.numel() - 1),
           call(max_gt=700, ws_p=ws.data_ptr() + 8, ws_n=ws.numel())]
    idx, boxes = i32(B, T), torch.rand(B, Q, 4, device=DEV)
    sz = i32(B, 2) + 16
    xyxy = torch.full((B, T, 4), -7.0, device=DEV)

    def call2(idx_p=idx.data_ptr(), Kx=K, Qx=Q, Tx=T, out_p=xyxy.data_ptr()):
        return lib.fx_detr_eval_boxes_f32(idx_p, boxes.data_ptr(), sz.data_ptr(), B, Qx, Kx, Tx, rank.data_ptr(), out_p,
                                          rank.data_ptr(), out_p, s)

    rcs += [call2(idx_p=None), call2(idx_p=idx.data_ptr() + 2), call2(Kx=0), call2(Qx=0), call2(Tx=-1), call2(out_p=xyxy.data_ptr() + 2), call2(out_p=None)]
    assert all(rc == -1 for rc in rcs), rcs
    torch.cuda.synchronize()
    for t in (rank, m, ig, npig, status):
        assert bool((t == -7).all())
    assert bool((xyxy == -7.0).all())


def _detection_data(fm, n=12, size=640, seed=0):
    """n images at two original sizes; ground truth = the model's own 8 best detections per image, jittered by a seeded +-3 px, one a crowd"""
    rs = np.random.RandomState(seed)
    data = []
    for i in range(n):
        img = torch.from_numpy(synth_image_structured(500 + i, size, size)).permute(2, 0, 1).contiguous()
        H, W = ((480, 640), (333, 500))[i % 2]
        e = DetectionDatasetEntry(image=img, height=H, width=W, image_id=i)
        out = fm.model.forward(img.permute(1, 2, 0)[None].contiguous().to(DEV))
        inst = fm.processor.eval_postprocess(out, [e])[0]["instances"]
        anns = []
        for j in range(min(8, len(inst))):
            b = inst.boxes.tensor[j].cpu().numpy().astype(np.float64) + rs.randint(-3, 4, size=4)
            x0, y0, x1, y1 = np.clip(b[0], 0, W), np.clip(b[1], 0, H), np.clip(b[2], 0, W), np.clip(b[3], 0, H)
            if x1 - x0 < 1 or y1 - y0 < 1:
                continue
            anns.append({"bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)], "category_id": int(inst.classes[j]), "iscrowd": 0})
        e.annotations = anns
        data.append(e)
    next(a for e in data for a in e.annotations)["iscrowd"] = 1
    return data


def test_eval_detection_end_to_end(tmp_path, flat_small_shapes):
    """Kernel routing is pinned (flat_small_shapes), as in test_gpu_e2e.py::test_full_size_batch_properties: in production a layer's conv
    kernel is chosen by M = B * H * W, so the engine's outputs for one image at batch 4 and at batch 1 agree to bf16 rounding, not bit for
    bit; with one routing an image is computed independently of its batch, and the evaluator's dicts must then be equal exactly."""
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-detr-l-coco", device=DEV, seed=1)
    names = list(fm.model_info.classes)
    data = _detection_data(fm)
    n_plans = len(fm.model.engine.plans)
    t = time.perf_counter()
    res4 = fm.eval_detection(TrainerArgs(run_name="det4", output_dir=str(tmp_path), batch_size=4), data)
    dt4 = time.perf_counter() - t
    res1 = fm.eval_detection(TrainerArgs(run_name="det1", output_dir=str(tmp_path), batch_size=1), data, save_json=False)
    assert len(fm.model.engine.plans) == n_plans
    ev = D.DetectionEvaluator(names)
    for e in data:
        out = fm.model.forward(e.image.permute(1, 2, 0)[None].contiguous().to(DEV))
        ev.process([e], fm.processor.eval_postprocess(out, [e]))
    host = ev.evaluate()
    ap = res4["bbox"]["AP"]
    n_ann = sum(len(e.annotations) for e in data)
    print(f"MEASURED eval_detection end to end: 12 images, {n_ann} gt boxes, AP {ap}, AP50 {res4['bbox']['AP50']}, "
          f"{sum(v is not None for v in res4['bbox'].values())} of {len(res4['bbox'])} values computable, batch 4 run {dt4:.2f} s")
    assert list(res4["bbox"])[:6] == D.METRICS and len(res4["bbox"]) == 6 + len(names)
    assert res4 == res1, "batch 4 and batch 1 disagree"
    assert res4 == host, "the device path and DetectionEvaluator fed from eval_postprocess disagree"
    assert ap is not None and 0.0 < ap < 100.0
    out = tmp_path / "det4_eval"
    metrics = json.loads((out / "metrics.json").read_text())[0]
    info = json.loads((out / "model_info.json").read_text())
    assert list(metrics)[:6] == ["bbox/" + m for m in D.METRICS] and metrics["bbox/AP"] == ap and info["val_metrics"] == metrics
    assert not (tmp_path / "det1_eval").exists()


def test_runtime_report():
    print(f"MEASURED test_gpu_detection_eval.py runtime so far {time.perf_counter() - T0:.1f} s")
