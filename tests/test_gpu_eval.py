"""FocoosModel.eval on the MI355X: fx_semseg_eval_accumulate (csrc/semseg_eval.hip) against an fp64 CPU restatement of the two resizes,
the einsum and the argmax; the semantic eval end to end against the existing torch path (eval_postprocess -> argmax -> bincount); the
classifier eval against the reference formulas on the engine's own probabilities.  Gates: DESIGN.md section 10; measured values are
printed (``MEASURED``)."""
import json
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from focoos_amd import _lib
from focoos_amd.evaluation import classification_metrics, sem_seg_metrics, semseg_accumulate
from focoos_amd.ports import ClassificationDatasetDict, SemanticSegmentationDatasetEntry, TrainerArgs
from focoos_amd.synth import synth_image_structured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = time.perf_counter()


def _ref_scores(lo, probs, Hin, Win, H, W):
    """m = F.interpolate(F.interpolate(lo -> (Hin, Win)) -> (H, W)) on the CPU in fp32 (stage 1 is fx_mf_upsample_probs_f32's arithmetic,
    stage 2 the processor's), s = einsum in fp64: [K, H, W] float64."""
    m = F.interpolate(F.interpolate(lo[None], size=(Hin, Win), mode="bilinear", align_corners=False), size=(H, W), mode="bilinear",
                      align_corners=False)[0]
    return torch.einsum("qk,qhw->khw", probs.double(), m.double())


def _gate(s64, pred, Q):
    """Every pixel whose fp64 top-2 margin exceeds delta = 2 Q 2^-24 max_k s_k must carry the fp64 argmax.  Returns the near-tie count."""
    top2 = s64.topk(2, dim=0).values if s64.shape[0] > 1 else torch.cat([s64, s64 - 1e30])
    delta = 2 * Q * 2.0 ** -24 * top2[0].abs()
    clear = (top2[0] - top2[1]) > delta
    want = s64.argmax(0)
    bad = (pred.long() != want) & clear
    assert int(bad.sum()) == 0, f"{int(bad.sum())} clear pixels disagree with the fp64 argmax"
    return int((~clear).sum())


def _run(lo, probs, Hin, Win, sizes, gts, ignore, conf=None, want=True):
    K = probs.shape[-1]
    conf = torch.zeros((K + 1) ** 2, dtype=torch.int64, device=DEV) if conf is None else conf
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    pred, score, offs = semseg_accumulate(lo.to(DEV).contiguous(), probs.to(DEV).contiguous(), Hin, Win, sizes, gts, ignore, conf, status,
                                          want_pred=want, want_score=want)
    torch.cuda.synchronize()
    return conf, status, pred, score, offs


@pytest.mark.parametrize("K,case", [(150, "up"), (150, "down"), (19, "up"), (19, "mixed_i32")])
def test_kernel_vs_fp64(K, case):
    g = torch.Generator().manual_seed(K * 7 + len(case))
    Q = 100
    h, w, Hin, Win = {"up": (16, 20, 64, 80), "down": (24, 32, 96, 128), "mixed_i32": (12, 16, 48, 64)}[case]
    sizes = {"up": [(131, 173)], "down": [(41, 57)], "mixed_i32": [(77, 101), (30, 45), (64, 64)]}[case]
    B = len(sizes)
    lo = torch.rand(B, Q, h, w, generator=g)
    probs = torch.softmax(torch.randn(B, Q, K, generator=g) * 3, -1)
    ignore = 255
    gts = []
    for H, W in sizes:
        gt = torch.randint(0, K, (H, W), generator=g)
        gt[torch.rand(H, W, generator=g) < 0.1] = ignore
        gts.append(gt.numpy().astype(np.int32 if case == "mixed_i32" else np.uint8))
    conf, status, pred, score, offs = _run(lo, probs, Hin, Win, sizes, gts, ignore)
    assert int(status.item()) == 0
    near, want_conf = 0, torch.zeros((K + 1) ** 2, dtype=torch.int64)
    for i, (H, W) in enumerate(sizes):
        p = pred[offs[i]: offs[i] + H * W].view(H, W).cpu()
        s64 = _ref_scores(lo[i], probs[i], Hin, Win, H, W)
        near += _gate(s64, p, Q)
        gt = torch.from_numpy(gts[i].astype(np.int64))
        gt[gt == ignore] = K
        want_conf += torch.bincount(((K + 1) * p.long() + gt).view(-1), minlength=(K + 1) ** 2)
    print(f"MEASURED kernel_vs_fp64 K={K} {case}: near-tie pixels {near} of {sum(H * W for H, W in sizes)}")
    assert torch.equal(conf.cpu(), want_conf)
    conf2 = _run(lo, probs, Hin, Win, sizes, gts, ignore, conf=conf, want=False)[0]
    assert torch.equal(conf2.cpu(), 2 * want_conf)


@pytest.mark.parametrize("h,w,Hin,Win,H,W", [(16, 20, 64, 80, 131, 173), (24, 32, 96, 128, 41, 57), (13, 17, 100, 60, 77, 300)])
def test_two_stage_sampling_bit_exact(h, w, Hin, Win, H, W):
    """Q = K = 1, prob 1: the winning score is m itself; it must equal the device F.interpolate of fx_mf_upsample_probs_f32's output bit
    for bit."""
    lo = torch.rand(1, 1, h, w, generator=torch.Generator().manual_seed(h))
    up = torch.empty(1, 1, Hin, Win, device=DEV)
    lib = _lib.load("bf16")
    _lib.check(lib.fx_mf_upsample_probs_f32(lo.to(DEV).data_ptr(), h, w, up.data_ptr(), Hin, Win, 1, torch.cuda.current_stream().cuda_stream))
    # the processor's F.interpolate runs on the device (ATen's GPU upsample_bilinear2d: source index + lambda taps); ATen's CPU kernel takes a
    # separable path with normalised filter weights for outputs this size and is printed for information only
    want = F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0, 0].cpu()
    want_cpu = F.interpolate(up.cpu(), size=(H, W), mode="bilinear", align_corners=False)[0, 0]
    gt = np.zeros((H, W), np.uint8)
    _, _, _, score, _ = _run(lo, torch.ones(1, 1, 1), Hin, Win, [(H, W)], [gt], 255)
    got = score.view(H, W).cpu()
    ndiff = int((got != want).sum())
    print(f"MEASURED two-stage sampling {h}x{w}->{Hin}x{Win}->{H}x{W}: {ndiff} pixels differ from the device F.interpolate, "
          f"{int((got != want_cpu).sum())} from the CPU one")
    assert ndiff == 0


def test_refusals_leave_conf_untouched():
    lib = _lib.load("bf16")
    K, Q, h, w = 150, 100, 8, 8
    lo = torch.rand(1, 129, h, w, device=DEV)
    probs = torch.rand(1, 129, 256, device=DEV)
    conf = torch.full(((K + 1) ** 2 + 1,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    sz = torch.tensor([[8, 8]], dtype=torch.int32, device=DEV)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    gt = torch.zeros(64, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def call(Qx=Q, Kx=K, lo_p=lo.data_ptr(), conf_p=conf.data_ptr(), gt_p=gt.data_ptr(), i32=1, st=status.data_ptr()):
        return lib.fx_semseg_eval_accumulate(lo_p, probs.data_ptr(), 1, Qx, Kx, h, w, 32, 32, sz.data_ptr(), 64, gt_p, off.data_ptr(), i32, 255,
                                             conf_p, st, None, None, s)

    for rc in (call(Qx=129), call(Kx=256), call(Qx=0), call(lo_p=None), call(conf_p=conf.data_ptr() + 4), call(gt_p=gt.data_ptr() + 2),
               call(i32=2), call(st=None)):
        assert rc == -1, rc
    torch.cuda.synchronize()
    assert bool((conf == -7).all())


def _semseg_data(K, n=8, seed=0):
    sizes_in = [(96, 128), (128, 96), (64, 64)]
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        Hin, Win = sizes_in[(i // 3) % 3]
        img = synth_image_structured(300 + i, Hin, Win)
        H, W = int(Hin * (1.37 if i % 2 else 0.71)), int(Win * (1.21 if i % 2 else 0.83))
        gt = rs.randint(0, K, size=(H, W)).astype(np.uint8)
        gt[rs.rand(H, W) < 0.08] = 255
        out.append(SemanticSegmentationDatasetEntry(image=torch.from_numpy(img).permute(2, 0, 1).contiguous(), height=H, width=W, sem_seg=gt))
    return out


def _torch_path(fm, data, ignore=255):
    """The existing path: forward (masks at input size) -> eval_postprocess -> argmax -> bincount; also the near-tie count by the delta rule."""
    K = fm.model.num_classes
    conf = np.zeros((K + 1) ** 2, np.int64)
    near = 0
    for e in data:
        x = e.image.permute(1, 2, 0)[None].contiguous().to(DEV)
        out = fm.model.forward(x)
        res = fm.processor.eval_postprocess(out, [e])[0]["sem_seg"]
        pred = res.argmax(0).cpu().numpy()
        m = F.interpolate(out.masks[0:1], size=(e.height, e.width), mode="bilinear", align_corners=False)[0]
        s64 = torch.einsum("qk,qhw->khw", out.logits[0].double(), m.double())
        t2 = s64.topk(2, dim=0).values
        near += int(((t2[0] - t2[1]) <= 2 * out.logits.shape[1] * 2.0 ** -24 * t2[0].abs()).sum())
        gt = e.sem_seg.astype(np.int64)
        gt[gt == ignore] = K
        conf += np.bincount(((K + 1) * pred + gt).reshape(-1), minlength=conf.size)
    return conf, near


@pytest.mark.parametrize("name", ["bisenetformer-s-ade", "fai-mf-m-ade"])
def test_semseg_eval_end_to_end(name, tmp_path):
    from focoos_amd.evaluation import accumulate
    from focoos_amd.model import ModelManager

    fm = ModelManager.get(name, device=DEV, seed=3)
    K = fm.model.num_classes
    data = _semseg_data(K)
    n_plans = len(fm.model.engine.plans)
    args = TrainerArgs(run_name="ev", output_dir=str(tmp_path), batch_size=4)
    res = fm.eval(args, data)
    assert len(fm.model.engine.plans) == n_plans
    conf4 = accumulate(fm, data, range(len(data)), "semseg", 255, 4).cpu().numpy()
    conf1 = accumulate(fm, data, range(len(data)), "semseg", 255, 1).cpu().numpy()
    assert len(fm.model.engine.plans) == n_plans
    ref, near = _torch_path(fm, data)
    d = int(np.abs(conf4 - ref).sum())
    d1 = int(np.abs(conf4 - conf1).sum())
    print(f"MEASURED {name}: sum|dconf| fused vs torch {d}, batch 4 vs 1 {d1}, near-tie pixels {near}, mIoU {res['sem_seg']['mIoU']}")
    assert d <= 2 * near and d1 <= 2 * near
    names = list(fm.model_info.classes)
    assert res["sem_seg"] == sem_seg_metrics(conf4.reshape(K + 1, K + 1), names)
    m_ref = sem_seg_metrics(ref.reshape(K + 1, K + 1), names)["mIoU"]
    npix = int(ref.sum())
    # each moved pixel changes at most two classes' TP / union by 1: |dmIoU| <= 100 * 2 d / min union; loose but non-vacuous bound
    assert abs((res["sem_seg"]["mIoU"] or 0) - (m_ref or 0)) <= 100.0 * 2 * d / max(1, npix / K) + 1e-9
    out = tmp_path / "ev_eval"
    metrics = json.loads((out / "metrics.json").read_text())[0]
    info = json.loads((out / "model_info.json").read_text())
    assert list(metrics)[0] == "sem_seg/mIoU" and info["val_metrics"] == metrics


def test_classification_eval(tmp_path):
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-cls-n-coco", device=DEV, seed=1)
    K = fm.model.num_classes
    rs = np.random.RandomState(5)
    data = []
    for i in range(12):
        img = synth_image_structured(400 + i, 224, 224)
        data.append(ClassificationDatasetDict(image=torch.from_numpy(img).permute(2, 0, 1).contiguous(), height=224, width=224,
                                              label=sorted(set(rs.randint(0, K, size=3).tolist()))))
    res = fm.eval(TrainerArgs(run_name="cls", output_dir=str(tmp_path), batch_size=4), data)["classification"]
    logits = torch.cat([fm.model.forward(torch.stack([e.image.permute(1, 2, 0) for e in data[i: i + 4]]).contiguous().to(DEV)).logits.cpu()
                        for i in range(0, len(data), 4)])   # the batches eval runs
    pred = (torch.sigmoid(logits.float()) > 0.5).int()
    true = torch.zeros(len(data), K, dtype=torch.int)
    for i, e in enumerate(data):
        true[i, e.label] = 1
    tp, fp, fn = (true * pred).sum(0), ((1 - true) * pred).sum(0), (true * (1 - pred)).sum(0)
    assert res == classification_metrics(tp, fp, fn, fm.model_info.classes)
    assert json.loads((tmp_path / "cls_eval" / "metrics.json").read_text())[0]["classification/F1"] == res["F1"]


def test_scoped_plans_releases_what_the_block_created():
    from focoos_amd.model import ModelManager

    eng = ModelManager.get("fai-cls-n-coco", device=DEV, seed=1).model.engine
    x = torch.stack([torch.from_numpy(synth_image_structured(i, 64, 96)) for i in range(2)]).contiguous().to(DEV)
    kept = eng.forward(x)
    before = dict(eng.plans)
    assert any(p is kept for p in before.values())
    for retain in (False, True):
        eng.retain_plans = retain
        with eng.scoped_plans():
            assert eng.forward(x) is kept                      # an existing plan is reused ...
            eng.forward(x.float())                             # ... a new input dtype and the pipeline get entries of their own
            eng.pipeline(2, 64, 96, 2)
            assert len(eng.plans) == len(before) + 2
        created = set(eng.plans) - set(before)
        assert len(created) == (2 if retain else 0)
        assert all(eng.plans[k] is p for k, p in before.items())   # what existed before is the same object afterwards
    eng.retain_plans = False
    eng.drop_plans_except(set(before))
    assert set(eng.plans) == set(before) and eng.forward(x) is kept


def test_runtime_report():
    print(f"MEASURED test_gpu_eval.py runtime so far {time.perf_counter() - T0:.1f} s")
