"""Validation during ``FocoosModel.train`` (validation.py) on a real MI355X: records in metrics.json, the best checkpoint as
model_final.pth, early stopping, and - the check that a stale engine cannot pass - the metrics of the best record reproduced EXACTLY by
the public eval entry point after training, i.e. the weights the run validated (published on the device) are the weights it saved."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE = 256


def _det_entries(n, nc, seed=0):
    from focoos_amd.ports import Boxes, DatasetEntry, Instances
    from focoos_amd.synth import synth_image_structured

    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        t = rs.randint(1, 6)
        cx, cy = rs.uniform(0.25, 0.75, t) * SIZE, rs.uniform(0.25, 0.75, t) * SIZE
        w, h = rs.uniform(0.08, 0.3, t) * SIZE, rs.uniform(0.08, 0.3, t) * SIZE
        xyxy = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
        img = torch.from_numpy(synth_image_structured(i, SIZE, SIZE)).permute(2, 0, 1).contiguous()
        out.append(DatasetEntry(image=img, height=SIZE, width=SIZE,
                                instances=Instances((SIZE, SIZE), boxes=Boxes(torch.from_numpy(xyxy)), classes=torch.from_numpy(rs.randint(0, nc, t)))))
    return out


def _sem_entries(n, nc, seed=0):
    """Mask-family training targets (``instances`` with rectangle masks) and, for validation, a ``sem_seg`` label map of 16 x 16 blocks
    that uses every class: whatever class random weights predict, some of its pixels are right, so mIoU is not zero."""
    from focoos_amd.ports import Instances, SemanticSegmentationDatasetEntry
    from focoos_amd.synth import synth_image_structured

    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        t = rs.randint(1, 5)
        m = np.zeros((t, SIZE, SIZE), bool)
        for j in range(t):
            y0, x0 = rs.randint(0, SIZE // 2), rs.randint(0, SIZE // 2)
            m[j, y0:y0 + rs.randint(16, SIZE // 2), x0:x0 + rs.randint(16, SIZE // 2)] = True
        blocks = (np.arange(256).reshape(16, 16) * 7 + 11 * i) % nc
        gt = np.kron(blocks, np.ones((SIZE // 16, SIZE // 16), np.int64)).astype(np.uint8)
        img = torch.from_numpy(synth_image_structured(50 + i, SIZE, SIZE)).permute(2, 0, 1).contiguous()
        out.append(SemanticSegmentationDatasetEntry(image=img, height=SIZE, width=SIZE, sem_seg=gt,
                                                    instances=Instances((SIZE, SIZE), classes=torch.from_numpy(rs.randint(0, nc, t)),
                                                                        masks=torch.from_numpy(m))))
    return out


def _args(tmp_path, name, **kw):
    from focoos_amd.ports import TrainerArgs

    base = dict(run_name=name, output_dir=str(tmp_path), num_gpus=1, max_iters=4, batch_size=4, learning_rate=1e-4, freeze_bn=True,
                scheduler="FIXED", log_period=1, seed=3, eval_period=2, early_stop=False)
    base.update(kw)
    return TrainerArgs(**base)


def _artifacts(tmp_path, name):
    folder = os.path.join(str(tmp_path), name)
    with open(os.path.join(folder, "metrics.json")) as f:
        records = [json.loads(line) for line in f if line.strip()]
    info = json.load(open(os.path.join(folder, "model_info.json")))
    ck = torch.load(os.path.join(folder, "model_final.pth"), map_location="cpu", weights_only=True)
    return folder, records, info, ck


def _expected_best(records, metric):
    """The record with the greatest task metric, the earlier one on a tie (None / NaN never wins)."""
    best = None
    for r in records:
        v = r.get(metric)
        if v is not None and not np.isnan(v) and (best is None or v > best[metric]):
            best = r
    return best


def _check_run(tmp_path, name, records, info, ck, folder, metric, iterations):
    assert [r["iteration"] for r in records] == iterations
    assert all(metric in r for r in records)
    best = _expected_best(records, metric)
    print(f"MEASURED {name}: " + ", ".join(f"iter {r['iteration']} {metric} {r[metric]}" for r in records) + f" -> best iter {best and best['iteration']}")
    assert best is not None
    assert info["val_metrics"] == best and info["val_history"] == records
    assert ck["iteration"] == best["iteration"]
    assert not os.path.exists(os.path.join(folder, "model_best.pth"))
    return best


@pytest.mark.parametrize("ema", [False, True], ids=["live", "ema"])
def test_detr_validation_records_best_checkpoint_and_engine(tmp_path, ema):
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-detr-l-coco", seed=1)
    data = _det_entries(8, fm.model.num_classes)
    name = f"val_detr_{int(ema)}"
    args = _args(tmp_path, name, ema_enabled=ema, ema_warmup=2)
    plans_before = set(fm.model.engine.plans)
    fm.train(args, data, data)
    folder, records, info, ck = _artifacts(tmp_path, name)
    best = _check_run(tmp_path, name, records, info, ck, folder, "bbox/AP", [2, 4])
    assert set(fm.model.engine.plans) == plans_before and not fm.model.engine.retain_plans
    # the engine holds the best weights, and they are the weights that record was measured on: the same evaluator, run through the public
    # entry point on the reloaded model_final.pth, returns the record's numbers exactly
    res = fm.eval_detection(args, data, save_json=False)["bbox"]
    assert {f"bbox/{k}": v for k, v in res.items()} == {k: v for k, v in best.items() if k != "iteration"}
    assert all(torch.equal(v, fm.model.state_dict()[k]) for k, v in ck["model"].items() if k in fm.model.state_dict())


def test_bisenetformer_validation_semantic(tmp_path):
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("bisenetformer-l-ade", seed=4, criterion_num_points=1024)
    assert fm.model_info.config.get("postprocessing_type") == "semantic"
    data = _sem_entries(8, fm.model.num_classes)
    args = _args(tmp_path, "val_bf")
    fm.train(args, data, data)
    folder, records, info, ck = _artifacts(tmp_path, "val_bf")
    best = _check_run(tmp_path, "val_bf", records, info, ck, folder, "sem_seg/mIoU", [2, 4])
    assert best["sem_seg/mIoU"] > 0.0          # not a degenerate comparison of zeros: a stale engine would score other numbers
    res = fm.eval(args, data, save_json=False)["sem_seg"]
    assert {f"sem_seg/{k}": v for k, v in res.items()} == {k: v for k, v in best.items() if k != "iteration"}


def test_early_stop_ends_the_run(tmp_path):
    """Weights that never move (learning rate 0, frozen BatchNorm, no EMA): no validation after the first can improve, patience 2 ends the
    run at iteration 3 of 8 and model_final.pth is the first validation's checkpoint."""
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-detr-l-coco", seed=1)
    data = _det_entries(8, fm.model.num_classes)
    args = _args(tmp_path, "val_stop", learning_rate=0.0, eval_period=1, patience=2, max_iters=8, early_stop=True, ema_enabled=False)
    fm.train(args, data, data)
    folder, records, info, ck = _artifacts(tmp_path, "val_stop")
    assert [r["iteration"] for r in records] == [1, 2, 3]
    assert all({k: v for k, v in r.items() if k != "iteration"} == {k: v for k, v in records[0].items() if k != "iteration"} for r in records)
    assert ck["iteration"] == 1 and info["val_metrics"] == records[0]
    assert not os.path.exists(os.path.join(folder, "model_best.pth"))


@pytest.mark.parametrize("case", ["no_data_val", "period_above_max_iters"])
def test_runs_without_validation_are_unchanged(tmp_path, case):
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-detr-l-coco", seed=1)
    data = _det_entries(8, fm.model.num_classes)
    args = _args(tmp_path, case, max_iters=2, eval_period=1 if case == "no_data_val" else 3)
    fm.train(args, data, None if case == "no_data_val" else data)
    folder = os.path.join(str(tmp_path), case)
    assert sorted(os.listdir(folder)) == ["model_final.pth", "model_info.json"]
    info = json.load(open(os.path.join(folder, "model_info.json")))
    assert "val_metrics" not in info and "val_history" not in info
    assert torch.load(os.path.join(folder, "model_final.pth"), map_location="cpu", weights_only=True)["iteration"] == 2
