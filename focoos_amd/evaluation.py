"""FocoosModel.eval (focoos/models/focoos_model.py:276-320, trainer/trainer.py:226-286) on the engine.

Semantic segmentation (bisenetformer-*-ade, fai-mf-*-ade): the engine's low-resolution mask probabilities and class probabilities go
straight into fx_semseg_eval_accumulate (csrc/semseg_eval.hip), which resizes, scores, takes the argmax and counts the confusion matrix
of SemSegEvaluator.process (trainer/evaluation/sem_seg_evaluation.py:87-103) without a full-resolution tensor.  Classification
(fai-cls-*): sigmoid of the engine logits, ``> 0.5``, per-class TP / FP / FN counted on the device with torch (an [N, 80] tensor: no
kernel warranted).  Both metric sets are functions of integer sums, so a multi-GPU run all-reduces the counters once (int64 SUM) and
gets the single-GPU result exactly; the metrics are the reference's own formulas (numpy float64 / torch fp32) on those sums.

Detection and instance segmentation AP need pycocotools' COCOeval and are refused (NotImplementedError) before anything is created."""
from __future__ import annotations

import ctypes
import json
import os
from collections import OrderedDict
from dataclasses import fields
from typing import List, Optional, Sequence

import numpy as np
import torch

TASK_METRICS = {"detection": "bbox/AP", "semseg": "sem_seg/mIoU", "instseg": "segm/AP", "classification": "classification/F1",
                "keypoint": "keypoints/AP"}


def _add_prefix(metric: dict, key: str) -> dict:
    """trainer.py:908-919"""
    return {f"{key}/{k}": v for k, v in metric.items()}


# ---------------------------------------------------------------------------------------------------------------- metric formulas
def sem_seg_metrics(conf: np.ndarray, class_names: Sequence[str]) -> "OrderedDict[str, Optional[float]]":
    """SemSegEvaluator.evaluate (sem_seg_evaluation.py:105-160) on the int64 [(K+1), (K+1)] matrix, same numpy float64 operations."""
    conf = np.asarray(conf, dtype=np.int64)
    K = conf.shape[0] - 1
    acc = np.full(K, np.nan, dtype=float)
    iou = np.full(K, np.nan, dtype=float)
    tp = conf.diagonal()[:-1].astype(float)
    pos_gt = np.sum(conf[:-1, :-1], axis=0).astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        class_weights = pos_gt / np.sum(pos_gt)
        pos_pred = np.sum(conf[:-1, :-1], axis=1).astype(float)
        acc_valid = pos_gt > 0
        acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
        union = pos_gt + pos_pred - tp
        iou_valid = np.logical_and(acc_valid, union > 0)
        iou[iou_valid] = tp[iou_valid] / union[iou_valid]
        macc = np.sum(acc[acc_valid]) / np.sum(acc_valid)
        miou = np.sum(iou[iou_valid]) / np.sum(iou_valid)
        fiou = np.sum(iou[iou_valid] * class_weights[iou_valid])
        pacc = np.sum(tp) / np.sum(pos_gt)
    res = OrderedDict()
    res["mIoU"] = 100 * miou
    res["fwIoU"] = 100 * fiou
    for i, name in enumerate(class_names):
        res[f"IoU-{name}"] = 100 * iou[i]
    res["mACC"] = 100 * macc
    res["pACC"] = 100 * pacc
    for i, name in enumerate(class_names):
        res[f"ACC-{name}"] = 100 * acc[i]
    return OrderedDict((k, (float(v) if np.isfinite(v) else None)) for k, v in res.items())


def classification_metrics(tp, fp, fn, class_names: Optional[Sequence[str]]) -> "OrderedDict[str, float]":
    """ClassificationEvaluator.evaluate (classification_evaluation.py:211-262) from per-class integer counts, same torch fp32 operations
    in the same order (the reference's ``(y_true * y_pred).sum(0)`` etc. are these counts)."""
    tp, fp, fn = (torch.as_tensor(t).cpu().to(torch.int64) for t in (tp, fp, fn))
    n = tp.numel()
    precision = torch.zeros(n, dtype=torch.float)
    for i in range(n):
        if tp[i] + fp[i] > 0:
            precision[i] = 100.0 * tp[i].float() / (tp[i] + fp[i]).float()
    recall = torch.zeros(n, dtype=torch.float)
    for i in range(n):
        if tp[i] + fn[i] > 0:
            recall[i] = 100.0 * tp[i].float() / (tp[i] + fn[i]).float()
    f1 = torch.zeros(n, dtype=torch.float)
    for i in range(n):
        if precision[i] + recall[i] > 0:
            f1[i] = 2 * (precision[i] * recall[i]) / (precision[i] + recall[i])
    valid = (tp + fn > 0).sum().item()
    macro_p = precision.sum() / max(valid, 1)
    macro_r = recall.sum() / max(valid, 1)
    macro_f1 = 2 * (macro_p * macro_r) / (macro_p + macro_r) if macro_p + macro_r > 0 else torch.tensor(0.0)
    res = OrderedDict()
    res["F1"] = macro_f1.item()
    res["Precision"] = macro_p.item()
    res["Recall"] = macro_r.item()
    if class_names is not None:
        for i, name in enumerate(class_names):
            if i < n:
                res[f"F1-{name}"] = f1[i].item()
                res[f"Precision-{name}"] = precision[i].item()
                res[f"Recall-{name}"] = recall[i].item()
    return res


# ---------------------------------------------------------------------------------------------------------------- ground truth
def load_sem_seg(entry, ignore_label: int) -> np.ndarray:
    """[H, W] labels of a SemanticSegmentationDatasetEntry: ``sem_seg`` (in memory) or ``sem_seg_file_name`` read with PIL as
    load_image_into_numpy_array does.  uint8 when every label fits (ignore included), else int32."""
    sem = getattr(entry, "sem_seg", None)
    if sem is None:
        fname = getattr(entry, "sem_seg_file_name", None)
        if fname is None:
            raise ValueError("semantic evaluation needs sem_seg_file_name (or sem_seg) on every dataset entry")
        from PIL import Image

        with Image.open(fname) as im:
            sem = np.array(im)
    sem = np.asarray(sem.cpu() if isinstance(sem, torch.Tensor) else sem)
    if sem.ndim != 2:
        raise ValueError(f"ground-truth label map must be [H, W], got {sem.shape}")
    if sem.dtype == np.uint8:
        return np.ascontiguousarray(sem)
    return np.ascontiguousarray(sem.astype(np.int32))


def classification_target(entry, num_classes: int) -> torch.Tensor:
    """ClassificationEvaluator.process's label vector (int [num_classes])."""
    label_list = None
    if isinstance(entry, dict) and entry.get("label") is not None:
        label_list = entry["label"]
    elif getattr(entry, "label", None) is not None:
        label_list = entry.label
    else:
        anns = entry.get("annotations") if isinstance(entry, dict) else getattr(entry, "annotations", None)
        if anns:
            label_list = [a.get("category_id", None) for a in anns]
    if label_list is None:
        raise ValueError(f"Could not find label in input item: {entry}")
    t = torch.zeros(num_classes, dtype=torch.int)
    for i in label_list:
        if i is not None:
            t[i] = 1
    return t


# ---------------------------------------------------------------------------------------------------------------- device side
def semseg_accumulate(mask_probs: torch.Tensor, probs: torch.Tensor, Hin: int, Win: int, sizes: Sequence[Sequence[int]], gts: List[np.ndarray],
                      ignore_label: int, conf: torch.Tensor, status: torch.Tensor, want_pred: bool = False, want_score: bool = False):
    """One fx_semseg_eval_accumulate call on the engine's buffers (mask_probs [B,Q,h,w] f32, probs [B,Q,K] f32) for a batch whose
    images share (Hin, Win); ``gts`` the per-image [H_i, W_i] label maps (all uint8 or all int32), ``conf`` int64 [(K+1)^2] and ``status``
    int32 [1] on the device, accumulated.  Returns (pred, score) flat device buffers (or None) at the gt offsets."""
    from . import _lib

    dev = mask_probs.device
    B, Q, h, w = mask_probs.shape
    K = probs.shape[-1]
    assert probs.shape[:2] == (B, Q) and len(sizes) == B == len(gts)
    i32 = any(g.dtype != np.uint8 for g in gts)
    flat = np.concatenate([g.astype(np.int32 if i32 else np.uint8, copy=False).reshape(-1) for g in gts])
    offs = np.cumsum([0] + [g.size for g in gts])[:-1].astype(np.int64)
    for g, (H, W) in zip(gts, sizes):
        if g.shape != (int(H), int(W)):
            raise ValueError(f"ground truth {g.shape} does not match the original size {(H, W)}")
    gt_d = torch.from_numpy(flat).to(dev, non_blocking=False)
    off_d = torch.from_numpy(offs).to(dev)
    sz_d = torch.tensor([[int(H), int(W)] for H, W in sizes], dtype=torch.int32, device=dev)
    pred = torch.full((flat.size,), -1, dtype=torch.int32, device=dev) if want_pred else None
    score = torch.full((flat.size,), float("nan"), dtype=torch.float32, device=dev) if want_score else None
    lib = _lib.load("bf16")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.fx_semseg_eval_accumulate(mask_probs.data_ptr(), probs.data_ptr(), B, Q, K, h, w, int(Hin), int(Win), sz_d.data_ptr(),
                                       int(max(int(H) * int(W) for H, W in sizes)), gt_d.data_ptr(), off_d.data_ptr(), int(i32), int(ignore_label),
                                       conf.data_ptr(), status.data_ptr(), pred.data_ptr() if want_pred else None,
                                       score.data_ptr() if want_score else None, ctypes.c_void_p(stream))
    _lib.check(rc, "fx_semseg_eval_accumulate")
    return pred, score, offs


# ---------------------------------------------------------------------------------------------------------------- driver
def _metadata(data_test):
    ds = getattr(data_test, "dataset", None)
    meta = getattr(ds, "metadata", None) if ds is not None else None
    return meta if meta is not None else getattr(data_test, "metadata", None)


def _task_of(model_info) -> str:
    cfg = model_info.config
    fam = getattr(model_info.model_family, "value", model_info.model_family)
    if fam in ("fai_mf", "bisenetformer") and cfg.get("postprocessing_type", "instance") == "semantic":
        return "semseg"
    return getattr(model_info.task, "value", model_info.task)


def check_supported(focoos_model) -> str:
    """The task eval runs for this model; NotImplementedError for detection / instance segmentation (nothing created before)."""
    fam = focoos_model.model.family
    task = _task_of(focoos_model.model_info)
    if fam == "fai_detr" or task in ("detection", "instseg") or (fam in ("fai_mf", "bisenetformer")
                                                                  and focoos_model.model_info.config.get("postprocessing_type", "instance") == "instance"):
        raise NotImplementedError(f"FocoosModel.eval: {task} evaluation (COCO bbox / segm AP) needs pycocotools' COCOeval, which this engine "
                                  "does not port; semantic segmentation and classification are evaluated")
    if task not in ("semseg", "classification"):
        raise NotImplementedError(f"FocoosModel.eval: task {task!r} is not evaluated by this engine")
    return task


def resolve(focoos_model, data_test):
    """(task, class names, ignore label, dataset name) from the dataset metadata, checked against the model (trainer.py's checks)."""
    task = check_supported(focoos_model)
    info = focoos_model.model_info
    meta = _metadata(data_test)
    names, ignore, dname = list(info.classes), 255, None
    if meta is not None:
        mt = getattr(meta, "task", None)
        mt = getattr(mt, "value", mt)
        if mt is not None and mt != task and not (task == "semseg" and mt == "semseg"):
            raise ValueError(f"Task mismatch: model task {task} != dataset task {mt}")
        cls = getattr(meta, "stuff_classes", None) if task == "semseg" else None
        cls = cls if cls is not None else getattr(meta, "thing_classes", None)
        if cls is None:
            cls = getattr(meta, "classes", None)
        if cls is not None:
            if len(cls) != focoos_model.model.num_classes:
                raise ValueError(f"dataset has {len(cls)} classes, the model {focoos_model.model.num_classes}: num_classes must match")
            names = list(cls)
        il = getattr(meta, "ignore_label", None)
        ignore = 255 if il is None else int(il)
        dname = getattr(meta, "name", None)
    return task, names, ignore, dname


def _entry_image(entry) -> torch.Tensor:
    img = entry.image if not isinstance(entry, dict) or hasattr(entry, "image") else entry["image"]
    t = torch.as_tensor(np.asarray(img) if not isinstance(img, torch.Tensor) else img)
    if t.dim() != 3:
        raise ValueError("dataset entry image must be CHW (or HWC) with 3 channels")
    if t.shape[0] == 3 and t.shape[-1] != 3:
        t = t.permute(1, 2, 0)
    return t if t.dtype == torch.uint8 else t.to(torch.float32)


def _batches(data_test, indices: Sequence[int], bs: int):
    """Consecutive entries of one input size, at most ``bs`` per batch (each image keeps the batch-1 semantics: no padding)."""
    cur, key = [], None
    for i in indices:
        e = data_test[i]
        img = _entry_image(e)
        k = (tuple(img.shape), img.dtype)
        if cur and (k != key or len(cur) >= bs):
            yield cur
            cur = []
        cur.append((e, img))
        key = k
    if cur:
        yield cur


def accumulate(focoos_model, data_test, indices: Sequence[int], task: str, ignore: int, batch_size: int):
    """Run the engine over ``indices`` and return the integer counters: int64 conf [(K+1)^2] (semseg) or int64 [3, K] TP/FP/FN
    (classification), on the model's device.  Plans eval creates are released afterwards."""
    model = focoos_model.model
    eng = model.engine
    dev = model.device
    K = model.num_classes
    with eng.scoped_plans():
        if task == "semseg":
            conf = torch.zeros((K + 1) * (K + 1), dtype=torch.int64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            for batch in _batches(data_test, indices, batch_size):
                x = torch.stack([img for _, img in batch]).to(dev).contiguous()
                pl = eng.forward(x, full_masks=False)
                sizes = [(int(e.height), int(e.width)) for e, _ in batch]
                gts = [load_sem_seg(e, ignore) for e, _ in batch]
                semseg_accumulate(pl.mask_probs, pl.probs, x.shape[1], x.shape[2], sizes, gts, ignore, conf, status)
            bad = int(status.item())
            if bad:
                raise ValueError(f"{bad} ground-truth pixels carry a label outside [0, {K}) that is not the ignore label {ignore}")
            return conf
        counts = torch.zeros(3, K, dtype=torch.int64, device=dev)
        for batch in _batches(data_test, indices, batch_size):
            x = torch.stack([img for _, img in batch]).to(dev).contiguous()
            pl = eng.forward(x)
            pred = (torch.sigmoid(pl.logits.float()) > 0.5).to(torch.int64)      # ClassificationProcessor.eval_postprocess + process
            true = torch.stack([classification_target(e, K) for e, _ in batch]).to(dev, torch.int64)
            counts[0] += (true * pred).sum(0)
            counts[1] += ((1 - true) * pred).sum(0)
            counts[2] += (true * (1 - pred)).sum(0)
        return counts


def metrics_from(task: str, counts: torch.Tensor, names: Sequence[str]) -> "OrderedDict":
    if task == "semseg":
        K = len(names)
        return OrderedDict({"sem_seg": sem_seg_metrics(counts.cpu().numpy().reshape(K + 1, K + 1), names)})
    c = counts.cpu()
    return OrderedDict({"classification": classification_metrics(c[0], c[1], c[2], names)})


def write_artifacts(focoos_model, args, task: str, results: dict, dataset_name: Optional[str], save_json: bool) -> None:
    """trainer.eval (trainer.py:244-286): <output_dir>/<run_name>_eval/model_info.json (with val_metrics) and metrics.json."""
    key = TASK_METRICS[task].split("/")[0]
    raw = _add_prefix(results[key], key)
    info = focoos_model.model_info
    info.val_metrics = raw
    if dataset_name is not None:
        info.val_dataset = dataset_name
    if not save_json:
        return
    out = os.path.join(args.output_dir, f"{args.run_name.strip()}_eval")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "model_info.json"), "w") as f:
        json.dump({fl.name: getattr(info, fl.name) for fl in fields(info)}, f, indent=1, default=str)
    with open(os.path.join(out, "metrics.json"), "w") as f:
        f.write(json.dumps([raw]))


def _per_rank_batch(args) -> int:
    world = max(1, int(getattr(args, "num_gpus", 1)))
    return max(1, int(getattr(args, "batch_size", 1)) // world)


def _dist_worker(model_name_or_info, cfg, state, device_seed, args, data_test, task, ignore, out_path):
    """One rank of a multi-GPU eval: rebuild the model on this rank's GPU, run its InferenceSampler shard, all-reduce the counters."""
    import torch.distributed as dist

    from .model import ModelManager
    from .train_data import InferenceSampler

    rank = dist.get_rank()
    dev = f"cuda:{torch.cuda.current_device()}"
    fm = ModelManager.get(model_name_or_info.name, model_info=model_name_or_info, device=dev, seed=device_seed)
    fm.model.load_state_dict(state, strict=False)
    counts = accumulate(fm, data_test, list(InferenceSampler(len(data_test))), task, ignore, _per_rank_batch(args))
    dist.all_reduce(counts, op=dist.ReduceOp.SUM)
    if rank == 0:
        torch.save(counts.cpu(), out_path)


def run_eval(focoos_model, args, data_test, save_json: bool = True) -> dict:
    """FocoosModel.eval: returns the results dict ({"sem_seg": {...}} or {"classification": {...}}) and writes the artifacts."""
    task, names, ignore, dname = resolve(focoos_model, data_test)
    if len(data_test) == 0:
        raise ValueError("FocoosModel.eval: empty dataset")
    world = max(1, int(getattr(args, "num_gpus", 1)))
    if world > 1:
        import copy
        import tempfile

        from .launch import launch

        info = copy.deepcopy(focoos_model.model_info)
        info.weights_uri = None
        with tempfile.TemporaryDirectory() as tmp:
            out_path = os.path.join(tmp, "counts.pt")
            launch(_dist_worker, world, args=(info, info.config, focoos_model.model.state_dict(), 0, args, data_test, task, ignore, out_path))
            counts = torch.load(out_path)
    else:
        counts = accumulate(focoos_model, data_test, range(len(data_test)), task, ignore, _per_rank_batch(args))
    results = metrics_from(task, counts, names)
    write_artifacts(focoos_model, args, task, results, dname, save_json)
    return results
