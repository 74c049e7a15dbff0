"""Validation inside ``trainer.run_train``: the reference's periodic evaluation, ``BestCheckpointer`` and
``EarlyStoppingHook`` (focoos/trainer/trainer.py:375-416, :463-469, hooks/early_stop.py).

Every ``eval_period`` iterations (and once more after the last one) rank 0 hands the weights being trained - the EMA copy when EMA is on -
to the inference engine with ``publish_state_dict``: device to device, in place, the engine's plans stay alive (csrc/publish.hip).  It then
runs the evaluator of the model's task - the existing entry points of evaluation.py / detection_eval.py / segm_eval.py - and keeps the
books: one JSON line per validation in ``<run>/metrics.json``, ``model_best.pth`` on a strictly greater task metric, the early-stop
count.  At the end of the run the best weights become ``model_final.pth``.

The schedule, the tracker and the task dispatch are plain Python (tests/test_validation_cpu.py); only ``Validator`` touches the GPU."""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Tuple

METRICS_NAME = "metrics.json"       # focoos.ports.ArtifactName.METRICS
BEST_NAME = "model_best.pth"


def validation_iterations(max_iters: int, eval_period: int) -> List[int]:
    """Iteration counts (1-based: ``it + 1``) after which a run validates: every multiple of ``eval_period``, and ``max_iters`` itself
    if it is not one.  Empty - the run validates nowhere - unless ``0 < eval_period <= max_iters``."""
    if not 0 < eval_period <= max_iters:
        return []
    its = list(range(eval_period, max_iters + 1, eval_period))
    if its[-1] != max_iters:
        its.append(max_iters)
    return its


def task_of(family: str, config: dict, task) -> str:
    """The evaluation task of a model: the mask families score semantic segmentation when they post-process semantically
    (evaluation._task_of), else the model's own task."""
    if family in ("fai_mf", "bisenetformer") and config.get("postprocessing_type", "instance") == "semantic":
        return "semseg"
    return getattr(task, "value", task)


def evaluator_for(family: str, task: str) -> Tuple[str, str]:
    """(evaluator, task-metric key) for a model family and task: which of the three existing evaluators scores it and the metric that
    decides "best" (evaluation.TASK_METRICS).  A pair nobody evaluates raises NotImplementedError."""
    from .evaluation import TASK_METRICS

    if family == "fai_detr" and task == "detection":
        kind = "detection"
    elif family == "fai_mf" and task == "instseg":
        kind = "instseg"
    elif family in ("fai_mf", "bisenetformer") and task == "semseg":
        kind = "semseg"
    else:
        raise NotImplementedError(f"validation during training: no evaluator for family {family!r} with task {task!r}")
    return kind, TASK_METRICS[task]


def _value(record: dict, metric: str) -> float:
    v = record.get(metric)
    return float("nan") if v is None else float(v)


class BestTracker:
    """BestCheckpointer + EarlyStoppingHook on the records of a run: ``update(record)`` returns (improved, stop).  A record improves when
    its task metric is strictly greater than the best so far (the first finite one always does; NaN / None never wins); ``stop`` is set
    when early stopping is on and ``patience`` consecutive records did not improve."""

    def __init__(self, metric: str, early_stop: bool = True, patience: int = 10):
        self.metric, self.early_stop, self.patience = metric, bool(early_stop), int(patience)
        self.best: Optional[dict] = None
        self.bad = 0
        self.history: List[dict] = []

    def update(self, record: dict) -> Tuple[bool, bool]:
        self.history.append(record)
        v = _value(record, self.metric)
        improved = not math.isnan(v) and (self.best is None or v > _value(self.best, self.metric))
        if improved:
            self.best, self.bad = record, 0
        else:
            self.bad += 1
        return improved, self.early_stop and self.bad >= self.patience


def evaluate(eval_model, processor, model_info, data_val, kind: str, batch_size: int) -> Dict[str, Optional[float]]:
    """One pass of the task's evaluator over ``data_val`` on the engine behind ``eval_model``; the metrics with their ``<prefix>/`` keys
    (what FocoosModel.eval* write to metrics.json)."""
    from . import detection_eval, evaluation, segm_eval

    fm = SimpleNamespace(model=eval_model, processor=processor, model_info=model_info)
    idx = range(len(data_val))
    if kind == "semseg":
        task, names, ignore, _ = evaluation.resolve(fm, data_val)
        res = evaluation.metrics_from(task, evaluation.accumulate(fm, data_val, idx, task, ignore, batch_size), names)
    elif kind == "detection":
        names, _ = detection_eval.resolve(fm, data_val)
        res = detection_eval.results_from(detection_eval.collect(fm, data_val, idx, batch_size), names)
    else:
        names, _ = segm_eval.resolve(fm, data_val)
        res = detection_eval.results_from(segm_eval.collect(fm, data_val, idx, batch_size), names, "segm")
    (key, metrics), = res.items()
    return evaluation._add_prefix(metrics, key)


class Validator:
    """Rank 0's validation state of one training run.  ``weights()`` returns the state dict to validate, tensors on the device (views of
    the optimizer's flat buffer or of the EMA copy: nothing is cloned); ``checkpoint(iteration)`` returns what ``model_best.pth`` holds."""

    def __init__(self, eval_model, processor, model_info, data_val, folder: str, batch_size: int, early_stop: bool, patience: int,
                 weights: Callable[[], dict], checkpoint: Callable[[int], dict]):
        self.model, self.processor, self.info, self.data = eval_model, processor, model_info, data_val
        self.folder, self.bs = folder, max(1, int(batch_size))
        self.weights, self.checkpoint = weights, checkpoint
        task = task_of(eval_model.family, model_info.config, model_info.task)
        self.kind, metric = evaluator_for(eval_model.family, task)
        self.tracker = BestTracker(metric, early_stop, patience)
        eng = eval_model.engine
        self._plans_before = set(eng.plans)
        eng.retain_plans = True      # the evaluators release the plans they create; a run keeps them from one validation to the next
        os.makedirs(folder, exist_ok=True)
        open(os.path.join(folder, METRICS_NAME), "w").close()

    def run(self, iteration: int) -> bool:
        """Validate the weights as they are after ``iteration`` steps; True: stop the run (early stopping)."""
        import torch

        from . import _lib

        with _lib.using_compute_dtype("bf16"):     # an fp16 run steps in fp16; the inference engine computes in bf16 (restored on exit)
            self.model.publish_state_dict(self.weights())
            record = {"iteration": int(iteration)}
            record.update(evaluate(self.model, self.processor, self.info, self.data, self.kind, self.bs))
        with open(os.path.join(self.folder, METRICS_NAME), "a") as f:
            f.write(json.dumps(record) + "\n")
        improved, stop = self.tracker.update(record)
        if improved:
            torch.save(self.checkpoint(int(iteration)), os.path.join(self.folder, BEST_NAME))
        print(f"[focoos_amd.train] validation at iter {iteration}: {self.tracker.metric} = {record.get(self.tracker.metric)}"
              + (" (best)" if improved else f" ({self.tracker.bad} without improvement)"), flush=True)
        return stop

    def finish(self, final_path: str) -> Optional[dict]:
        """End of run: the best checkpoint replaces ``final_path`` (its "iteration" is the best record's) and ``model_best.pth`` is gone.
        Returns the best record (None: no validation produced a finite metric, ``final_path`` keeps the last weights)."""
        best = os.path.join(self.folder, BEST_NAME)
        if self.tracker.best is not None and os.path.exists(best):
            os.replace(best, final_path)
        return self.tracker.best

    def close(self) -> None:
        """Whatever ended the run: the engine's plan table is what it was before it."""
        eng = self.model.engine
        eng.retain_plans = False
        eng.drop_plans_except(self._plans_before)
