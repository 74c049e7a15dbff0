"""The plain-Python parts of validation during training (focoos_amd/validation.py): when a run validates, which record is best and when
early stopping ends the run, which evaluator and task metric a model gets.  No GPU."""
import math

import pytest

from focoos_amd.validation import BestTracker, evaluator_for, task_of, validation_iterations


@pytest.mark.parametrize("max_iters,period,expected", [
    (4, 2, [2, 4]),                  # the period divides max_iters: the last iteration is a validation point already
    (5, 2, [2, 4, 5]),               # it does not: once more after the last iteration
    (8, 1, [1, 2, 3, 4, 5, 6, 7, 8]),
    (7, 7, [7]),
    (3, 200, []),                    # a period above max_iters: the run does not validate (FocoosModel.train's default on a short run)
    (10, 0, []),
    (10, -5, []),
    (1000, 300, [300, 600, 900, 1000]),
])
def test_validation_schedule(max_iters, period, expected):
    assert validation_iterations(max_iters, period) == expected


def _run(values, **kw):
    tr = BestTracker("bbox/AP", **kw)
    out = [tr.update({"iteration": i + 1, "bbox/AP": v}) for i, v in enumerate(values)]
    return tr, out


def test_tracker_strictly_greater_wins_and_ties_keep_the_earlier():
    tr, out = _run([0.0, 0.0, 1.5, 1.5, 1.0], early_stop=False, patience=1)
    assert [o[0] for o in out] == [True, False, True, False, False]
    assert not any(o[1] for o in out)                     # early_stop off: never stops, whatever the patience
    assert tr.best == {"iteration": 3, "bbox/AP": 1.5}
    assert [r["iteration"] for r in tr.history] == [1, 2, 3, 4, 5]


def test_tracker_nan_and_none_never_win():
    tr, out = _run([float("nan"), None, 0.25, float("nan"), 0.5], early_stop=False)
    assert [o[0] for o in out] == [False, False, True, False, True]
    assert tr.best["iteration"] == 5
    tr, out = _run([float("nan"), None], early_stop=False)
    assert tr.best is None and tr.bad == 2
    tr, out = _run([-1.0, float("nan")], early_stop=False)    # COCO's -1 (no ground truth in range) is a number: it can be the best so far
    assert tr.best["iteration"] == 1 and not math.isnan(tr.best["bbox/AP"])


def test_tracker_patience_counts_consecutive_misses():
    tr, out = _run([1.0, 1.0, 1.0], early_stop=True, patience=2)           # weights that never move: stop at the third validation
    assert [o[1] for o in out] == [False, False, True] and tr.best["iteration"] == 1
    tr, out = _run([1.0, 0.5, 2.0, 2.0, 1.0, 0.0], early_stop=True, patience=3)
    assert [o[1] for o in out] == [False, False, False, False, False, True]   # the improvement at 3 resets the count
    assert tr.best["iteration"] == 3
    tr, out = _run([float("nan"), float("nan")], early_stop=True, patience=2)
    assert out[-1] == (False, True)


def test_task_and_evaluator_dispatch():
    from focoos_amd.evaluation import TASK_METRICS

    assert task_of("bisenetformer", {"postprocessing_type": "semantic"}, "semseg") == "semseg"
    assert task_of("fai_mf", {"postprocessing_type": "semantic"}, "instseg") == "semseg"
    assert task_of("fai_mf", {"postprocessing_type": "instance"}, "instseg") == "instseg"
    assert task_of("fai_mf", {}, "instseg") == "instseg"
    assert task_of("fai_detr", {}, "detection") == "detection"

    class _Enum:
        value = "detection"

    assert task_of("fai_detr", {}, _Enum()) == "detection"
    assert evaluator_for("fai_detr", "detection") == ("detection", "bbox/AP") == ("detection", TASK_METRICS["detection"])
    assert evaluator_for("fai_mf", "instseg") == ("instseg", "segm/AP")
    assert evaluator_for("fai_mf", "semseg") == ("semseg", "sem_seg/mIoU")
    assert evaluator_for("bisenetformer", "semseg") == ("semseg", "sem_seg/mIoU")
    for fam, task in (("fai_cls", "classification"), ("fai_detr", "instseg"), ("bisenetformer", "instseg"), ("fai_detr", "semseg")):
        with pytest.raises(NotImplementedError):
            evaluator_for(fam, task)
