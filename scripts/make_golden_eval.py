#!/usr/bin/env python
"""Generate tests/golden/eval_metrics.json by running the REAL reference evaluators (imported through oracle/ref_import.py, which this script
only uses): SemSegEvaluator.evaluate on fixed confusion matrices (classes absent from the ground truth, an all-ignore row) and
ClassificationEvaluator.process + evaluate on fixed probabilities and labels (classes never seen, probabilities of exactly 0.5).  The inputs
are stored next to the results, so tests/test_eval_cpu.py needs no reference tree.  Run where the reference tree exists:
    python scripts/make_golden_eval.py
"""
from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.json")


def semseg_cases():
    rs = np.random.RandomState(7)
    cases = []
    for K, absent in ((5, [3]), (19, [0, 7, 18])):
        conf = rs.randint(0, 50, size=(K + 1, K + 1)).astype(np.int64)
        conf[:, absent] = 0                       # classes absent from the ground truth: IoU / ACC NaN -> None
        conf[-1, :] = rs.randint(0, 9, size=K + 1)  # predictions on ignore pixels are not counted by evaluate()
        cases.append({"names": [f"c{i}" for i in range(K)], "conf": conf.tolist()})
    cases.append({"names": ["a", "b", "c"], "conf": np.zeros((4, 4), np.int64).tolist()})   # all-ignore: every metric None
    z = np.zeros((4, 4), np.int64)
    z[:, 3] = [4, 0, 2, 9]
    cases.append({"names": ["a", "b", "c"], "conf": z.tolist()})
    return cases


def cls_cases():
    rs = np.random.RandomState(3)
    K, N = 6, 9
    probs = rs.rand(N, K).astype(np.float32)
    probs[0, :3] = 0.5
    probs[4, 2] = 0.5
    labels = [sorted(set(rs.randint(0, K - 1, size=2).tolist())) for _ in range(N)]   # class K-1 never in the ground truth
    return [{"names": [f"k{i}" for i in range(K)], "probs": probs.tolist(), "labels": labels}]


def reference_semseg(names, conf):
    from focoos.trainer.evaluation.sem_seg_evaluation import SemSegEvaluator

    ev = SemSegEvaluator.__new__(SemSegEvaluator)
    ev._distributed, ev._num_classes, ev._class_names = False, len(names), names
    ev._conf_matrix = np.asarray(conf, dtype=np.int64)
    ev._predictions = []
    return dict(ev.evaluate()["sem_seg"])


def reference_cls(names, probs, labels):
    from focoos.trainer.evaluation.classification_evaluation import ClassificationEvaluator

    ev = ClassificationEvaluator.__new__(ClassificationEvaluator)
    ev._distributed, ev.num_classes, ev.class_names = False, len(names), names
    ev._cpu_device = torch.device("cpu")
    ev.reset()
    ev.process([{"label": lb} for lb in labels], [{"logits": torch.tensor(p)} for p in probs])
    return dict(ev.evaluate()["classification"])


def main():
    ref_import.install()
    out = {"semseg": [], "classification": []}
    for c in semseg_cases():
        out["semseg"].append(dict(c, metrics=reference_semseg(c["names"], c["conf"])))
    for c in cls_cases():
        out["classification"].append(dict(c, metrics=reference_cls(c["names"], c["probs"], c["labels"])))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote {GOLDEN}")


if __name__ == "__main__":
    main()
