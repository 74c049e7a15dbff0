#!/usr/bin/env python
"""Generate tests/golden/augment_defaults.json from the REAL reference (imported through oracle/ref_import.py): the field names and defaults
of focoos.data.default_aug.DatasetAugmentations and what get_default_by_task returns for every task, plain and advanced, at two resolutions.
Only the recorded values are stored, so tests/test_augment_cpu.py needs no reference tree.  Run where the reference tree exists:
    python scripts/make_golden_augment.py
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "augment_defaults.json")


def main():
    ref_import.install()
    from focoos.data import default_aug as D
    from focoos.ports import Task

    out = {"fields": [[f.name, f.default] for f in dataclasses.fields(D.DatasetAugmentations)], "by_task": []}
    for task in (Task.DETECTION, Task.SEMSEG, Task.INSTANCE_SEGMENTATION, Task.CLASSIFICATION, Task.KEYPOINT):
        for advanced in (False, True):
            for resolution in (640, 512, [384, 512]):
                res = tuple(resolution) if isinstance(resolution, list) else resolution
                train, val = D.get_default_by_task(task, res, advanced)
                out["by_task"].append({"task": task.value, "advanced": advanced, "resolution": resolution,
                                       "train": dataclasses.asdict(train), "val": dataclasses.asdict(val)})
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(out['fields'])} fields, {len(out['by_task'])} presets")


if __name__ == "__main__":
    main()
