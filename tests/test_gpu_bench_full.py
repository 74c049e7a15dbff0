"""bench.py's plain run against its `--full` run, in process on a small shape (2 images of 320x320, 2 timed steps): the plain line
carries the headline fields and none of the measurements that take work of their own; `--full` adds them back; and what
`--dump-outputs` writes - the last timed step's packed detections - is the same arrays either way, so the extras change nothing the
timed steps compute."""
import glob
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
EXTRAS = ("roofline", "composite_roofline", "single_batch_in_flight")   # cpu_baseline / other_configs: skipped below, they take minutes


def _run(monkeypatch, capsys, extra):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "320"] + extra)
    bench.run(bench.parse())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_lean_and_full_adds_the_extras(monkeypatch, capsys, tmp_path):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    plain = _run(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "plain")])
    assert all(k in plain for k in HEADLINE), sorted(plain)
    assert not [k for k in EXTRAS + ("cpu_baseline", "other_configs") if k in plain], sorted(plain)
    assert plain["value"] > 0 and plain["unit"] == "images/s" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 / 2 - 1.0) < 1e-2        # images/s = batch / seconds per step

    per_op = tmp_path / "per_op.txt"
    full = _run(monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--no-other-configs", "--per-op", str(per_op),
                                      "--dump-outputs", str(tmp_path / "full")])
    assert all(k in full for k in HEADLINE + EXTRAS), sorted(full)
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config")} == \
           {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config")}
    assert full["roofline"]["sum_of_kernel_ms_per_step"] > 0 and full["single_batch_in_flight"]["value"] > 0
    assert per_op.stat().st_size > 0

    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "plain" / "*.npy")))
    assert names and names == sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "full" / "*.npy")))
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n), err_msg=n)
