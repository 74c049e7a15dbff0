"""FocoosModel.eval without a GPU: the metric formulas against golden fixtures of the reference evaluators (scripts/make_golden_eval.py) and,
when the reference tree is present, against the live evaluators; refusals of detection / instance tasks before anything is created; the
2-rank merge of integer counters; ground-truth loading."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from focoos_amd import evaluation as E
from focoos_amd.ports import ClassificationDatasetDict, DatasetEntry, ModelInfo, SemanticSegmentationDatasetEntry, TrainerArgs
from focoos_amd.registry import ModelRegistry

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "eval_metrics.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _cls_counts(probs, labels, K):
    pred = (torch.tensor(probs, dtype=torch.float32) > 0.5).int()
    true = torch.zeros(len(labels), K, dtype=torch.int)
    for i, lb in enumerate(labels):
        true[i, lb] = 1
    return (true * pred).sum(0), ((1 - true) * pred).sum(0), (true * (1 - pred)).sum(0)


def test_semseg_metrics_equal_golden():
    for c in _golden()["semseg"]:
        got = E.sem_seg_metrics(np.array(c["conf"], dtype=np.int64), c["names"])
        assert list(got) == list(c["metrics"])
        assert dict(got) == c["metrics"]


def test_classification_metrics_equal_golden():
    for c in _golden()["classification"]:
        got = E.classification_metrics(*_cls_counts(c["probs"], c["labels"], len(c["names"])), c["names"])
        assert list(got) == list(c["metrics"])
        assert dict(got) == c["metrics"]


def test_live_reference():
    from oracle import ref_import

    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("make_golden_eval", os.path.join(os.path.dirname(__file__), "..", "scripts", "make_golden_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ref_import.install()
    for c in mod.semseg_cases():
        ref = mod.reference_semseg(c["names"], c["conf"])
        assert dict(E.sem_seg_metrics(np.array(c["conf"]), c["names"])) == ref
    for c in mod.cls_cases():
        ref = mod.reference_cls(c["names"], c["probs"], c["labels"])
        assert dict(E.classification_metrics(*_cls_counts(c["probs"], c["labels"], len(c["names"])), c["names"])) == ref
    assert "focoos" in sys.modules


class _FakeModel:
    def __init__(self, family):
        self.family = family
        self.num_classes = 3


def _fm(name):
    from focoos_amd.model import FocoosModel

    info = ModelInfo.from_json(ModelRegistry.get_model_info(name))
    fm = FocoosModel.__new__(FocoosModel)
    fm.model, fm.model_info = _FakeModel(info.model_family), info
    return fm


@pytest.mark.parametrize("name", ["fai-detr-l-coco", "fai-mf-l-coco-ins"])
def test_detection_and_instance_refused_before_anything_spawns(name, monkeypatch, tmp_path):
    from focoos_amd.model import FocoosModel

    called = []
    monkeypatch.setattr("focoos_amd.launch.launch", lambda *a, **k: called.append("launch"))
    for cls in ("ClsEngine", "MfEngine", "BfEngine", "DetrEngine"):
        monkeypatch.setattr(f"focoos_amd.model.{cls}", lambda *a, **k: called.append("engine"))
    fm = _fm(name)
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match="COCOeval"):
        FocoosModel.eval(fm, TrainerArgs(run_name="x", output_dir=str(out), num_gpus=2), [DatasetEntry()])
    assert called == [] and not out.exists()


def test_metadata_checks():
    fm = _fm("bisenetformer-l-ade")
    fm.model.num_classes = 150
    ds = SimpleNamespace(metadata=SimpleNamespace(task="semseg", ignore_label=0, stuff_classes=[f"s{i}" for i in range(150)], name="ade"))
    assert E.resolve(fm, ds) == ("semseg", [f"s{i}" for i in range(150)], 0, "ade")
    bad = SimpleNamespace(dataset=SimpleNamespace(metadata=SimpleNamespace(task="semseg", ignore_label=255, stuff_classes=["a"], name="x")))
    with pytest.raises(ValueError, match="num_classes"):
        E.resolve(fm, bad)
    with pytest.raises(ValueError, match="mismatch"):
        E.resolve(fm, SimpleNamespace(metadata=SimpleNamespace(task="classification", ignore_label=255, stuff_classes=None, name="x")))
    assert E.resolve(fm, [1])[2] == 255


def _merge_worker(rank, world, port, out):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(rank)
    c = torch.randint(0, 1 << 40, (5 * 5,), generator=g, dtype=torch.int64)
    dist.all_reduce(c, op=dist.ReduceOp.SUM)
    if rank == 0:
        torch.save(c, out)
    dist.destroy_process_group()


def test_two_rank_merge_equals_single_process_sum(tmp_path):
    import torch.multiprocessing as mp

    from focoos_amd.launch import _find_free_port

    out = str(tmp_path / "c.pt")
    mp.start_processes(_merge_worker, args=(2, _find_free_port(), out), nprocs=2, start_method="spawn")
    merged = torch.load(out)
    want = sum(torch.randint(0, 1 << 40, (25,), generator=torch.Generator().manual_seed(r), dtype=torch.int64) for r in range(2))
    assert torch.equal(merged, want)
    names = ["a", "b", "c", "d"]
    assert E.sem_seg_metrics(merged.numpy().reshape(5, 5), names) == E.sem_seg_metrics(want.numpy().reshape(5, 5), names)


def test_ground_truth_loading(tmp_path):
    from PIL import Image

    gt = np.array([[0, 1, 255], [2, 255, 1]], dtype=np.uint8)
    p = tmp_path / "gt.png"
    Image.fromarray(gt).save(p)
    e = SemanticSegmentationDatasetEntry(height=2, width=3, sem_seg_file_name=str(p))
    got = E.load_sem_seg(e, 255)
    assert got.dtype == np.uint8 and np.array_equal(got, gt)
    e2 = SemanticSegmentationDatasetEntry(height=2, width=3, sem_seg=gt.astype(np.int64) * 2)
    assert E.load_sem_seg(e2, 255).dtype == np.int32
    # the ignore label maps to K in the counted bin: conf[(K+1) pred + gt']
    K = 3
    gtp = got.astype(np.int64)
    gtp[gtp == 255] = K
    assert gtp.max() == K
    lab = ClassificationDatasetDict(label=[0, 2])
    assert E.classification_target(lab, 4).tolist() == [1, 0, 1, 0]
    ann = ClassificationDatasetDict(annotations=[{"category_id": 1}])
    assert E.classification_target(ann, 4).tolist() == [0, 1, 0, 0]


def test_model_info_fields_appended():
    names = [f.name for f in __import__("dataclasses").fields(ModelInfo)]
    assert names[-2:] == ["val_metrics", "val_dataset"]
