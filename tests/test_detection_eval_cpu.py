"""COCO bbox AP without a GPU: focoos_amd/detection_eval.py (DetectionEvaluator, accumulate, summarize, the record merge) against the
hand-derived cases of tests/golden/coco_bbox_cases.json and the naive restatement tests/cocoeval_ref.py; the refusals of
FocoosModel.eval_detection.  The pycocotools comparison runs only where pycocotools is importable."""
import json
import os

import numpy as np
import pytest
import torch

from focoos_amd import detection_eval as D
from focoos_amd.ports import Boxes, DatasetEntry, DetectionDatasetEntry, Instances, ModelInfo, TrainerArgs
from focoos_amd.registry import ModelRegistry
from tests import cocoeval_ref as R
from tests import detection_scenes as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "coco_bbox_cases.json")
N_SCENES = 200


def _evaluate(scene):
    ev = D.DetectionEvaluator(scene["class_names"])
    ev.process(*S.entries_and_outputs(scene))
    return ev.evaluate()


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_hand_derived_cases(case):
    scene = S.golden_scene(case)
    for name, got in (("restatement", R.evaluate(S.ref_images(scene), scene["class_names"])), ("DetectionEvaluator", _evaluate(scene))):
        got = got["bbox"]
        assert set(got) == set(case["expect"]), (name, sorted(got))
        for k, want in case["expect"].items():
            if want is None:
                assert got[k] is None, (name, k, got[k])
            else:
                assert got[k] is not None and abs(got[k] - want) <= 1e-9, (name, k, got[k], want)


def test_random_scenes_equal_restatement():
    n_none = n_img = 0
    for seed in range(N_SCENES):
        scene = S.make_scene(seed)
        want = R.evaluate(S.ref_images(scene), scene["class_names"])
        got = _evaluate(scene)
        assert dict(got.get("bbox", {})) == dict(want.get("bbox", {})), f"scene {seed}"     # == on floats, None for None
        assert bool(got) == bool(want)
        n_none += sum(v is None for v in got.get("bbox", {}).values())
        n_img += len(scene["images"])
    print(f"MEASURED {N_SCENES} scenes, {n_img} images, {n_none} None values: DetectionEvaluator == restatement exactly")


def test_instances_and_raw_arrays_agree_and_key_order():
    scene = S.make_scene(7, n_images=4, n_classes=3)
    inputs, raw = S.entries_and_outputs(scene)
    inst = [{"instances": Instances((256, 256), boxes=Boxes(torch.from_numpy(o["boxes"].copy())), scores=torch.from_numpy(o["scores"].copy()),
                                    classes=torch.from_numpy(o["classes"].copy()))} for o in raw]
    a, b = D.DetectionEvaluator(scene["class_names"]), D.DetectionEvaluator(scene["class_names"])
    a.process(inputs, raw)
    for i in range(len(inputs)):                       # image by image, in another order: the evaluator sorts by image id
        j = len(inputs) - 1 - i
        b.process([inputs[j]], [inst[j]])
    ra, rb = a.evaluate(), b.evaluate()
    assert ra == rb and list(ra) == ["bbox"]
    assert list(ra["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] + ["AP-" + n for n in scene["class_names"]]
    one = S.make_scene(3, n_images=2, n_classes=1)
    assert list(_evaluate(one)["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]      # per-category rows need more than one class
    # ground truth given as instances (absolute XYXY) instead of annotations: same result when nothing is crowd
    scene2 = S.make_scene(11, n_images=3, n_classes=2)
    for im in scene2["images"]:
        for g in im["gts"]:
            g["iscrowd"] = 0
    inputs2, raw2 = S.entries_and_outputs(scene2)
    as_inst = []
    for e in inputs2:
        bb = np.array([a_["bbox"] for a_ in e.annotations], np.float64).reshape(-1, 4)
        xyxy = np.stack([bb[:, 0], bb[:, 1], bb[:, 0] + bb[:, 2], bb[:, 1] + bb[:, 3]], 1)
        as_inst.append(DatasetEntry(image_id=e.image_id, height=256, width=256,
                                    instances=Instances((256, 256), boxes=Boxes(torch.from_numpy(xyxy)),
                                                        classes=torch.tensor([a_["category_id"] for a_ in e.annotations], dtype=torch.int64))))
    c, d = D.DetectionEvaluator(scene2["class_names"]), D.DetectionEvaluator(scene2["class_names"])
    c.process(inputs2, raw2)
    d.process(as_inst, raw2)
    assert c.evaluate() == d.evaluate()
    assert D.DetectionEvaluator(["a", "b"]).evaluate() == {}


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    scene = S.make_scene(21, n_images=6, n_classes=4)
    inputs, raw = S.entries_and_outputs(scene)
    ev = D.DetectionEvaluator(scene["class_names"])
    mine = [i for i in range(len(inputs)) if i % world == (world - 1 - rank)]      # interleaved shards, rank 0 does not hold image 0
    ev.process([inputs[i] for i in mine], [raw[i] for i in mine])
    rec = ev.records() or D.MatchRecords(len(scene["class_names"]))
    merged = D.gather_records(rec, dst=0)
    if rank == 0:
        torch.save(merged.state(), out)
    dist.destroy_process_group()


def test_two_rank_gather_equals_single_process(tmp_path):
    import torch.multiprocessing as mp

    from focoos_amd.launch import _find_free_port

    out = str(tmp_path / "rec.pt")
    mp.start_processes(_gather_worker, args=(2, _find_free_port(), out), nprocs=2, start_method="spawn")
    scene = S.make_scene(21, n_images=6, n_classes=4)
    merged = D.MatchRecords(len(scene["class_names"]), **torch.load(out, weights_only=False))
    assert list(merged.image_id) == sorted(merged.image_id)
    got = D.results_from(merged, scene["class_names"])
    assert got == _evaluate(scene) and got["bbox"]["AP"] is not None


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


@pytest.mark.parametrize("name", ["bisenetformer-l-ade", "fai-cls-n-coco", "fai-mf-l-coco-ins"])
def test_eval_detection_refuses_other_families_before_anything_spawns(name, monkeypatch, tmp_path):
    from focoos_amd.model import FocoosModel

    called = []
    monkeypatch.setattr("focoos_amd.launch.launch", lambda *a, **k: called.append("launch"))
    for cls in ("ClsEngine", "MfEngine", "BfEngine", "DetrEngine"):
        monkeypatch.setattr(f"focoos_amd.model.{cls}", lambda *a, **k: called.append("engine"))
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match="fai_detr"):
        FocoosModel.eval_detection(_fm(name), TrainerArgs(run_name="x", output_dir=str(out), num_gpus=2), [DatasetEntry()])
    assert called == [] and not out.exists()


def test_eval_still_refuses_detection(monkeypatch, tmp_path):
    from focoos_amd.model import FocoosModel

    called = []
    monkeypatch.setattr("focoos_amd.launch.launch", lambda *a, **k: called.append("launch"))
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match="COCOeval"):
        FocoosModel.eval(_fm("fai-detr-l-coco"), TrainerArgs(run_name="x", output_dir=str(out)), [DatasetEntry()])
    assert called == [] and not out.exists()


def test_eval_detection_metadata_checks():
    from types import SimpleNamespace

    fm = _fm("fai-detr-l-coco")
    fm.model.num_classes = 80
    names = [f"t{i}" for i in range(80)]
    assert D.resolve(fm, SimpleNamespace(metadata=SimpleNamespace(task="detection", thing_classes=names, name="coco"))) == (names, "coco")
    with pytest.raises(ValueError, match="num_classes"):
        D.resolve(fm, SimpleNamespace(dataset=SimpleNamespace(metadata=SimpleNamespace(task="detection", thing_classes=["a"], name="x"))))
    with pytest.raises(ValueError, match="mismatch"):
        D.resolve(fm, SimpleNamespace(metadata=SimpleNamespace(task="semseg", thing_classes=names, name="x")))
    assert D.resolve(fm, [1]) == (list(fm.model_info.classes), None)


def test_ground_truth_forms():
    e = DetectionDatasetEntry(annotations=[{"bbox": [1, 2, 3, 4], "category_id": 2}, {"bbox": [0, 0, 5, 5], "category_id": 0, "iscrowd": 1, "area": 7.5},
                                           {"bbox": [0, 0, 1, 1], "category_id": 1, "ignore": 1}])
    box, cat, flag, area = D.ground_truth(e)
    assert box.dtype == np.float64 and box.tolist() == [[1, 2, 3, 4], [0, 0, 5, 5], [0, 0, 1, 1]]
    assert cat.tolist() == [2, 0, 1] and flag.tolist() == [0, 1, 2] and area.tolist() == [12.0, 7.5, 1.0]
    assert [f.name for f in __import__("dataclasses").fields(DatasetEntry)] == ["image", "height", "width", "instances", "file_name", "image_id"]


def test_against_pycocotools_when_installed():
    """The hook for a machine that has pycocotools: the random scenes through the real COCOeval (maxDets [1, 10, 100]), equal to 1e-12."""
    try:
        import pycocotools.cocoeval as ce
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except Exception:
        pytest.skip("pycocotools is not installed")
    if getattr(ce, "__file__", None) is None or not hasattr(COCOeval, "evaluateImg"):
        pytest.skip("pycocotools is not installed (an import stub of another test is)")

    for seed in range(N_SCENES):                      # the scenes of test_random_scenes_equal_restatement
        scene = S.make_scene(seed)
        names = scene["class_names"]
        imgs = [im for im in S.ref_images(scene) if im["dets"]]
        got = _evaluate(scene)
        if not imgs:
            assert got == {}
            continue

        def coco(anns):
            c = COCO()
            c.dataset["images"] = [{"id": im["image_id"], "height": 256, "width": 256} for im in imgs]
            c.dataset["categories"] = [{"id": k, "name": n} for k, n in enumerate(names)]
            for i, a in enumerate(anns):
                a["id"], a["area"] = i + 1, a.get("area", a["bbox"][2] * a["bbox"][3])
                a.setdefault("iscrowd", 0)
            c.dataset["annotations"] = anns
            c.createIndex()
            return c

        gt = coco([dict(g, image_id=im["image_id"]) for im in imgs for g in im["gts"]])
        dt = coco([dict(d, image_id=im["image_id"]) for im in imgs for d in im["dets"]])
        coco_eval = COCOeval(gt, dt, "bbox")
        coco_eval.params.maxDets = [1, 10, 100]
        coco_eval.evaluate()
        coco_eval.accumulate()
        coco_eval.summarize()
        want = {m: (coco_eval.stats[i] * 100 if coco_eval.stats[i] >= 0 else None) for i, m in enumerate(D.METRICS)}
        if len(names) > 1:
            for k, n in enumerate(names):
                p = coco_eval.eval["precision"][:, :, k, 0, -1]
                p = p[p > -1]
                want["AP-" + n] = float(np.mean(p) * 100) if p.size else None
        assert list(got["bbox"]) == list(want), seed
        for m, w in want.items():
            assert (got["bbox"][m] is None) == (w is None) and (w is None or abs(got["bbox"][m] - w) <= 1e-12), (seed, m)
