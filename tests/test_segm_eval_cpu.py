"""COCO segm AP without a GPU: InstanceSegmentationEvaluator (focoos_amd/detection_eval.py) against the hand-derived cases of
tests/golden/coco_segm_cases.json and the naive per-pixel restatement tests/cocoeval_segm_ref.py; the ground-truth input forms and refusals;
the record merge; the refusals of FocoosModel.eval_instance_segmentation; the share of near-threshold pixels of the GPU sampling test's
inputs.  The pycocotools comparison runs only where pycocotools is importable (it has not run where this project is built)."""
import json
import os

import numpy as np
import pytest
import torch

from focoos_amd import detection_eval as D
from focoos_amd import segm_eval as G
from focoos_amd.ports import BitMasks, DatasetEntry, DetectionDatasetEntry, Instances, ModelInfo, TrainerArgs
from focoos_amd.registry import ModelRegistry
from tests import cocoeval_segm_ref as R
from tests import segm_scenes as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "coco_segm_cases.json")
N_SCENES = 200


def _evaluate(scene, form="dense"):
    ev = D.InstanceSegmentationEvaluator(scene["class_names"])
    ev.process(*S.entries_and_outputs(scene, form))
    return ev.evaluate()


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_hand_derived_cases(case):
    scene = S.golden_scene(case)
    for name, got in (("restatement", R.evaluate(S.ref_images(scene), scene["class_names"])), ("InstanceSegmentationEvaluator", _evaluate(scene))):
        got = got["segm"]
        assert set(got) == set(case["expect"]), (name, sorted(got))
        for k, want in case["expect"].items():
            if want is None:
                assert got[k] is None, (name, k, got[k])
            else:
                assert got[k] is not None and abs(got[k] - want) <= 1e-9, (name, k, got[k], want)


def test_hand_derived_cases_cover_the_protocol():
    cases = _cases()
    gts = [g for c in cases for im in c["images"] for g in im["gts"]]
    dets = [d for c in cases for im in c["images"] for d in im["dets"]]
    assert any(g.get("iscrowd") for g in gts) and any("area" in g for g in gts) and any(d["rects"] == [] for d in dets)
    assert {"a_iou_exactly_0.5", "b_iou_exactly_0.75", "g_equal_iou_later_gt_wins", "h_one_sided_categories"} <= {c["name"] for c in cases}


def test_random_scenes_equal_restatement():
    n_none = n_img = n_crowd = n_w = 0
    for seed in range(N_SCENES):
        scene = S.make_scene(seed)
        want = R.evaluate(S.ref_images(scene), scene["class_names"])
        got = _evaluate(scene, "rle" if seed % 2 else "dense")
        assert dict(got.get("segm", {})) == dict(want.get("segm", {})), f"scene {seed}"     # == on floats, None for None
        assert bool(got) == bool(want)
        n_none += sum(v is None for v in got.get("segm", {}).values())
        n_img += len(scene["images"])
        n_crowd += sum(g["iscrowd"] for im in scene["images"] for g in im["gts"])
        n_w += sum(im["width"] % 64 == 0 for im in scene["images"])
    assert n_w == 0 and n_crowd > 0
    print(f"MEASURED {N_SCENES} scenes, {n_img} images, {n_crowd} crowds, {n_none} None values: InstanceSegmentationEvaluator == restatement")


def test_input_forms_agree():
    scene = S.make_scene(7, n_images=3, n_classes=3)
    for im in scene["images"]:
        for g in im["gts"]:
            g.pop("area", None)
    dense, rle = _evaluate(scene, "dense"), _evaluate(scene, "rle")
    assert dense == rle and list(dense) == ["segm"]
    assert list(dense["segm"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] + ["AP-" + n for n in scene["class_names"]]
    inputs, raw = S.entries_and_outputs(scene)
    inst = [{"instances": Instances((im["height"], im["width"]), masks=BitMasks(torch.from_numpy(o["masks"].copy())),
                                    scores=torch.from_numpy(o["scores"].copy()), classes=torch.from_numpy(o["classes"].copy()))}
            for im, o in zip(scene["images"], raw)]
    b = D.InstanceSegmentationEvaluator(scene["class_names"])
    for i in reversed(range(len(inputs))):                  # image by image, in another order: the evaluator sorts by image id
        b.process([inputs[i]], [inst[i]])
    assert b.evaluate() == dense
    # ground truth given as instances.masks: same result when nothing is crowd and no area is given
    for im in scene["images"]:
        for g in im["gts"]:
            g["iscrowd"] = 0
    inputs2, raw2 = S.entries_and_outputs(scene)
    as_inst = []
    for e, im in zip(inputs2, scene["images"]):
        H, W = im["height"], im["width"]
        gm = np.stack([g["mask"] for g in im["gts"]]) if im["gts"] else np.zeros((0, H, W), bool)
        masks = BitMasks(torch.from_numpy(gm)) if e.image_id % 2 else torch.from_numpy(gm)
        as_inst.append(DatasetEntry(image_id=e.image_id, height=H, width=W, instances=Instances(
            (H, W), masks=masks, classes=torch.tensor([g["category_id"] for g in im["gts"]], dtype=torch.int64))))
    c, d = D.InstanceSegmentationEvaluator(scene["class_names"]), D.InstanceSegmentationEvaluator(scene["class_names"])
    c.process(inputs2, raw2)
    d.process(as_inst, raw2)
    assert c.evaluate() == d.evaluate() and c.evaluate()["segm"]["AP"] is not None
    assert D.InstanceSegmentationEvaluator(["a", "b"]).evaluate() == {}
    one = S.make_scene(3, n_images=2, n_classes=1)
    assert list(_evaluate(one)["segm"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def test_ground_truth_refusals_and_fields():
    m = np.zeros((4, 70), np.uint8)
    m[1:3, 60:70] = 1
    ent = lambda seg, **kw: DetectionDatasetEntry(height=4, width=70, annotations=[dict({"segmentation": seg, "category_id": 1}, **kw)])   # noqa: E731
    mask, cat, flag, area = D.ground_truth_masks(ent(m, iscrowd=1))
    assert mask.dtype == bool and mask.shape == (1, 4, 70) and cat.tolist() == [1] and flag.tolist() == [1] and area.tolist() == [20.0]
    assert D.ground_truth_masks(ent(m, area=7.5, ignore=1))[2:] == (np.array([2]), np.array([7.5]))
    rle = {"size": [4, 70], "counts": [241] + [2] * 19 + [1]}       # column-major: 60 columns and one row of zeros, then ten columns 0 1 1 0
    assert np.array_equal(D.ground_truth_masks(ent(rle))[0][0], m.astype(bool))
    with pytest.raises(NotImplementedError, match="polygon"):
        D.ground_truth_masks(ent([[1.0, 1.0, 5.0, 1.0, 5.0, 3.0]]))
    with pytest.raises(NotImplementedError, match="compressed RLE string"):
        D.ground_truth_masks(ent({"size": [4, 70], "counts": "abc"}))
    with pytest.raises(ValueError, match="does not match"):
        D.ground_truth_masks(ent(np.zeros((4, 64), np.uint8)))
    with pytest.raises(ValueError, match="does not match"):
        D.ground_truth_masks(ent({"size": [70, 4], "counts": [280]}))
    packed = D.pack_rows(m[None].astype(bool))
    assert packed.shape == (1, 4, 16) and D.popcount(packed).tolist() == [20]
    from focoos_amd.processor import MaskFormerProcessor

    assert np.array_equal(MaskFormerProcessor.unpack_masks(torch.from_numpy(packed.view(np.int32)), 4, 70)[0], m.astype(bool))


def test_match_image_category_is_unchanged_by_the_refactor():
    """the bbox form is now bbox_iou + match_from_iou; the mask form shares match_from_iou"""
    rs = np.random.RandomState(0)
    d = np.abs(rs.randn(30, 4)) * 20 + 1
    g = np.abs(rs.randn(9, 4)) * 20 + 1
    flag, area = (rs.rand(9) < 0.2).astype(np.int32), g[:, 2] * g[:, 3]
    a = D.match_image_category(d, g, flag, area)
    b = D.match_from_iou(D.bbox_iou(d, g, (flag & 1).astype(bool)), d[:, 2] * d[:, 3], flag, area)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    scene = S.make_scene(21, n_images=4, n_classes=3)
    inputs, raw = S.entries_and_outputs(scene)
    ev = D.InstanceSegmentationEvaluator(scene["class_names"])
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
    scene = S.make_scene(21, n_images=4, n_classes=3)
    merged = D.MatchRecords(len(scene["class_names"]), **torch.load(out, weights_only=False))
    got = D.results_from(merged, scene["class_names"], "segm")
    assert got == _evaluate(scene) and got["segm"]["AP"] is not None


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


@pytest.mark.parametrize("name,match", [("bisenetformer-l-ade", "bisenetformer"), ("fai-cls-n-coco", "fai_cls"), ("fai-detr-l-coco", "fai_detr"),
                                        ("fai-mf-l-ade", "semantic")])
def test_eval_instance_segmentation_refuses_before_anything_spawns(name, match, monkeypatch, tmp_path):
    from focoos_amd.model import FocoosModel

    called = []
    monkeypatch.setattr("focoos_amd.launch.launch", lambda *a, **k: called.append("launch"))
    for cls in ("ClsEngine", "MfEngine", "BfEngine", "DetrEngine"):
        monkeypatch.setattr(f"focoos_amd.model.{cls}", lambda *a, **k: called.append("engine"))
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match=match):
        FocoosModel.eval_instance_segmentation(_fm(name), TrainerArgs(run_name="x", output_dir=str(out), num_gpus=2), [DatasetEntry()])
    assert called == [] and not out.exists()


def test_eval_keeps_refusing_instance_segmentation(tmp_path):
    from focoos_amd.model import FocoosModel

    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match="COCOeval"):
        FocoosModel.eval(_fm("fai-mf-l-coco-ins"), TrainerArgs(run_name="x", output_dir=str(out)), [DatasetEntry()])
    assert not out.exists()


def test_metadata_checks():
    from types import SimpleNamespace

    fm = _fm("fai-mf-l-coco-ins")
    fm.model.num_classes = 80
    names = [f"t{i}" for i in range(80)]
    assert G.resolve(fm, SimpleNamespace(metadata=SimpleNamespace(task="instseg", thing_classes=names, name="coco"))) == (names, "coco")
    with pytest.raises(ValueError, match="num_classes"):
        G.resolve(fm, SimpleNamespace(dataset=SimpleNamespace(metadata=SimpleNamespace(task="instseg", thing_classes=["a"], name="x"))))
    with pytest.raises(ValueError, match="mismatch"):
        G.resolve(fm, SimpleNamespace(metadata=SimpleNamespace(task="detection", thing_classes=names, name="x")))
    assert G.resolve(fm, [1]) == (list(fm.model_info.classes), None)


@pytest.mark.parametrize("name", sorted(S.SAMPLING_CASES))
def test_sampling_inputs_keep_clear_of_the_threshold(name):
    """the condition of the GPU test's fp64 gate, checked on the fp64 restatement alone: at most 0.1 % of the pixels lie within delta"""
    h, w, Hin, Win, sizes = S.SAMPLING_CASES[name]
    lo, _ = S.sampling_inputs(name)
    delta = S.sampling_delta(h, w, Hin, Win)
    near = total = 0
    for b, (H, W) in enumerate(sizes):
        m = S.sample_fp64(lo[b], Hin, Win, H, W)
        near += int(((m - S.MASK_THRESHOLD).abs() <= delta).sum())
        total += m.numel()
    print(f"MEASURED sampling inputs {name}: {near} of {total} fp64 values within delta = {delta:.3e} of the threshold")
    assert near / total <= 1e-3


def test_against_pycocotools_when_installed():
    """The hook for a machine that has pycocotools: the random scenes through the real COCOeval with iouType "segm" (ground truth and
    detections as uncompressed RLE turned into RLE objects by pycocotools itself), equal to 1e-12."""
    try:
        import pycocotools.cocoeval as ce
        import pycocotools.mask as mask_util
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except Exception:
        pytest.skip("pycocotools is not installed")
    if getattr(ce, "__file__", None) is None or not hasattr(COCOeval, "evaluateImg"):
        pytest.skip("pycocotools is not installed (an import stub of another test is)")
    for seed in range(N_SCENES):
        scene = S.make_scene(seed)
        names = scene["class_names"]
        got = _evaluate(scene)
        enc = lambda m: mask_util.encode(np.asfortranarray(np.asarray(m, np.uint8)))   # noqa: E731

        def coco(anns):
            c = COCO()
            c.dataset["images"] = [{"id": im["image_id"], "height": im["height"], "width": im["width"]} for im in scene["images"]]
            c.dataset["categories"] = [{"id": k, "name": n} for k, n in enumerate(names)]
            for i, a in enumerate(anns):
                a["id"] = i + 1
                a.setdefault("area", float(mask_util.area(a["segmentation"])))
                a.setdefault("iscrowd", 0)
            c.dataset["annotations"] = anns
            c.createIndex()
            return c

        gt = coco([dict({k: v for k, v in g.items() if k != "mask"}, segmentation=enc(g["mask"]), image_id=im["image_id"])
                   for im in scene["images"] for g in im["gts"]])
        dt = coco([{"segmentation": enc(im["masks"][j]), "score": float(im["score"][j]), "category_id": int(im["cls"][j]),
                    "image_id": im["image_id"]} for im in scene["images"] for j in range(len(im["cls"]))])
        coco_eval = COCOeval(gt, dt, "segm")
        coco_eval.evaluate()
        coco_eval.accumulate()
        coco_eval.summarize()
        want = {m: (coco_eval.stats[i] * 100 if coco_eval.stats[i] >= 0 else None) for i, m in enumerate(D.METRICS)}
        for m, w in want.items():
            assert (got["segm"][m] is None) == (w is None) and (w is None or abs(got["segm"][m] - w) <= 1e-12), (seed, m)


def test_score_order_inversions_matches_pairwise_count():
    """segm_eval.score_order_inversions (the end-to-end rule of the GPU test and the bench) against the pairwise definition: a pair of one
    category is inverted when the two stable descending orders place it differently; the largest gap is taken over exactly those pairs."""
    rs = np.random.RandomState(5)
    assert G.score_order_inversions(np.zeros(4, np.int32), np.array([.5, .5, .2, .9]), np.array([.4, .4, .1, .8])) == (0, 0.0)
    seen = 0
    for _ in range(50):
        n = int(rs.randint(2, 40))
        cat = rs.randint(0, 3, n).astype(np.int32)
        a = np.round(rs.rand(n), 2).astype(np.float32)                       # duplicates on purpose
        b = (a + rs.choice([0.0, 0.0, 0.01, -0.01, 0.3], n)).astype(np.float32)
        pa, pb = np.empty(n, np.int64), np.empty(n, np.int64)
        pa[np.lexsort((np.arange(n), -a))] = np.arange(n)
        pb[np.lexsort((np.arange(n), -b))] = np.arange(n)
        same = cat[:, None] == cat[None, :]
        inv = same & (pa[:, None] < pa[None, :]) & (pb[:, None] > pb[None, :])      # [i, j]: a puts i first, b puts j first
        want_n = int(inv.any(0).sum())
        want_gap = float((a[:, None].astype(np.float64) - a[None, :])[inv].max()) if inv.any() else 0.0
        assert G.score_order_inversions(cat, a, b) == (want_n, want_gap)
        seen += want_n
    assert seen > 0


def test_check_supported_needs_the_postprocessing_type_key():
    """a fai-mf config that does not say which kind it is is refused, not taken for an instance model"""
    fm = _fm("fai-mf-l-coco-ins")
    G.check_supported(fm)
    del fm.model_info.config["postprocessing_type"]
    with pytest.raises(NotImplementedError, match="fai_mf.*postprocessing_type None"):
        G.check_supported(fm)
