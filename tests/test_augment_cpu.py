"""Host side of the device augmentation (focoos_amd/augment.py): the public dataclass against values recorded from the reference
(tests/golden/augment_defaults.json, scripts/make_golden_augment.py), the refusals, the sampling distributions, the box geometry against the
fp64 restatement of the resample (tests/augment_ref.py), and run_train's batch assembly with the engine mocked."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

from focoos_amd import augment as A
from focoos_amd.train_data import rank_seed

from . import augment_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "augment_defaults.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _norm(v):
    return list(v) if isinstance(v, (tuple, list)) else v


def test_fields_and_defaults_equal_the_reference():
    want = _golden()["fields"]
    got = [[f.name, f.default] for f in dataclasses.fields(A.DatasetAugmentations)]
    assert got == want


def test_get_default_by_task_equals_the_reference():
    cases = _golden()["by_task"]
    assert len(cases) == 30
    for c in cases:
        res = tuple(c["resolution"]) if isinstance(c["resolution"], list) else c["resolution"]
        train, val = A.get_default_by_task(c["task"], res, c["advanced"])
        for got, want in ((train, c["train"]), (val, c["val"])):
            assert {k: _norm(v) for k, v in dataclasses.asdict(got).items()} == want, (c["task"], c["advanced"], res)
    a, b = A.get_default_by_task("semseg", 512)
    a.crop = False
    assert A.get_default_by_task("semseg", 512)[0].crop is True     # presets are copies


@pytest.mark.parametrize("field,value", [("rotation", 0.25), ("zoom_out", 0.5), ("aspect_ratio", 0.5), ("square", 1.0), ("color_base_hue", 9)])
def test_refused_fields_raise_by_name(field, value):
    augs = A.DatasetAugmentations(**{field: value})
    for make in (lambda: A.DeviceAugmenter(augs, "detection", "cuda:0"), lambda: A.AugmentedDataset([], augs),
                 lambda: A.sample_params(augs, [(100, 100)], torch.Generator())):
        with pytest.raises(NotImplementedError, match=field):
            make()
    A.DeviceAugmenter(A.DatasetAugmentations(), "detection", "cuda:0")     # the defaults construct without touching a device
    with pytest.raises(NotImplementedError, match="classification"):
        A.DeviceAugmenter(A.DatasetAugmentations(), "classification", "cuda:0")


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


AUGS = A.DatasetAugmentations(resolution=320, crop=True, scale_ratio=0.5, color_augmentation=1.0, horizontal_flip=0.5, vertical_flip=0.2)


def test_sample_params_is_deterministic_per_seed_and_differs_per_rank():
    sizes = [(240, 320), (333, 500), (480, 360)] * 3
    a = A.sample_params(AUGS, sizes, _gen(rank_seed(7, 0)))
    b = A.sample_params(AUGS, sizes, _gen(rank_seed(7, 0)))
    c = A.sample_params(AUGS, sizes, _gen(rank_seed(7, 1)))
    assert a == b and a != c


def test_sample_params_distributions_over_10000_draws():
    n = 10000
    rs = np.random.RandomState(3)
    sizes = [(int(h), int(w)) for h, w in zip(rs.randint(120, 700, n), rs.randint(120, 700, n))]
    recs = A.sample_params(AUGS, sizes, _gen(11))
    for p, count in ((AUGS.horizontal_flip, sum(r.hflip for r in recs)), (AUGS.vertical_flip, sum(r.vflip for r in recs))):
        assert abs(count - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (p, count)
    lo, hi = A.short_edge_range(AUGS)
    assert (lo, hi) == (int(2 ** -0.5 * 320), int(2 ** 0.5 * 320))       # ResizeShortestEdge's [min, max] (default_aug.py:170-178)
    edges = np.array([r.short_edge for r in recs])
    assert edges.min() >= lo and edges.max() <= hi
    assert edges.min() == lo and edges.max() == hi                       # 10 000 draws over 227 values reach both ends
    for r in recs:
        assert min(r.res_h, r.res_w) == r.short_edge                     # no max_size clamp at these sizes
        assert (r.out_h, r.out_w) == (320, 320) and r.pad_x == 0 and r.pad_y == 0
        assert r.crop_w == min(320, r.res_w) and r.crop_h == min(320, r.res_h)
        assert 0 <= r.crop_x <= r.res_w - r.crop_w and 0 <= r.crop_y <= r.res_h - r.crop_h
        # the window in source pixels lies inside its source image
        assert -1e-9 <= r.x0 and r.x0 + r.crop_w * r.sx <= r.src_w + 1e-9
        assert -1e-9 <= r.y0 and r.y0 + r.crop_h * r.sy <= r.src_h + 1e-9
        assert 1 - 32 / 255 <= r.brightness <= 1 + 32 / 255 and 0.5 <= r.contrast <= 1.5 and 0.5 <= r.saturation <= 1.5
        assert r.order in (A.ORDER_BCS, A.ORDER_BSC)
    for on in (sum(r.brightness != 1 for r in recs), sum(r.contrast != 1 for r in recs), sum(r.order == A.ORDER_BCS for r in recs)):
        assert abs(on - n / 2) <= 4 * math.sqrt(n / 4)                    # ColorAugSSD's coin flips


def test_no_crop_batches_to_the_largest_resized_size_and_max_size_clamps():
    augs = A.DatasetAugmentations(resolution=256, max_size=300)
    recs = A.sample_params(augs, [(100, 400), (300, 200)], _gen(0))
    assert [(r.res_h, r.res_w) for r in recs] == [(75, 300), (300, 200)]  # ResizeShortestEdge.get_output_shape with the max_size clamp
    assert all((r.out_h, r.out_w) == (300, 300) for r in recs) and all(r.order == A.ORDER_NONE for r in recs)
    rect = A.sample_params(A.DatasetAugmentations(resolution=(128, 192)), [(100, 400)], _gen(0))[0]
    assert (rect.res_h, rect.res_w) == (128, 192)                        # non-square resolution: Resize to the exact shape


def test_flipping_boxes_twice_is_the_identity():
    r = A.identity_record(200, 300)
    r.hflip = r.vflip = True
    boxes = torch.tensor([[10.0, 20.0, 110.0, 90.0], [0.0, 0.0, 300.0, 200.0], [250.5, 100.25, 299.0, 199.0]], dtype=torch.float64)
    once, keep = A.transform_boxes(boxes, r)
    twice, keep2 = A.transform_boxes(once, r)
    assert keep.all() and keep2.all() and torch.equal(twice, boxes)
    assert torch.equal(once[0], torch.tensor([190.0, 110.0, 290.0, 180.0], dtype=torch.float64))
    pts = A.transform_points(A.transform_points(boxes[:, :2], r), r)
    assert torch.equal(pts, boxes[:, :2])


def _painted(h, w, rects):
    img = np.zeros((h, w, 3), np.uint8)
    for i, (x0, y0, x1, y1) in enumerate(rects):
        img[y0:y1, x0:x1, i] = 255          # rectangle i lives in channel i
    return img


@pytest.mark.parametrize("rec", [
    A.AugRecord(src_h=240, src_w=320, out_h=200, out_w=200, res_h=300, res_w=400, crop_x=90, crop_y=40, crop_w=200, crop_h=200, hflip=True),
    A.AugRecord(src_h=240, src_w=320, out_h=160, out_w=224, res_h=150, res_w=200, crop_x=0, crop_y=0, crop_w=200, crop_h=150, pad_x=12, pad_y=5,
                vflip=True),
    A.AugRecord(src_h=301, src_w=203, out_h=128, out_w=128, res_h=190, res_w=128, crop_x=0, crop_y=31, crop_w=128, crop_h=128),
])
def test_boxes_land_on_the_painted_rectangles(rec):
    rects = [(40, 30, 140, 100), (150, 120, 260, 200)] if rec.src_w == 320 else [(20, 60, 120, 160), (100, 170, 190, 280)]
    img = _painted(rec.src_h, rec.src_w, rects)
    out = R.image_f64(img, rec)
    boxes, keep = A.transform_boxes(torch.tensor(rects, dtype=torch.float64), rec)
    assert keep.all()
    for i, bx in enumerate(boxes.tolist()):
        ys, xs = np.nonzero(out[:, :, i] >= 127.5)                        # more than half covered by the rectangle
        seen = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        assert np.abs(np.array(seen) - np.array(bx)).max() <= 1.0, (seen, bx)


def test_boxes_outside_the_crop_are_dropped_and_partial_ones_clipped():
    rec = A.AugRecord(src_h=100, src_w=100, out_h=50, out_w=50, res_h=100, res_w=100, crop_x=50, crop_y=50, crop_w=50, crop_h=50)
    boxes = torch.tensor([[0.0, 0.0, 40.0, 40.0], [40.0, 40.0, 70.0, 120.0], [60.0, 60.0, 60.0, 80.0]])
    out, keep = A.transform_boxes(boxes, rec)
    assert keep.tolist() == [False, True, False]
    assert out[1].tolist() == [0.0, 0.0, 20.0, 50.0]
    inside = A.points_inside(A.transform_points(torch.tensor([[55.0, 55.0], [10.0, 55.0]]), rec), rec)
    assert inside.tolist() == [True, False]


def test_restatement_stays_clear_of_rounding_boundaries_and_identity_is_exact():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    rec = A.identity_record(37, 53)
    assert np.array_equal(R.round_u8(R.image_f64(img, rec)), img)
    rec.hflip = True
    assert np.array_equal(R.round_u8(R.image_f64(img, rec)), img[:, ::-1])
    lab = rs.randint(0, 5, (37, 53)).astype(np.uint8)
    assert np.array_equal(R.labels_ref(lab, rec, 255), lab[:, ::-1])


class _Processor:
    def __init__(self):
        self.calls = []

    def preprocess(self, entries, device=None):
        self.calls.append((entries, device))
        return "images", "targets"


def test_augmented_dataset_and_batch_assembly(monkeypatch):
    from focoos_amd import trainer

    data = ["e0", "e1", "e2"]
    proc = _Processor()
    assemble = trainer.batch_assembler(data, "fai_detr", proc, torch.device("cuda", 0), seed=5, rank=1)
    assert assemble(data[:2]) == ("images", "targets")                    # a plain list: processor.preprocess, as before
    assert proc.calls == [(data[:2], torch.device("cuda", 0))]

    ds = A.AugmentedDataset(data, AUGS)
    assert ds.augmentations is AUGS and len(ds) == 3 and ds[1] == "e1"
    seen = []

    class _Augmenter:
        def __init__(self, augs, task, device):
            seen.append((augs, task, device))

        def __call__(self, entries, generator):
            return entries, float(torch.rand(1, generator=generator))

    monkeypatch.setattr(A, "DeviceAugmenter", _Augmenter)
    assemble = trainer.batch_assembler(ds, "bisenetformer", proc, torch.device("cuda", 0), seed=5, rank=1)
    assert seen == [(AUGS, "semseg", torch.device("cuda", 0))] and len(proc.calls) == 1
    first = assemble(data[:1])
    assert first[0] == data[:1] and first[1] == float(torch.rand(1, generator=_gen(rank_seed(5, 1))))   # the rank's seed drives the draws
    assert assemble(data[:1])[1] != first[1]                              # one generator for the whole run: the stream advances
    with pytest.raises(NotImplementedError, match="square"):
        A.AugmentedDataset(data, A.DatasetAugmentations(square=1.0))


def test_gpu_cases_keep_the_near_boundary_share_under_one_percent():
    """The cases tests/test_gpu_augment.py runs: the fp64 restatement alone puts fewer than 1 % of each case's bytes within the derived margin
    of a rounding boundary (where the device byte may differ by 1), so that test's exact statement covers > 99 % of every case."""
    for name, srcs, recs in R.case_batches():
        assert len(srcs) >= 3 and len({s.shape for s in srcs}) >= 3
        for i, (s, r) in enumerate(zip(srcs, recs)):
            share = R.near_boundary_share(s, r)
            print(f"{name}[{i}] margin {R.near_tie_margin(r):.2e} near-boundary share {share:.4%}")
            assert share < 0.01, (name, i, share)
