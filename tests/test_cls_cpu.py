"""fai-cls classifiers, host side (no GPU): registry entries, STDC size resolution, state layout, the post-process, config refusals and the fp32
CPU reference (tests/cls_ref.py) against the golden fixtures of scripts/make_golden_cls.py.  ``reference``-marked tests compare with the live
reference tree (build container only)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd.engine_stdc import StdcEngineMixin, resolve_stdc_size
from focoos_amd.registry import ModelRegistry
from focoos_amd.state_spec import cls_state_spec
from focoos_amd.synth import synth_image_structured, synth_state_dict
from oracle import ref_import
from tests import cls_ref

NAMES = ("fai-cls-n-coco", "fai-cls-s-coco", "fai-cls-m-coco")
needs_ref = [pytest.mark.reference, pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")]


def _cfg(name):
    return ModelRegistry.get_model_info(name)["config"]


def _golden(golden_dir, tag):
    return np.load(os.path.join(golden_dir, f"cls_{tag}_b3.npz"))


def _ref_cls(cfg):
    ref_import.install()
    import focoos.models.fai_cls as fam
    from focoos.model_manager import ConfigManager
    from focoos.models.fai_cls.modelling import FAIClassification
    from focoos.models.fai_cls.processor import ClassificationProcessor
    from focoos.ports import ModelFamily

    for attr in dir(fam):
        if attr.startswith("_register"):
            getattr(fam, attr)()
    rc = ConfigManager.from_dict(ModelFamily.IMAGE_CLASSIFIER, dict(cfg))
    return FAIClassification(rc).eval(), ClassificationProcessor(rc, image_size=224).eval()


# ---------------------------------------------------------------- registry
def test_registry_entries():
    for name, feat, size in zip(NAMES, ("res4", "res4", "res5"), ("nano", "small", "small")):
        info = ModelRegistry.get_model_info(name)
        assert info["model_family"] == "fai_cls" and info["task"] == "classification" and info["im_size"] == 224
        cfg = info["config"]
        assert cfg["features"] == feat and cfg["backbone_config"]["size"] == size and cfg["num_layers"] == 1 and cfg["num_classes"] == 80
        assert "layers" not in cfg["backbone_config"] and cfg["dense_prediction"] is False


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_registry_config_equals_reference_json(name):
    ref = json.load(open(os.path.join(ref_import.REFERENCE_ROOT, "focoos", "model_registry", f"{name}.json")))
    info = ModelRegistry.get_model_info(name)
    assert info["config"] == ref["config"]
    for k in ("model_family", "task", "im_size"):
        assert info[k] == ref[k], k


# ---------------------------------------------------------------- STDC size resolution
def test_size_resolution():
    assert resolve_stdc_size({"size": "nano"}) == ((2, 2, 2), 32)
    assert resolve_stdc_size({"size": "small"}) == ((2, 2, 2), 64)
    assert resolve_stdc_size({"size": "large"}) == ((4, 5, 3), 64)
    # size wins over explicit layers / base (the reference warns and uses the preset)
    assert resolve_stdc_size({"size": "nano", "layers": [4, 5, 3], "base": 64}) == ((2, 2, 2), 32)
    assert resolve_stdc_size({}) == ((4, 5, 3), 64)
    with pytest.raises(_lib.FocoosAmdError, match="Invalid size"):
        resolve_stdc_size({"size": "huge"})


def test_existing_stdc_families_resolve_as_before():
    """DETR-m, BF-* and MF-m-ade keep the geometry their configs state; base 32 stays refused outside the classifier."""
    names = ["fai-detr-m-coco", "bisenetformer-l-ade", "bisenetformer-m-ade", "bisenetformer-s-ade", "fai-mf-m-ade"]
    for name in names:
        bb = _cfg(name)["backbone_config"]
        o = object.__new__(StdcEngineMixin)
        o._init_stdc(bb)
        assert o.layers == tuple(bb["layers"]) and o.base == bb["base"], name
        assert resolve_stdc_size(bb) == (o.layers, o.base), name
    o = object.__new__(StdcEngineMixin)
    with pytest.raises(_lib.FocoosAmdError, match="base must be 64"):
        o._init_stdc(dict(_cfg("bisenetformer-s-ade")["backbone_config"], base=32))
    o._init_stdc(_cfg("fai-cls-n-coco")["backbone_config"], resolve_size=True)
    assert (o.layers, o.base) == ((2, 2, 2), 32)


# ---------------------------------------------------------------- state layout
@pytest.mark.parametrize("tag", ["n", "s"])
def test_state_spec_matches_reference_keys(golden_dir, tag):
    ref = json.load(open(os.path.join(golden_dir, f"cls_{tag}_state_keys.json")))
    spec = cls_state_spec(_cfg(f"fai-cls-{tag}-coco"))
    assert list(spec) == list(ref)
    assert {k: list(v[0]) for k, v in spec.items()} == ref
    assert len(spec) == 177


def test_state_spec_m_head_reads_res5():
    spec = cls_state_spec(_cfg("fai-cls-m-coco"))
    assert spec["cls_head.classifier.2.weight"][0] == (80, 1024, 1, 1) and len(spec) == 177
    two = dict(_cfg("fai-cls-s-coco"), num_layers=2)
    spec2 = cls_state_spec(two)
    assert spec2["cls_head.classifier.1.weight"][0] == (512, 512, 1, 1) and spec2["cls_head.classifier.4.weight"][0] == (80, 512, 1, 1)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_synthetic_state_loads_strict_into_reference(name):
    cfg = _cfg(name)
    model, _ = _ref_cls(cfg)
    res = model.load_state_dict(synth_state_dict(cfg, 3, family="fai_cls"), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


# ---------------------------------------------------------------- post-process
def _fixed_logits():
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(4, 80, generator=g) * 3
    lg[3] = -20.0   # an image without any class above any threshold: the empty result
    lg[0, 7] = 0.0  # sigmoid exactly 0.5: not kept at 0.5 (strict >)
    return lg


def _as_rows(dets):
    return [[(d.cls_id, d.conf, d.label, d.bbox, d.mask) for d in r.detections] for r in dets]


def test_postprocess_semantics():
    from focoos_amd.ports import ClassificationModelOutput
    from focoos_amd.processor import ClassificationProcessor

    proc = ClassificationProcessor(_cfg("fai-cls-n-coco"), image_size=224)
    lg = _fixed_logits()
    names = [f"c{i}" for i in range(80)]
    out = ClassificationModelOutput(logits=lg, loss=None)
    p = torch.sigmoid(lg)
    for thr in (None, 0, 0.3, 0.999):
        t = thr or 0.5
        got = proc.postprocess(out, [None] * 4, class_names=names, threshold=thr)
        for i, r in enumerate(got):
            ids = [d.cls_id for d in r.detections]
            assert ids == sorted(ids) == (p[i] > t).nonzero().flatten().tolist()
            assert all(d.bbox is None and d.mask is None and d.label == f"c{d.cls_id}" and d.conf == p[i, d.cls_id].item() for d in r.detections)
        assert got[3].detections == []
    assert 7 not in [d.cls_id for d in proc.postprocess(out, [None] * 4)[0].detections]
    ev = proc.eval_postprocess(out, [])
    assert len(ev) == 4 and torch.equal(ev[0]["logits"], p[0])


@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_postprocess_equals_reference():
    from focoos_amd.ports import ClassificationModelOutput
    from focoos_amd.processor import ClassificationProcessor

    cfg = _cfg("fai-cls-n-coco")
    _, rproc = _ref_cls(cfg)
    from focoos.models.fai_cls.ports import ClassificationModelOutput as RefOut

    proc = ClassificationProcessor(cfg, image_size=224)
    lg = _fixed_logits()
    names = [f"c{i}" for i in range(80)]
    for thr in (None, 0, 0.3, 0.999):
        mine = proc.postprocess(ClassificationModelOutput(logits=lg, loss=None), [None] * 4, class_names=names, threshold=thr)
        ref = rproc.postprocess(RefOut(logits=lg, loss=None), [None] * 4, class_names=names, threshold=thr)
        assert _as_rows(mine) == _as_rows(ref), thr
    ev, rev = proc.eval_postprocess(ClassificationModelOutput(logits=lg, loss=None), []), rproc.eval_postprocess(RefOut(logits=lg, loss=None), [])
    assert all(torch.equal(a["logits"], b["logits"]) for a, b in zip(ev, rev))


@pytest.mark.parametrize("tag", ["n", "s", "m"])
def test_postprocess_equals_golden_lists(golden_dir, tag):
    from focoos_amd.processor import ClassificationProcessor

    g = _golden(golden_dir, tag)
    for thr_tag, thr in (("none", None), ("0.3", 0.3)):
        dets = ClassificationProcessor.pack_detections(torch.from_numpy(g["logits"]), (), thr)
        rows = np.array([[i, d.cls_id, d.conf] for i, r in enumerate(dets) for d in r.detections], dtype=np.float64).reshape(-1, 3)
        np.testing.assert_array_equal(rows, g[f"post_{thr_tag}"])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("patch,match", [
    ({"num_layers": 3}, "num_layers"),
    ({"dense_prediction": True}, "dense_prediction"),
    ({"backbone_config": {"model_type": "resnet", "depth": 50}}, "model_type"),
    ({"backbone_config": {"model_type": "stdc", "size": "small", "block_type": "add"}}, "block_type"),
    ({"features": "res6"}, "features"),
    ({"backbone_config": {"model_type": "stdc", "size": "small", "out_features": ["res2", "res3"]}}, "features"),
])
def test_config_refusals(patch, match):
    from focoos_amd.engine_cls import ClsEngine

    cfg = dict(_cfg("fai-cls-s-coco"), **patch)
    with pytest.raises(_lib.FocoosAmdError, match=match):
        ClsEngine(cfg, {}, "cuda:0")


def test_train_refused_before_anything_spawns(monkeypatch):
    from focoos_amd import model as M

    called = []
    monkeypatch.setattr("focoos_amd.trainer.train", lambda *a, **k: called.append(1))
    fm = object.__new__(M.FocoosModel)
    fm.model = types.SimpleNamespace(family="fai_cls")
    with pytest.raises(NotImplementedError, match="classification training is not built"):
        fm.train(None, [])
    assert not called


def test_managers_know_the_family():
    from focoos_amd.model import FAIClassification, ModelManager, ProcessorManager
    from focoos_amd.processor import ClassificationProcessor

    assert ModelManager._MODEL_MAPPING["fai_cls"]() is FAIClassification
    assert isinstance(ProcessorManager.get_processor("fai_cls", _cfg("fai-cls-m-coco"), 224), ClassificationProcessor)


# ---------------------------------------------------------------- CPU reference vs fixtures / live reference
@pytest.mark.parametrize("tag", ["n", "s", "m"])
def test_cpu_reference_matches_golden(golden_dir, tag):
    g = _golden(golden_dir, tag)
    cfg = _cfg(f"fai-cls-{tag}-coco")
    sd = synth_state_dict(cfg, int(g["seed"]), family="fai_cls")
    imgs = torch.from_numpy(np.stack([synth_image_structured(int(i), 224, 224) for i in g["image_index"]]))
    with torch.no_grad():
        logits, feats = cls_ref.cls_forward(sd, cfg, imgs)
    np.testing.assert_allclose(logits.numpy(), g["logits"], rtol=1e-4, atol=1e-4)
    last = int(cfg["features"][3])
    for k in range(2, last + 1):
        t = feats[k].permute(0, 2, 3, 1).contiguous()
        assert list(t.shape) == g[f"res{k}_shape"].tolist()
        f = t.reshape(-1)
        step = max(1, f.numel() // 1024)
        np.testing.assert_allclose(f[::step][:1024].numpy(), g[f"res{k}_sample"], rtol=1e-4, atol=1e-4)
    if tag == "n":
        img = torch.from_numpy(synth_image_structured(777, 250, 330)[None])
        with torch.no_grad():
            lo, fo = cls_ref.cls_forward(sd, cfg, img)
        np.testing.assert_allclose(lo.numpy(), g["odd_logits"], rtol=1e-4, atol=1e-4)
        assert [list(fo[k].permute(0, 2, 3, 1).shape) for k in (2, 3, 4)] == [g[f"odd_res{k}_shape"].tolist() for k in (2, 3, 4)]


@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("name,hw", [("fai-cls-n-coco", (96, 130)), ("fai-cls-m-coco", (101, 64))])
def test_cpu_reference_matches_live_reference(name, hw):
    cfg = _cfg(name)
    model, _ = _ref_cls(cfg)
    sd = synth_state_dict(cfg, 21, family="fai_cls")
    model.load_state_dict(sd, strict=True)
    imgs = np.stack([synth_image_structured(900 + i, *hw) for i in range(2)])
    x = torch.from_numpy(imgs).permute(0, 3, 1, 2).float()
    with torch.no_grad():
        ref = model((x - model.pixel_mean) / model.pixel_std).logits
        mine, _ = cls_ref.cls_forward(sd, cfg, torch.from_numpy(imgs))
    torch.testing.assert_close(mine, ref, rtol=1e-4, atol=1e-4)


@pytest.mark.reference
@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_integration_registers_the_classifier():
    """integration.register(): the reference's ModelManager builds the engine-backed FAIClassification (the engine itself is built on the first
    forward, on the GPU); parameters and state_dict stay the reference module's."""
    ref_import.install()
    from focoos.model_manager import ModelManager as RefMM
    from focoos.models.fai_cls.modelling import FAIClassification as RefCls
    from focoos.ports import ModelFamily

    from focoos_amd import integration

    integration.register()
    adapter = integration.make_cls_engine_class()
    assert RefMM._models_family_map[ModelFamily.IMAGE_CLASSIFIER.value]() is adapter
    assert issubclass(adapter, RefCls)
    model, _ = _ref_cls(_cfg("fai-cls-n-coco"))
    m2 = adapter(model.config)
    assert list(m2.state_dict()) == list(model.state_dict())
