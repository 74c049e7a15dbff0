"""The class-loss variants of the mask criterion, without a GPU: (1) tests/golden/mask_class_loss.npz is what the REAL reference computes
on the fixture's own inputs (where the reference tree is importable; scripts/make_golden_mask_class_loss.py drives it - for
bce_focal_loss through the reference's call site with sigmoid_focal_loss written from the published formula, not torchvision's code);
(2) the host mirror's constructor and shape rules (focoos_amd/mask_criterion.py)."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_import
from tests import mask_class_loss_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_mask_class_loss", os.path.join(ROOT, "scripts", "make_golden_mask_class_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_cases_and_is_finite():
    cases = MC.load_cases()
    assert [(c["B"], c["Q"], c["K"]) for c in cases] == [(1, 1, 1), (2, 7, 80), (3, 5, 149), (2, 100, 19)]
    assert cases[2]["sizes"][1] == 0                                     # an image without targets
    for c in cases:
        assert {"focal", "bce", "bce_drop", "bce_focal"} <= set(c["variants"])
        assert float(c["logits"].abs().max()) == 30.0
        for v in c["variants"].values():
            assert np.isfinite(v["loss64"]) and np.isfinite(v["loss32"]) and bool(torch.isfinite(v["dlogits64"]).all())
            assert v["dlogits64"].shape == (c["B"], c["Q"], v["width"]) and v["dlogits64"].dtype == torch.float64
            if v["name"] == "bce_drop":                                   # the dropped column's gradient is exactly 0
                assert v["width"] == c["K"] + 1 and bool((v["dlogits64"][..., -1] == 0).all())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mask_class_loss.npz")) < 512 * 1024


@pytest.mark.skipif(not ref_import.reference_available(), reason="the reference tree is not on this machine (the fixture was recorded where it is)")
def test_fixture_reproduces_through_the_reference():
    gen = _generator()
    for c in MC.load_cases():
        logits, labels, pred, tgt, num_masks = gen.make_inputs(c["ci"])
        assert torch.equal(logits, c["logits"]) and num_masks == c["num_masks"]
        assert torch.equal(torch.cat(labels), c["labels"]) and torch.equal(torch.cat(pred), c["pred_idx"]) and torch.equal(torch.cat(tgt), c["tgt_idx"])
        for v in c["variants"].values():
            args = (logits[..., : v["width"]], labels, pred, tgt, num_masks, c["K"], MC.MODE_NAMES[v["mode"]], v["cls_sigmoid"], v["alpha"], v["gamma"])
            l32, _ = gen.run_reference(*args, dtype=torch.float32)
            l64, d64 = gen.run_reference(*args, dtype=torch.float64)
            np.testing.assert_allclose(float(l32), v["loss32"], rtol=1e-6)
            np.testing.assert_allclose(float(l64), v["loss64"], rtol=1e-13)
            np.testing.assert_allclose(d64.numpy(), v["dlogits64"].numpy(), rtol=1e-12, atol=1e-300)
    assert torch.get_default_dtype() == torch.float32 and torch.ones(1, dtype=torch.float64).float().dtype == torch.float32   # the generator's patches are undone


def _matcher():
    from focoos_amd.mask_criterion import MaskHungarianMatcher

    return MaskHungarianMatcher(2, 5, 5, num_points=16, cls_sigmoid=True)


WD = {"loss_ce": 2, "loss_mask": 5, "loss_dice": 5}


@pytest.mark.parametrize("lct", ["ce_loss", "focal_loss", "bce_loss", "bce_focal_loss"])
def test_constructor_accepts_the_four_class_losses(lct):
    from focoos_amd.mask_criterion import SetCriterion

    crit = SetCriterion(80, _matcher(), WD, num_points=16, loss_class_type=lct, cls_sigmoid=True)
    assert crit.loss_class_type == lct and crit.cls_sigmoid is True
    assert (crit.focal_alpha, crit.focal_gamma, crit.use_focal) == (0.75, 2.0, False)      # the reference's defaults (loss.py:363-367)


def test_constructor_defaults_stay_ce():
    from focoos_amd.mask_criterion import SetCriterion

    crit = SetCriterion(80, _matcher(), WD, num_points=16)
    assert crit.loss_class_type == "ce_loss" and crit.cls_sigmoid is False


@pytest.mark.parametrize("given,mapped", [("ce_loss", "focal_loss"), ("bce_loss", "bce_focal_loss"), ("focal_loss", "focal_loss"),
                                          ("bce_focal_loss", "bce_focal_loss")])
def test_use_focal_maps_like_the_reference(given, mapped):
    from focoos_amd.mask_criterion import SetCriterion

    with pytest.warns(DeprecationWarning, match="use_focal is deprecated"):
        crit = SetCriterion(80, _matcher(), WD, num_points=16, use_focal=True, loss_class_type=given, focal_alpha=0.25, focal_gamma=1.5)
    assert crit.loss_class_type == mapped and (crit.focal_alpha, crit.focal_gamma) == (0.25, 1.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        SetCriterion(80, _matcher(), WD, num_points=16, loss_class_type=given)               # no warning without use_focal


def test_constructor_still_refuses():
    from focoos_amd.mask_criterion import SetCriterion

    with pytest.raises(NotImplementedError):
        SetCriterion(80, _matcher(), WD, losses=("labels",), num_points=16, loss_class_type="bce_loss")
    with pytest.raises(NotImplementedError):
        SetCriterion(80, _matcher(), WD, losses=("labels", "masks", "boxes"), num_points=16)
    with pytest.raises(NotImplementedError):
        SetCriterion(80, _matcher(), WD, num_points=0, loss_class_type="bce_loss")
    with pytest.raises(AssertionError, match="loss_class_type must be in"):
        SetCriterion(80, _matcher(), WD, num_points=16, loss_class_type="vfl")


def test_columns_follow_the_reference():
    """Which logit columns loss_labels feeds to the loss, and ValueError (with the shapes) where the reference itself fails."""
    from focoos_amd.mask_criterion import class_loss_columns

    K = 80
    assert class_loss_columns("bce_loss", True, K, K + 1) == K            # cls_sigmoid head: last column dropped (loss.py:441-442)
    assert class_loss_columns("bce_loss", True, K, K) == K
    assert class_loss_columns("bce_loss", False, K, K) == K
    assert class_loss_columns("bce_focal_loss", False, K, K) == K
    assert class_loss_columns("focal_loss", False, K, K + 1) == K + 1
    for args in [("bce_loss", False, K, K + 1),       # nothing dropped without cls_sigmoid: [.., 81] against the one-hot [.., 80]
                 ("bce_loss", True, K, K + 2),        # one column dropped, still one too many
                 ("bce_loss", True, K, K - 1),
                 ("bce_focal_loss", True, K, K + 1),  # never dropped (loss.py:450-456): the K + 1 columns of the heads do not fit
                 ("bce_focal_loss", False, K, K + 1),
                 ("focal_loss", False, K, K)]:        # no column for the no-object class
        with pytest.raises(ValueError, match=str(args[3])):
            class_loss_columns(*args)


@pytest.mark.skipif(not ref_import.reference_available(), reason="the reference tree is not on this machine")
def test_reference_fails_on_the_refused_shapes():
    """The ValueErrors above are the reference's own failures, not a guess."""
    gen = _generator()
    c = MC.load_cases()[1]
    logits, labels, pred, tgt, num_masks = gen.make_inputs(1)
    K = c["K"]
    for lct, sig, width in [("bce_loss", False, K + 1), ("bce_focal_loss", True, K + 1), ("bce_focal_loss", False, K + 1), ("focal_loss", False, K)]:
        with pytest.raises((ValueError, RuntimeError, IndexError)):
            gen.run_reference(logits[..., :width], labels, pred, tgt, num_masks, K, lct, sig, 0.75, 2.0)
