#!/usr/bin/env python
"""Generate tests/golden/mask_class_loss.npz from the REAL reference (imported through oracle/ref_import.py): the class loss of the mask
families' SetCriterion.loss_labels (focoos/models/fai_mf/loss.py:413-462 == bisenetformer/loss.py) for loss_class_type focal_loss,
bce_loss (with and without the dropped last logit column) and bce_focal_loss, driven with fixed ``indices`` and ``num_masks``.  Per case
and variant the file holds the inputs, the reference's own fp32 loss, the same code run in float64 and d loss / d logits from autograd in
float64.  Only recorded values are stored, so the GPU tests need no reference tree.  Run where the reference tree exists:
    python scripts/make_golden_mask_class_loss.py

float64: loss_labels casts its logits with ``.float()``; for the float64 run that method (and the default dtype, for ``target * 1.0``)
means float64 while the reference's code runs - nothing of its arithmetic is restated here.

bce_focal_loss calls ``torchvision.ops.sigmoid_focal_loss``; torchvision is not installed where this runs, so ``sigmoid_focal_loss``
below is written from the published formula (Lin et al., Focal Loss for Dense Object Detection, eq. 5 with the alpha-balanced form:
FL = -alpha_t (1 - p_t)^gamma log(p_t)).  What the fixture mirrors is the reference's CALL SITE (loss.py:446-457: which logits and
targets it passes, alpha, gamma, reduction="none", then ``loss.mean(1).sum() * Q / num_masks``), not torchvision's source."""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "mask_class_loss.npz")

# (B, Q, K, targets per image)
CASES = [
    (1, 1, 1, [1]),             # minimum; one row in a four-row block
    (2, 7, 80, [3, 7]),         # 14 rows: tail block; K + 1 = 81 = one wave of 64 lanes + a remainder; an image with every query matched
    (3, 5, 149, [2, 0, 4]),     # K + 1 = 150: three passes of a wave, ragged last; the middle image has no target
    (2, 100, 19, [17, 40]),     # K + 1 < 64; the tests give this one a padded leading dimension
]
# (name, loss_class_type, cls_sigmoid, logit columns minus K, focal_alpha, focal_gamma)
VARIANTS = [
    ("focal", "focal_loss", False, 1, 0.75, 2.0),
    ("bce_drop", "bce_loss", True, 1, 0.75, 2.0),
    ("bce", "bce_loss", False, 0, 0.75, 2.0),
    ("bce_focal", "bce_focal_loss", False, 0, 0.75, 2.0),
]
EXTRA = [   # a non-integer gamma and another alpha, on the two middle cases
    ("focal_a25g15", "focal_loss", False, 1, 0.25, 1.5),
    ("bce_focal_a25g15", "bce_focal_loss", False, 0, 0.25, 1.5),
]


MODES = {"focal_loss": 1, "bce_loss": 2, "bce_focal_loss": 3}   # FX_CLASS_LOSS_* (include/focoos_amd.h); stored with every variant


def variants_of(case_index: int):
    return VARIANTS + (EXTRA if case_index in (1, 2) else [])


def sigmoid_focal_loss(inputs, targets, alpha: float = 0.25, gamma: float = 2, reduction: str = "none"):
    """FL(p_t) = -alpha_t (1 - p_t)^gamma log(p_t), p_t = p for target 1 and 1 - p for target 0, alpha_t likewise (alpha < 0: none)."""
    p = torch.sigmoid(inputs)
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    assert reduction == "none"
    return loss


def make_inputs(ci: int):
    """Seeded inputs of case ci: logits [B,Q,K+1] ~ N(0, 3^2) with +-30 planted (on a matched target's own column, on another column of
    a matched row and in no-object rows), labels and fixed matches (pred_idx distinct per image, tgt_idx a permutation)."""
    B, Q, K, sizes = CASES[ci]
    g = torch.Generator().manual_seed(10 + ci)
    logits = torch.randn(B, Q, K + 1, generator=g) * 3
    labels = [torch.randint(0, K, (t,), generator=g) for t in sizes]
    pred = [torch.randperm(Q, generator=g)[:t] for t in sizes]
    tgt = [torch.randperm(t, generator=g) for t in sizes]
    flat = logits.view(-1)
    n = flat.numel()
    for k, v in enumerate([30.0, -30.0, 30.0, -30.0, 30.0, -30.0]):
        if n > 1:
            flat[(k * 37 + 5) % n] = v
    for b in range(B):   # the matched class itself at +-30: p_t -> 1 and p_t -> 0
        if sizes[b] >= 1:
            logits[b, pred[b][0], labels[b][tgt[b][0]]] = 30.0 if ci != 0 else -30.0
        if sizes[b] >= 2:
            logits[b, pred[b][1], labels[b][tgt[b][1]]] = -30.0
    return logits, labels, pred, tgt, float(max(sum(sizes), 1))


@contextlib.contextmanager
def _float_means(dtype):
    prev, orig = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(dtype)
    torch.Tensor.float = lambda self, *a, **k: self.to(dtype)
    try:
        yield
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(prev)


def run_reference(logits, labels, pred, tgt, num_masks, K, loss_class_type, cls_sigmoid, alpha, gamma, dtype=torch.float32):
    """(loss, dlogits) of the reference's SetCriterion.loss_labels on ``logits`` (already cut to the variant's width) in ``dtype``."""
    from oracle import ref_import

    ref_import.install()
    import focoos.models.fai_mf.loss as L
    from focoos.models.fai_mf.ports import MaskFormerTargets

    L.torchvision.ops.sigmoid_focal_loss = sigmoid_focal_loss
    B, Q = logits.shape[:2]
    crit = L.SetCriterion(num_classes=K, matcher=None, weight_dict={"loss_ce": 1.0}, losses=["labels"], loss_class_type=loss_class_type,
                          focal_alpha=alpha, focal_gamma=gamma, cls_sigmoid=cls_sigmoid)
    targets = [MaskFormerTargets(labels=l.long(), masks=torch.zeros(len(l), 1, 1)) for l in labels]
    indices = [(p.long(), t.long()) for p, t in zip(pred, tgt)]
    x = logits.to(dtype).clone().requires_grad_(True)
    with _float_means(dtype):
        loss = crit.loss_labels({"pred_logits": x}, targets, indices, num_masks)["loss_ce"]
        loss.backward()
    assert x.grad.dtype == dtype and loss.dtype == dtype
    return loss.detach(), x.grad


def main():
    g = {"cases": np.array([c[:3] for c in CASES], np.int64)}
    for ci, (B, Q, K, sizes) in enumerate(CASES):
        logits, labels, pred, tgt, num_masks = make_inputs(ci)
        g[f"c{ci}_logits"] = logits.numpy()
        g[f"c{ci}_sizes"] = np.array(sizes, np.int64)
        g[f"c{ci}_labels"] = torch.cat(labels).numpy().astype(np.int64)
        g[f"c{ci}_pred_idx"] = torch.cat(pred).numpy().astype(np.int64)
        g[f"c{ci}_tgt_idx"] = torch.cat(tgt).numpy().astype(np.int64)
        g[f"c{ci}_num_masks"] = np.float64(num_masks)
        g[f"c{ci}_variants"] = np.array([v[0] for v in variants_of(ci)])
        for name, lct, sig, extra_cols, alpha, gamma in variants_of(ci):
            x = logits[..., : K + extra_cols]
            l32, _ = run_reference(x, labels, pred, tgt, num_masks, K, lct, sig, alpha, gamma, torch.float32)
            l64, d64 = run_reference(x, labels, pred, tgt, num_masks, K, lct, sig, alpha, gamma, torch.float64)
            assert torch.isfinite(l64) and torch.isfinite(d64).all() and torch.isfinite(l32)
            g[f"c{ci}_{name}_params"] = np.array([MODES[lct], float(sig), K + extra_cols, alpha, gamma], np.float64)
            g[f"c{ci}_{name}_loss32"] = np.float32(l32.item())
            g[f"c{ci}_{name}_loss64"] = np.float64(l64.item())
            g[f"c{ci}_{name}_dlogits64"] = d64.numpy()
            print(f"case {ci} B{B} Q{Q} K{K} {name:18s} loss32 {l32.item():.9g} loss64 {l64.item():.17g} |fp32 - fp64| / fp64 {abs(l32.item() - l64.item()) / abs(l64.item()):.2e}")
    np.savez_compressed(GOLDEN, **g)
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
