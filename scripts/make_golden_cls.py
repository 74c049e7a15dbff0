#!/usr/bin/env python
"""Generate tests/golden/cls_{n,s,m}_b3.npz and cls_{n,s}_state_keys.json by running the REAL reference FAIClassification (imported through
oracle/ref_import.py, which this script only uses) on seeded synthetic weights (focoos_amd.synth.synth_state_dict) and
synth_image_structured images at 224^2, plus one fai-cls-n forward at 250 x 330 (the ceil chain of every stride-2 layer down to stride 16).

Each .npz holds the logits, the sigmoid probabilities, strided samples + statistics of res2..res5 (NHWC order, like make_golden.py) and the
reference processor's post-process as (image, cls_id, conf) rows at threshold None and 0.3.  Run where the reference tree exists:
    python scripts/make_golden_cls.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image_structured, synth_state_dict  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = {"n": 11, "s": 12, "m": 13}


def strided_sample(t: torch.Tensor, n: int = 1024) -> np.ndarray:
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n].to(torch.float32).numpy().copy()


def stats(t: torch.Tensor) -> np.ndarray:
    t = t.detach().to(torch.float64)
    return np.array([t.mean().item(), t.abs().mean().item(), t.abs().max().item(), (t * t).mean().sqrt().item()])


def build_reference_cls(cfg: dict):
    """FAIClassification + ClassificationProcessor from a registry config (the recipe of ref_import.build_reference_*)."""
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
    model = FAIClassification(rc).eval()
    proc = ClassificationProcessor(rc, image_size=224).eval()
    return model, proc


def run(model, proc, sd, images):
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    cap = {}
    model.backbone.register_forward_hook(lambda m, i, o: cap.update(o))
    batch = torch.from_numpy(np.stack(images)).permute(0, 3, 1, 2).float()
    x = (batch - model.pixel_mean) / model.pixel_std
    with torch.no_grad():
        out = model(x)
    return out, cap


def main():
    out_keys = {}
    for tag in ("n", "s", "m"):
        name = f"fai-cls-{tag}-coco"
        cfg = ModelRegistry.get_model_info(name)["config"]
        model, proc = build_reference_cls(cfg)
        if tag in ("n", "s"):
            out_keys[tag] = {k: list(v.shape) for k, v in model.state_dict().items()}
        sd = synth_state_dict(cfg, SEEDS[tag], family="fai_cls")
        imgs = [synth_image_structured(300 + 10 * SEEDS[tag] + i, 224, 224) for i in range(3)]
        out, cap = run(model, proc, sd, imgs)
        d = {"logits": out.logits.numpy(), "probs": torch.sigmoid(out.logits).numpy(), "image_index": np.array([300 + 10 * SEEDS[tag] + i for i in range(3)])}
        for k in ("res2", "res3", "res4", "res5"):
            t = cap[k].permute(0, 2, 3, 1).contiguous()
            d[f"{k}_sample"], d[f"{k}_stats"], d[f"{k}_shape"] = strided_sample(t), stats(t), np.array(t.shape)
        for thr_tag, thr in (("none", None), ("0.3", 0.3)):
            dets = proc.postprocess(out, imgs, threshold=thr)
            d[f"post_{thr_tag}"] = np.array([[i, dt.cls_id, dt.conf] for i, r in enumerate(dets) for dt in r.detections],
                                            dtype=np.float64).reshape(-1, 3)
        if tag == "n":
            img = synth_image_structured(777, 250, 330)
            o2, c2 = run(model, proc, sd, [img])
            d["odd_logits"] = o2.logits.numpy()   # image: synth_image_structured(777, 250, 330)
            for k in ("res2", "res3", "res4"):
                t = c2[k].permute(0, 2, 3, 1).contiguous()
                d[f"odd_{k}_sample"], d[f"odd_{k}_shape"] = strided_sample(t), np.array(t.shape)
        d["seed"] = np.array(SEEDS[tag])
        np.savez_compressed(os.path.join(GOLDEN, f"cls_{tag}_b3.npz"), **d)
        print(name, "logits", d["logits"].shape, "probs in (0.05, 0.95):", float(((d["probs"] > 0.05) & (d["probs"] < 0.95)).mean()),
              "dets@0.5", len(d["post_none"]), "dets@0.3", len(d["post_0.3"]))
    for tag, keys in out_keys.items():
        with open(os.path.join(GOLDEN, f"cls_{tag}_state_keys.json"), "w") as f:
            json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
