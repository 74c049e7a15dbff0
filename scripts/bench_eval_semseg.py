"""Eval images/s of the semantic entries (bisenetformer-l-ade, fai-mf-l-ade) on a fixed synthetic set of 64 images at ADE-like mixed original
sizes, for two paths on the same engine forward: the fused FocoosModel.eval path (forward with full_masks=False + fx_semseg_eval_accumulate)
and the existing torch path (forward with full masks -> eval_postprocess -> argmax -> np.bincount on the host).  Not a bench.py leg.

    python scripts/bench_eval_semseg.py [--models bisenetformer-l-ade fai-mf-l-ade] [--n 64] [--input 512]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from focoos_amd.evaluation import accumulate  # noqa: E402
from focoos_amd.model import ModelManager  # noqa: E402
from focoos_amd.ports import SemanticSegmentationDatasetEntry  # noqa: E402
from focoos_amd.synth import synth_image_structured  # noqa: E402

DEV = "cuda:0"
# ADE20K-val-like original sizes (short side 512 class, mixed aspect ratios); the engine input is the --input square
ORIG = [(512, 683), (512, 768), (683, 512), (512, 512), (384, 512), (512, 640), (640, 512), (427, 640)]


def dataset(n, inp, K):
    rs = np.random.RandomState(0)
    out = []
    for i in range(n):
        H, W = ORIG[i % len(ORIG)]
        gt = rs.randint(0, K, size=(H, W)).astype(np.uint8)
        gt[rs.rand(H, W) < 0.1] = 255
        img = torch.from_numpy(synth_image_structured(i, inp, inp)).permute(2, 0, 1).contiguous()
        out.append(SemanticSegmentationDatasetEntry(image=img, height=H, width=W, sem_seg=gt))
    return out


def torch_path(fm, data, K):
    conf = np.zeros((K + 1) ** 2, np.int64)
    for e in data:
        out = fm.model.forward(e.image.permute(1, 2, 0)[None].contiguous().to(DEV))
        pred = fm.processor.eval_postprocess(out, [e])[0]["sem_seg"].argmax(0).cpu().numpy()
        gt = e.sem_seg.astype(np.int64)
        gt[gt == 255] = K
        conf += np.bincount(((K + 1) * pred + gt).reshape(-1), minlength=conf.size)
    return conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["bisenetformer-l-ade", "fai-mf-l-ade"])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--input", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    for name in a.models:
        fm = ModelManager.get(name, device=DEV, seed=0)
        K = fm.model.num_classes
        data = dataset(a.n, a.input, K)
        res = {"model": name, "images": a.n, "input": a.input, "batch_fused": a.batch}
        for path in ("fused", "torch"):
            fn = (lambda: accumulate(fm, data, range(len(data)), "semseg", 255, a.batch).cpu()) if path == "fused" else (lambda: torch_path(fm, data, K))
            fn()   # warm-up (plans, graphs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            conf = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[f"{path}_images_per_s"] = round(a.n / dt, 2)
            res[f"{path}_conf_pixels"] = int(np.asarray(conf).sum())
        print(json.dumps(res), flush=True)
        del fm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
