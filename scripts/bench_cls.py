#!/usr/bin/env python
"""Throughput of the fai-cls classifiers: images/s at bs = 256, 224^2 uint8 input, in the throughput mode (engine.pipeline(): `depth` batches
in flight, one whole-batch hipGraph per lane).  One JSON line per registry entry.  Synthetic weights and images (the numbers do not depend on
the values).  Usage: python scripts/bench_cls.py [--bs 256] [--steps 50] [--warmup 10] [--depth 3] [--names fai-cls-n-coco,...]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focoos_amd.model import FAIClassification  # noqa: E402
from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--names", default="fai-cls-n-coco,fai-cls-s-coco,fai-cls-m-coco")
    a = ap.parse_args()
    dev = "cuda:0"
    x = torch.from_numpy(np.stack([synth_image(i, a.size, a.size) for i in range(a.bs)])).to(dev)
    for name in a.names.split(","):
        m = FAIClassification(ModelRegistry.get_model_info(name)["config"], device=dev)
        pipe = m.engine.pipeline(a.bs, a.size, a.size, a.depth, False)
        host = [{"logits": torch.empty(a.bs, m.num_classes, pin_memory=True)} for _ in range(pipe.depth)]
        t = None
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                pipe.synchronize()
                t = time.perf_counter()
            pipe.submit(x, None, None, host[i % pipe.depth])
        pipe.synchronize()
        dt = time.perf_counter() - t
        print(json.dumps({"model": name, "bs": a.bs, "size": a.size, "depth": pipe.depth, "steps": a.steps,
                          "img_per_s": round(a.bs * a.steps / dt, 1), "ms_per_batch": round(1e3 * dt / a.steps, 3)}), flush=True)
        del pipe, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
