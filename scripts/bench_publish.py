"""Cost of one weight hand-off from a training run to the inference engine, fai-detr-l-coco at bs=16 640 x 640 by default:

  publish   engine.publish_state_dict(device weights) + one forward            (plans kept: csrc/publish.hip)
  reload    weights to the host + engine.load_state_dict + the first forward   (what a validation cost before: the plan is rebuilt)

next to the steady forward and one training step, so that both can be read as a share of a 200-iteration validation period.  The weights
are the trainable graph's own state dict (views of the optimizer's flat buffer), as validation.py publishes them.  Prints one JSON line;
``--out`` also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _entries(n, size, nc):
    from focoos_amd.ports import Boxes, DatasetEntry, Instances
    from focoos_amd.synth import synth_image_structured

    rs = np.random.RandomState(0)
    out = []
    for i in range(n):
        t = rs.randint(1, 6)
        cx, cy = rs.uniform(0.25, 0.75, t) * size, rs.uniform(0.25, 0.75, t) * size
        w, h = rs.uniform(0.08, 0.3, t) * size, rs.uniform(0.08, 0.3, t) * size
        xyxy = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
        img = torch.from_numpy(synth_image_structured(i, size, size)).permute(2, 0, 1).contiguous()
        out.append(DatasetEntry(image=img, height=size, width=size,
                                instances=Instances((size, size), boxes=Boxes(torch.from_numpy(xyxy)), classes=torch.from_numpy(rs.randint(0, nc, t)))))
    return out


def _timed(fn, dev, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fai-detr-l-coco")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--period", type=int, default=200, help="iterations between validations (TrainerArgs.eval_period default)")
    ap.add_argument("--no-train-step", action="store_true", help="skip the training-step measurement (shares are then not reported)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from focoos_amd.model import ModelManager
    from focoos_amd.train_detr import FAIDetrTrainable, TrainStep

    dev = torch.device("cuda", 0)
    fm = ModelManager.get(a.model, seed=1)
    model, eng = fm.model, fm.model.engine
    entries = _entries(a.batch, a.size, model.num_classes)
    fm.processor.train(True)
    images, targets = fm.processor.preprocess(entries, device=dev)
    fm.processor.eval()
    net = FAIDetrTrainable(model.config, norm="FrozenBN").to(dev)
    net.load_state_dict(model.state_dict(), strict=True)
    net.train()
    stepper = TrainStep(net, lr=1e-4, max_iters=1000, scheduler="FIXED")
    step_ms = None
    if not a.no_train_step:
        for _ in range(3):
            stepper.step(images, targets)
        step_ms = statistics.median(_timed(lambda: stepper.step(images, targets), dev, a.reps))
    weights = {k: v.detach() for k, v in net.state_dict().items() if k in model.state_dict()}

    x = images.contiguous()
    for _ in range(3):
        eng.forward(x)
    forward = _timed(lambda: eng.forward(x), dev, a.reps)

    def publish():
        eng.publish_state_dict(weights)
        eng.forward(x)

    def reload():
        eng.load_state_dict({k: v.cpu() for k, v in weights.items()})
        eng.forward(x)

    publish()
    pub = _timed(publish, dev, a.reps)
    rel = _timed(reload, dev, max(2, a.reps // 2))
    res = {"model": a.model, "batch": a.batch, "size": a.size, "forward_ms": round(statistics.median(forward), 3),
           "publish_plus_forward_ms": round(statistics.median(pub), 3), "publish_plus_forward_ms_all": [round(t, 3) for t in pub],
           "reload_plus_forward_ms": round(statistics.median(rel), 3), "reload_plus_forward_ms_all": [round(t, 3) for t in rel],
           "train_step_ms": None if step_ms is None else round(step_ms, 3)}
    if step_ms is not None:
        period_ms = a.period * step_ms
        res.update(period_iters=a.period, publish_share_of_period=round(statistics.median(pub) / period_ms, 6),
                   reload_share_of_period=round(statistics.median(rel) / period_ms, 6))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
