"""fp32 PyTorch-CPU restatement of the fai-cls classifiers (focoos/models/fai_cls/modelling.py:16-76, 201-261 on the STDC backbone,
focoos/nn/backbone/stdc.py:35-48 ConvX, :108-166 CatBottleneck, :192-212 size presets, :302-320 layers / forward) - the checker the GPU tests
compare against for shapes and batch sizes the golden fixtures do not hold.  It is pinned to the fixtures (tests/test_cls_cpu.py) and to the
live reference (``reference``-marked test there).  Inputs: NHWC images on the 0..255 scale (uint8 or float32), like the engine's."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from focoos_amd.engine_stdc import resolve_stdc_size

BN_EPS = 1e-5


def _convx(sd, p: str, x: torch.Tensor, stride: int = 1) -> torch.Tensor:
    w = sd[f"{p}.conv.weight"].float()
    y = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
    y = F.batch_norm(y, sd[f"{p}.bn.running_mean"].float(), sd[f"{p}.bn.running_var"].float(), sd[f"{p}.bn.weight"].float(),
                     sd[f"{p}.bn.bias"].float(), False, 0.0, BN_EPS)
    return F.relu(y)


def _cat_block(sd, p: str, x: torch.Tensor, stride: int) -> torch.Tensor:
    out1 = _convx(sd, f"{p}.conv_list.0", x)
    if stride == 2:
        c = out1.shape[1]
        a = F.conv2d(out1, sd[f"{p}.avd_layer.0.weight"].float(), None, 2, 1, 1, c)
        a = F.batch_norm(a, sd[f"{p}.avd_layer.1.running_mean"].float(), sd[f"{p}.avd_layer.1.running_var"].float(),
                         sd[f"{p}.avd_layer.1.weight"].float(), sd[f"{p}.avd_layer.1.bias"].float(), False, 0.0, BN_EPS)
        o = _convx(sd, f"{p}.conv_list.1", a)
        skip = F.avg_pool2d(out1, 3, 2, 1)
    else:
        o = _convx(sd, f"{p}.conv_list.1", out1)
        skip = out1
    o2 = _convx(sd, f"{p}.conv_list.2", o)
    o3 = _convx(sd, f"{p}.conv_list.3", o2)
    return torch.cat([skip, o, o2, o3], 1)


def stdc_forward(sd, bb_cfg: Dict, x: torch.Tensor, prefix: str = "backbone", last_stage: int = 5) -> Dict[int, torch.Tensor]:
    """x: normalised NCHW fp32 -> {2: res2, ..., last_stage} (NCHW fp32)."""
    layers, _ = resolve_stdc_size(bb_cfg)
    x = _convx(sd, f"{prefix}.features.0", x, 2)
    x = _convx(sd, f"{prefix}.features.1", x, 2)
    feats = {2: x}
    idx = 2
    for i, n in enumerate(layers):
        if i + 3 > last_stage:
            break
        for j in range(n):
            x = _cat_block(sd, f"{prefix}.features.{idx}", x, 2 if j == 0 else 1)
            idx += 1
        feats[i + 3] = x
    return feats


def normalise(images_nhwc: torch.Tensor, cfg: Dict) -> torch.Tensor:
    x = images_nhwc.to(torch.float32).permute(0, 3, 1, 2)
    mean = torch.tensor(cfg["pixel_mean"], dtype=torch.float32).view(1, -1, 1, 1)
    std = torch.tensor(cfg["pixel_std"], dtype=torch.float32).view(1, -1, 1, 1)
    return (x - mean) / std


def cls_forward(sd, cfg: Dict, images_nhwc: torch.Tensor) -> Tuple[torch.Tensor, Dict[int, torch.Tensor]]:
    """FAIClassification.forward (eval) on [B,H,W,3] images (0..255): (logits [B, num_classes], {stage: NCHW feature})."""
    feat = int(str(cfg.get("features", "res5"))[3])
    feats = stdc_forward(sd, cfg["backbone_config"], normalise(images_nhwc, cfg), last_stage=feat)
    v = feats[feat].mean(dim=(2, 3))
    if int(cfg.get("num_layers", 1)) == 2:
        w1, b1 = sd["cls_head.classifier.1.weight"].float(), sd["cls_head.classifier.1.bias"].float()
        v = F.relu(v @ w1.flatten(1).t() + b1)
        w, b = sd["cls_head.classifier.4.weight"].float(), sd["cls_head.classifier.4.bias"].float()
    else:
        w, b = sd["cls_head.classifier.2.weight"].float(), sd["cls_head.classifier.2.bias"].float()
    return v @ w.flatten(1).t() + b, feats
