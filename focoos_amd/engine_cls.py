"""Image-classifier inference engine (fai-cls-*: STDC backbone + pooled 1x1-conv head): packs a reference-layout state_dict for the gfx950
kernels and runs FAIClassification.forward (eval) as one hipGraph of C-ABI calls; the logits come back in one D2H copy and the sigmoid /
threshold of ClassificationProcessor.postprocess run on the host, in fp32, as in the reference.

Reference path being replaced (file:line in FocoosAI/focoos):
  FAIClassification.forward               focoos/models/fai_cls/modelling.py:234-261
  ClassificationHead (num_layers 1 / 2)   modelling.py:16-76
  STDC.forward / CatBottleneck            focoos/nn/backbone/stdc.py:313-320, 108-166 (size presets :192-212)
  normalisation of preprocess             focoos/models/fai_cls/processor.py:98-99 (fused into the stem kernel)

Restructured relative to the reference (same arithmetic): the backbone stops at the ``features`` stage - the reference computes res5 for the
res4 models (``out_features`` lists it) and drops it; AdaptiveAvgPool2d(1) is fx_global_mean_nhwc_bf16 (f32 [B, C]); the head's 1x1 convs on
the pooled vector are fx_pooled_linear_f32 (f32 weights); Dropout is the identity in eval.  STDC-nano's 16-channel layers (fai-cls-n) run on
csrc/stdc_nano.hip, everything else on the kernels the other STDC families use."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from .engine import NT, PackedConv, _EngineBase, _PlanBase
from .engine_stdc import StdcEngineMixin, StdcPlanMixin

BACKBONE = "backbone"
FX_ACT_NONE, FX_ACT_RELU = 0, 1


class ClsEngine(StdcEngineMixin, _EngineBase):
    split_batch = False

    def __init__(self, config: Dict, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0"):
        bb = config.get("backbone_config") or {}
        nl = int(config.get("num_layers", 1))
        if nl not in (1, 2):
            raise _lib.FocoosAmdError(f"num_layers must be 1 or 2 (ClassificationHead, fai_cls/modelling.py:41-63), got {nl}")
        if bool(config.get("dense_prediction", False)):
            raise _lib.FocoosAmdError("dense_prediction: true is not built (the engine covers the pooled head)")
        if bb.get("model_type") != "stdc":
            raise _lib.FocoosAmdError(f"backbone_config.model_type {bb.get('model_type')!r}: the classification engine covers STDC backbones")
        if bb.get("block_type", "cat") != "cat":
            raise _lib.FocoosAmdError(f"backbone_config.block_type {bb.get('block_type')!r}: the engine covers CatBottleneck ('cat') blocks")
        feat = str(config.get("features", "res5"))
        outs = list(bb.get("out_features", ["res2", "res3", "res4", "res5"]))
        if feat not in outs or feat not in ("res2", "res3", "res4", "res5"):
            raise _lib.FocoosAmdError(f"features {feat!r} is not in backbone_config.out_features {outs}")
        super().__init__(config, device)
        self._init_stdc(bb, resolve_size=True)
        self.last_stage = int(feat[3])
        self.nc = int(config["num_classes"])
        self.nl = nl
        self.hidden = int(config.get("hidden_dim", 512))
        self.threshold = 0.5   # ClassificationProcessor.postprocess: `threshold or 0.5` (the config's threshold is never read)
        self.load_state_dict(state_dict)

    def feature_channels(self) -> int:
        return {2: 1, 3: 4, 4: 8, 5: 16}[self.last_stage] * self.base   # STDC out_feature_channels (stdc.py:240-245)

    def _pack_all(self, sd: Dict[str, torch.Tensor]) -> None:
        """The packing sequence, for host tensors (load_state_dict) and device tensors (publish_state_dict) alike."""
        P: Dict[str, PackedConv] = {}
        self.vec: Dict[str, torch.Tensor] = {}
        self._pack_stdc(sd, P, prefix=BACKBONE, last_stage=self.last_stage)
        H = "cls_head.classifier"
        layers = [(f"{H}.1", FX_ACT_RELU), (f"{H}.4", FX_ACT_NONE)] if self.nl == 2 else [(f"{H}.2", FX_ACT_NONE)]
        self.head = []
        for key, act in layers:
            w = sd[f"{key}.weight"].float()
            self.head.append((self._dev(w.reshape(w.shape[0], -1).contiguous()), self._dev(sd[f"{key}.bias"].float()), act))
        if self.head[0][0].shape[1] != self.feature_channels():
            raise _lib.FocoosAmdError(f"head input {self.head[0][0].shape[1]} != {self.feature_channels()} channels of {self.cfg.get('features')}")
        self.P = P

    def plan(self, B: int, H: int, W: int, f32_input: bool = False) -> "_ClsPlan":
        return self._plan(B, H, W, f32_input, 1)

    def pipeline(self, B: int, H: int, W: int, depth: Optional[int] = None, f32_input: bool = False):
        """Throughput mode: `depth` batches in flight, each on its own whole-batch plan and stream (engine._Pipeline)."""
        return self._pipeline(B, H, W, depth, f32_input, 1)

    def forward(self, images: torch.Tensor, use_graph: bool = True) -> "_ClsPlan":
        """images: uint8 [B,H,W,3] or float32 [B,H,W,3] (0..255 scale) on the engine device, at the size the model runs at (the
        processor resizes to im_size).  Returns the plan; ``plan.logits`` (f32 [B, num_classes]) holds the result until the next call."""
        return self._forward(images, None, None, None, use_graph)


class _ClsPlan(StdcPlanMixin, _PlanBase):
    """fai-cls launch sequence for one (batch, height, width, input dtype)."""

    size_multiple = 1   # any size >= 32: ceil(H/2) at every stride-2 layer, like the reference's convolutions

    def _build(self):
        e, B = self.eng, self.B
        feats = self.build_stdc(prefix=BACKBONE, last_stage=e.last_stage)
        x: NT = feats[e.last_stage]
        self.pooled = torch.empty(B, x.C, dtype=torch.float32, device=self.dev)
        self._op(self.lib.fx_global_mean_nhwc_bf16, x.ptr, x.ld, self.pooled.data_ptr(), x.C, B, x.H * x.W, x.C)
        v = self.pooled
        for i, (w, b, act) in enumerate(e.head):
            N, Cc = w.shape
            out = self._io("logits", (B, N), torch.float32) if i == len(e.head) - 1 else torch.empty(B, N, dtype=torch.float32, device=self.dev)
            self._op(self.lib.fx_pooled_linear_f32, v.data_ptr(), Cc, w.data_ptr(), b.data_ptr(), act, out.data_ptr(), N, B, Cc, N)
            self.keep.append(out)
            v = out
        self.logits = v


ClsEngine.plan_cls = _ClsPlan
