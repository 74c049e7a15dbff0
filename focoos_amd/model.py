"""Host-side mirror of the reference's public surface for the RT-DETR and MaskFormer paths:

  ModelManager.get()        focoos/model_manager.py:42-155
  FocoosModel.__call__/infer focoos/models/focoos_model.py:370-416,575-621
  FAIDetr (BaseModelNN)     focoos/models/fai_detr/modelling.py:1273-1358, focoos/models/base_model.py:17-143
  FAIMaskFormer             focoos/models/fai_mf/modelling.py:633-725
  FAIClassification         focoos/models/fai_cls/modelling.py:201-261 (inference only)

Same names, argument meaning and error behaviour; the compute is the HIP engine (engine.py).
``FocoosModel.train`` drives the HIP training step (trainer.py; RT-DETR and BiSeNetFormer families); ``FocoosModel.eval`` evaluates the
semantic-segmentation and classification entries (evaluation.py), ``FocoosModel.eval_detection`` scores RT-DETR with COCO bbox AP
(detection_eval.py); ``.export()`` is out of scope and raises
NotImplementedError (loudly — never a silent fallback)."""
from __future__ import annotations

import os
import warnings
from collections import OrderedDict
from time import perf_counter
from typing import Callable, Dict, List, Optional, Tuple, Type, Union

import numpy as np
import torch

from .engine import DetrEngine
from .engine_bf import BfEngine
from .engine_cls import ClsEngine
from .engine_mf import MfEngine
from .ports import MODELS_DIR, BisenetFormerOutput, ClassificationModelOutput, DETRModelOutput, FocoosDetections, InferLatency, MaskFormerModelOutput, ModelInfo
from .processor import BisenetFormerProcessor, ClassificationProcessor, DETRProcessor, MaskFormerProcessor
from .registry import ModelRegistry
from .state_spec import state_spec
from .synth import synth_state_dict


class IncompatibleKeys:
    def __init__(self, missing_keys, unexpected_keys, incorrect_shapes):
        self.missing_keys, self.unexpected_keys, self.incorrect_shapes = missing_keys, unexpected_keys, incorrect_shapes

    def __repr__(self):
        return f"IncompatibleKeys(missing={self.missing_keys}, unexpected={self.unexpected_keys}, incorrect_shapes={self.incorrect_shapes})"


class _EngineModel:
    """BaseModelNN surface shared by the engine-backed model classes (focoos/models/base_model.py:17-143).
    ``state_dict()`` keeps the reference's key names and fp32 values, so checkpoints round-trip; the packed bf16 copies the
    kernels read are rebuilt on ``load_state_dict``."""

    family = ""

    def _make_engine(self):  # pragma: no cover - overridden
        raise NotImplementedError

    def __init__(self, config: dict, device: Union[str, torch.device] = "cuda:0", seed: int = 0, **engine_kwargs):
        self.config = dict(config)
        self.training = False
        self._spec = state_spec(self.config, self.family)
        self._state = synth_state_dict(self.config, seed, family=self.family)  # "random init" (no network -> no pretrained weights)
        self._device = torch.device(device)
        self._engine_kwargs = engine_kwargs
        self.engine = self._make_engine()
        self.num_classes = int(self.config["num_classes"])

    # ---- BaseModelNN surface
    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32  # pixel_mean.dtype in the reference (modelling.py:1340-1342)

    def __call__(self, *args, **kwargs):
        """nn.Module semantics of the reference's BaseModelNN: ``model(images, targets)`` is ``model.forward(images, targets)``."""
        return self.forward(*args, **kwargs)

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        """nn.Module.train: the engine-backed module itself is the inference graph; the trainable graph (train_detr.FAIDetrTrainable)
        is built from its state_dict by FocoosModel.train / trainer.run_train.  Calling forward in training mode raises."""
        self.training = bool(mode)
        return self

    def cuda(self, device=None):
        return self

    def to(self, *a, **k):
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, v.clone()) for k, v in self._state.items())

    def load_state_dict(self, checkpoint_state_dict: Dict[str, torch.Tensor], strict: bool = True) -> IncompatibleKeys:
        """base_model.py:98-143: strips a DDP ``module.`` prefix, skips shape-mismatched tensors (reported),
        reports missing / unexpected keys; raises only when ``strict`` and something is off."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in checkpoint_state_dict.items()}
        missing, unexpected, bad = [], [], []
        new = OrderedDict(self._state)
        for k, (shape, _) in self._spec.items():
            if k not in sd:
                missing.append(k)
                continue
            v = sd[k].detach().cpu()
            if tuple(v.shape) != tuple(shape):
                bad.append((k, tuple(v.shape), tuple(shape)))
                continue
            new[k] = v.to(self._state[k].dtype).clone()
        unexpected = [k for k in sd if k not in self._spec]
        if strict and (missing or unexpected or bad):
            raise RuntimeError(f"Error(s) in loading state_dict: missing={missing[:5]} unexpected={unexpected[:5]} incorrect_shapes={bad[:5]}")
        self._state = new
        self.engine.load_state_dict(new)
        return IncompatibleKeys(missing, unexpected, bad)

    def publish_state_dict(self, state_dict: Dict[str, torch.Tensor]) -> None:
        """Hand weights that live on the engine's device (a training run's parameters or EMA copy) to the inference engine in place
        (``engine.publish_state_dict``: no host copy, the plans stay alive).  ``state_dict`` must hold every key of the model at its
        shape; other keys are ignored.  ``state_dict()`` returns these values afterwards (fetched from the device on first use)."""
        from ._lib import FocoosAmdError

        cur = self._state_dev if self._state_dev is not None else self._state_host
        new = OrderedDict()
        for k, (shape, _) in self._spec.items():
            if k not in state_dict:
                raise FocoosAmdError(f"publish_state_dict: {k} is missing")
            v = state_dict[k].detach()
            if tuple(v.shape) != tuple(shape):
                raise FocoosAmdError(f"publish_state_dict: {k} has shape {tuple(v.shape)}, the model holds {tuple(shape)}")
            new[k] = v.to(cur[k].dtype)
        self.engine.publish_state_dict(new)
        self._state_dev = OrderedDict((k, v.clone()) for k, v in new.items())

    @property
    def _state(self) -> "OrderedDict[str, torch.Tensor]":
        if self._state_dev is not None:     # the values of the last publish_state_dict: one device-to-host copy, when somebody asks
            self._state_host, self._state_dev = OrderedDict((k, v.cpu()) for k, v in self._state_dev.items()), None
        return self._state_host

    @_state.setter
    def _state(self, value) -> None:
        self._state_host, self._state_dev = value, None

    # ---- forward
    def _to_nhwc(self, images: torch.Tensor) -> torch.Tensor:
        if images.dim() != 4:
            raise ValueError("images must be [B,3,H,W] float (reference contract) or [B,H,W,3] uint8/float32")
        if images.shape[1] == 3 and images.shape[-1] != 3:  # reference contract: NCHW, 0..255, un-normalised
            images = images.permute(0, 2, 3, 1)
        if images.dtype != torch.uint8:
            images = images.to(torch.float32)
        return images.to(self._device).contiguous()



class FAIDetr(_EngineModel):
    """Engine-backed RT-DETR (focoos/models/fai_detr/modelling.py:1273-1358)."""

    family = "fai_detr"

    def _make_engine(self):
        return DetrEngine(self.config, self._state, str(self._device))

    def forward(self, images: torch.Tensor, targets: list = [], forced_topk: Optional[torch.Tensor] = None,
                use_graph: bool = True) -> DETRModelOutput:
        if self.training or (targets is not None and len(targets) > 0):
            raise NotImplementedError("the engine-backed module is the inference graph; the training forward (losses) runs in "
                                      "train_detr.FAIDetrTrainable, reached through FocoosModel.train / trainer.run_train")
        pl = self.engine.forward(self._to_nhwc(images), forced_topk=forced_topk, use_graph=use_graph)
        self.last_plan = pl
        return DETRModelOutput(logits=pl.probs.clone(), boxes=pl.boxes.clone(), loss=None)

    __call__ = forward

    def detect(self, images: torch.Tensor, sizes: Optional[torch.Tensor] = None, threshold: Optional[float] = None):
        """Fused forward + device post-process.  Returns the plan; ``det_scores/det_labels/det_boxes/det_count``
        hold the packed results."""
        pl = self.engine.forward(self._to_nhwc(images), sizes=sizes, threshold=threshold)
        self.last_plan = pl
        return pl


class FAIMaskFormer(_EngineModel):
    """Engine-backed MaskFormer (focoos/models/fai_mf/modelling.py:633-725).  ``forward`` returns the reference's
    ``MaskFormerModelOutput`` (full-resolution fp32 ``masks``, a separate plan that adds the upsample kernel);
    ``detect`` is the fused forward + device post-process that never materialises the [B,Q,H,W] tensor."""

    family = "fai_mf"

    def _make_engine(self):
        return MfEngine(self.config, self._state, str(self._device), **self._engine_kwargs)

    def forward(self, images: torch.Tensor, targets: list = [], forced_attn=None, use_graph: bool = True) -> MaskFormerModelOutput:
        if self.training or (targets is not None and len(targets) > 0):
            raise NotImplementedError("the engine-backed module is the inference graph; the training forward (losses) runs in "
                                      "train_detr.FAIDetrTrainable, reached through FocoosModel.train / trainer.run_train")
        pl = self.engine.forward(self._to_nhwc(images), forced_attn=forced_attn, use_graph=use_graph, full_masks=True)
        self.last_plan = pl
        return MaskFormerModelOutput(masks=pl.masks.clone(), logits=pl.probs.clone(), loss=None)

    __call__ = forward

    def detect(self, images: torch.Tensor, sizes: Optional[torch.Tensor] = None, threshold: Optional[float] = None):
        pl = self.engine.forward(self._to_nhwc(images), threshold=threshold, full_masks=False)
        self.last_plan = pl
        return pl


class BisenetFormer(FAIMaskFormer):
    """Engine-backed BiSeNetFormer (focoos/models/bisenetformer/modelling.py:523-609): same contract as FAIMaskFormer
    (``forward`` -> BisenetFormerOutput with the full-resolution fp32 ``masks``; ``detect`` -> fused forward + device post-process,
    whose plan also holds ``winner`` [B,H,W] uint8, the per-pixel query index of the predict_all_pixels branch)."""

    family = "bisenetformer"

    def _make_engine(self):
        return BfEngine(self.config, self._state, str(self._device), **self._engine_kwargs)

    def forward(self, images: torch.Tensor, targets: list = [], forced_attn=None, use_graph: bool = True) -> BisenetFormerOutput:
        out = super().forward(images, targets, forced_attn, use_graph)
        return BisenetFormerOutput(masks=out.masks, logits=out.logits, loss=None)

    __call__ = forward


class FAIClassification(_EngineModel):
    """Engine-backed image classifier (focoos/models/fai_cls/modelling.py:201-261).  ``forward`` returns the reference's
    ``ClassificationModelOutput`` with the f32 logits [B, num_classes] (one D2H-able buffer; the sigmoid is the processor's)."""

    family = "fai_cls"

    def _make_engine(self):
        return ClsEngine(self.config, self._state, str(self._device))

    def forward(self, images: torch.Tensor, targets: list = [], use_graph: bool = True) -> ClassificationModelOutput:
        if self.training or (targets is not None and len(targets) > 0):
            raise NotImplementedError("classification training is not built: the engine-backed module is the classifier's inference graph")
        pl = self.engine.forward(self._to_nhwc(images), use_graph=use_graph)
        self.last_plan = pl
        return ClassificationModelOutput(logits=pl.logits.clone(), loss=None)

    __call__ = forward

    def detect(self, images: torch.Tensor, sizes: Optional[torch.Tensor] = None, threshold: Optional[float] = None):
        pl = self.engine.forward(self._to_nhwc(images))
        self.last_plan = pl
        return pl


class ProcessorManager:
    """focoos/processor/processor_manager.py:8-46 — family -> processor class registry (seam B1) with lazy loaders."""

    _PROCESSOR_MAPPING: Dict[str, Callable[[], Type]] = {
        "fai_detr": lambda: DETRProcessor, "fai_mf": lambda: MaskFormerProcessor, "bisenetformer": lambda: BisenetFormerProcessor,
        "fai_cls": lambda: ClassificationProcessor}

    @classmethod
    def register_processor(cls, model_family, processor_loader: Callable[[], Type]):
        cls._PROCESSOR_MAPPING[getattr(model_family, "value", model_family)] = processor_loader

    @classmethod
    def get_processor(cls, model_family, model_config: dict, image_size=None):
        fam = getattr(model_family, "value", model_family)
        if fam not in cls._PROCESSOR_MAPPING:
            raise ValueError(f"Processor for {model_family} not supported")
        return cls._PROCESSOR_MAPPING[fam]()(config=model_config, image_size=image_size)


class FocoosModel:
    """focoos/models/focoos_model.py:88-147 — model + processor + model_info."""

    def __init__(self, model: _EngineModel, model_info: ModelInfo):
        self.model = model
        self.model_info = model_info
        # the mask families' processors ignore image_size (fai_mf/processor.py:96: no resize)
        self.processor = ProcessorManager.get_processor(model.family, model_info.config, image_size=model_info.im_size).eval()
        self.model.eval()

    @property
    def device(self):
        return self.model.device

    def infer_batch(self, inputs: list, threshold: Optional[float] = None, annotate=False, tracker=None,
                    mask_format: str = "png", zones=None, dwell=None, heatmap=None, tiling=None, classify=None) -> List[FocoosDetections]:
        """Batched inference: list of images in, list of FocoosDetections out (per-image result == the
        reference at B=1; the reference's own __call__ drops all but image 0 — focoos_model.py:615-621).  ``inputs`` may also be a
        ``frames.FrameBatch`` of NV12 / I420 / BGR / RGB video frames, host or device: the results are those of the same frames passed as
        RGB arrays (frames.py).  ``annotate``: every result
        also carries ``.image``, the uint8 input at its original size with the detections drawn on it on the device (annotate.py);
        non-uint8 inputs then raise ValueError; an ``annotate.Overlay`` also draws the track ids, the zones with their counts and the traces
        (it needs the ``tracker`` / ``zones`` it draws from, and its traces as a ``DeviceTraces``).  ``tracker``: a ``tracking.DeviceTracker`` of ``len(inputs)`` streams, for callers who
        feed one batch per call - image b is the next frame of stream b, and every tracked detection gets its ``track_id`` (the
        detections themselves are those of ``tracker=None``).  ``mask_format``: how the mask families hand out their masks - "png" (the
        reference's base64 PNG in ``FocoosDet.mask``, the default), "rle" (``FocoosDet.rle``: the full-frame uncompressed COCO RLE, encoded on
        the device, ``mask`` is None; mask_rle.py), "polygon" (``FocoosDet.polygons``: every ring of the mask's boundary, holes too,
        traced on the device, ``mask`` and ``rle`` are None; mask_polygon.py) or "none" (boxes, scores and labels only); anything
        else raises ValueError, "rle" or "polygon" on a family without masks NotImplementedError.  ``annotate`` and ``tracker`` read the
        packed device results, so they compose.  ``zones``: a ``zones.DeviceZones`` of ``len(inputs)`` streams, the counterpart of
        ``tracker`` for zone and line counting (zones.py): every result carries ``.zones``; a DeviceZones built on a tracker
        runs that tracker (``tracker`` must be None or that one).  ``dwell``: a ``zones.DeviceDwell`` built on that DeviceZones - the dicts
        of its zones also carry the dwell times; ``heatmap``: a ``heat.DeviceHeatmap`` of ``len(inputs)`` streams, updated from
        every batch and drawn by ``annotate=Overlay(heat=True)`` (heat.py).  ``tiling``: a ``tiled.Tiling`` - every input is a
        large frame of stream b (a ``FrameBatch``, or a list of ``Frame`` s and / or uint8 RGB arrays, all of one size) that is cut into
        windows, run through the engine in chunks and merged per stream on the device into one packed result in frame pixels, which the
        tracker, the zones, the heat map, the overlay and the detections then read as they read the engine's (tiled.py); fai_detr
        only (NotImplementedError otherwise), mixed sizes or non-uint8 inputs raise ValueError, all before anything touches the GPU.
        ``classify``: a ``cascade.DeviceCascade`` of ``len(inputs)`` streams - a second model on every detected object (cascade.py, DESIGN
        25): after the tracker, at most ``Cascade.max_objects`` detections per stream are cropped from the resident frames on the device,
        run through the cascade's fai_cls classifier and handed ``attr_id`` / ``attr_label`` / ``attr_conf``; a cascade built on a tracker
        runs that tracker (``tracker`` must be None or that one) and remembers the attribute per track.  The inputs are uint8 frames (a
        list of RGB arrays is wrapped into one ``FrameBatch``; sizes may differ without ``tiling``); everything else is that of
        ``classify=None``.  A family without boxes raises NotImplementedError, anything but a DeviceCascade TypeError, a classifier on
        another device or non-uint8 inputs ValueError, all before anything touches the GPU."""
        from .analytics import StreamAnalytics, batch_size
        from .frames import drawable

        an = StreamAnalytics.resolve(self, "infer_batch", device_only=True, track=tracker, zones=zones, dwell=dwell, heatmap=heatmap,
                                     annotate=annotate, classify=classify, tiling=tiling, detections=True, mask_format=mask_format,
                                     threshold=threshold)
        inputs = an.frames(inputs)      # a FrameBatch (or one Frame) goes where a list of images goes (frames.py)
        an.prepare(inputs, batch_size(inputs))
        t0 = perf_counter()
        if tiling is not None:       # the views of every frame in one launch, the chunks on one plan, one merge: `pl` is the merged result
            from . import tiled as TL

            t1 = t0
            pl, tiler = TL.infer_batch_tiled(self, inputs, tiling, an.thr)
            images = tiler.rgb(inputs) if annotate else None      # the full-size frames, already resident, are what is drawn on
        else:
            images, _ = self.processor.preprocess(inputs, device=self.model.device, dtype=self.model.dtype)
            t1 = perf_counter()
            sizes = torch.tensor(self.processor.get_image_sizes(inputs), dtype=torch.int32)
            pl = self.model.detect(images, sizes=sizes, threshold=an.thr)
        torch.cuda.current_stream(self.model.device).synchronize()
        t2 = perf_counter()
        out = an.analyse(pl, batch_size(inputs), inputs)
        if tiling is not None:
            TL.warn_dropped(tiler.status, "infer_batch")
        t3 = perf_counter()
        if annotate:
            an.draw((drawable(inputs, images, self.model.device), images), pl, out)
        t4 = perf_counter()
        an.close()
        for o in out:
            o.latency = InferLatency(preprocess=round(t1 - t0, 3), inference=round(t2 - t1, 3), postprocess=round(t3 - t2, 3),
                                     annotate=round(t4 - t3, 3) if annotate else None)
        return out

    def infer_stream(self, batches, threshold: Optional[float] = None, depth: Optional[int] = None, annotate=False, track=None,
                     mask_format: str = "png", zones=None, detections: bool = True, dwell=None, heatmap=None, tiling=None, classify=None):
        """Throughput inference (round 6): iterate over ``batches`` (each a list of images of ONE common shape after preprocessing and one
        batch size) and yield each batch's ``List[FocoosDetections]`` in order, with up to ``depth`` batches in flight on the engine's
        pipeline (engine.pipeline(): batch i+1's backbone runs beside batch i's decoder tail; default depth 3).  Same results as
        ``infer_batch`` per batch, bit for bit - the lanes share nothing but the read-only weights; what changes is that the GPU is not
        drained between batches (RT-DETR-L bs = 32: +8 % images/s, MaskFormer-L +15 %, BiSeNetFormer-L +36 %).
        ``annotate``: as in ``infer_batch`` - each batch is drawn after its lane finished, from the lane's still-valid results and the
        submitted frames, on the current stream; the detections are those of ``annotate=False``.  ``annotate.Overlay(ids, zones, traces)``
        in the place of ``True`` also draws what ``track`` / ``zones`` know: "#17 " in front of a tracked label, the regions
        tinted and outlined with "door: 3" / "gate: 12/9", and a tail of the last ``traces`` anchors behind every track (one more launch
        after the zones'); a field that has nothing to draw from (ids or traces without ``track``, zones without ``zones``) raises
        ValueError before anything touches the GPU, ``True`` draws exactly what it always drew.  ``Overlay(redact=annotate.Redact(...))``
        first makes the selected objects unreadable on the device (pixelate / blur / fill; box, ellipse or the instance's mask; with
        ``hold`` also the predicted boxes of tracks the detector has just missed) and ``Overlay(draw=False)`` leaves out boxes, masks and
        labels; ``Redact.hold`` without ``track``, ``shape="mask"`` on a family without masks or an unknown class name raise on
        the host.
        ``track``: identity across frames on the device (tracking.py) - batch index b is stream b (camera b), consecutive batches
        are consecutive frames.  ``True`` (the defaults), a ``TrackerConfig``, or a ``DeviceTracker`` whose state then outlives the call.
        Each batch is one more launch after its lane finished (batches finish in order) and every tracked detection carries ``track_id``;
        the detections themselves are those of ``track=None``.  The first batch fixes the batch size, another size raises ValueError;
        a family without boxes raises NotImplementedError before anything touches the GPU; births dropped for want of a free slot warn
        once per call.
        ``mask_format``: as in ``infer_batch``; with "rle" each batch's masks are encoded on the device after its lane finished and only the
        counts come back (one encoder serves every lane: batches finish in order on the current stream); "polygon" works the same way.
        ``zones``: zone and line counting on the device (zones.py) - a list of ``Zone`` / ``Line``, or a ``DeviceZones`` whose
        state then outlives the call (built on a tracker, it runs that tracker).  One more launch per batch right after the tracker's;
        every result carries ``.zones`` = ``{name: {"kind", "count", "detections", "entered", "exited", "crossed_in", "crossed_out"}}``:
        this frame's occupancy and the indices into ``.detections`` of the detections inside, the running totals of the events, and the
        indices of this frame's events.  Events need identity: a ``Line`` without ``track`` raises ValueError before anything touches the
        GPU, zones without ``track`` count occupancy only.  The detections are those of ``zones=None``, which changes nothing.
        ``detections=False`` (needs ``zones``; ValueError with ``annotate`` or another ``mask_format`` than the default): the analytics-only
        mode - the detection objects are not built, every result is ``FocoosDetections(detections=[], zones=...)`` with the same zone
        dicts.
        ``dwell``: dwell times on the device (zones.py ``DeviceDwell``) - ``True`` (every ``Zone``), a list of zone names, or a
        ``DeviceDwell`` whose state then outlives the call; needs ``zones`` and ``track`` (ValueError otherwise).  One more launch right
        after the zones'; the dict of a dwell zone also carries ``dwell`` (frames, aligned with its ``detections``), ``visits``,
        ``dwell_total``, ``dwell_max`` and ``dwell_mean``.  ``heatmap``: a ``heat.Heatmap`` or a ``heat.DeviceHeatmap`` (heat.py) -
        every batch's anchors are accumulated on a grid on the device, nothing is copied back per frame (``DeviceHeatmap.grid()`` reads the
        map) and ``annotate=Overlay(heat=True)`` blends it in under everything else; every input must have the heat map's size.  Both run
        with ``detections=False`` too, and with both unset nothing changes.
        ``tiling``: a ``tiled.Tiling`` - tiled inference of video streams (tiled.py).  Every input of a batch (a ``FrameBatch``,
        or a list of ``Frame`` s and / or uint8 RGB arrays, all of one size) is a large frame of stream b; it is cut into the windows of
        ``tiled.views_of``, all windows of all frames run through ONE engine pipeline in chunks of ``Tiling.batch_size`` (the chunks of
        frame batch i+1 are in flight while batch i is merged and packed) and are merged per stream on the device into one packed result in
        frame pixels.  Everything above then reads that result exactly as it reads the engine's: ``track``, ``zones``, ``dwell``,
        ``heatmap``, ``annotate`` (drawn on the full-size frames, which are resident), ``detections=False``.  fai_detr only
        (NotImplementedError before anything touches the GPU); frames of one batch that differ in size, or non-uint8 inputs, raise
        ValueError; candidates dropped by the suppression cap warn once per call.  With ``None`` nothing changes.
        ``classify``: a ``cascade.Cascade`` or a ``cascade.DeviceCascade`` whose state then outlives the call - a second model on every
        detected object, on the device (cascade.py).  Per batch, after the tracker: one launch picks at most
        ``Cascade.max_objects`` detections per stream (the classes, sizes and scores the cascade asks for; tracks that were never
        classified first, then the ones whose answer is oldest), one launch crops and resizes their padded boxes straight from the
        resident frames (NV12 / I420 / BGR / RGB) to the classifier's input size, the cascade's fai_cls classifier runs on that buffer,
        and one launch hands every detection its attribute and remembers it per track (``interval``: frames before a track is classified
        again; ``hold``: "latest" or "best").  Three small arrays more come back with the packed copy; a detection whose
        ``attr_conf`` = sigmoid(logit) exceeds ``Cascade.threshold`` carries ``attr_id`` / ``attr_label`` / ``attr_conf``.  The inputs are
        uint8 frames: a list of RGB arrays or tensors is wrapped into one ``FrameBatch`` (one upload; sizes may differ per stream without
        ``tiling``), with ``tiling`` the crops come from the tiler's resident full-size frames and the merged result.  The detections,
        ids, zone dicts and drawn images are those of ``classify=None``.  A family without boxes raises NotImplementedError; anything but
        a Cascade / DeviceCascade TypeError; a classifier on another device, non-uint8 inputs, ``detections=False``, ``interval > 1`` or
        ``hold="best"`` without ``track``, or more than 65535 crops per batch ValueError - all before anything touches the GPU; eligible
        objects left out for want of crop budget warn once per call.  With ``None`` nothing changes."""
        from collections import deque
        from types import SimpleNamespace

        from .analytics import StreamAnalytics, batch_size
        from .frames import drawable

        an = StreamAnalytics.resolve(self, "infer_stream", device_only=False, track=track, zones=zones, dwell=dwell, heatmap=heatmap,
                                     annotate=annotate, classify=classify, tiling=tiling, detections=detections, mask_format=mask_format,
                                     threshold=threshold)
        if tiling is not None:      # the same tail on the merged result of every frame batch, in the tiler's own loop (tiled.py)
            from . import tiled as TL

            yield from TL.infer_stream_tiled(self, batches, tiling, an.thr, depth, an)
            an.close()
            return
        fam = self.model.family
        # one record per ticket in flight: what the batch's tail reads stays referenced until the ticket is finished - the frames the
        # crops are taken from (`classify`), what is drawn on (`annotate`), the pinned host buffer a classifier lane copies its logits into
        pipe, key, pending = None, None, deque()

        def finish():
            t = pending.popleft()
            pl = pipe.wait(t.ticket)
            out = an.analyse(pl, pipe.B, t.frames, None if t.host is None else t.host["logits"])
            if t.drawn is not None:
                an.draw(t.drawn, pl, out)
            return out

        for inputs in batches:
            inputs = an.frames(inputs)
            an.prepare(inputs, batch_size(inputs))
            images, _ = self.processor.preprocess(inputs, device=self.model.device, dtype=self.model.dtype)
            x = self.model._to_nhwc(images)
            B, H, W, _ = x.shape
            if key != (B, H, W, x.dtype):      # the input buffer's dtype is part of a plan: uint8 and resized float32 batches never share one
                while pending:
                    yield finish()
                eng, f32 = self.model.engine, x.dtype == torch.float32
                pipe = eng.pipeline(B, H, W, depth, f32, 1, False) if fam in ("fai_mf", "bisenetformer") else eng.pipeline(B, H, W, depth, f32)
                key = (B, H, W, x.dtype)
            if len(pending) >= pipe.depth:      # the lane about to be reused still holds an unread result
                yield finish()
            sizes = host = None
            if fam == "fai_cls":      # the lane copies its logits into pinned host memory on its own stream; sigmoid / threshold run on the host
                host = {"logits": torch.empty(B, self.model.num_classes, dtype=torch.float32, pin_memory=True)}
            else:
                sizes = torch.tensor(self.processor.get_image_sizes(inputs), dtype=torch.int32, device=x.device)
            pending.append(SimpleNamespace(ticket=pipe.submit(x, sizes, an.thr, host), host=host, frames=inputs if classify is not None else None,
                                           drawn=(drawable(inputs, x, x.device), x) if annotate else None))
        while pending:
            yield finish()
        an.close()

    def __call__(self, inputs, **kwargs) -> FocoosDetections:
        from .frames import as_frame_batch

        lst = as_frame_batch(inputs) or (inputs if isinstance(inputs, list) else [inputs])
        return self.infer_batch(lst, threshold=kwargs.get("threshold"), mask_format=kwargs.get("mask_format", "png"))[0]

    def infer(self, image, threshold: Optional[float] = None, annotate: bool = False, mask_format: str = "png") -> FocoosDetections:
        """focoos_model.py:370-416: one picture (path, PIL image, array, tensor) -> FocoosDetections.  ``annotate``: ``.image`` is the
        picture (np.uint8 [H, W, 3] RGB, original size) with the detections drawn on it on the device (annotate.py; the input itself
        when nothing was detected) and ``.latency.annotate`` / ``.latency.imload`` are set.  ``mask_format``: as in ``infer_batch``.
        ``image`` may also be a ``frames.Frame`` (NV12, I420, BGR or RGB video frame, host or device)."""
        from .frames import Frame, FrameBatch
        from .mask_rle import check_mask_format

        if annotate:
            from .annotate import refuse_overlay

            refuse_overlay(annotate, "infer")
        check_mask_format(mask_format, self.model.family, "infer")
        t0 = perf_counter()
        if isinstance(image, (str, os.PathLike)):
            from PIL import Image

            image = np.array(Image.open(image).convert("RGB"))
        if not annotate:
            return self(image, threshold=threshold, mask_format=mask_format)
        imload = perf_counter() - t0
        res = self.infer_batch(image if isinstance(image, (Frame, FrameBatch)) else [image], threshold=threshold, annotate=True,
                               mask_format=mask_format)[0]
        res.latency.imload = round(imload, 3)
        return res

    def infer_tiled(self, image, tile: Union[None, int, Tuple[int, int]] = None, overlap: float = 0.2, threshold: Optional[float] = None,
                    merge_threshold: float = 0.5, merge_metric: str = "iou", include_full: bool = True, batch_size: Optional[int] = None,
                    max_detections: int = 300, annotate: bool = False, mask_format: str = "png") -> FocoosDetections:
        """Tiled RT-DETR inference of ONE large picture (an engine-native mode like ``infer_stream``; the reference has none): ``image`` (what
        ``infer`` takes) is cut into overlapping windows of ``tile`` (int or (h, w), default ``model_info.im_size``; both the window cut from
        the frame and the size the model runs at) that share at least ``overlap`` in [0, 1) of a tile with their neighbours
        (``tiled.tile_grid``); ``include_full`` adds the whole frame resized to the tile, so objects larger than a tile are still found.
        The views run through the engine in chunks of ``batch_size`` (default min(views, 32)), the boxes above ``threshold`` (as in
        ``infer``) are moved into frame pixels and duplicates are removed by class-aware greedy NMS: a detection removes the lower-scored
        ones of its class whose IoU (``merge_metric="iou"``) or intersection over the smaller area (``"ios"``) with it exceeds
        ``merge_threshold`` in (0, 1].  Returns one ``FocoosDetections`` with at most ``max_detections`` integer xyxy boxes in frame
        pixels, best first.  Cropping, resizing and merging run on the device (fx_tile_gather_u8_f32, fx_merge_detections_nms; tiled.py):
        the frame goes up once, one packed result comes back.  Bad arguments raise ValueError; every family but fai_detr raises
        NotImplementedError before anything touches the GPU.  ``annotate``: ``.image`` is the frame with the merged detections drawn on
        it (the resident frame is drawn on the device and copied back beside the packed result; annotate.py).  ``mask_format``: tiled
        inference has no masks to hand out - "rle" and "polygon" raise NotImplementedError, another unknown value ValueError."""
        from .frames import refuse_frames
        from .mask_rle import check_mask_format

        refuse_frames(image, "infer_tiled")      # before anything loads the library
        if annotate:
            from .annotate import refuse_overlay

            refuse_overlay(annotate, "infer_tiled")
        from .tiled import infer_tiled as _infer_tiled

        if check_mask_format(mask_format, None, "infer_tiled") in ("rle", "polygon"):
            raise NotImplementedError(f"infer_tiled: mask_format={mask_format!r} is not built: tiled inference merges boxes only (model family "
                                      f"{self.model.family!r})")

        return _infer_tiled(self, image, tile, overlap, threshold, merge_threshold, merge_metric, include_full, batch_size, max_detections,
                            annotate)

    def train(self, args, data_train, data_val=None, hub=None):
        """focoos_model.py:221-274: fine-tune on ``data_train`` (indexable, entries = ports.DatasetEntry) with ``args`` (ports.TrainerArgs):
        one process per GPU, TrainStep on every rank, artifacts in ``args.output_dir/args.run_name``, weights reloaded into the engine."""
        if self.model.family == "fai_cls":
            raise NotImplementedError("classification training is not built: fai-cls models run inference only on this engine")
        from .trainer import train as _train

        return _train(self, args, data_train, data_val, hub)

    def eval(self, args, data_test, save_json: bool = True) -> dict:
        """focoos_model.py:276-320 + trainer.py:226-286: evaluate on ``data_test`` (indexable; ports.SemanticSegmentationDatasetEntry /
        ClassificationDatasetDict items, metadata from ``data_test.dataset.metadata`` or ``data_test.metadata``), write
        ``args.output_dir/<run_name>_eval/{model_info,metrics}.json`` and return the results dict.  Semantic segmentation runs the fused
        fx_semseg_eval_accumulate kernel, classification counts TP / FP / FN on the device (evaluation.py).  Detection and instance
        segmentation raise NotImplementedError here: ``eval_detection`` scores RT-DETR (COCO bbox AP) and ``eval_instance_segmentation`` the
        instance-segmentation MaskFormer models (COCO segm AP)."""
        from .evaluation import run_eval

        return run_eval(self, args, data_test, save_json)

    def eval_detection(self, args, data_test, save_json: bool = True) -> dict:
        """COCO bbox AP of an RT-DETR model on ``data_test`` (indexable; ports.DetectionDatasetEntry items with ``annotations`` or
        ``instances`` ground truth): same arguments and artifacts as ``eval``, returns ``{"bbox": {"AP", "AP50", "AP75", "APs", "APm",
        "APl", "AP-<class>"...}}`` like the reference's DetectionEvaluator.  The detections are matched on the device
        (fx_detr_eval_boxes_f32 + fx_coco_match_bbox), accumulated in numpy float64 (detection_eval.py).  Every family but fai_detr raises
        NotImplementedError before anything is created."""
        from .detection_eval import check_supported, run_eval_detection

        check_supported(self)
        return run_eval_detection(self, args, data_test, save_json)

    def eval_instance_segmentation(self, args, data_test, save_json: bool = True) -> dict:
        """COCO segm AP of an instance-segmentation MaskFormer model (fai-mf-*-coco-ins) on ``data_test`` (indexable; entries with ``image``,
        ``height``, ``width`` and ground-truth masks as ``annotations[i]["segmentation"]`` - a 2-D array or an uncompressed RLE dict - or
        ``instances.masks``): same arguments and artifacts as ``eval``, returns ``{"segm": {"AP", "AP50", "AP75", "APs", "APm", "APl",
        "AP-<class>"...}}`` like the reference's InstanceSegmentationEvaluator.  Masks are thresholded into bit-packed words, intersected and
        matched on the device (fx_mf_eval_masks + fx_coco_mask_inter + fx_coco_match_segm; segm_eval.py), accumulated in numpy float64.
        Every other family, and a semantic fai_mf, raises NotImplementedError before anything is created."""
        from .segm_eval import check_supported, run_eval_instance_segmentation

        check_supported(self)
        return run_eval_instance_segmentation(self, args, data_test, save_json)

    def export(self, *a, **k):
        raise NotImplementedError("FocoosModel.export: the ONNX/TensorRT export path is out of scope (BASELINE north_star)")


class ModelManager:
    """focoos/model_manager.py:17-155 — lazy family registry + ``get``."""

    _MODEL_MAPPING: Dict[str, Callable[[], Type]] = {"fai_detr": lambda: FAIDetr, "fai_mf": lambda: FAIMaskFormer,
                                                              "bisenetformer": lambda: BisenetFormer,
                                                              "fai_cls": lambda: FAIClassification}

    @classmethod
    def register_model(cls, model_family: str, model_loader: Callable[[], Type]):
        cls._MODEL_MAPPING[getattr(model_family, "value", model_family)] = model_loader

    @classmethod
    def _from_local_dir(cls, name: str) -> ModelInfo:
        """model_manager.py:158-188: a run directory (as given, or under the models directory) holding ``model_info.json``; a bare
        ``model_final.pth`` in it is resolved against the directory."""
        run_dir = name
        if not os.path.exists(run_dir):
            run_dir = os.path.join(MODELS_DIR, name)
            if not os.path.exists(run_dir):
                raise ValueError(f"Run {run_dir} not exists.")
        info_path = os.path.join(run_dir, "model_info.json")
        if not os.path.exists(info_path):
            raise ValueError(f"Model info not found in {run_dir}")
        info = ModelInfo.from_json(info_path)
        if info.weights_uri == "model_final.pth":
            info.weights_uri = os.path.join(run_dir, info.weights_uri)
        return info

    @classmethod
    def get(cls, name: str, model_info: Optional[ModelInfo] = None, config: Optional[dict] = None, device: str = "cuda:0", seed: int = 0,
            **kwargs) -> FocoosModel:
        if model_info is None:
            # model_manager.py:74-91: hub reference / registry name / local run directory, in this order
            name = os.fspath(name)
            if name.startswith("hub://"):
                raise NotImplementedError("hub:// references need the Focoos Hub client (network; outside this engine): download the run and pass its folder")
            if ModelRegistry.exists(name):
                model_info = ModelInfo.from_json(ModelRegistry.get_model_info(name))
            else:
                model_info = cls._from_local_dir(name)
        fam = getattr(model_info.model_family, "value", model_info.model_family)
        if fam not in cls._MODEL_MAPPING:
            raise ValueError(f"Model {fam} not supported")
        cfg = dict(model_info.config)
        if config:
            cfg.update(config)
        cfg.update(kwargs)
        model_info.config = cfg
        nn = cls._MODEL_MAPPING[fam]()(cfg, device=device, seed=seed)
        fm = FocoosModel(nn, model_info)
        if model_info.weights_uri:
            if not os.path.exists(model_info.weights_uri):
                raise FileNotFoundError(f"Weights file not found: {model_info.weights_uri}")
            state = torch.load(model_info.weights_uri, map_location="cpu", weights_only=True)
            nn.load_state_dict(state.get("model", state) if isinstance(state, dict) else state, strict=False)
        else:
            warnings.warn(f"⚠️ Model {model_info.name} has no pretrained weights (offline): seeded synthetic weights (seed={seed})")
        return fm
