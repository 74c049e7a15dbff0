"""What ``infer_batch``, ``infer_stream`` and ``tiled.infer_stream_tiled`` run beyond the engine, written once: the tracker, the
zones, the dwell times, the heat map, the traces, the cascade and the overlay of one call.  ``StreamAnalytics.resolve`` turns the call's
arguments into validated objects on the host, ``prepare`` checks one batch and creates the device state the first batch creates,
``analyse`` and ``draw`` are the tail on a packed result, ``close`` issues the once-per-call warnings.  ``cascade``, ``tiled`` and
``heat`` are imported only by a call that passes their argument."""
from __future__ import annotations

from . import tracking as TR
from . import zones as Z
from .annotate import DeviceTraces, OverlayPass, annotate_results, check_inputs, check_overlay, traces_for_batch
from .frames import FrameBatch, as_frame_batch
from .mask_rle import MASK_FAMILIES, check_mask_format
from .ports import FocoosDetections


def batch_size(inputs) -> int:
    """The images of one batch as preprocess counts them: a list or a FrameBatch has its length, anything else is one picture."""
    return len(inputs) if isinstance(inputs, (list, FrameBatch)) else 1


class StreamAnalytics:
    """The analytics state of one call.  ``track`` / ``zones`` / ``dwell`` / ``heatmap`` / ``classify`` hold what ``resolve`` made of the
    arguments - None, a validated config, or a device object - and, from the first ``prepare`` on, device objects only."""

    def __init__(self, fm, what: str, annotate, detections: bool, tiling, mask_format: str, threshold):
        self.fm = fm                      # the FocoosModel
        self.what = what                  # "infer_batch" / "infer_stream": the prefix of the messages
        self.annotate = annotate          # the argument: False, True or an Overlay
        self.detections = detections
        self.tiling = tiling
        self.mask_format = mask_format
        self.threshold = threshold        # the argument; ``thr`` is the value that runs
        self.track = None                 # TrackerConfig, then DeviceTracker
        self.zones = None                 # list of Zone / Line, then DeviceZones
        self.dwell = None                 # (names, None), then DeviceDwell
        self.heatmap = None               # Heatmap, then DeviceHeatmap
        self.classify = None              # Cascade, then DeviceCascade
        self.overlay = None               # the Overlay of ``annotate``, None for True / False
        self.traces = None                # the overlay's DeviceTraces
        self.ids = None                   # the track ids of the batch ``analyse`` saw last, which ``draw`` reads

    @classmethod
    def resolve(cls, fm, what: str, *, device_only: bool, track, zones, dwell, heatmap, annotate, classify, tiling, detections: bool,
                mask_format: str, threshold=None) -> "StreamAnalytics":
        """Every argument check of the entry points, in one order, on the host: nothing is loaded or launched.  ``device_only``
        (``infer_batch``, which sees one batch per call): only a DeviceTracker, DeviceZones, DeviceDwell, DeviceHeatmap, DeviceCascade and
        DeviceTraces are taken, whose state outlives the call.  ``what`` is the prefix of the messages."""
        fam = fm.model.family
        Z.check_detections_flag(detections, zones, annotate, mask_format, what)
        check_mask_format(mask_format, fam, what)
        if tiling is not None:
            from . import tiled as TL

            TL.check_tiling(fm, tiling, what)
        if classify is not None:
            from . import cascade as CS

            CS.check(fm, classify, detections, what, device_only=device_only)
        if annotate and fam == "fai_cls":
            check_overlay(annotate, False, False, fam, what)
        track = TR.resolve(track, fam, device=None, what=what, device_only=device_only)      # the device is not read
        if classify is not None and track is None:
            track = getattr(classify, "tracker", None)      # a DeviceCascade built on a tracker runs that tracker, for the zones too
        zones, track = Z.resolve(zones, track, fam, what, device_only)
        dwell = Z.resolve_dwell(dwell, zones, track, fam, what, device_only)
        if classify is not None:
            classify, track = CS.bind_tracker(classify, track, what)
        if heatmap is not None:
            from . import heat as HM

            heatmap = HM.resolve(heatmap, track is not None, fam, what, device_only)
        an = cls(fm, what, annotate, detections, tiling, mask_format, threshold)
        an.track, an.zones, an.dwell, an.heatmap, an.classify = track, zones, dwell, heatmap, classify
        if annotate:
            an.overlay = check_overlay(annotate, track is not None, zones is not None, fam, what, heatmap is not None, fm, device_only)
        if an.overlay is not None and isinstance(an.overlay.traces, DeviceTraces):
            an.traces = traces_for_batch(an.overlay, track, what)      # the caller's own: it must follow the tracker that runs
        return an

    @property
    def thr(self) -> float:
        """The score threshold that runs: the argument, or the processor's (read after ``resolve`` has passed, not before)."""
        return self.threshold or self.fm.processor.threshold

    def frames(self, inputs):
        """One batch's inputs as the call reads them: with ``tiling`` a FrameBatch of one size, with ``classify`` a FrameBatch (the
        detector's preprocess and the crops then read the same resident planes), otherwise a FrameBatch where one or a Frame was passed
        and the inputs as they came.  ValueError for inputs the argument cannot take; host only."""
        if self.tiling is not None:
            from . import tiled as TL

            inputs = TL.stream_frames(inputs, self.what)
        if self.classify is not None:
            from . import cascade as CS

            return CS.stream_frames(inputs, self.what)
        return as_frame_batch(inputs) or inputs

    def prepare(self, inputs, B: int) -> None:
        """One batch of B streams, on the host: every check that needs the batch, and only then the device state that the first batch
        creates (it fixes B), so no refusal comes after anything has loaded the library."""
        what, track, zones, heatmap, classify = self.what, self.track, self.zones, self.heatmap, self.classify
        if classify is not None:
            from . import cascade as CS

            CS.check_budget(classify, B, what)
        if self.annotate:
            check_inputs(inputs, what)
        if heatmap is not None:
            from . import heat as HM

            HM.check_sizes(heatmap, self.fm.processor.get_image_sizes(inputs), what)
        if track is None and zones is None and heatmap is None and classify is None:
            return      # dwell and traces need zones and a tracker: nothing to compare or create, the model's device is not read
        device = self.fm.model.device
        # a device object - the caller's, or the one an earlier batch created - is compared with B by its for_batch helper ...
        if isinstance(track, TR.DeviceTracker):
            TR.for_batch(track, B, device, what)
        if classify is not None and isinstance(classify, CS.DeviceCascade):
            CS.for_batch(classify, B, track, device, what)
        if isinstance(zones, Z.DeviceZones):
            Z.for_batch(zones, B, track, device, what)
        if heatmap is not None and isinstance(heatmap, HM.DeviceHeatmap):
            HM.for_batch(heatmap, B, device, what)
        # ... and only then the same helpers build a device object from every config (what was compared above comes back as it is)
        if track is not None:
            track = self.track = TR.for_batch(track, B, device, what)
        if classify is not None:
            self.classify = CS.for_batch(classify, B, track, device, what)
        if zones is not None:
            self.zones = Z.for_batch(zones, B, track, device, what)
        if heatmap is not None:
            self.heatmap = HM.for_batch(heatmap, B, device, what)
        if self.dwell is not None and not isinstance(self.dwell, Z.DeviceDwell):
            self.dwell = Z.DeviceDwell(self.zones, self.dwell[0])      # from the validated names, on the call's DeviceZones
        if self.overlay is not None and self.overlay.traced and self.traces is None:
            self.traces = traces_for_batch(self.overlay, track, what)      # like the tracker it follows

    def analyse(self, pl, B: int, fb=None, logits=None) -> list:
        """The tail on one packed result, on the current stream: ``pl`` is a lane's plan, ``model.detect``'s plan, or the tiler's merged
        result, which has the same packed fields.  The launches - tracker, zones, dwell, heat map, traces, cascade (on the batch's own
        frames ``fb``) - then the family's ``pack_detections`` (``logits``: a classifier lane's pinned host copy) and the attaches.
        Batches finish in order, so the frames reach the tracker in order."""
        fm, fam = self.fm, self.fm.model.family
        track, zones, dwell, classify, names = self.track, self.zones, self.dwell, self.classify, fm.model_info.classes
        ids = None
        if track is not None:      # one launch on the packed device results; the ids come back beside the packed copy
            ids = track.update(pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count)
        if zones is not None:      # one more launch, right after the tracker's, on the same packed results
            zv = zones.update(pl.det_labels, pl.det_boxes, pl.det_count, ids if zones.tracker is not None else None)
            if dwell is not None:  # and the dwell times, from the masks the zones just wrote
                dwell.update(pl.det_count, ids, zv["det_inside"])
        if self.heatmap is not None:    # this frame's anchors onto the grid; nothing comes back
            self.heatmap.update(pl.det_labels, pl.det_boxes, pl.det_count, ids)
        if self.traces is not None:     # the tail of every track, appended right after the tracker (and the zones)
            self.traces.update(pl.det_labels, pl.det_boxes, pl.det_count, ids)
        if classify is not None:   # select, crop, classify, attribute: four steps on the current stream, nothing comes back yet
            classify.update(pl, fb, ids, names)
        if not self.detections:    # analytics only: no detection objects, no ids on the host
            out = [FocoosDetections(detections=[]) for _ in range(B)]
        elif fam == "fai_cls":     # the one D2H copy of the batch's logits, unless the lane made it already
            out = fm.processor.pack_detections(logits if logits is not None else pl.logits.cpu(), names, self.thr)
        elif fam in MASK_FAMILIES:
            out = fm.processor.pack_detections(pl, names, mask_format=self.mask_format)
        else:
            out = fm.processor.pack_detections(pl.det_scores, pl.det_labels, pl.det_boxes, pl.det_count, names)
        if ids is not None and self.detections:
            TR.attach_ids(out, ids.cpu().tolist())
        if zones is not None:
            Z.attach(out, zones.fetch() if dwell is None else dwell.fetch(zones.fetch()))
        if classify is not None:
            from . import cascade as CS

            CS.attach(out, classify.fetch(), classify.cascade)
        self.ids = ids
        return out

    def draw(self, drawn, pl, out: list) -> None:
        """``out[i].image`` of the batch ``analyse`` just saw: ``drawn`` = (what is drawn on, the preprocessed batch).  A lane's results
        stay valid until the lane is submitted to again, which happens after this returns."""
        ov = self.overlay
        ovl = None if ov is None else OverlayPass(ov, self.ids, self.zones if ov.zones else None, self.traces, self.heatmap if ov.heat else None,
                                                  self.track if ov.redact is not None and ov.redact.hold > 0 else None)
        annotate_results(self.fm, *drawn, pl, out, ovl)

    def close(self) -> None:
        """The once-per-call warnings: births dropped for want of a free slot, eligible objects left out for want of crop budget."""
        if isinstance(self.track, TR.DeviceTracker):
            TR.warn_drops(self.track, self.what)
        if self.classify is not None:
            from . import cascade as CS

            CS.warn_left(self.classify, self.what)
