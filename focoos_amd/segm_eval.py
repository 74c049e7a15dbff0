"""COCO segm AP for the instance-segmentation MaskFormer models: the device path of FocoosModel.eval_instance_segmentation (DESIGN.md
section 13).  The protocol, the records, accumulate / summarize and the host evaluator (InstanceSegmentationEvaluator) live in
detection_eval.py; this module drives the kernels of csrc/coco_segm_eval.hip and fx_coco_match_segm on the engine's buffers:

    engine forward (full_masks=False) -> top-k over [Q K] -> fx_mf_eval_masks (bit-packed original-size masks, counts, boxes, scores)
    -> fx_coco_mask_inter (popcounts against the host-packed ground truth) -> fx_coco_match_segm -> records.

Nothing is read back before the last batch; the packed masks of a batch are dropped when its matching has been queued."""
from __future__ import annotations

import ctypes
import os
from typing import List, Sequence

import numpy as np
import torch

from .detection_eval import _NA, MatchRecords, gather_records, ground_truth_masks, pack_rows, results_from


class DeviceMasks:
    """Outputs of fx_mf_eval_masks for one batch (device tensors) and the host copies of the layout."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def plane_words(self, b: int, q: int) -> torch.Tensor:
        """int32 [H_b, 2 ceil(W_b / 64)] of query q of image b (MaskFormerProcessor.unpack_masks reads it with a leading axis)"""
        H, W = (int(v) for v in self.sizes_host[b])
        ww = (W + 63) // 64
        o = int(self.word_off_host[b]) + q * H * ww
        return self.words[o: o + H * ww].view(torch.int32).view(H, 2 * ww)


def _word_offsets(sizes: np.ndarray, planes: Sequence[int]) -> np.ndarray:
    n = np.array([int(p) * int(h) * ((int(w) + 63) // 64) for p, (h, w) in zip(planes, sizes)], np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def eval_masks(mask_probs: torch.Tensor, probs: torch.Tensor, Hin: int, Win: int, sizes: Sequence[Sequence[int]], top_k: int,
               mask_threshold: float) -> DeviceMasks:
    """The batched eval_postprocess + instance_inference: top-k over [Q K] (fx_topk_rows_ws_f32) + fx_mf_eval_masks on the engine's
    low-resolution ``mask_probs`` [B, Q, h, w] and ``probs`` [B, Q, K] of a batch run at (Hin, Win); ``sizes`` the original (H, W)."""
    from . import _lib

    lib = _lib.load("bf16")
    mask_probs, probs = mask_probs.contiguous().float(), probs.contiguous().float()
    dev = probs.device
    B, Q, K = probs.shape
    h, w = mask_probs.shape[-2:]
    assert mask_probs.shape[:2] == (B, Q) and len(sizes) == B, (tuple(mask_probs.shape), len(sizes))
    T = min(int(top_k), Q * K)
    stream = torch.cuda.current_stream(dev).cuda_stream
    val = torch.empty(B, T, dtype=torch.float32, device=dev)
    idx = torch.empty(B, T, dtype=torch.int32, device=dev)
    tws = torch.empty(max(int(lib.fx_topk_rows_workspace_bytes(B, Q * K, T)), 8), dtype=torch.uint8, device=dev)
    _lib.check(lib.fx_topk_rows_ws_f32(probs.data_ptr(), Q * K, B, Q * K, T, val.data_ptr(), idx.data_ptr(), tws.data_ptr(), tws.numel(), stream),
               "fx_topk_rows_ws_f32")
    sizes_host = np.ascontiguousarray([[int(a), int(b)] for a, b in sizes], dtype=np.int32).reshape(B, 2)
    word_off_host = _word_offsets(sizes_host, [Q] * B)
    n_words = int(word_off_host[-1])
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)   # noqa: E731
    out = DeviceMasks(B=B, Q=Q, K=K, T=T, sizes_host=sizes_host, word_off_host=word_off_host, n_words=n_words, val=val, idx=idx,
                      sizes=torch.from_numpy(sizes_host).to(dev), word_off=torch.from_numpy(word_off_host).to(dev),
                      words=torch.zeros(max(n_words, 1), dtype=torch.int64, device=dev), qlist=i32(B, Q), nref=i32(B), count=i32(B, Q),
                      box=i32(B, Q, 4), psum=torch.empty(B, Q, dtype=torch.float32, device=dev), label=i32(B, T), query=i32(B, T),
                      score=torch.empty(B, T, dtype=torch.float32, device=dev))
    need = int(lib.fx_mf_eval_masks_workspace_bytes(B, Q, int(sizes_host[:, 0].max())))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    rc = lib.fx_mf_eval_masks(mask_probs.data_ptr(), val.data_ptr(), idx.data_ptr(), B, Q, K, T, int(h), int(w), int(Hin), int(Win),
                              out.sizes.data_ptr(), sizes_host.ctypes.data, out.word_off.data_ptr(), word_off_host.ctypes.data, n_words,
                              float(mask_threshold), out.words.data_ptr(), out.qlist.data_ptr(), out.nref.data_ptr(), out.count.data_ptr(),
                              out.box.data_ptr(), out.psum.data_ptr(), out.label.data_ptr(), out.query.data_ptr(), out.score.data_ptr(),
                              ws.data_ptr(), ws.numel(), ctypes.c_void_p(stream))
    _lib.check(rc, "fx_mf_eval_masks")
    return out


def _tight_boxes(m: np.ndarray) -> np.ndarray:
    """bool [G, H, W] -> int32 [G, 4] x0, y0, x1 + 1, y1 + 1 (zeros for an empty mask)"""
    G = len(m)
    box = np.zeros((G, 4), np.int32)
    for g in range(G):
        ys, xs = np.flatnonzero(m[g].any(1)), np.flatnonzero(m[g].any(0))
        if len(ys):
            box[g] = xs[0], ys[0], xs[-1] + 1, ys[-1] + 1
    return box


def device_mask_inter(dm: DeviceMasks, gts: List[tuple]):
    """fx_coco_mask_inter on a batch: ``gts`` the per-image ground_truth_masks() tuples, packed here into the kernels' word layout and
    uploaded as one buffer + offsets.  Returns (inter int32 [Q n_gt], gcount int32 [n_gt], gt offsets host / device, n_gt)."""
    from . import _lib

    lib = _lib.load("bf16")
    dev = dm.words.device
    B, Q = dm.B, dm.Q
    assert len(gts) == B
    for g, (H, W) in zip(gts, dm.sizes_host):
        if g[0].shape[1:] != (int(H), int(W)):
            raise ValueError(f"ground-truth masks {g[0].shape[1:]} do not match the original size {(int(H), int(W))}")
    offs = np.zeros(B + 1, np.int64)
    offs[1:] = np.cumsum([len(g[1]) for g in gts])
    n_gt = int(offs[-1])
    gw_off = _word_offsets(dm.sizes_host, [len(g[1]) for g in gts])
    off_d, gw_off_d = torch.from_numpy(offs).to(dev), torch.from_numpy(gw_off).to(dev)
    if n_gt == 0:
        return None, None, offs, off_d, 0
    packed = np.concatenate([pack_rows(g[0]).reshape(-1) for g in gts])
    gt_words = torch.from_numpy(packed.view(np.int64)).to(dev)
    gt_box = torch.from_numpy(np.concatenate([_tight_boxes(g[0]) for g in gts])).to(dev)
    inter = torch.zeros(Q * n_gt, dtype=torch.int32, device=dev)
    gcount = torch.zeros(n_gt, dtype=torch.int32, device=dev)
    rc = lib.fx_coco_mask_inter(dm.words.data_ptr(), dm.word_off.data_ptr(), dm.word_off_host.ctypes.data, dm.n_words, dm.qlist.data_ptr(),
                                dm.nref.data_ptr(), dm.box.data_ptr(), B, Q, dm.T, dm.sizes.data_ptr(), dm.sizes_host.ctypes.data,
                                gt_words.data_ptr(), gw_off_d.data_ptr(), gw_off.ctypes.data, int(gw_off[-1]), gt_box.data_ptr(),
                                off_d.data_ptr(), offs.ctypes.data, n_gt, inter.data_ptr(), gcount.data_ptr(),
                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "fx_coco_mask_inter")
    return inter, gcount, offs, off_d, n_gt


def device_match_segm(label, score, query, dcount, inter, gcount, offs: np.ndarray, off_d, gts: List[tuple], K: int, npig, status):
    """One fx_coco_match_segm call on a batch (label / score / query [B, T], dcount [B, Q], inter / gcount of device_mask_inter).  Returns
    (rank int32 [B, T], matched int64 [B, T], ignored int64 [B, T]) on the device; ``npig`` and ``status`` are accumulated."""
    from . import _lib

    lib = _lib.load("bf16")
    dev = label.device
    B, T = label.shape
    Q = dcount.shape[1]
    n_gt = int(offs[-1])
    max_gt = 0
    for g in gts:
        if len(g[1]):
            max_gt = max(max_gt, int(np.unique(g[1], return_counts=True)[1].max()))
    up = lambda i, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([g[i] for g in gts]), dtype=dt)).to(dev)   # noqa: E731
    cat_d, flag_d, area_d = (up(1, np.int32), up(2, np.int32), up(3, np.float64)) if n_gt else (None, None, None)
    rank = torch.full((B, T), -1, dtype=torch.int32, device=dev)
    matched = torch.zeros(B, T, dtype=torch.int64, device=dev)
    ignored = torch.zeros(B, T, dtype=torch.int64, device=dev)
    need = int(lib.fx_coco_match_workspace_bytes(max_gt))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.fx_coco_match_segm(label.data_ptr(), score.data_ptr(), query.data_ptr(), dcount.data_ptr(), B, T, int(K), int(Q), ptr(inter),
                                ptr(gcount), ptr(cat_d), ptr(flag_d), ptr(area_d), off_d.data_ptr(), offs.ctypes.data, n_gt, max_gt,
                                rank.data_ptr(), matched.data_ptr(), ignored.data_ptr(), npig.data_ptr(), status.data_ptr(), ptr(ws), need,
                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "fx_coco_match_segm")
    return rank, matched, ignored


def match_batch(dm: DeviceMasks, gts: List[tuple], K: int, npig, status):
    inter, gcount, offs, off_d, _ = device_mask_inter(dm, gts)
    return device_match_segm(dm.label, dm.score, dm.query, dm.count, inter, gcount, offs, off_d, gts, K, npig, status)


def records_from_device(image_ids: Sequence[int], label, score, rank, matched, ignored, npig, K: int) -> MatchRecords:
    """Device outputs of one or more batches ([N, T] tensors) -> MatchRecords; every image has predictions (top-k slots are never dropped)."""
    ids = np.asarray(image_ids, np.int64)
    r = rank.cpu().numpy()
    sel = r >= 0
    return MatchRecords(K, image_id=np.broadcast_to(ids[:, None], r.shape)[sel], category=label.cpu().numpy()[sel], rank=r[sel],
                        score=score.cpu().numpy()[sel].astype(np.float64), matched=matched.cpu().numpy().view(np.uint64)[sel],
                        ignored=ignored.cpu().numpy().view(np.uint64)[sel], npig=npig.cpu().numpy(), images=ids)


def score_order_inversions(category: np.ndarray, a: np.ndarray, b: np.ndarray):
    """Two score vectors ``a`` and ``b`` of the same detections (laid out images ascending, slots in order): how far do the orders they
    induce differ?  The result dict depends on the scores only through each category's stable descending order over all images (the
    per-image ranking is its restriction to an image, accumulate() sorts the category the same way), so equal orders give equal dicts and
    every differing decision comes from an inverted pair.  Returns (number of detections that ``b`` places before a detection ``a`` places
    before them, the largest ``a`` gap of an inverted pair)."""
    n, worst = 0, 0.0
    for c in np.unique(category):
        sl = np.flatnonzero(category == c)
        oa = np.argsort(-a[sl], kind="mergesort")
        pb = np.empty(len(sl), np.int64)
        pb[np.argsort(-b[sl], kind="mergesort")] = np.arange(len(sl))
        p = pb[oa]                                                  # position under b, walked in a's order: sorted iff the orders agree
        first = np.searchsorted(np.maximum.accumulate(p), p, side="right")      # the earliest element of a's order that b puts after this one
        inv = first < np.arange(len(p))
        if inv.any():
            sa = a[sl][oa].astype(np.float64)
            n += int(inv.sum())
            worst = max(worst, float((sa[first[inv]] - sa[inv]).max()))
    return n, worst


# ---------------------------------------------------------------------------------------------------------------- driver
def check_supported(focoos_model) -> None:
    """A config without ``postprocessing_type`` is refused too: the key is what tells an instance fai-mf from a semantic one."""
    fam = focoos_model.model.family
    kind = focoos_model.model_info.config.get("postprocessing_type")
    if fam != "fai_mf" or kind != "instance":
        what = f"{fam!r}" if fam != "fai_mf" else f"{fam!r} with postprocessing_type {kind!r}"
        raise NotImplementedError(f"FocoosModel.eval_instance_segmentation: COCO segm AP is evaluated for the fai_mf family with "
                                  f"postprocessing_type 'instance' only, not {what}")


def resolve(focoos_model, data_test):
    """(class names, dataset name) from the dataset metadata with detection_eval.resolve's checks: task mismatch, thing_classes count."""
    from .evaluation import _metadata

    check_supported(focoos_model)
    info = focoos_model.model_info
    meta = _metadata(data_test)
    names, dname = list(info.classes), None
    if meta is not None:
        mt = getattr(meta, "task", None)
        mt = getattr(mt, "value", mt)
        if mt is not None and mt != "instseg":
            raise ValueError(f"Task mismatch: model task instseg != dataset task {mt}")
        cls = getattr(meta, "thing_classes", None)
        if cls is None:
            cls = getattr(meta, "classes", None)
        if cls is not None:
            if len(cls) != focoos_model.model.num_classes:
                raise ValueError(f"dataset has {len(cls)} classes, the model {focoos_model.model.num_classes}: num_classes must match")
            names = list(cls)
        dname = getattr(meta, "name", None)
    return names, dname


def collect(focoos_model, data_test, indices: Sequence[int], batch_size: int) -> MatchRecords:
    """Run the engine over ``indices`` (image id = dataset index), build and match every batch's masks on the device; the per-slot outputs
    stay on the device until the last batch, a batch's mask words are dropped with it.  Plans created on the way are released afterwards."""
    from .evaluation import _batches

    model = focoos_model.model
    eng, dev, K = model.engine, model.device, model.num_classes
    proc = focoos_model.processor
    indices = list(indices)
    npig = torch.zeros(K, _NA, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    outs, pos = [], 0
    with eng.scoped_plans():
        for batch in _batches(data_test, indices, batch_size):
            x = torch.stack([img for _, img in batch]).to(dev).contiguous()
            pl = eng.forward(x, full_masks=False)
            sizes = [(int(e.height), int(e.width)) for e, _ in batch]
            dm = eval_masks(pl.mask_probs, pl.probs, x.shape[1], x.shape[2], sizes, proc.top_k, proc.mask_threshold)
            rank, matched, ignored = match_batch(dm, [ground_truth_masks(e) for e, _ in batch], K, npig, status)
            outs.append((dm.label, dm.score, rank, matched, ignored))
            pos += len(batch)
            del dm
        if int(status.item()):
            raise RuntimeError("fx_coco_match_segm: a ground-truth group exceeded the workspace it was sized for")
        if not outs:
            return MatchRecords(K)
        return records_from_device(indices[:pos], *[torch.cat([o[i] for o in outs]) for i in range(5)], npig, K)


def _dist_worker(model_info, cfg, state, device_seed, args, data_test, out_path):
    """One rank of a multi-GPU run: its InferenceSampler shard -> match records, gathered (the records, not sums) to rank 0."""
    import torch.distributed as dist

    from .evaluation import _per_rank_batch
    from .model import ModelManager
    from .train_data import InferenceSampler

    dev = f"cuda:{torch.cuda.current_device()}"
    fm = ModelManager.get(model_info.name, model_info=model_info, device=dev, seed=device_seed)
    fm.model.load_state_dict(state, strict=False)
    rec = collect(fm, data_test, list(InferenceSampler(len(data_test))), _per_rank_batch(args))
    merged = gather_records(rec, dst=0)
    if dist.get_rank() == 0:
        torch.save(merged.state(), out_path)


def run_eval_instance_segmentation(focoos_model, args, data_test, save_json: bool = True) -> dict:
    """FocoosModel.eval_instance_segmentation: ``{"segm": {...}}`` and the artifacts of FocoosModel.eval (``segm/...`` keys)."""
    from .evaluation import _per_rank_batch, write_artifacts

    names, dname = resolve(focoos_model, data_test)
    if len(data_test) == 0:
        raise ValueError("FocoosModel.eval_instance_segmentation: empty dataset")
    world = max(1, int(getattr(args, "num_gpus", 1)))
    K = focoos_model.model.num_classes
    if world > 1:
        import copy
        import tempfile

        from .launch import launch

        info = copy.deepcopy(focoos_model.model_info)
        info.weights_uri = None
        with tempfile.TemporaryDirectory() as tmp:
            out_path = os.path.join(tmp, "records.pt")
            launch(_dist_worker, world, args=(info, info.config, focoos_model.model.state_dict(), 0, args, data_test, out_path))
            rec = MatchRecords(K, **torch.load(out_path, weights_only=False))
    else:
        rec = collect(focoos_model, data_test, range(len(data_test)), _per_rank_batch(args))
    results = results_from(rec, names, "segm")
    write_artifacts(focoos_model, args, "instseg", results, dname, save_json)
    return results
