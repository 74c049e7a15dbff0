#!/usr/bin/env python
"""bench.py — images/sec of the focoos RT-DETR hot path on MI355X (BASELINE.json metric); with
`--model fai-mf-l-coco-ins` the MaskFormer path of BASELINE configs[2] (bs=16, 800x800).

A "step" = one pass of the hot path over one batch of synthetic input already resident in HBM:
uint8 HWC images -> fused normalise+stem -> ResNet50-vd -> hybrid encoder -> query selection ->
6 decoder layers -> sigmoid/xyxy -> device post-process (top-300, labels, int32 boxes, count) ->
D2H of the packed (<=300x6 per image) results.  Workload at N=1: BASELINE configs[1]
(fai-detr-l-obj365, bf16 MFMA, bs=32, 640x640, random-init weights, synthetic images).
N>1: one process per GPU, independent replicas (inference shards by image, no data-path collective:
SURVEY §8e) -> weak scaling; timing = barrier + synchronize, max over ranks.

Prints ONE JSON line on rank 0.  A plain run does what the headline figure needs and no more: set-up, warm-up, the timed steps,
`--dump-outputs`, the line.  `--full` adds every measurement that takes work of its own: `cpu_baseline` (the CPU fp32 oracle = "port"
of the reference path, timed on this host's cores on a bounded sample), `single_batch_in_flight`, `roofline` / `composite_roofline`
(dominant kernel: the implicit-GEMM conv template, live HIP-event timing on the engine's stream; `--per-op` writes the table),
`other_configs` (the other BASELINE configs, briefly) and, with `--train`, the weight-gradient `roofline` and `dp_check`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense MFMA bf16 peak, MI355X_MICROARCH.md (2:1-sparse marketing figure NOT used)
PEAK_HBM_GBS = 8000.0       # HBM3E peak, MI355X_MICROARCH.md (6.3 TB/s is what a float4 copy achieves)
ALG_GFLOP_PER_IMAGE = 139.05  # RT-DETR-L inference @640^2, algorithmic (dead mask_features conv excluded)
ALG_GFLOP_PER_IMAGE_MF_800 = 372.7  # fai-mf-l-coco-ins @800^2 as executed by the reference (scaled by area for other sizes)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-graphs", default=None, choices=["auto", "0", "1"],
                    help="--train: eager launches (0), hipGraph replays (1), or both timed during warm-up and the faster kept (auto, default; FX_TRAIN_GRAPH overrides the default)")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step (default 32; 16 for fai-mf-*)")
    ap.add_argument("--size", type=int, default=None, help="square input size (default 640; 800 for fai-mf-*)")
    ap.add_argument("--train", action="store_true",
                    help="training step instead of inference: fai-detr-l-obj365 forward + 7-set criterion + backward + DP gradient "
                         "all-reduce + fused AdamW, bs=16/GPU (BASELINE config 4 with BatchNorm frozen)")
    ap.add_argument("--norm", default="FrozenBN", choices=["FrozenBN", "BN", "SyncBN"],
                    help="--train: BatchNorm mode (FrozenBN = reference freeze_bn; BN / SyncBN = batch statistics, SyncBN all-reduces them)")
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp16"],
                    help="--train: 16-bit element type of activations / gradients / weight images (default bf16; bisenetformer-* training: fp16 = "
                         "BASELINE configs[4], the reference's fp16 autocast + GradScaler: fp16 MFMA, fp32 masters, dynamic loss scale with "
                         "skip-on-overflow inside the fused AdamW launch)")
    ap.add_argument("--pipeline", type=int, default=(int(os.environ["FX_BENCH_PIPELINE"]) if "FX_BENCH_PIPELINE" in os.environ else None),
                    help="RT-DETR inference: batches in flight (engine.pipeline(); default 3).  1 = one batch at a time as two concurrent half-batch "
                         "parts (engine.forward()'s form)")
    ap.add_argument("--streams", type=int, default=None, help="concurrent batch parts per step (default: engine default / FX_STREAMS)")
    ap.add_argument("--mf-full-masks", action="store_true", help="fai-mf-*: also write the reference's [B,Q,H,W] fp32 `masks` tensor")
    ap.add_argument("--mf-masks-dtype", default="fp32", choices=["fp32", "bf16"], help="fai-mf-* with --mf-full-masks: element type of the [B,Q,H,W] masks tensor")
    ap.add_argument("--mf-masks-d2h", action="store_true", help="fai-mf-*: include the D2H copy of the bit-packed mask buffer in the step")
    ap.add_argument("--model", default="fai-detr-l-obj365")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything that takes work of its own: CPU baseline, one batch in flight, per-kernel "
                         "and composite roofline (--per-op), the other BASELINE configs; --train: weight-gradient roofline, dp_check.  Off by "
                         "default: a plain run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--cpu-iters", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=64, help="upper bound of the CPU baseline's thread sweep (8 / 16 / 32 / 64)")
    ap.add_argument("--dry-run", action="store_true", help="CPU-only plumbing check (gloo): no GPU work, fake step")
    ap.add_argument("--per-op", default="", help="--full: write per-op timing table to this path")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, <= 64 MB in all; "
                         "bench_out/ is git-ignored)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full default run only: skip the short extra legs (RT-DETR / BiSeNetFormer training step, MaskFormer / BiSeNetFormer inference) "
                         "reported under `other_configs` of the one JSON line")
    ap.add_argument("--other-configs-budget", type=float, default=240.0, help="seconds after which the extra legs are abandoned (watchdog)")
    a = ap.parse_args()
    if a.per_op and not a.full:
        ap.error("--per-op writes the table of the per-kernel timing pass, which runs under --full")
    a.default_run = len([x for x in sys.argv[1:] if x.startswith("--model") or x in ("--train", "--dry-run")]) == 0
    mf = a.model.startswith("fai-mf")
    a.family = "fai_mf" if mf else ("bisenetformer" if a.model.startswith("bisenetformer") else "fai_detr")
    bf_train = a.train and a.family == "bisenetformer"   # BASELINE config 5: 1024 x 1024, 8 images per GPU
    a.dtype = a.dtype or ("fp16" if bf_train else "bf16")   # BASELINE configs[4] names fp16
    a.batch = a.batch or (8 if bf_train else (16 if (mf or a.train) else 32))
    a.size = a.size or (1024 if bf_train else (800 if mf else 640))
    return a


def dist_setup(args):
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the scale contract: `--gpus N` IS the number of ranks, whichever launcher started them (torchrun or our own spawn)
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus} (one rank per GPU; pass the same N to both)")
    if world > 1 and not dist.is_initialized():   # torchrun path; focoos_amd.launch initialises the group itself
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        backend = "gloo" if args.dry_run else "nccl"
        if not args.dry_run:
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    if world > 1:
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
    return world, rank, local


def barrier(world, dry):
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.barrier()
    if not dry:
        torch.cuda.synchronize()


def max_over_ranks(val: float, world: int, dry: bool) -> float:
    import torch
    import torch.distributed as dist

    if world == 1:
        return val
    t = torch.tensor([val], dtype=torch.float64, device="cpu" if dry else "cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def cpu_baseline(args):
    """The reference's PyTorch-CPU path on this host's cores.  kind "reference": the REAL reference model + processor (imported through
    oracle/ref_import where /root/reference exists - the build container; RT-DETR family); kind "port": the oracle's restatement of the same path
    (the GPU box has no reference tree).  The two are tied together once on the build box: profiles/r06_cpu_baseline_tie.json
    (scripts/cpu_baseline_tie.py) holds both timings of one run, and a "port" line quotes that ratio as `reference_tie`."""
    import torch

    from focoos_amd.registry import ModelRegistry
    from focoos_amd.synth import synth_image, synth_state_dict
    from oracle import bf_oracle as BFO
    from oracle import detr_oracle as O
    from oracle import mf_oracle as M

    cfg = ModelRegistry.get_model_info(args.model)["config"]
    sd = synth_state_dict(cfg, 0, family=args.family)
    mf = args.family == "fai_mf"
    bf = args.family == "bisenetformer"
    if mf:
        args.cpu_batch = 1
    ref = None
    if not mf and not bf and not getattr(args, "cpu_force_port", False):
        try:
            from oracle import ref_import

            if ref_import.reference_available():
                rcfg = dict(cfg)
                rcfg["resolution"] = args.size
                rmodel, rproc, _ = ref_import.build_reference_detr(rcfg)
                rmodel.load_state_dict(sd, strict=True)
                ref = (rmodel, rproc)
        except Exception:
            ref = None
    # Thread count actually used (reported as `cores`): PyTorch's CPU convs stop scaling (and at 256 threads collapse:
    # 0.03 img/s measured on the 256-core GPU host) well before a big host's core count.  Round 5: the count is the one that
    # MAXIMISES img/s on this box - one bs=1 pass (after a warm-up) at 8 / 16 / 32 / 64 threads, capped at --cpu-threads (default 64) and at
    # the host's cores - and the timed passes below run at it.
    cores = min(os.cpu_count() or 1, args.cpu_threads)
    torch.set_num_threads(cores)
    sweep = {}

    def timed(nb, iters):
        imgs = [synth_image(i, args.size, args.size) for i in range(nb)]
        times = []
        with torch.no_grad():
            for it in range(iters + 1):
                t0 = time.perf_counter()
                if ref is not None:     # the real thing: DETRProcessor.preprocess -> FAIDetr.forward -> DETRProcessor.postprocess (focoos_model.py:575-621)
                    xr, _ = ref[1].preprocess(imgs, device=torch.device("cpu"), dtype=torch.float32)
                    ref[1].postprocess(ref[0](xr), imgs, threshold=0.5)
                    dt = time.perf_counter() - t0
                    if it > 0:
                        times.append(dt)
                    elif dt > 15.0:
                        times.append(dt)
                        break
                    continue
                x = O.get_torch_batch(imgs, (args.size, args.size))
                if mf:
                    p, m = M.mf_forward(sd, cfg, x)
                    M.postprocess(p, m, [(args.size, args.size)] * len(imgs), cfg["mask_threshold"], cfg["threshold"], cfg["use_mask_score"])
                elif bf:
                    p, m = BFO.bf_forward(sd, cfg, x)
                    for i in range(len(imgs)):   # the reference post-process is batch-1 (see oracle/mf_oracle.postprocess)
                        BFO.postprocess(p[i:i + 1], m[i:i + 1], [(args.size, args.size)], cfg)
                else:
                    p, b = O.detr_forward(sd, cfg, x)
                    O.postprocess(p, b, [(args.size, args.size)] * len(imgs), 300, 0.5)
                dt = time.perf_counter() - t0
                if it > 0:
                    times.append(dt)
                elif dt > 15.0:  # bounded sample: a very slow host gets the warm-up pass as its only sample
                    times.append(dt)
                    break
        times.sort()
        return nb / times[len(times) // 2], len(times)

    for nthr in sorted({t for t in (8, 16, 32, 64) if t <= cores} | {cores}):
        torch.set_num_threads(nthr)
        sweep[nthr] = round(timed(1, 1)[0], 3)
    cores = max(sweep, key=sweep.get)
    torch.set_num_threads(cores)
    # bs=1 and a batch, warm-up + >= 5 timed passes each, median; bounded to ~20 s of CPU work
    v1, n1 = timed(1, args.cpu_iters)
    vb, nb_ = timed(args.cpu_batch, args.cpu_iters) if args.cpu_batch > 1 else (v1, n1)
    tie = None
    if ref is None:
        try:
            tie = json.load(open(os.path.join(ROOT, "profiles", "r06_cpu_baseline_tie.json")))
            tie = {k: tie[k] for k in ("reference_images_per_s", "port_images_per_s", "port_over_reference", "threads", "host_cores", "where")}
        except Exception:
            tie = None
    return {"value": round(max(v1, vb), 3), "unit": "images/s", "cores": torch.get_num_threads(), "cores_of": os.cpu_count(), "kind": "reference" if ref is not None else "port",
            "bs1_images_per_s": round(v1, 3), f"bs{args.cpu_batch}_images_per_s": round(vb, 3), "reference_tie": tie,
            "sample": ("the REAL reference (focoos FAIDetr + DETRProcessor through oracle/ref_import) " if ref is not None else
                       f"oracle/{'mf' if mf else ('bf' if bf else 'detr')}_oracle.py (CPU fp32 restatement of the reference path) ") + "preprocess+forward+postprocess at "
                      f"{args.size}x{args.size}: bs=1 median of {n1} passes and bs={args.cpu_batch} median of {nb_} passes, each after 1 warm-up; value = the better of the two; "
                      f"{cores} threads of {os.cpu_count()} host cores - the best of the one-pass thread sweep {sweep} (img/s at bs=1)",
            "thread_sweep_bs1_images_per_s": sweep}


def pmc_kernel_prefix(variant: str) -> str:
    """Engine variant label -> prefix of the (space-free) kernel name in the rocprofv3 PMC summaries."""
    import re

    m = re.match(r"conv3x3_flat<(\d+)>", variant)
    if m:
        return {"64": "conv3x3_flat_kernel<9,64,1,4,2,2", "128": "conv3x3_flat_kernel<9,64,2,4,2,2", "256": "conv3x3_flat_kernel<9,64,2,4,4,1"}[m.group(1)]
    m = re.match(r"conv3x3_kplane<(\d+)>", variant)   # tile forms of the N class (the 256-channel tile also serves N = 512; 64-pixel form for small M)
    if m:
        return {"64": ("conv3x3_kplane_kernel<2,2,1,4,", "conv3x3_kplane_kernel<2,4,1,4,"), "128": "conv3x3_kplane_kernel<2,4,2,2,"}.get(
            m.group(1), ("conv3x3_kplane_kernel<2,4,4,1,", "conv3x3_kplane_kernel<2,2,4,1,"))
    m = re.match(r"conv3x3_c32<(\d+)>", variant)
    if m:
        return f"conv3x3_c32_kernel<{int(m.group(1)) // 32},"
    m = re.match(r"pw_kplane<K(\d+)>", variant)
    if m:
        return f"conv_pw_kplane_kernel<{m.group(1)},"
    if variant.startswith("pw_flat"):
        return "conv3x3_flat_kernel<1,256"
    m = re.match(r"pw_chain<(\d+),(\d+),(\d+)>", variant)
    if m:
        return f"pw_chain_kernel<{m.group(1)},{m.group(2)},{m.group(3)},"
    m = re.match(r"conv_igemm_dma<(\d+),(\d+)>", variant)
    if m:
        return f"conv_igemm_dma_kernel<{m.group(1)},{m.group(2)},"
    m = re.match(r"conv_igemm<(\d+),(\d+),(\d+)", variant)
    if m:
        return f"conv_igemm_kernel<{m.group(1)},{m.group(2)},{m.group(3)},"
    return {"row_chain": "row_chain_kernel", "score_head": "score_head_kernel", "stem_c3+pool": "stem_c3_pool8_kernel", "stem_c1+c2": "stem12_kernel"}.get(variant.split("<")[0], "")


def per_op_timing(eng, pl, args):
    """Live HIP-event timing of every launch of one forward, in sequence (cold-ish caches), on the engine's stream.
    A spin kernel is queued first so the host enqueues the whole sequence ahead of the GPU (no launch gaps inside the
    bracketed intervals)."""
    import ctypes as C

    import torch

    from focoos_amd._lib import check

    st = eng.stream
    n = len(pl.ops)
    with torch.cuda.stream(st):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        acc = [0.0] * n
        reps = 3
        # calibrate the cost of an event->event interval with nothing in between (subtracted from every bracket)
        torch.cuda._sleep(int(4e7))
        for e in evs[:65]:
            e.record(st)
        st.synchronize()
        gaps = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(64))
        empty = gaps[len(gaps) // 2]
        for _ in range(reps):
            torch.cuda._sleep(int(4e7))
            evs[0].record(st)
            for i, (fn, a) in enumerate(pl.ops):
                check(fn(*pl.patch_args(fn, a, 0.5), C.c_void_p(st.cuda_stream)), fn.__name__)
                evs[i + 1].record(st)
            st.synchronize()
            for i in range(n):
                acc[i] += max(evs[i].elapsed_time(evs[i + 1]) - empty, 0.0)
    return [a / reps for a in acc]


ALG_GFLOP_PER_IMAGE_BF_1024 = 83.5   # bisenetformer-l-ade forward @1024^2 (FlopCounterMode on the reference)


def _wgrad_roofline(nn_, stepper, imgs, targets, family="fai_detr"):
    """`roofline` of the training step's dominant kernel family (the weight-gradient kernel): one extra step outside the timed region with
    every fx_conv2d_wgrad_partial launch bracketed by events on the stream it runs on; achieved = algorithmic FLOPs (2 M N K per
    launch) / summed durations, and the algorithmic bytes (x + dz read once, the fp32 partial slabs written once) against HBM."""
    import torch

    orig = nn_._conv_param_grads
    rec = []

    def timed(layer, x, dz, scale):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(layer, x, dz, scale)
        e1.record()
        B, H, W_, Cc = x.shape
        _, Ho, Wo, N = dz.shape
        k = layer.k
        rec.append((e0, e1, 2.0 * B * Ho * Wo * N * Cc * k * k, 2.0 * (x.numel() + dz.numel()) + 4.0 * N * Cc * k * k, (B * Ho * Wo, N, Cc, k, layer.stride)))
        return out

    nn_._conv_param_grads = timed
    side, stepper.wgrad_stream = stepper.wgrad_stream, None   # this one step keeps the weight gradients on the main stream, where the events are
    graphs, stepper.use_graphs = stepper.use_graphs, False     # ... and runs eagerly (a graph replay never enters the Python hook)
    try:
        stepper.step(imgs, targets)
    finally:
        nn_._conv_param_grads = orig
        stepper.wgrad_stream = side
        stepper.use_graphs = graphs
    torch.cuda.synchronize()
    ms = sum(r[0].elapsed_time(r[1]) for r in rec)
    if os.environ.get("FX_WGRAD_TABLE"):   # per-shape table of the weight-gradient launches (+ slab sum): M N C k stride launches ms TFLOP/s
        by_shape = {}
        for r in rec:
            d = by_shape.setdefault(r[4], [0, 0.0, 0.0])
            d[0] += 1
            d[1] += r[0].elapsed_time(r[1])
            d[2] += r[2]
        with open(os.environ["FX_WGRAD_TABLE"], "w") as f:
            f.write("# M N C k stride launches ms TFLOP/s   (weight-gradient kernel + slab sum per conv layer shape, serial on the main stream)\n")
            for sh, (n, t, fl_) in sorted(by_shape.items(), key=lambda kv: -kv[1][1]):
                f.write(f"{sh[0]:8d} {sh[1]:5d} {sh[2]:5d} {sh[3]} {sh[4]} {n:3d} {t:8.3f} {fl_ / (t * 1e-3) / 1e12:8.1f}\n")
    fl, by = sum(r[2] for r in rec), sum(r[3] for r in rec)
    tf, gbs = fl / (ms * 1e-3) / 1e12, by / (ms * 1e-3) / 1e9
    ai = fl / by
    # HBM bytes per launch of the weight-gradient kernel from the committed PMC passes of the RT-DETR training step (same recipe and
    # calibration as the inference line; None for the other families / when the file is absent)
    traffic, traffic_src = None, None
    try:
        if family == "fai_detr":
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_train_hbm_latest.json")))
            hits = [v for k, v in pmc.items() if k.startswith(("conv_wgrad_kernel", "conv_wgrad_dma_kernel"))]   # 128x128 tiles (pointwise / im2col) + the wide-layer form
            n_ = sum(v["launches"] for v in hits)
            traffic = round(sum((v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"]) * v["launches"] for v in hits) / n_)
            traffic_src = ("profiles/pmc_train_hbm_latest.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --train`, calibrated counter "
                           "units; launch-weighted average over ALL conv_wgrad_kernel / conv_wgrad_dma_kernel launches of a step - the 96 conv layers the event bracket covers plus the ~100 smaller Linear layers - partial-slab stores included)")
    except Exception:
        pass
    return {"bound": "mfma" if ai >= PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9) else "hbm", "kernel": "conv_wgrad_kernel / conv_wgrad_dma_kernel (+ slab sum / unpack)",
            "achieved": round(tf, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
            "traffic_source": traffic_src, "alg_bytes_per_launch": round(by / max(len(rec), 1)),
            "launches_per_step": len(rec), "ms_per_step": round(ms, 3), "arithmetic_intensity_flop_per_byte": round(ai, 1),
            "hbm": {"achieved_gbs_algorithmic": round(gbs, 1), "peak_gbs": PEAK_HBM_GBS, "frac": round(gbs / PEAK_HBM_GBS, 4)},
            "note": "events bracket the wgrad launch + its slab-sum/unpack pass of every conv layer in one extra step run with the weight gradients on the main stream (in the timed steps they run on a side stream, concurrently with the input-gradient chain)"}


DUMP_LIMIT_BYTES = 60 << 20   # under the 64 MB of the --dump-outputs contract, .npy headers included


def dump_outputs(path, arrays):
    """--dump-outputs: write {name: tensor} as <path>/<name>.npy, floating point as float32 and integers as float64 (exact up to 2**53), so
    that two builds can be compared output for output.  An array that would take the total over DUMP_LIMIT_BYTES is replaced by a fixed,
    seeded sample of its flattened elements (`<name>.npy`, with the sampled flat indices in `<name>.index.npy`)."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    total = 0
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())     # small arrays first: the large ones share what is left
    for i, (name, t) in enumerate(items):
        t = t.detach().cpu()
        a = (t.float() if t.is_floating_point() else t.double()).numpy()
        budget = (DUMP_LIMIT_BYTES - total) // (len(items) - i)
        if a.nbytes > budget:
            n = budget // (a.itemsize + 8)
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=n, replace=False))
            np.save(os.path.join(path, f"{name}.index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
            total += idx.size * 8
        np.save(os.path.join(path, f"{name}.npy"), a)
        total += a.nbytes
    assert total <= DUMP_LIMIT_BYTES, total
    return total


def synth_train_targets(family, rank, it, B, S, K, dev):
    """The synthetic targets of training step ``it`` on ``rank`` (seed = rank*1000 + it): RT-DETR - T_i ~ U{1..20} boxes per image, centres in
    [0.2, 0.8], sizes in [0.05, 0.35], labels U{0..K-1}; mask families - 5-15 random rectangular masks per image.  Module-level so that the
    parity tests at the BASELINE shapes (tests/test_gpu_train_baseline_configs.py) run on EXACTLY the step the bench times."""
    import numpy as np
    import torch

    from focoos_amd.ports import DETRTargets, MaskFormerTargets

    rs = np.random.RandomState(rank * 1000 + it)
    out = []
    for _ in range(B):
        if family in ("bisenetformer", "fai_mf"):
            t = rs.randint(5, 16)
            m = np.zeros((t, S, S), bool)
            for i in range(t):
                y0, x0 = rs.randint(0, S - 32), rs.randint(0, S - 32)
                m[i, y0:y0 + rs.randint(32, S // 2), x0:x0 + rs.randint(32, S // 2)] = True
            out.append(MaskFormerTargets(labels=torch.from_numpy(rs.randint(0, K, (t,))).to(dev), masks=torch.from_numpy(m).to(dev)))
        else:
            t = rs.randint(1, 21)
            bx = np.concatenate([rs.uniform(0.2, 0.8, (t, 2)), rs.uniform(0.05, 0.35, (t, 2))], -1).astype(np.float32)
            out.append(DETRTargets(labels=torch.from_numpy(rs.randint(0, K, (t,))).to(dev), boxes=torch.from_numpy(bx).to(dev)))
    return out


def train_measure(args, world, rank, local, with_roofline=True):
    """BASELINE config 4 per GPU: 16 synthetic 640^2 images + COCO-shaped targets (T_i ~ U{1..20}, seed = rank*1000 + iter);
    config 5 (--model bisenetformer-l-ade): 8 synthetic 1024^2 images + 5-15 random rectangular masks per image, labels U{0..149}.
    One optimisation step = forward (training mode) + criterion + backward + gradient all-reduce + AdamW."""
    import numpy as np
    import torch

    from focoos_amd import train_nn
    from focoos_amd.registry import ModelRegistry
    from focoos_amd.synth import synth_image, synth_state_dict
    from focoos_amd.train_detr import FAIDetrTrainable, TrainStep

    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    cfg = ModelRegistry.get_model_info(args.model)["config"]
    K, B, S = int(cfg["num_classes"]), args.batch, args.size
    bf = args.family == "bisenetformer"
    from focoos_amd import _lib as fxlib

    dtype = getattr(args, "dtype", None) or "bf16"
    prev_dtype = fxlib.set_compute_dtype(dtype)   # the element type of everything built below (restored before returning)
    if bf:
        from focoos_amd.train_bf import BisenetFormerTrainable

        model = BisenetFormerTrainable(cfg, norm=args.norm).to(dev)
    elif args.family == "fai_detr":
        model = FAIDetrTrainable(cfg, norm=args.norm).to(dev)
    else:
        from focoos_amd.train_mf import FAIMaskFormerTrainable

        model = FAIMaskFormerTrainable(cfg, norm=args.norm).to(dev)
    model.load_state_dict(synth_state_dict(cfg, 0, family=args.family), strict=True)
    model.train()
    graphs_mode = getattr(args, "train_graphs", None) or os.environ.get("FX_TRAIN_GRAPH", "auto")
    stepper = TrainStep(model, graphs=graphs_mode)
    if str(graphs_mode).lower() == "auto":
        args.warmup = max(args.warmup, 8)   # TrainStep's own eager / replay comparison takes steps 1-7 (train_detr.TrainStep.__init__): outside the timed region
    imgs = torch.stack([torch.from_numpy(synth_image(rank * B + i, S, S)) for i in range(B)]).to(dev)

    def targets(it):
        return synth_train_targets(args.family, rank, it, B, S, K, dev)

    # targets of every step are created (and moved to HBM) BEFORE the timed region, like the images: a data loader hands them over
    # asynchronously, and a pageable host->device copy inside the loop would stall the launch queue once per copy
    all_targets = [targets(it) for it in range(max(args.warmup, 1) + args.steps)]
    torch.cuda.synchronize()
    for it in range(max(args.warmup, 1)):
        losses = stepper.step(imgs, all_targets[it])
    barrier(world, False)
    t0 = time.perf_counter()
    for it in range(args.steps):
        losses = stepper.step(imgs, all_targets[max(args.warmup, 1) + it])
    barrier(world, False)
    dt = max_over_ranks(time.perf_counter() - t0, world, False)
    if rank == 0 and with_roofline and args.dump_outputs:
        # the last timed step's losses and the fp32 master weights it produced
        dump_outputs(args.dump_outputs, {**{k: v.reshape(-1) for k, v in losses.items()}, "master_weights": stepper.opt.flat_p})
    total = float(sum(v.detach().float() for v in losses.values()))
    value = world * B * args.steps / dt
    fwd = (ALG_GFLOP_PER_IMAGE_BF_1024 * (S / 1024.0) ** 2 if bf else
           (ALG_GFLOP_PER_IMAGE_MF_800 * (S / 800.0) ** 2 if args.family == "fai_mf" else ALG_GFLOP_PER_IMAGE * (S / 640.0) ** 2))
    alg = 3 * fwd  # training ~ 3 x forward (fwd + dgrad + wgrad)
    # data-parallel consistency: after the timed steps every rank must hold bit-identical fp32 master weights (same all-reduced
    # gradients, same optimizer arithmetic).  Checked under --full with one MIN and one MAX all-reduce of a float64 checksum.
    dp_check = None
    if world > 1 and args.full:
        import torch.distributed as dist

        chk = stepper.opt.flat_p.double().sum().reshape(1)
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dp_check = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "master_weights_identical_across_ranks": bool((lo == hi).item()),
                    "checksum": float(chk.item())}
    class stepper_graphs:   # noqa: N801  (tiny record read by the JSON line below)
        on = stepper._graph_state is not None
    roof = _wgrad_roofline(train_nn, stepper, imgs, all_targets[0], args.family) if (rank == 0 and with_roofline and args.full) else None
    barrier(world, False)
    out = None
    if rank == 0:
        crit = ("point-sampled mask Hungarian set criterion over 7 prediction sets" if bf else
                ("point-sampled mask Hungarian set criterion over 10 prediction sets" if args.family == "fai_mf" else "Hungarian set criterion over 7 prediction sets"))
        out = ({
            "metric": f"images/sec @ {S}^2 (train bs={B}/GPU" + ("; bf16 variant of BASELINE configs[4], which names fp16" if (bf and dtype != "fp16") else "") + ")", "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype, "data": "synthetic",
            "config": {"steps_are": "hipGraph replays (forward graph, backward graph) around an eager criterion + optimizer" if stepper_graphs.on else "eager launches",
                       "graphs": {"mode": str(graphs_mode), "choice": stepper.graph_choice},   # auto: both forms timed during the warm-up steps, the faster one kept
                       "workload": f"{args.model} training step: forward (train mode, norm={args.norm}) + {crit} "
                                   f"+ backward + gradient all-reduce + fused AdamW/clip, bs={B}/GPU, {S}x{S}, {dtype} activations and gradients"
                                   + (" (fp16 MFMA; dynamic loss scale as torch.amp.GradScaler: init 2**10, unscale / skip-on-inf / scale update "
                                      "inside the fused AdamW launch), " if dtype == "fp16" else ", ")
                                   + "fp32 master weights; HIP autograd nodes; "
                                   + ("forward and backward replayed as two hipGraphs around an eager criterion" if getattr(stepper_graphs, "on", False) else "eager launches, no graph")
                                   + ("; DEVIATION from BASELINE configs[4] ('fp16'): this run computes in bf16 without a GradScaler (--dtype bf16) - on the real "
                                      "reference the training losses under fp16 autocast deviate 0.66 % from fp32, under bf16 autocast 1.7 % "
                                      "(tests/test_oracle_vs_reference.py::test_reference_fp16_amp_losses_vs_fp32_and_bf16_autocast)" if (bf and dtype != "fp16") else ""),
                       "global_batch": B * world, "parallelism": f"dp{world} (RCCL all-reduce of one flat fp32 gradient buffer, 64 MiB buckets, "
                                                                 "segments launched from backward hooks)"},
            "alg_gflop_per_image": round(alg, 1), "frac_of_bf16_mfma_roofline_whole_path": round(value / world * alg * 1e9 / (PEAK_BF16_TFLOPS * 1e12), 4),
            "roofline": roof, "final_total_loss": round(total, 4), "dp_check": dp_check,
            "loss_scale": stepper.opt.scaler_state() if stepper.opt.scaler is not None else None})
    del stepper, model
    torch.cuda.empty_cache()
    fxlib.set_compute_dtype(prev_dtype)
    return out


def train_main(args, world, rank, local):
    out = train_measure(args, world, rank, local)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


def _spawned_rank(argv):
    """Entry of a rank started by focoos_amd.launch (process group already initialised, RANK/LOCAL_RANK/WORLD_SIZE exported)."""
    sys.argv = [os.path.join(ROOT, "bench.py")] + list(argv)
    run(parse())


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: spawn the N ranks here, one process per GPU, like the reference's launch()
        # (focoos/utils/distributed/dist.py:38-95) does for FocoosModel.train(num_gpus=N).  Under torchrun WORLD_SIZE is set
        # and each rank comes straight through run().
        from focoos_amd.launch import launch

        launch(_spawned_rank, args.gpus, dist_url="auto", args=(sys.argv[1:],), backend="gloo" if args.dry_run else "nccl")
        return
    run(args)


def run(args):
    world, rank, local = dist_setup(args)
    if args.dry_run:
        # plumbing only: same sharding / barrier / max-over-ranks / JSON code path with a fake 1 ms step
        barrier(world, True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            time.sleep(0.001)
        barrier(world, True)
        dt = max_over_ranks(time.perf_counter() - t0, world, True)
        if rank == 0:
            line = {"metric": "dry-run", "value": world * args.batch * args.steps / dt, "unit": "images/s", "n_gpus": world,
                    "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
                    "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "none", "config": {"workload": "dry-run"}}
            if args.train:
                # the per-rank plan of the data-parallel training step this command line would run: batch split, gradient segments and
                # buckets, bytes all-reduced per step - from the state spec alone (focoos_amd.train.dp_plan; no GPU, no model)
                from focoos_amd.registry import ModelRegistry
                from focoos_amd.train import dp_plan

                cfg = ModelRegistry.get_model_info(args.model)["config"]
                norm = "SyncBN" if (args.norm == "BN" and world > 1 and args.family == "bisenetformer") else args.norm
                line["dp_plan"] = dp_plan(cfg, args.family, norm, world, args.batch, grad_bytes=2 if os.environ.get("FX_DP_BF16", "0") == "1" else 4)
                line["dp_plan"]["ranks"] = [{"rank": r, "images": [r * args.batch, (r + 1) * args.batch], "target_seed": f"{r} * 1000 + iteration"}
                                            for r in range(world)]
            print(json.dumps(line))
        return

    if args.train:
        return train_main(args, world, rank, local)
    out = infer_measure(args, world, rank, local, light=False)
    if args.full and args.default_run and not args.no_other_configs:
        other_configs(args, world, rank, local, out)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


def other_configs(args, world, rank, local, out):
    """The other BASELINE.json configs, measured briefly in the same run and nested under `other_configs` of the ONE JSON line (rank 0's
    dict `out`): config 4 (RT-DETR training step, data-parallel over the same ranks), config 5 (BiSeNetFormer training step at 1024^2),
    config 3 (MaskFormer inference at 800^2) and BiSeNetFormer inference.  Each leg is the same code as `--train` / `--model ...`
    with fewer steps and without the per-kernel table.  A watchdog guards the headline: if the legs exceed their budget (or a
    collective hangs), rank 0 prints the line with what has been measured and every rank exits."""
    import copy
    import threading

    legs = {}
    if rank == 0:
        out["other_configs"] = legs

    def bail():
        if rank == 0:
            legs["watchdog"] = f"extra legs abandoned after {args.other_configs_budget:.0f} s"
            print(json.dumps(out), flush=True)
        os._exit(0)

    timer = threading.Timer(args.other_configs_budget + (0 if rank == 0 else 5), bail)
    timer.daemon = True
    timer.start()
    # inference legs first (replicas, no collective), the data-parallel training legs last
    plan = [("infer_fai-mf-l-coco-ins_bs16_800", dict(train=False, model="fai-mf-l-coco-ins", family="fai_mf", batch=16, size=800, steps=10, warmup=3)),
            ("infer_bisenetformer-l-ade_bs32_640", dict(train=False, model="bisenetformer-l-ade", family="bisenetformer", batch=32, size=640, steps=10, warmup=3)),
            ("train_fai-detr-l-obj365_bs16_640_frozenbn", dict(train=True, model="fai-detr-l-obj365", family="fai_detr", batch=16, size=640, norm="FrozenBN", steps=6, warmup=4)),
            # config 4 BOTH ways - frozen BatchNorm above, and the reference's own semantics here: live statistics, converted to
            # SyncBN whenever world_size > 1 (trainer/trainer.py:333-334) - so that a multi-GPU run records the mode the reference would train in
            (f"train_fai-detr-l-obj365_bs16_640_{'syncbn' if world > 1 else 'bn'}",
             dict(train=True, model="fai-detr-l-obj365", family="fai_detr", batch=16, size=640, norm="SyncBN" if world > 1 else "BN", steps=6, warmup=4)),
            # config 3 also WITH the reference's [B,Q,H,W] fp32 `masks` tensor written (4.1 GB per step at bs = 16, 800^2)
            ("infer_fai-mf-l-coco-ins_bs16_800_fullmasks", dict(train=False, model="fai-mf-l-coco-ins", family="fai_mf", batch=16, size=800, steps=6, warmup=2,
                                                               mf_full_masks=True)),
            ("infer_fai-mf-l-coco-ins_bs16_800_fullmasks_bf16", dict(train=False, model="fai-mf-l-coco-ins", family="fai_mf", batch=16, size=800, steps=6, warmup=2,
                                                                    mf_full_masks=True, mf_masks_dtype="bf16")),
            ("train_bisenetformer-l-ade_bs8_1024_bn_fp16", dict(train=True, model="bisenetformer-l-ade", family="bisenetformer", batch=8, size=1024,
                                                               norm="SyncBN" if world > 1 else "BN", steps=4, warmup=4, dtype="fp16"))]
    for name, over in plan:
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        try:
            r = train_measure(a, world, rank, local, with_roofline=False) if a.train else infer_measure(a, world, rank, local, light=True)
            if rank == 0:
                legs[name] = {k: r[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "alg_gflop_per_image",
                                                "frac_of_bf16_mfma_roofline_whole_path", "loss_scale", "final_total_loss") if k in r}
        except Exception as e:   # a failed leg must not take the headline with it
            if rank == 0:
                legs[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
            from focoos_amd import _lib as fxlib

            fxlib.set_compute_dtype("bf16")
    timer.cancel()


def infer_measure(args, world, rank, local, light=False):
    """One inference measurement (the bench contract's timed region); returns rank 0's dict.  The CPU baseline, the one-batch-in-flight
    steps and the per-kernel roofline table run under --full only, and never with ``light`` (the extra legs of the --full default run)."""
    import torch

    from focoos_amd.model import BisenetFormer, FAIDetr, FAIMaskFormer
    from focoos_amd.registry import ModelRegistry
    from focoos_amd.synth import synth_image

    dev = f"cuda:{local}"
    cfg = ModelRegistry.get_model_info(args.model)["config"]
    B = args.batch
    cpu = None
    extras = args.full and not light
    if rank == 0 and world == 1 and extras and not args.no_cpu_baseline:
        cpu = cpu_baseline(args)
    bf = args.family == "bisenetformer"
    mf = args.family == "fai_mf" or bf     # the two mask families share the engine interface (engine_maskdec.py)
    model = (BisenetFormer if bf else (FAIMaskFormer if mf else FAIDetr))(cfg, device=dev, seed=0)
    eng = model.engine
    if mf and getattr(args, "mf_masks_dtype", "fp32") != "fp32":
        eng.masks_dtype = args.mf_masks_dtype
    # image i of rank r = synth_image(r*B + i): seeded uint8 HWC, resident in HBM before the timed region
    imgs = torch.stack([torch.from_numpy(synth_image(rank * B + i, args.size, args.size)) for i in range(B)]).to(dev)
    sizes = torch.tensor([[args.size, args.size]] * B, dtype=torch.int32, device=dev)
    keys = ("det_scores", "det_labels", "det_boxes", "det_count") + (("det_query", "det_area") if mf else ())
    if mf and args.mf_masks_d2h:
        keys += ("mask_words",)
    # THROUGHPUT mode by default, all three families (engine.pipeline(): `depth` batches in flight, each a whole-batch plan on its own stream - batch
    # i+1's backbone beside batch i's decoder tail).  A step is still ONE batch through the whole path (D2D hand-over, graph replay, D2H of
    # the packed detections); the timed region is K such steps between two full synchronisations.  --pipeline 1 = one batch at a time
    # (engine.forward()'s form: two half-batch parts side by side), also measured below under --full and reported as `single_batch_in_flight`.
    depth = args.pipeline if args.pipeline is not None else int(os.environ.get("FX_PIPELINE_DEPTH", "3"))
    pipe = None
    if depth > 1:
        pipe = (eng.pipeline(B, args.size, args.size, depth, False, args.streams or 1, args.mf_full_masks) if mf
                else eng.pipeline(B, args.size, args.size, depth, False, args.streams or 1))
        depth = pipe.depth
    if pipe is not None and depth > 1:
        pl = pipe.lanes[0][0]
        hosts = [{k: torch.empty_like(getattr(p_, k), device="cpu").pin_memory() for k in keys} for p_, _ in pipe.lanes]

        def step():
            pipe.submit(imgs, sizes, 0.5, hosts[pipe.tickets % depth])

        def sync():
            pipe.synchronize()
    else:
        pl = eng.plan(B, args.size, args.size, False, args.mf_full_masks, args.streams) if mf else eng.plan(B, args.size, args.size, False, args.streams)
        host = {k: torch.empty_like(getattr(pl, k), device="cpu").pin_memory() for k in keys}
        st = eng.stream

        def step():
            with torch.cuda.stream(st):
                pl.input.copy_(imgs, non_blocking=True)       # device->device: hand the batch to the engine's input buffer
                pl.sizes.copy_(sizes, non_blocking=True)
                pl.run(st.cuda_stream, 0.5, None, True)
                for k, h in host.items():                      # D2H of the packed results (<= 300 x 6 per image; MaskFormer: <= 100 x 8)
                    h.copy_(getattr(pl, k), non_blocking=True)

        def sync():
            st.synchronize()

    for _ in range(max(args.warmup, depth, 1)):
        step()
    sync()
    barrier(world, False)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync()
    barrier(world, False)
    dt = max_over_ranks(time.perf_counter() - t0, world, False)
    ms_step = 1e3 * dt / args.steps
    if rank == 0 and not light and args.dump_outputs:
        # what a caller receives from the last timed step: the packed results copied to the host (the lane of the last ticket when pipelined)
        last = hosts[(pipe.tickets - 1) % depth] if (pipe is not None and depth > 1) else host
        dump_outputs(args.dump_outputs, last)
    value = world * B * args.steps / dt

    single = None
    if pipe is not None and depth > 1 and extras:
        # the same K steps with ONE batch in flight (engine.forward()'s structure: two half-batch parts side by side, next batch after the join)
        pl1 = eng.plan(B, args.size, args.size, False, args.mf_full_masks, None) if mf else eng.plan(B, args.size, args.size, False, None)
        host1 = {k: torch.empty_like(getattr(pl1, k), device="cpu").pin_memory() for k in keys}
        st1 = eng.stream

        def step1():
            with torch.cuda.stream(st1):
                pl1.input.copy_(imgs, non_blocking=True)
                pl1.sizes.copy_(sizes, non_blocking=True)
                pl1.run(st1.cuda_stream, 0.5, None, True)
                for k, h in host1.items():
                    h.copy_(getattr(pl1, k), non_blocking=True)

        for _ in range(max(args.warmup, 1)):
            step1()
        st1.synchronize()
        barrier(world, False)
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step1()
        st1.synchronize()
        barrier(world, False)
        dt1 = max_over_ranks(time.perf_counter() - t1, world, False)
        single = {"value": round(world * B * args.steps / dt1, 2), "ms_per_step": round(1e3 * dt1 / args.steps, 4),
                  "concurrent_batch_parts": getattr(pl1, "n", 1), "note": "one batch in flight: the next batch starts after the previous one's last kernel"}

    alg = ALG_GFLOP_PER_IMAGE_MF_800 * (args.size / 800.0) ** 2 if mf else ALG_GFLOP_PER_IMAGE * (args.size / 640.0) ** 2
    if bf:  # conv / linear layers of the reference as listed by the plan (the pooling / gate / attention-core flops are not counted)
        parts = getattr(pl, "parts", [pl])
        alg = sum(m["flops"] for part in parts for m in part.meta.values()) / B / 1e9
    out = {
        "metric": f"images/sec @ {args.size}^2 (infer bs={B})", "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"{args.model} inference, bf16 MFMA, bs={B}/GPU, {args.size}x{args.size}, random-init weights (seed 0), "
                               "uint8 HWC images resident in HBM, device post-process + D2H of packed detections included"
                               + ((", bit-packed binary masks of the detections " + ("copied D2H" if args.mf_masks_d2h else "left in HBM")
                                   + (f", [B,Q,H,W] {getattr(args, 'mf_masks_dtype', 'fp32')} masks tensor written" if args.mf_full_masks else ", [B,Q,H,W] fp32 masks tensor not materialised")) if mf else ""),
                   "global_batch": B * world, "parallelism": f"replicas x{world} (no data-path collective)", "steps_are": "hipGraph replays",
                   "batches_in_flight": depth, "concurrent_batch_parts": getattr(pl, "n", 1)},
        "alg_gflop_per_image": round(alg, 2),
        "frac_of_bf16_mfma_roofline_whole_path": round(value / world * alg * 1e9 / (PEAK_BF16_TFLOPS * 1e12), 4),
    }
    if single is not None:
        out["single_batch_in_flight"] = single
    if rank == 0 and extras:
        # ---- roofline of the dominant kernel (live, in-sequence HIP-event timing; world==1 or rank 0 only)
        ms = per_op_timing(eng, pl, args)
        by = {}
        for i, m in pl.meta.items():
            d = by.setdefault(m["variant"], {"ms": 0.0, "flops": 0.0, "flops_exec": 0.0, "bytes": 0.0, "launches": 0})
            d["ms"] += ms[i]
            d["flops"] += m["flops"]
            d["flops_exec"] += m.get("flops_executed", m["flops"])
            d["bytes"] += m.get("bytes", 0.0)
            d["launches"] += 1
        total_ms = sum(ms)
        name, d = max(by.items(), key=lambda kv: kv[1]["ms"])
        tflops = d["flops"] / (d["ms"] * 1e-3) / 1e12
        gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9
        # which roof bounds this kernel: arithmetic intensity of its launches (algorithmic flops / algorithmic bytes) against the
        # machine balance 2.5 PFLOP/s / 8 TB/s = 312 flop/byte - computed, not assumed
        ai = d["flops"] / max(d["bytes"], 1.0)
        bound = "mfma" if ai >= PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9) else "hbm"
        # HBM bytes per launch of that kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate
        # runs, gfx950 read-side x2 correction: scripts/pmc_summary.py); None when no PMC summary covers this kernel
        traffic, traffic_src = None, None
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_hbm_latest.json")))
            key = pmc_kernel_prefix(name)
            hits = [v for k, v in pmc.items() if key and k.replace(" ", "").startswith(key)]   # key: a prefix or a tuple of prefixes
            if hits:
                n_ = sum(v["launches"] for v in hits)
                traffic = round(sum((v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"]) * v["launches"] for v in hits) / n_)
                cal = pmc.get("__calibration__")
                traffic_src = ("profiles/pmc_hbm_latest.json (rocprofv3 --pmc FETCH_SIZE, WRITE_SIZE in separate passes; bytes per launch; "
                               + (f"counter units calibrated on known-byte kernels in the same passes: {cal['read_bytes_per_count']:.0f} B / FETCH count, "
                                  f"{cal['write_bytes_per_count']:.0f} B / WRITE count)" if cal else "read side x2 per the gfx950 note, write side uncalibrated)"))
        except Exception:
            pass
        achieved, peak, unit = (tflops, PEAK_BF16_TFLOPS, "TFLOP/s") if bound == "mfma" else (gbs, PEAK_HBM_GBS, "GB/s")
        out["roofline"] = {
            "bound": bound, "kernel": name, "achieved": round(achieved, 2), "peak": peak, "unit": unit, "frac": round(achieved / peak, 4),
            "traffic": traffic, "traffic_source": traffic_src, "launches_per_step": d["launches"],
            "arithmetic_intensity_flop_per_byte": round(ai, 1), "machine_balance_flop_per_byte": round(PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9), 1),
            # `frac` follows SURVEY 8(d)'s accounting (the reference's separate RepVGG 1x1 branch counted although the engine folds it into the
            # 3x3 filter); frac_executed = the MFMA work the kernel really executes (say both)
            "frac_executed": round((d["flops_exec"] / (d["ms"] * 1e-3) / 1e12 if bound == "mfma" else gbs) / peak, 4),
            "mfma": {"achieved_tflops": round(tflops, 2), "executed_tflops": round(d["flops_exec"] / (d["ms"] * 1e-3) / 1e12, 2), "peak_tflops": PEAK_BF16_TFLOPS,
                     "frac": round(tflops / PEAK_BF16_TFLOPS, 4)},
            "hbm": {"achieved_gbs_algorithmic": round(gbs, 1), "peak_gbs": PEAK_HBM_GBS, "frac": round(gbs / PEAK_HBM_GBS, 4),
                    "alg_bytes_per_launch": round(d["bytes"] / d["launches"])},
            "avg_launch_ms": round(d["ms"] / d["launches"], 5), "alg_gflop_per_launch": round(d["flops"] / d["launches"] / 1e9, 3),
            "share_of_step_time": round(d["ms"] / total_ms, 4),
            "all_conv_variants": {k: {"ms": round(v["ms"], 4), "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2),
                                      "alg_gbs": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1), "launches": v["launches"]}
                                  for k, v in sorted(by.items(), key=lambda kv: -kv[1]["ms"])},
            "sum_of_kernel_ms_per_step": round(total_ms, 4),
        }
        # Composite bound of THIS launch structure (SURVEY 8(d) "roofline bound" (ii)): every launch that carries an
        # algorithmic flop / byte count is charged max(flops / MFMA peak, bytes / HBM peak) at the datasheet peaks; the launches without one
        # (attention cores, deformable sampling, top-k, row chains, resizes: latency- / gather-bound, no closed form) are charged nothing, so the
        # bound is optimistic by their share, stated as `kernel_time_share_of_uncharged_launches`.  Progress is visible against BOTH ceilings:
        # `frac_of_bf16_mfma_roofline_whole_path` (pure MFMA) and `composite.frac` (bound / measured step).
        comp_s = sum(max(m["flops"] / (PEAK_BF16_TFLOPS * 1e12), m.get("bytes", 0.0) / (PEAK_HBM_GBS * 1e9)) for m in pl.meta.values())
        charged_ms = sum(ms[i] for i in pl.meta)
        out["composite_roofline"] = {
            "bound_ms_per_step": round(comp_s * 1e3, 4), "measured_ms_per_step": round(ms_step, 4), "frac": round(comp_s * 1e3 / ms_step, 4),
            "bound_images_per_s": round(B / comp_s, 1), "peaks": {"mfma_tflops": PEAK_BF16_TFLOPS, "hbm_gbs": PEAK_HBM_GBS},
            "mfma_bound_launches": sum(1 for m in pl.meta.values() if m["flops"] / (PEAK_BF16_TFLOPS * 1e12) >= m.get("bytes", 0.0) / (PEAK_HBM_GBS * 1e9)),
            "hbm_bound_launches": sum(1 for m in pl.meta.values() if m["flops"] / (PEAK_BF16_TFLOPS * 1e12) < m.get("bytes", 0.0) / (PEAK_HBM_GBS * 1e9)),
            "kernel_time_share_of_uncharged_launches": round(1.0 - charged_ms / max(total_ms, 1e-9), 4),
            "alg_bytes_per_step_of_charged_launches": round(sum(m.get("bytes", 0.0) for m in pl.meta.values())),
        }
        if cpu is not None:
            out["cpu_baseline"] = cpu
        if args.per_op:
            names = []
            for i, (fn, _) in enumerate(pl.ops):
                m = pl.meta.get(i)
                names.append((fn.__name__, m["variant"] + ":" + m["name"] + f" M={m['M']} N={m['N']} K={m['K']}" if m else "", ms[i],
                              (m["flops"] / (ms[i] * 1e-3) / 1e12) if m else 0.0))
            with open(args.per_op, "w") as f:
                for nm, desc, t, tf in names:
                    f.write(f"{t:9.4f} ms  {tf:8.1f} TF/s  {nm}  {desc}\n")
    barrier(world, False)
    pipe = step = sync = None     # the lanes' plans (8 GB each at bs = 32) go with the engine before the next leg allocates its own
    del pl, eng, model
    torch.cuda.empty_cache()
    return out if rank == 0 else None


if __name__ == "__main__":
    main()
