"""Oracle parity of the BASELINE.json configurations THEMSELVES, run as `bench.py --pipeline 1` runs them (VERDICT r3 "weak #1"):
full batch, production kernel routing (no `flat_small_shapes`: a layer's kernel is chosen by M = B*H*W, so bs=2 tests do not
exercise the `conv3x3_kplane<256>` / `pw_kplane` instances that carry the benchmark), two concurrent batch parts, hipGraph
replay (bench.py's default throughput mode, three whole-batch lanes, is tests/test_gpu_whole_batch.py), bench.py's own weights (seed 0) and images (`synth_image(i)`).

What is compared: a sample of images (first / last image of each batch part) against the CPU fp32 oracle with the
discontinuous selections teacher-forced FROM the engine (RT-DETR: the engine's own top-300 query set is handed to the oracle;
mask families: the engine's own attention bitmaps), so every stage and the final outputs are checked with the same gates as the
small-batch tests (tests/test_gpu_e2e.py::test_stage_parity_teacher_forced, test_gpu_mf.py, test_gpu_bf.py); the free-running
selection itself is checked through the encoder scores (RT-DETR) within TOL_SCORE.  Each test prints the kernel variants the
library routed to (`fx_conv2d_variant`, recorded in plan.meta) so that the log shows which instances ran under the oracle.

Reference: FAIDetr.forward fai_detr/modelling.py:1344-1358, DETRProcessor.postprocess fai_detr/processor.py:146-217,
FAIMaskFormer.forward fai_mf/modelling.py:712-725, BisenetFormer.forward bisenetformer/modelling.py:594-609.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image, synth_state_dict  # noqa: E402
from oracle import bf_oracle as BFO  # noqa: E402
from oracle import detr_oracle as O  # noqa: E402
from oracle import mf_oracle as M  # noqa: E402
from tests.helpers import attn_from_bits, detr_image_check, mask_family_check, plan_variants  # noqa: E402
from tests.test_gpu_e2e import TOL_BOX, TOL_PROB, TOL_SCORE  # noqa: E402

DEV = "cuda:0"


def _bench_step(eng, pl, imgs, thr, replays=2):
    """bench.py's step (infer_measure.step): device->device copy into the plan's input, graph replay on the engine's stream."""
    st = eng.stream
    sizes = torch.tensor([[imgs.shape[1], imgs.shape[2]]] * imgs.shape[0], dtype=torch.int32, device=DEV)
    for _ in range(replays):   # the first call captures (after its eager warm-up), the later ones are pure replays
        with torch.cuda.stream(st):
            pl.input.copy_(imgs, non_blocking=True)
            if hasattr(pl, "sizes"):
                pl.sizes.copy_(sizes, non_blocking=True)
            pl.run(st.cuda_stream, thr, None, True)
    st.synchronize()


_variants = plan_variants


def test_config1_detr_bs32_production_path_vs_oracle():
    """BASELINE configs[1]: fai-detr-l-obj365, bs=32, 640x640 - the step the driver times."""
    from focoos_amd.model import FAIDetr

    cfg = ModelRegistry.get_model_info("fai-detr-l-obj365")["config"]
    sd = synth_state_dict(cfg, 0)
    model = FAIDetr(cfg, device=DEV, seed=0)
    eng = model.engine
    B = 32
    images = [synth_image(i, 640, 640) for i in range(B)]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    pl = eng.plan(B, 640, 640, False)
    assert getattr(pl, "n", 1) == 2 and pl.parts[0].B == 16, "bench.py --pipeline 1 step = two concurrent 16-image parts"
    _bench_step(eng, pl, x, 0.5)
    assert isinstance(pl.graph, list) and len(pl.graph) == 2, "the --pipeline 1 parts must have been replayed as hipGraphs"
    var = _variants(pl)
    print("kernel variants under the oracle (launches per step):", dict(sorted(var.items(), key=lambda kv: -kv[1])))
    assert var.get("conv3x3_kplane<256>", 0) >= 30 and any(k.startswith("pw_kplane") for k in var) and any(k.startswith("pw_chain") for k in var)

    sample = [0, 15, 16, 31]
    topk = pl.enc_topk.cpu().long()
    col = {}
    with torch.no_grad():
        xo = O.get_torch_batch([images[i] for i in sample], (640, 640))
        probs_o, boxes_o = O.detr_forward(sd, cfg, xo, forced_topk=topk[sample], collect=col)
    worst = {}
    for j, b in enumerate(sample):
        detr_image_check(pl, b, j, col, probs_o, boxes_o, worst, TOL_SCORE, TOL_PROB, TOL_BOX)
    print("bs=32 production path vs oracle, worst over images", sample, ":", {k: round(v, 5) for k, v in worst.items()})


def test_config2_maskformer_bs16_800_production_path_vs_oracle():
    """BASELINE configs[2]: fai-mf-l-coco-ins, bs=16, 800x800 (bench.py --model fai-mf-l-coco-ins / the default line's other_configs leg)."""
    from focoos_amd.model import FAIMaskFormer

    cfg = ModelRegistry.get_model_info("fai-mf-l-coco-ins")["config"]
    sd = synth_state_dict(cfg, 0, family="fai_mf")
    model = FAIMaskFormer(cfg, device=DEV, seed=0)
    eng = model.engine
    B, S = 16, 800
    images = [synth_image(i, S, S) for i in range(B)]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    pl = eng.plan(B, S, S, False, False, None)
    assert getattr(pl, "n", 1) == 2 and pl.parts[0].B == 8, "bench.py --pipeline 1 step = two concurrent 8-image parts"
    _bench_step(eng, pl, x, 0.5)
    assert isinstance(pl.graph, list) and len(pl.graph) == 2
    print("kernel variants under the oracle (launches per step):", dict(sorted(_variants(pl).items(), key=lambda kv: -kv[1])))
    worst = {}
    sample = [0, 15]
    for j, b in enumerate(sample):
        forced = attn_from_bits(pl, b, eng.nq, eng.nl)
        col = {}
        with torch.no_grad():
            probs_o, _ = M.mf_forward(sd, cfg, O.get_torch_batch([images[b]], None), forced_attn=forced, collect=col, upsample=False)
        mask_family_check(pl, b, j, cfg, col, probs_o, ("res2", "res5", "msf0", "msf1", "msf2", "fpn_s4", "mask_features"), eng.nl, worst)
    print("MaskFormer bs=16 800^2 production path vs oracle, worst over images", sample, ":", {k: round(v, 5) for k, v in worst.items()})


def test_config5_bisenetformer_bs8_1024_production_path_vs_oracle():
    """The model and size of BASELINE configs[4] (bisenetformer-l-ade, 1024x1024, bs=8), inference path of the production engine."""
    from focoos_amd.model import BisenetFormer

    cfg = ModelRegistry.get_model_info("bisenetformer-l-ade")["config"]
    sd = synth_state_dict(cfg, 0, family="bisenetformer")
    model = BisenetFormer(cfg, device=DEV, seed=0)
    eng = model.engine
    B, S = 8, 1024
    images = [synth_image(i, S, S) for i in range(B)]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    pl = eng.plan(B, S, S, False, False, None)
    assert getattr(pl, "n", 1) == 2 and pl.parts[0].B == 4, "bench.py --pipeline 1 step = two concurrent 4-image parts"
    _bench_step(eng, pl, x, 0.5)
    assert isinstance(pl.graph, list) and len(pl.graph) == 2
    print("kernel variants under the oracle (launches per step):", dict(sorted(_variants(pl).items(), key=lambda kv: -kv[1])))
    worst = {}
    sample = [0, 7]
    for j, b in enumerate(sample):
        forced = attn_from_bits(pl, b, eng.nq, eng.nl)
        col = {}
        with torch.no_grad():
            probs_o, _ = BFO.bf_forward(sd, cfg, O.get_torch_batch([images[b]], None), forced_attn=forced, collect=col, upsample=False)
        mask_family_check(pl, b, j, cfg, col, probs_o, ("res2", "res3", "res4", "res5", "cp32", "cp16", "cp8", "ffm", "mask_features"), eng.nl, worst)
    print("BiSeNetFormer bs=8 1024^2 production path vs oracle, worst over images", sample, ":", {k: round(v, 5) for k, v in worst.items()})


def test_bisenetformer_bs32_640_production_path_vs_oracle():
    """BiSeNetFormer-L inference exactly as `bench.py --model bisenetformer-l-ade` (and the `other_configs` leg of the default run) times it:
    bs=32 at 640x640, two concurrent 16-image parts, hipGraph replay - the shape at which the masked decoder runs as fx_row_chain programs
    (1 600 rows per part; engine_maskdec._masked_decoder_row_chains).  Images 0 and 31 against the oracle, attention masks from the engine."""
    from focoos_amd.model import BisenetFormer

    cfg = ModelRegistry.get_model_info("bisenetformer-l-ade")["config"]
    sd = synth_state_dict(cfg, 0, family="bisenetformer")
    model = BisenetFormer(cfg, device=DEV, seed=0)
    eng = model.engine
    B, S = 32, 640
    images = [synth_image(i, S, S) for i in range(B)]
    x = torch.from_numpy(np.stack(images)).to(DEV)
    pl = eng.plan(B, S, S, False, False, None)
    assert getattr(pl, "n", 1) == 2 and pl.parts[0].B == 16, "bench.py --pipeline 1 step = two concurrent 16-image parts"
    _bench_step(eng, pl, x, 0.5)
    var = _variants(pl)
    print("kernel variants under the oracle (launches per step):", dict(sorted(var.items(), key=lambda kv: -kv[1])))
    assert var.get("row_chain", 0) == 2 * (2 * eng.nl + 1)
    worst = {}
    sample = [0, 31]
    for j, b in enumerate(sample):
        forced = attn_from_bits(pl, b, eng.nq, eng.nl)
        col = {}
        with torch.no_grad():
            probs_o, _ = BFO.bf_forward(sd, cfg, O.get_torch_batch([images[b]], None), forced_attn=forced, collect=col, upsample=False)
        mask_family_check(pl, b, j, cfg, col, probs_o, ("res2", "res3", "res4", "res5", "cp32", "cp16", "cp8", "ffm", "mask_features"), eng.nl, worst)
    print("BiSeNetFormer bs=32 640^2 production path vs oracle, worst over images", sample, ":", {k: round(v, 5) for k, v in worst.items()})
