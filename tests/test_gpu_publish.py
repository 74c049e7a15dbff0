"""Device-side weight publish on a real MI355X.

Kernel: one fx_publish_weights_f32 table launch against the host packer of the engines (``_pack(*_fold_bn(...))`` / ``_pack_linear`` /
``_pack_frag``) on the same values - the row image, the fragment-order copy and the bias must be EQUAL (the fold is specified bit for bit:
fp64, every operation rounded on its own, then fp32, then bf16 nearest-even), the padding zero, the words around every destination
untouched.

Engines: ``publish_state_dict`` of seed-2 weights into an engine built (and run) with seed-1 weights leaves every packed buffer equal to
those of an engine built with seed 2, at the same addresses, with the same plan objects, and the two engines then compute the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd.engine import BN_EPS, DetrEngine, PackedConv, _EngineBase, _fold_bn, publish_table  # noqa: E402
from focoos_amd.engine_bf import BfEngine  # noqa: E402
from focoos_amd.engine_cls import ClsEngine  # noqa: E402
from focoos_amd.engine_mf import MfEngine  # noqa: E402
from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image_structured, synth_state_dict  # noqa: E402

DEV = "cuda:0"
GUARD = 64          # bytes before and after every destination
FILL = 0xA5

# (N, C, KH, with BatchNorm, with conv bias)
LAYERS = [
    (80, 64, 1, False, True),      # N below 128, conv bias: padding rows and padded bias entries zero
    (32, 16, 3, True, False),      # 3x3 with K = 144 = 9 * 16: the smallest shape a fragment copy can be cut from (N % 32 == 0, K % 16 == 0)
    (32, 32, 3, True, False),      # the smallest fragment-ELIGIBLE 3x3 (conv_frag_eligible: the stem's C = 32, N = 32)
    (256, 64, 3, True, False),     # with BN, fragment-eligible
    (365, 256, 1, False, True),    # N not a multiple of 32: no fragment copy; ragged last tile of 5 rows
    (96, 48, 3, True, False),      # C not a multiple of 64
]


class _HostPacker(_EngineBase):
    """The engines' packing helpers without an engine around them."""

    def __init__(self):
        self.dev = torch.device(DEV)
        self._pub, self._slots = None, None


def _layer(N, Cc, KH, bn, bias, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {"w": torch.randn(N, Cc, KH, KH, generator=g) * 0.1}
    if bn:
        sd.update({"bn.weight": torch.rand(N, generator=g) + 0.5, "bn.bias": torch.randn(N, generator=g) * 0.3,
                   "bn.running_mean": torch.randn(N, generator=g) * 0.2, "bn.running_var": torch.rand(N, generator=g) * 2 + 1e-3})
    if bias:
        sd["b"] = torch.randn(N, generator=g)
    return sd


def _guarded(numel, dtype):
    """(raw byte buffer filled with FILL, typed view of ``numel`` elements GUARD bytes into it)"""
    nbytes = numel * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes].view(dtype)


def _guards_intact(raw):
    return bool((raw[:GUARD] == FILL).all()) and bool((raw[-GUARD:] == FILL).all())


@pytest.fixture(scope="module")
def packed_reference():
    """Host-packed images of LAYERS, computed once and shared."""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    hp = _HostPacker()
    out = []
    for i, (N, Cc, KH, bn, bias) in enumerate(LAYERS):
        sd = _layer(N, Cc, KH, bn, bias, 100 + i)
        pc = hp._pack(*_fold_bn(sd, "w", "bn")) if bn else hp._pack(sd["w"], sd.get("b"))
        wf = pc.wf
        if wf is None and N % 32 == 0 and (KH * KH * Cc) % 16 == 0:
            w, _ = _fold_bn(sd, "w", "bn") if bn else (sd["w"], None)
            wf = hp._pack_frag(w.permute(0, 2, 3, 1).reshape(N, KH * KH * Cc))
        out.append((sd, pc, wf))
    return out


def _publish(cases):
    """One table launch over ``cases`` ((sd, pc, wf) of packed_reference) into guarded destinations; returns them."""
    entries, dests = [], []
    for (N, Cc, KH, bn, bias), (sd, pc, wf) in cases:
        sdd = {k: v.to(DEV) for k, v in sd.items()}
        Np = pc.w.shape[0]
        r_rows, rows = _guarded(pc.w.numel(), torch.bfloat16)
        r_bias, b_out = _guarded(Np, torch.float32)
        r_frag, frag = _guarded(wf.numel(), torch.bfloat16) if wf is not None else (None, None)
        bnv = tuple(sdd[f"bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")) if bn else None
        entries.append((sdd["w"], bnv, sdd.get("b"), rows, frag, b_out, Np))
        dests.append((r_rows, rows, r_bias, b_out, r_frag, frag))
    publish_table(entries, torch.device(DEV))
    torch.cuda.synchronize()
    return dests


def _check(cases, dests):
    for (shape, (sd, pc, wf)), (r_rows, rows, r_bias, b_out, r_frag, frag) in zip(cases, dests):
        N = shape[0]
        assert torch.equal(rows.view_as(pc.w), pc.w), shape
        assert torch.equal(b_out, pc.b), shape
        assert not rows.view_as(pc.w)[N:].any() and not b_out[N:].any(), shape       # padding written as zeros over the 0xA5 fill
        assert _guards_intact(r_rows) and _guards_intact(r_bias), shape
        if wf is not None:
            assert torch.equal(frag.view_as(wf), wf), shape
            assert _guards_intact(r_frag), shape


def test_publish_kernel_one_launch_all_layers(packed_reference):
    """All six layers in ONE launch: different sizes, so every workgroup has to find its entry in the table."""
    cases = list(zip(LAYERS, packed_reference))
    assert packed_reference[2][1].wf is not None and packed_reference[3][1].wf is not None and packed_reference[4][1].wf is None
    _check(cases, _publish(cases))


@pytest.mark.parametrize("pair", [(0, 3), (4, 1), (5, 2)])
def test_publish_kernel_pairs(packed_reference, pair):
    """Two layers of different sizes per launch, in both size orders."""
    cases = [(LAYERS[i], packed_reference[i]) for i in pair]
    _check(cases, _publish(cases))


def test_publish_kernel_rounds_twice_like_the_host():
    """fp64 -> fp32 -> bf16 are TWO roundings on the host; a kernel that converts the fp64 product to bf16 in one step differs where the fp32
    value is an exact bf16 tie (one weight in ~65 000).  bisenetformer-l-ade's features.1 with the seed-2 synthetic weights has such an element."""
    cfg = ModelRegistry.get_model_info("bisenetformer-l-ade")["config"]
    full = synth_state_dict(cfg, 2, family="bisenetformer")
    n = "pixel_decoder.backbone.features.1"
    sd = {"w": full[f"{n}.conv.weight"], **{f"bn.{k}": full[f"{n}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")}}
    w32, _ = _fold_bn(sd, "w", "bn")
    ties = int(((w32.view(torch.int32) & 0xFFFF) == 0x8000).sum())
    assert ties >= 1, "the case lost its tie: pick another layer"
    N, Cc = sd["w"].shape[:2]
    pc = _HostPacker()._pack(w32, _fold_bn(sd, "w", "bn")[1])
    cases = [((N, Cc, 3, True, False), (sd, pc, pc.wf))]
    _check(cases, _publish(cases))


def test_publish_table_refuses_misfit():
    w = torch.zeros(64, 32, 1, 1, device=DEV)
    rows = torch.zeros(128 * 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.FocoosAmdError):
        publish_table([(w, None, None, rows[:-8], None, None, 128)], torch.device(DEV))
    with pytest.raises(_lib.FocoosAmdError):     # a fragment copy needs K % 16 == 0 and exactly N * K elements
        publish_table([(w, None, None, rows, rows[:64 * 32 - 8], None, 128)], torch.device(DEV))
    with pytest.raises(_lib.FocoosAmdError):
        publish_table([(w.cpu(), None, None, rows, None, None, 128)], torch.device(DEV))


# ------------------------------------------------------------------------------------------------ engines
def _tensors(obj, path, out, seen):
    """Every device tensor reachable from an engine's attributes (dicts, tuples, lists, PackedConv), keyed by its path."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            out[path] = obj
    elif isinstance(obj, PackedConv):
        for f in ("w", "b", "wf"):
            _tensors(getattr(obj, f), f"{path}.{f}", out, seen)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _tensors(v, f"{path}[{k!r}]", out, seen)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _tensors(v, f"{path}[{i}]", out, seen)


def engine_buffers(eng):
    out = {}
    for name, v in vars(eng).items():
        if name not in ("plans", "_slots", "_pub", "lib"):
            _tensors(v, name, out, None)
    return out


# B = 2 at the smallest size each engine plans: the mask families at 96 x 128; RT-DETR needs at least as many encoder tokens as queries
# (300), which 128 x 128 is the first square multiple of 32 to give (256 + 64 + 16)
ENGINES = [
    ("fai-detr-l-coco", "fai_detr", DetrEngine, (128, 128), ("probs", "boxes")),
    ("fai-detr-m-coco", "fai_detr", DetrEngine, (128, 128), ("probs", "boxes")),
    ("bisenetformer-l-ade", "bisenetformer", BfEngine, (96, 128), ("probs", "mask_probs")),
    ("fai-mf-l-coco-ins", "fai_mf", MfEngine, (96, 128), ("probs", "mask_probs")),
    ("fai-cls-n-coco", "fai_cls", ClsEngine, (64, 96), ("logits",)),   # STDC-nano: the 16-channel fragment images and their stem
    ("fai-cls-m-coco", "fai_cls", ClsEngine, (64, 96), ("logits",)),   # STDC base 64
]


@pytest.mark.parametrize("variant,family,cls,size,outs", ENGINES, ids=[e[0] for e in ENGINES])
def test_engine_publish_matches_load(variant, family, cls, size, outs):
    cfg = ModelRegistry.get_model_info(variant)["config"]
    sd1, sd2 = synth_state_dict(cfg, 1, family=family), synth_state_dict(cfg, 2, family=family)
    H, W = size
    x = torch.stack([torch.from_numpy(synth_image_structured(i, H, W)) for i in range(2)]).contiguous().to(DEV)
    A = cls(cfg, sd1, device=DEV)
    A.forward(x)
    torch.cuda.synchronize()
    plans = dict(A.plans)
    assert plans
    before = engine_buffers(A)
    ptrs = {k: v.data_ptr() for k, v in before.items()}
    old = {k: v.clone() for k, v in before.items()}

    # a wrong-shaped tensor, a missing key and a host tensor are refused before anything is written
    dev2 = {k: v.to(DEV) for k, v in sd2.items()}
    key = next(k for k, v in dev2.items() if v.dim() == 4)
    for bad in (dict(dev2, **{key: dev2[key][:, :-1].contiguous()}), {k: v for k, v in dev2.items() if k != key}, dict(dev2, **{key: sd2[key]})):
        with pytest.raises(_lib.FocoosAmdError):
            A.publish_state_dict(bad)
    torch.cuda.synchronize()
    assert all(torch.equal(v, old[k]) for k, v in engine_buffers(A).items())

    A.publish_state_dict(dev2)
    torch.cuda.synchronize()
    B = cls(cfg, sd2, device=DEV)
    bufA, bufB = engine_buffers(A), engine_buffers(B)
    assert set(bufA) == set(bufB) == set(before)
    assert {k: v.data_ptr() for k, v in bufA.items()} == ptrs                          # same addresses
    differ = [k for k in bufA if not torch.equal(bufA[k], bufB[k])]
    assert not differ, (len(differ), differ[:8])
    assert sum(not torch.equal(bufA[k], old[k]) for k in bufA) > len(bufA) // 2         # ... and the values did move
    assert set(A.plans) == set(plans) and all(A.plans[k] is plans[k] for k in plans)  # no plan cleared or rebuilt

    pa = A.forward(x)
    torch.cuda.synchronize()
    assert any(pa is p for p in plans.values())
    got = [getattr(pa, o).clone() for o in outs]
    pb = B.forward(x)
    torch.cuda.synchronize()
    for o, a in zip(outs, got):
        assert torch.equal(a, getattr(pb, o)), o
