"""bench.py's timed throughput mode against the oracle, and every conv launch of it against fp64.

bench.py times `engine.pipeline(B, S, S, 3, False, 1)` (three lanes, each a whole-batch plan on its own stream): the headline
fai-detr-l-obj365 bs 32 640^2, and the fai-mf-l-coco-ins bs 16 800^2 and bisenetformer-l-ade bs 32 640^2 legs.  Kernel routing depends on
M = B*H*W, and some instances run only at whole-batch M (the two-workgroup conv3x3_kplane forms from FX_C3K_DUO256_MIN_M, pw_kplane with
one workgroup walking every n-tile), so the half-batch parts of tests/test_gpu_baseline_configs.py never reach them.

1. Three DIFFERENT batches, one per lane, each lane replayed as its hipGraph; sampled images of every lane against the CPU fp32 oracle with
   the discontinuous selections teacher-forced from the engine, same gates as the two-part tests.
2. Routing census: every fx_conv2d_nhwc_bf16 / fx_pw_chain_bf16 launch of the lane plans, grouped into classes by routing label, shape,
   epilogue, leading dimensions and channel offsets.  The RT-DETR census must contain the whole-batch-only forms.
3. Every class launched stand-alone at its production shape (production routing: no FX_* variable is set anywhere in this file - fx_tune
   caches values in function statics, so one set here would reroute every later test of the process) with seeded position-dependent
   operands, output buffer pre-filled with NaN, against an fp64 reference of images 0, B/2 and B-1 under the per-element ulp / RNE
   agreement gate of tests/helpers.py, and nothing written outside the contracted output.
"""
import ctypes as C
import gc
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FxConvDesc, FxPwChainDesc, check  # noqa: E402
from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image, synth_state_dict  # noqa: E402
from oracle import bf_oracle as BFO  # noqa: E402
from oracle import detr_oracle as O  # noqa: E402
from oracle import mf_oracle as M  # noqa: E402
from tests.helpers import (ULP_GATE_AGREE, ULP_GATE_C, act64, attn_from_bits, bf16_rne, conv_ref64, detr_image_check, gemm_ref64,  # noqa: E402
                           mask_family_check, ulp_stats)
from tests.test_gpu_e2e import TOL_BOX, TOL_PROB, TOL_SCORE  # noqa: E402
from tests.test_gpu_kernels import frag_pack, pack_w  # noqa: E402

DEV = "cuda:0"
DEPTH = 3
CONFIGS = [("fai-detr-l-obj365", 32, 640), ("fai-mf-l-coco-ins", 16, 800), ("bisenetformer-l-ade", 32, 640)]
MF_STAGES = ("res2", "res5", "msf0", "msf1", "msf2", "fpn_s4", "mask_features")
BF_STAGES = ("res2", "res3", "res4", "res5", "cp32", "cp16", "cp8", "ffm", "mask_features")
ACT_NAME = {0: None, 1: "relu", 2: "silu", 3: "gelu"}

# Whole-batch-only routing, from the kernels' own constants (production defaults):
#   conv3x3_kplane.hip: FX_C3K_DUO256_MIN_M = 40 000 - N % 256 == 0 layers from this M on run the two-workgroup "duo256" forms, with and
#   without the LDS residual tile (FX_C3K_DUO256_RES = 1).
#   conv_pw_kplane.hip launch_pwk: BM = 128 pixel rows (TM = 4), want = FX_PWK_TARGET_WGS = 512 workgroups for K = 256 (256 for K = 512);
#   groups == 1 (one workgroup walks every n-tile, rotated) iff mt = ceil(M / 128) >= want * 3 / 4.
C3K_DUO256_MIN_M = 40000
PWK_BM, PWK_TARGET_WGS = 128, 512

_CENSUS = {}


def _family(name):
    from focoos_amd.model import BisenetFormer, FAIDetr, FAIMaskFormer

    cfg = ModelRegistry.get_model_info(name)["config"]
    if name.startswith("fai-detr"):
        return cfg, FAIDetr, "fai_detr"
    if name.startswith("fai-mf"):
        return cfg, FAIMaskFormer, "fai_mf"
    return cfg, BisenetFormer, "bisenetformer"


def _pipeline(eng, fam, B, S):
    """bench.py:683-684 with its defaults: depth 3, nsplit 1, uint8 input (and no full-resolution masks)."""
    if fam == "fai_detr":
        return eng.pipeline(B, S, S, DEPTH, False, 1)
    return eng.pipeline(B, S, S, DEPTH, False, 1, False)


def _release():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------- census
def _spans(pl):
    out = []
    for v in list(pl.bufs.values()) + [v for v in vars(pl).values() if torch.is_tensor(v)]:
        t = v if torch.is_tensor(v) else v.t
        if t.is_cuda and t.numel():
            out.append((t.data_ptr(), t.numel() * t.element_size()))
    return out


def _elem_off(spans, ptr, esize):
    """Element offset of `ptr` inside the plan buffer holding it (None: not a plan buffer)."""
    if not ptr:
        return None
    for base, n in spans:
        if base <= ptr < base + n:
            return (ptr - base) // esize
    return None


def _coff(spans, ptr, ld, esize):
    e = _elem_off(spans, ptr, esize)
    return 0 if e is None else e % ld


def census(pl):
    """{class key: {"n": launches, "names": [...], "desc": dict}} of the conv launches of one plan."""
    spans = _spans(pl)
    out = {}
    for i, (fn, args) in enumerate(pl.ops):
        fname = getattr(fn, "__name__", "")
        if fname not in ("fx_conv2d_nhwc_bf16", "fx_pw_chain_bf16"):
            continue
        m = pl.meta[i]
        d = args[0]._obj
        if fname == "fx_conv2d_nhwc_bf16":
            ye = 4 if d.out_f32 else 2
            res = bool(d.residual)
            k = dict(kind="conv", label=m["variant"], KH=d.KH, KW=d.KW, stride=d.stride, pad=d.pad, C=d.C, N=d.N, H=d.H, W=d.W, Ho=d.Ho, Wo=d.Wo,
                     B=d.B, act=d.act, res=res, res_after=int(d.residual_after_act) if res else 0, out_f32=int(d.out_f32), ybs=int(d.y_batch_stride) != 0,
                     ldx=d.ldx, ldy=d.ldy, ldr=d.ldr if res else 0, xoff=_coff(spans, d.x, d.ldx, 2), yoff=_coff(spans, d.y, d.ldy, ye),
                     roff=_coff(spans, d.residual, d.ldr, 2) if res else 0, pool2=int(d.pool2), frag=bool(d.w_frag),
                     ybs_val=int(d.y_batch_stride),
                     ystart=((_elem_off(spans, d.y, ye) or 0) // d.ldy) % max(1, int(d.y_batch_stride) // d.ldy) if d.y_batch_stride else 0)
        else:
            k = dict(kind="pw_chain", label=m["variant"], M=d.M, B=pl.B, K1a=d.K1a, K1b=d.K1b, N1=d.N1, N2=d.N2, ldx1=d.ldx1, ldx2=d.ldx2,
                     ldr=d.ldr, ldy1=d.ldy1, ldy2=d.ldy2, act1=d.act1, act2=d.act2, res=bool(d.residual), y1=bool(d.y1), pool=bool(d.pool),
                     ldp=d.ldp, img_h=d.img_h, img_w=d.img_w, x1off=_coff(spans, d.x1, d.ldx1, 2),
                     x2off=_coff(spans, d.x2, d.ldx2, 2) if d.x2 else 0, roff=_coff(spans, d.residual, d.ldr, 2) if d.residual else 0,
                     y1off=_coff(spans, d.y1, d.ldy1, 2) if d.y1 else 0, y2off=_coff(spans, d.y2, d.ldy2, 2) if d.y2 else 0,
                     poff=_coff(spans, d.pool, d.ldp, 2) if d.pool else 0)
        key = tuple(sorted(k.items()))   # every field the replay uses is in the key: launches that differ in any of them are separate classes
        e = out.setdefault(key, {"n": 0, "names": [], "desc": k})
        e["n"] += 1
        e["names"].append(m.get("name", "?"))
    return out


def _cls_m(k):
    return k["M"] if k["kind"] == "pw_chain" else k["B"] * k["Ho"] * k["Wo"]


def _fmt(k):
    if k["kind"] == "pw_chain":
        return (f"{k['label']:<28} M={k['M']:>7} K={k['K1a']}+{k['K1b']} N1={k['N1']} N2={k['N2']} res={int(k['res'])} y1={int(k['y1'])} "
                f"pool={int(k['pool'])} ld=({k['ldx1']},{k['ldr']},{k['ldy1']},{k['ldy2']})")
    return (f"{k['label']:<28} {k['KH']}x{k['KW']}/s{k['stride']} C={k['C']:>4} N={k['N']:>4} {k['B']}x{k['H']}x{k['W']} M={_cls_m(k):>7} "
            f"act={ACT_NAME[k['act']]} res={int(k['res'])}{'a' if k['res_after'] else ''} f32={k['out_f32']} ybs={int(k['ybs'])} "
            f"ld=({k['ldx']},{k['ldy']},{k['ldr']}) off=({k['xoff']},{k['yoff']},{k['roff']}) pool2={k['pool2']}")


def print_census(name, cen):
    print(f"\n{name}: {len(cen)} conv launch classes, {sum(e['n'] for e in cen.values())} launches per lane")
    for e in sorted(cen.values(), key=lambda e: (e["desc"]["label"], -_cls_m(e["desc"]))):
        print(f"  {e['n']:>3} x {_fmt(e['desc'])}   [{e['names'][0]}]")


def assert_whole_batch_forms(cen):
    """The RT-DETR headline's whole-batch-only instances are present in the census."""
    ks = [e["desc"] for e in cen.values()]
    duo = [k for k in ks if k["kind"] == "conv" and k["label"].startswith("conv3x3_kplane<") and k["N"] % 256 == 0 and _cls_m(k) >= C3K_DUO256_MIN_M]
    assert any(k["res"] for k in duo) and any(not k["res"] for k in duo), "no duo256 conv3x3_kplane class with and without a residual"
    pwk1 = [k for k in ks if k["kind"] == "conv" and k["label"] == "pw_kplane<K256>" and k["N"] >= 512
            and -(-_cls_m(k) // PWK_BM) >= PWK_TARGET_WGS * 3 // 4]
    assert pwk1, "no pw_kplane K = 256, N >= 512 class in the groups == 1 regime"


# ----------------------------------------------------------------------------------------------------------------- part 1 (+ census)
@pytest.mark.parametrize("name,B,S", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_throughput_lanes_vs_oracle(name, B, S):
    cfg, cls, fam = _family(name)
    sd = synth_state_dict(cfg, 0, **({} if fam == "fai_detr" else {"family": fam}))
    model = cls(cfg, device=DEV, seed=0)
    eng = model.engine
    pipe = _pipeline(eng, fam, B, S)
    assert pipe.depth == DEPTH and len(pipe.lanes) == DEPTH
    sizes = torch.tensor([[S, S]] * B, dtype=torch.int32, device=DEV)
    images = [[synth_image(j * B + i, S, S) for i in range(B)] for j in range(DEPTH)]   # three different batches, one per lane
    batches = [torch.from_numpy(np.stack(im)).to(DEV) for im in images]
    # as bench.py's step: submit without waiting, so the three whole-batch lanes run side by side on their streams.  The first round
    # captures each lane's graph; the second replays all three concurrently and is the one compared below.
    for rnd in range(2):
        tickets = [pipe.submit(batches[j], sizes, 0.5) for j in range(DEPTH)]
    lanes = [pipe.wait(t) for t in tickets]
    pipe.synchronize()
    for j, pl in enumerate(lanes):
        assert pl is pipe.lanes[j][0], "ticket j must run on lane j"
        assert getattr(pl, "parts", None) is None and pl.B == B and (pl.H, pl.W) == (S, S), "each lane is ONE plan of the whole batch"
        assert pl.graph is not None and not isinstance(pl.graph, list) and pl.graph_thr == 0.5, "each lane must have been replayed as a hipGraph"
    assert len({pl.input.data_ptr() for pl in lanes}) == DEPTH and len({pl.probs.data_ptr() for pl in lanes}) == DEPTH, "own buffers per lane"
    assert len({id(st) for _, st in pipe.lanes}) == DEPTH, "own stream per lane"
    assert not torch.equal(lanes[0].probs, lanes[1].probs), "the lanes ran different batches"

    # sampled images: 0, B/2, B-1 of lane 0 and the last image of lanes 1 and 2
    sample = [(0, 0), (0, B // 2), (0, B - 1), (1, B - 1), (2, B - 1)]
    worst = {}
    if fam == "fai_detr":
        topk = torch.stack([lanes[j].enc_topk[b].cpu().long() for j, b in sample])
        col = {}
        with torch.no_grad():
            xo = O.get_torch_batch([images[j][b] for j, b in sample], (S, S))
            probs_o, boxes_o = O.detr_forward(sd, cfg, xo, forced_topk=topk, collect=col)
        for i, (j, b) in enumerate(sample):
            detr_image_check(lanes[j], b, i, col, probs_o, boxes_o, worst, TOL_SCORE, TOL_PROB, TOL_BOX)
    else:
        fwd, stages = (M.mf_forward, MF_STAGES) if fam == "fai_mf" else (BFO.bf_forward, BF_STAGES)
        for j, b in sample:
            forced = attn_from_bits(lanes[j], b, eng.nq, eng.nl)
            col = {}
            with torch.no_grad():
                probs_o, _ = fwd(sd, cfg, O.get_torch_batch([images[j][b]], None), forced_attn=forced, collect=col, upsample=False)
            mask_family_check(lanes[j], b, 0, cfg, col, probs_o, stages, eng.nl, worst)
    print(f"\n{name} bs={B} {S}^2 throughput lanes vs oracle, worst over (lane, image) {sample}:", {k: round(v, 5) for k, v in worst.items()})

    # part 2: routing census of every lane (the lanes are the same plan over their own buffers)
    cens = [census(pl) for pl in lanes]
    assert all(set(c) == set(cens[0]) for c in cens), "the lanes must launch the same conv classes"
    assert cens[0], "no conv launches found"
    _CENSUS[name] = cens[0]
    print_census(f"{name} bs={B} {S}^2", cens[0])
    if fam == "fai_detr":
        assert_whole_batch_forms(cens[0])
    if fam == "bisenetformer":
        var = [m["variant"] for m in lanes[0].meta.values()]
        assert var.count("row_chain") == 2 * eng.nl + 1, "the masked decoder runs as row_chain programs on the whole batch"
    del lanes, pl, pipe, eng, model, batches
    _release()


# ----------------------------------------------------------------------------------------------------------------- part 3
def _census_of(name, B, S):
    if name not in _CENSUS:     # this test alone (-k): build the lane plan without running it
        cfg, cls, fam = _family(name)
        model = cls(cfg, device=DEV, seed=0)
        pipe = _pipeline(model.engine, fam, B, S)
        _CENSUS[name] = census(pipe.lanes[0][0])
        print_census(f"{name} bs={B} {S}^2", _CENSUS[name])
        del pipe, model
        _release()
    return _CENSUS[name]


def _lin(n, lo, hi):
    return torch.linspace(lo, hi, n, device=DEV)


def _strided(rows, ld, off, cols, fill, dtype=torch.bfloat16):
    """A [rows, ld] buffer (+ slack) filled with `fill` and its [rows, cols] view at channel offset `off`."""
    buf = torch.full((rows * ld + off + 64,), fill, dtype=dtype, device=DEV)
    return buf, torch.as_strided(buf, (rows, cols), (ld, 1), off)


def _outside_untouched(buf, view):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    torch.as_strided(inside, view.shape, view.stride(), view.storage_offset()).fill_(True)
    return bool(torch.isnan(buf.float()[~inside]).all())


def _variant(lib, d):
    out = C.create_string_buffer(64)
    check(lib.fx_conv2d_variant(C.byref(d), out, 64), "fx_conv2d_variant")
    return out.value.decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _replay_conv(lib, k, seed):
    B, H, W, Cc, N, KH, KW, s = k["B"], k["H"], k["W"], k["C"], k["N"], k["KH"], k["KW"], k["stride"]
    Ho, Wo = k["Ho"], k["Wo"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    gc_ = torch.Generator().manual_seed(seed)
    xbuf, xv = _strided(B * H * W, k["ldx"], k["xoff"], Cc, 7.0)
    xval = (torch.randn(B, H, W, Cc, generator=g, device=DEV) + _lin(W, -1, 1)[None, None, :, None] + _lin(H, -0.5, 0.5)[None, :, None, None]
            + _lin(Cc, -0.25, 0.25))
    xv.copy_(xval.reshape(-1, Cc))
    del xval
    W4 = (torch.randn(N, Cc, KH, KW, generator=gc_) / math.sqrt(Cc * KH * KW) + torch.linspace(-0.03, 0.03, KH * KW).view(1, 1, KH, KW)
          + torch.linspace(-0.02, 0.02, N).view(N, 1, 1, 1))
    bias = torch.randn(N, generator=gc_) * 0.5
    wd, bd = pack_w(W4, bias)
    wf = frag_pack(W4.permute(0, 2, 3, 1).reshape(N, KH * KW * Cc)) if k["frag"] else None
    rv = None
    if k["res"]:
        rbuf, rv = _strided(B * Ho * Wo, k["ldr"], k["roff"], N, 7.0)
        rv.copy_(torch.randn(B * Ho * Wo, N, generator=g, device=DEV))
    dt = torch.float32 if k["out_f32"] else torch.bfloat16
    if k["ybs"]:
        Srows = k["ybs_val"] // k["ldy"]
        assert k["ystart"] + Ho * Wo <= Srows
        ybuf = torch.full((B * Srows * k["ldy"],), float("nan"), dtype=dt, device=DEV)
        yv = torch.as_strided(ybuf, (B, Ho * Wo, N), (Srows * k["ldy"], k["ldy"], 1), k["ystart"] * k["ldy"] + k["yoff"])
    else:
        ybuf = torch.full(((B * Ho * Wo + 64) * k["ldy"],), float("nan"), dtype=dt, device=DEV)   # + 64 guard rows past M
        yv = torch.as_strided(ybuf, (B, Ho * Wo, N), (Ho * Wo * k["ldy"], k["ldy"], 1), k["yoff"])
    d = FxConvDesc()
    d.x, d.w, d.bias, d.y = xv.data_ptr(), wd.data_ptr(), bd.data_ptr(), yv.data_ptr()
    if rv is not None:
        d.residual, d.ldr = rv.data_ptr(), k["ldr"]
    d.B, d.H, d.W, d.C, d.ldx = B, H, W, Cc, k["ldx"]
    d.Ho, d.Wo, d.N, d.ldy = Ho, Wo, N, k["ldy"]
    d.KH, d.KW, d.stride, d.pad = KH, KW, s, k["pad"]
    d.pool2, d.act, d.out_f32, d.residual_after_act = k["pool2"], k["act"], k["out_f32"], k["res_after"]
    d.y_batch_stride = k["ybs_val"]
    d.w_frag = wf.data_ptr() if wf is not None else None
    assert _variant(lib, d) == k["label"], "stand-alone routing differs from the plan's"
    check(lib.fx_conv2d_nhwc_bf16(C.byref(d), _stream()), "fx_conv2d_nhwc_bf16")
    torch.cuda.synchronize()
    assert not torch.isnan(yv.float()).any(), "NaN left inside the contracted output"
    # the stored width is N rounded up to 8 (fx_conv2d_nhwc_bf16 requires ldy >= that; the implicit-GEMM tiles write the zero-weight columns)
    nstore = (N + 7) // 8 * 8
    stored = torch.as_strided(ybuf, (B, Ho * Wo, nstore), yv.stride(), yv.storage_offset())
    assert _outside_untouched(ybuf, stored), "written outside the contracted output (rows past M / channels past the stored width / other rows)"
    imgs = sorted({0, B // 2, B - 1})
    xs = torch.as_strided(xbuf, (B, H, W, Cc), (H * W * k["ldx"], W * k["ldx"], k["ldx"], 1), k["xoff"])[imgs]
    rs = torch.as_strided(rbuf, (B, Ho, Wo, N), (Ho * Wo * k["ldr"], Wo * k["ldr"], k["ldr"], 1), k["roff"])[imgs] if rv is not None else None
    ref, mag = conv_ref64(xs, bf16_rne(W4.double()).to(DEV), bias.to(DEV), s, ACT_NAME[k["act"]], rs, bool(k["res_after"]), bool(k["pool2"]))
    got = yv[imgs].reshape(len(imgs), Ho, Wo, N)
    return {"out": ulp_stats(got, ref, mag, bool(k["out_f32"]))}, (xs, W4, bias, k)


def _replay_pw_chain(lib, k, seed):
    Mr, B, K1a, K1b, N1, N2 = k["M"], k["B"], k["K1a"], k["K1b"], k["N1"], k["N2"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    gc_ = torch.Generator().manual_seed(seed)
    _, x1 = _strided(Mr, k["ldx1"], k["x1off"], K1a, 7.0)
    x1.copy_(torch.randn(Mr, K1a, generator=g, device=DEV) + _lin(Mr, -1, 1)[:, None] + _lin(K1a, -0.25, 0.25))
    x2 = None
    if K1b:
        _, x2 = _strided(Mr, k["ldx2"], k["x2off"], K1b, 7.0)
        x2.copy_(torch.randn(Mr, K1b, generator=g, device=DEV) * 0.5 + _lin(K1b, -0.25, 0.25))
    r = None
    if k["res"]:
        _, r = _strided(Mr, k["ldr"], k["roff"], N1, 7.0)
        r.copy_(torch.randn(Mr, N1, generator=g, device=DEV))
    K1 = K1a + K1b
    W1 = torch.randn(N1, K1, generator=gc_) / math.sqrt(K1) + torch.linspace(-0.05, 0.05, N1)[:, None]
    b1 = torch.randn(N1, generator=gc_) * 0.3
    W2 = torch.randn(max(N2, 32), N1, generator=gc_) / math.sqrt(N1)
    b2 = torch.randn(max(N2, 32), generator=gc_) * 0.3
    w1d, b1d = frag_pack(W1), b1.to(DEV)
    w2d, b2d = (frag_pack(W2), b2.to(DEV)) if N2 else (None, None)
    H2, W2i = k["img_h"] // 2, k["img_w"] // 2

    def launch(with_y1):
        y1buf = y1 = y2buf = y2 = pbuf = pv = None
        if with_y1:
            y1buf, y1 = _strided(Mr + 64, k["ldy1"] or N1, k["y1off"], N1, float("nan"))
            y1 = y1[:Mr]
        if N2:
            y2buf, y2 = _strided(Mr + 64, k["ldy2"], k["y2off"], N2, float("nan"))
            y2 = y2[:Mr]
        if k["pool"]:
            pbuf, pv = _strided(Mr // 4 + 64, k["ldp"], k["poff"], N1, float("nan"))
            pv = pv[:Mr // 4]
        d = FxPwChainDesc()
        d.x1, d.ldx1, d.K1a = x1.data_ptr(), k["ldx1"], K1a
        if K1b:
            d.x2, d.ldx2, d.K1b = x2.data_ptr(), k["ldx2"], K1b
        if r is not None:
            d.residual, d.ldr = r.data_ptr(), k["ldr"]
        d.w1, d.bias1, d.N1, d.M = w1d.data_ptr(), b1d.data_ptr(), N1, Mr
        if y1 is not None:
            d.y1, d.ldy1 = y1.data_ptr(), k["ldy1"] or N1
        d.act1, d.act2 = k["act1"], k["act2"]
        if N2:
            d.w2, d.bias2, d.y2, d.ldy2, d.N2 = w2d.data_ptr(), b2d.data_ptr(), y2.data_ptr(), k["ldy2"], N2
        if pv is not None:
            d.pool, d.ldp, d.img_h, d.img_w = pv.data_ptr(), k["ldp"], k["img_h"], k["img_w"]
        check(lib.fx_pw_chain_bf16(C.byref(d), _stream()), "fx_pw_chain_bf16")
        torch.cuda.synchronize()
        for buf, v in ((y1buf, y1), (y2buf, y2), (pbuf, pv)):
            if v is not None:
                assert not torch.isnan(v.float()).any(), "NaN left inside the contracted output"
                assert _outside_untouched(buf, v), "written outside the contracted output"
        return y1, y2, pv

    # the label engine.py's pw_chain() gives this launch: the replay runs the instance the plan runs
    label = f"pw_chain<{K1a},{K1b},{N2}>" + ("+pool" if k["pool"] else "") + ("-y1" if not k["y1"] else "")
    assert label == k["label"], (label, k["label"])
    assert lib.fx_pw_chain_supported(K1a, K1b, N1, N2) == 1 and (not k["pool"] or lib.fx_pw_chain_pool_supported(K1a, K1b, N1, N2) == 1)
    y1, y2, pv = launch(True)
    if not k["y1"]:   # the production form does not store y1: y2 and the pooled output must equal the launch that does
        _, y2b, pvb = launch(False)
        assert (y2 is None or torch.equal(y2, y2b)) and (pv is None or torch.equal(pv, pvb))
    HW = Mr // B
    imgs = sorted({0, B // 2, B - 1})
    rows = torch.cat([torch.arange(b * HW, (b + 1) * HW, device=DEV) for b in imgs])
    X = torch.cat([x1[rows]] + ([x2[rows]] if K1b else []), 1)
    ref1, mag1 = gemm_ref64(X, bf16_rne(W1.double()), b1, None, r[rows] if r is not None else None)
    ref1 = act64(ref1, ACT_NAME[k["act1"]])
    stats = {"y1": ulp_stats(y1[rows], ref1, mag1)}
    if N2:   # from the kernel's own bf16 y1: isolates the second GEMM
        ref2, mag2 = gemm_ref64(y1[rows], bf16_rne(W2.double()), b2, ACT_NAME[k["act2"]])
        stats["y2"] = ulp_stats(y2[rows], ref2, mag2)
    if pv is not None:   # AvgPool2d(2, 2) of the kernel's own y1
        yi = y1.double().reshape(B, k["img_h"], k["img_w"], N1)[imgs].permute(0, 3, 1, 2)
        pref = F.avg_pool2d(yi, 2, 2).permute(0, 2, 3, 1)
        pmag = F.avg_pool2d(yi.abs(), 2, 2).permute(0, 2, 3, 1)
        stats["pool"] = ulp_stats(pv.reshape(B, H2, W2i, N1)[imgs], pref, pmag)
    return stats, None


def _cross_check_unfold(xs, W4, bias, k):
    """The device im2col + fp64 matmul reference against CPU fp64 F.conv2d on image 0 of one class."""
    x0 = xs[:1].double()
    w = bf16_rne(W4.double())
    ref, _ = conv_ref64(x0, w.to(DEV), bias.to(DEV), k["stride"], None)
    cpu = F.conv2d(x0.cpu().permute(0, 3, 1, 2), w, bias.double(), stride=k["stride"], padding=k["pad"]).permute(0, 2, 3, 1)
    assert (ref.cpu() - cpu).abs().max().item() <= 1e-9 * cpu.abs().max().item()


@pytest.mark.parametrize("name,B,S", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_conv_classes_at_production_shape_vs_fp64(name, B, S):
    lib = _lib.load()
    cen = _census_of(name, B, S)
    rows, bad = [], []
    smallest = min((e["desc"] for e in cen.values() if e["desc"]["kind"] == "conv" and e["desc"]["KH"] == 3 and not e["desc"]["pool2"]),
                   key=lambda k: k["B"] * k["H"] * k["W"] * k["C"] * k["N"], default=None)
    for i, e in enumerate(sorted(cen.values(), key=lambda e: (e["desc"]["label"], _cls_m(e["desc"])))):
        k = e["desc"]
        stats, keep = (_replay_conv if k["kind"] == "conv" else _replay_pw_chain)(lib, k, 1000 + i)
        if keep is not None and k is smallest:
            _cross_check_unfold(*keep)
        del keep
        for out, s in stats.items():
            c_ok = s["c_needed"] <= ULP_GATE_C
            a_ok = s["agree"] >= ULP_GATE_AGREE
            rows.append(f"  {_fmt(k)} [{out}]  ulp_max={s['ulp_max']:.3f} c_needed={s['c_needed']:.2e} agree={s['agree']:.5f}"
                        + ("" if c_ok and a_ok else "   <-- FAIL"))
            if not (c_ok and a_ok and s["finite"]):
                bad.append((_fmt(k), out, s))
        _release()
    print(f"\n{name} bs={B} {S}^2: {len(cen)} classes vs fp64 (gate: 1 ulp + {ULP_GATE_C:.3g}*mag, RNE agreement >= {ULP_GATE_AGREE})")
    print("\n".join(rows))
    assert not bad, f"{len(bad)} class outputs fail the ulp / agreement gate: {bad[:4]}"
