"""tests/infer_token_cases.py without a GPU: every float64 reference the GPU tests of the inference-side token, pixel and selection kernels
gate against is checked here against an INDEPENDENT formulation of the same operation (torch's own operators in float64, the oracle's
functions), so a reference cannot be wrong unnoticed; and the properties the GPU cases rely on (which queries a mask plants, where the
sampling taps fall, which products are rounding ties) are asserted on the inputs themselves."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import detr_oracle as O
from tests import infer_token_cases as IC
from tests.helpers import bf16_rne

TIGHT = 1e-12          # float64 formulations of the same arithmetic


def close(a, b, tol=TIGHT):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(((a - b).abs() <= tol * (1 + b.abs())).all()), float((a - b).abs().max())


def is_bf16(t):
    return torch.equal(t, t.to(torch.bfloat16).float())


@pytest.mark.parametrize("case", IC.ADD_ROWS_CASES)
def test_add_rows_reference_is_one_rounding(case):
    rows, cols, y_rows = case
    c = IC.add_rows_case(*case)
    assert is_bf16(c["x"]) and is_bf16(c["y"])
    yy = c["y"][torch.arange(rows) % y_rows]
    s32 = c["x"] + yy                                                     # torch's fp32 addition
    assert torch.equal(s32.double(), c["sum"]), "an fp32 sum of this case is inexact: bit equality would need a second rounding"
    assert torch.equal(c["ref"], s32.to(torch.bfloat16).double())         # torch's fp32 -> bf16 is round-to-nearest-even
    assert torch.equal(c["ref"], bf16_rne(c["sum"]))
    if rows > y_rows:
        assert rows % y_rows != 0                                          # the wrap does not divide


@pytest.mark.parametrize("case", IC.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}{'+res' if c[2] else ''}-{c[3]}")
def test_layernorm_reference(case):
    cols, rows, res, variant = case
    c = IC.layernorm_case(*case)
    assert is_bf16(c["x"]) and (c["res"] is None) == (not res)
    v = c["x"].double() + (c["res"].double() if res else 0.0)
    close(c["ref"], F.layer_norm(v, (cols,), c["gamma"].double(), c["beta"].double(), 1e-5), 1e-9)
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())
    if variant == "mean40":
        assert bool(((v.mean(1) - 40).abs() < 0.5).all()) and bool(((v.std(1) - 0.5).abs() < 0.1).all())
        # what the case is for: a one-pass E[x^2] - mean^2 in fp32 misses the variance by far more than fp32 roundoff (6e-8) on some row
        v32 = v.float()
        one_pass = (v32 * v32).mean(1) - v32.mean(1) ** 2
        var = v.var(1, unbiased=False)
        assert bool(((one_pass.double() - var).abs() > 1e-5 * var).any())


def _mha_params():
    return [(Lq, Lk, 8, m, False) for Lq, Lk in IC.MHA_PAIRS for m in (False, True)] + [(37, 31, 2, False, False), (37, 31, 2, True, False),
                                                                                      (77, 449, 8, False, True), (77, 449, 8, True, True)]


@pytest.mark.parametrize("case", _mha_params(), ids=lambda c: f"{c[0]}x{c[1]}h{c[2]}{'m' if c[3] else ''}{'big' if c[4] else ''}")
def test_attention_reference(case):
    Lq, Lk, heads, masked, big = case
    c = IC.mha_case(Lq, Lk, heads, masked, big)
    B = c["B"]
    assert all(is_bf16(c[n]) for n in "qkv")
    qh, kh, vh = (c[n].double().view(B, -1, heads, 32).transpose(1, 2) for n in "qkv")
    allowed = None
    if masked:
        m = c["mask"]
        full = m.all(-1)
        assert bool(full.any()), "no fully masked query"
        assert bool((~m).all(-1).any()), "no fully open query"
        last_only = (~m).sum(-1).eq(1) & ~m[..., Lk - 1]
        assert bool(last_only.any()), "no query whose only allowed key is the last one"
        assert (Lk - 1) // 32 == (Lk + 31) // 32 - 1                      # it lies in the last tile
        if B * Lq >= 6:                                                    # the planted rows at the end of the query range
            assert bool(full.view(-1)[-1]) and bool(last_only.view(-1)[-2])
        allowed = (~m | full[..., None])[:, None]                          # SDPA: True = takes part
        w = IC.mask_words(m)
        assert w.shape == (B * Lq, (Lk + 31) // 32) and w.dtype == torch.int32
        bits = ((w.long()[:, :, None] >> torch.arange(32)) & 1).bool().reshape(B * Lq, -1)
        assert torch.equal(bits[:, :Lk], m.reshape(B * Lq, Lk)) and bool(bits[:, Lk:].all())
    sdpa = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=allowed)   # its own scale 1 / sqrt(32)
    close(c["ref"], sdpa.transpose(1, 2).reshape(B, Lq, heads * 32), 1e-9)
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())
    if big:
        assert 40 < c["smax"] < 120
    # a second formulation through nn.MultiheadAttention's functional form with identity projections
    if heads == 8 and Lk <= 64:
        E = heads * 32
        eye = torch.eye(E, dtype=torch.float64)
        am = None
        if masked:
            am = (~allowed[:, 0]).repeat_interleave(heads, 0)              # [B * heads, Lq, Lk], True = not allowed
        out, _ = F.multi_head_attention_forward(c["q"].double().transpose(0, 1), c["k"].double().transpose(0, 1), c["v"].double().transpose(0, 1), E, heads,
                                                torch.cat([eye, eye, eye]), torch.zeros(3 * E, dtype=torch.float64), None, None, False, 0.0, eye,
                                                torch.zeros(E, dtype=torch.float64), training=False, need_weights=False, attn_mask=am)
        close(c["ref"], out.transpose(0, 1), 1e-9)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("geom", [(IC.MSDA_L3, 4), (IC.MSDA_L2, 3)], ids=["L3P4", "L2P3"])
def test_deformable_sampling_reference(geom, mode):
    shapes, P = geom
    c = IC.msda_case(shapes, P, mode)
    B, Q, S, L = c["B"], c["Q"], c["S"], c["L"]
    assert is_bf16(c["value"]) and S == sum(h * w for h, w in shapes)
    if mode == 0:
        loc, w = c["loc"].double(), c["attn"].double()
        close(w.sum((-1, -2)), torch.ones(B, Q, 8), 1e-6)
    else:                                                                  # modelling.py:860-874 as the oracle's ms_deformable_attention writes it
        r = c["ref4"].double()
        loc = r[:, :, None, None, None, :2] + c["off"].double() / P * r[:, :, None, None, None, 2:] * 0.5
        w = F.softmax(c["logits"].double(), -1).reshape(B, Q, 8, L, P)
    ref = O.ms_deform_attn_core(c["value"].double().view(B, S, 8, 32), [list(s) for s in shapes], loc, w)
    close(c["ref"], ref, 1e-9)
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())
    for st in c["stats"]:                                                  # taps on all four borders and beyond them, on every level
        x0, y0, H, W = st["x0"], st["y0"], st["H"], st["W"]
        assert bool((x0 == -1).any()) and bool((x0 == W - 1).any()) and bool((y0 == -1).any()) and bool((y0 == H - 1).any())
        assert bool((x0 < -1).any()) and bool((x0 >= W).any()) and bool((y0 < -1).any()) and bool((y0 >= H).any())
        assert bool((x0.abs() > 1e5).any()) and bool((y0.abs() > 1e5).any())
    if mode == 0:
        flat = c["loc"].reshape(-1, 2)
        assert bool((flat == 0.0).any()) and bool((flat == 1.0).any())


@pytest.mark.parametrize("sizes", IC.RESIZE_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_references(sizes):
    """F.interpolate forms its scale in float64 where the kernels (and the reference) use the fp32 quotient: the two differ by up to
    2^-24 * scale in the source coordinate, i.e. by <= 1e-6 * (value range) here."""
    (H, W), (Ho, Wo) = sizes
    u = IC.resize_u8_case(*sizes)
    it = F.interpolate(u["x"].double().permute(2, 0, 1)[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    assert bool(((u["ref"] - it).abs() <= 1e-6 * 255 * max(H, W)).all())
    assert bool((u["mag"] >= u["ref"].abs() * (1 - 1e-12)).all())
    for Cc in (8, 24):
        c = IC.resize_nhwc_case(*sizes, Cc)
        assert is_bf16(c["x"])
        it = F.interpolate(c["x"].double().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert bool(((c["ref"] - it).abs() <= 1e-6 * float(c["x"].abs().max()) * max(H, W)).all())
        if (H, W) == (Ho, Wo):
            assert torch.equal(c["ref"], c["x"].double())


@pytest.mark.parametrize("case", IC.MAXPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}{'neg' if c[2] else ''}")
def test_maxpool_reference(case):
    c = IC.maxpool_case(*case)
    ref = F.max_pool2d(c["x"].double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(c["ref"], ref)
    if case[2]:
        assert bool((c["ref"] < 0).all())


@pytest.mark.parametrize("case", IC.AVGPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_avgpool_reference(case):
    c = IC.avgpool_case(*case)
    ref = F.avg_pool2d(c["x"].double().permute(0, 3, 1, 2), 2, 2, 0, ceil_mode=True).permute(0, 2, 3, 1)
    close(c["ref"], ref)
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())


def test_selection_references():
    for cols in IC.ROWMAX_COLS:
        c = IC.rowmax_case(cols)
        assert torch.equal(c["ref"], c["x"].max(1).values) and c["ref"][3] == float("-inf")
    for cols in (8, 256):
        c = IC.gather_fill_case(cols)
        assert torch.equal(c["gathered"], c["src"].gather(1, c["idx"].long()[..., None].expand(-1, -1, cols)))
        assert len(set(c["idx"][0].tolist())) < 4 and len(set(c["rows_idx"].tolist())) < 4      # repeated indices
        hit = torch.zeros(11, dtype=torch.bool)
        hit[c["rows_idx"].long()] = True
        assert torch.equal(c["filled"][:, hit], c["rowv"].expand(3, int(hit.sum()), cols)) and torch.equal(c["filled"][:, ~hit], c["src"][:, ~hit])
    for N in (8, 512):
        c = IC.linear_k4_case(N)
        close(c["ref"], F.relu(F.linear(c["x"].double(), c["w"].double(), c["b"].double())))
        assert bool((c["ref"] == 0).any()) and bool((c["ref"] > 0).any())


@pytest.mark.parametrize("K", [128, 256])
def test_bbox_head_references(K):
    c = IC.bbox_head_case(K, 0)
    assert c["ref4"].view(-1)[:6].tolist() == torch.tensor(IC.BBOX_REF_EDGES[:6]).tolist()
    close(c["third"], O.inverse_sigmoid(c["ref4"].double()))
    close(c["new"], torch.sigmoid(F.linear(c["h"].double(), c["w"].double(), c["b"].double()) + O.inverse_sigmoid(c["ref4"].double())))
    assert math.isclose(float(c["third"].view(-1)[0]), math.log(1e-5 / 1.0)) and math.isclose(float(c["third"].view(-1)[1]), math.log(1.0 / 1e-5))
    assert c["third"].view(-1)[4] == c["third"].view(-1)[0] and c["third"].view(-1)[5] == c["third"].view(-1)[1]     # outside [0, 1]: clamped
    c = IC.bbox_head_case(K, 1)
    close(c["u"], F.linear(c["h"].double(), c["w"].double(), c["b"].double()) + c["anchors"].double()[c["idx"].long()])
    close(c["new"], torch.sigmoid(c["u"]))


@pytest.mark.parametrize("K", [4, 365])
def test_head_out_reference(K):
    c = IC.head_out_case(K)
    close(c["probs"], torch.sigmoid(c["logits"].double()))
    close(c["boxes"], O.box_cxcywh_to_xyxy(c["ref4"].double()))
    assert bool((c["mag_p"] >= c["probs"]).all()) and bool((c["mag_b"] >= c["boxes"].abs()).all())


def test_postprocess_reference_and_ties():
    c = IC.postprocess_case()
    B, Q, K, top_k, thr = c["B"], c["Q"], c["K"], c["top_k"], c["thr"]
    # every product is exactly j + 0.5, in fp32 too (what the kernel forms), with both parities of j and negative ones
    div = torch.tensor([1024.0, 512.0, 1024.0, 512.0])
    q = c["queries"].long()
    p32 = c["boxes"][torch.arange(B)[:, None], q] * div
    assert torch.equal(p32.double(), c["prod"])
    fl = torch.floor(c["prod"])
    assert bool((c["prod"] - fl == 0.5).all())
    assert bool((fl % 2 == 0).any()) and bool((fl % 2 == 1).any()) and bool((c["prod"] < 0).any())
    assert bool((c["obox"] % 2 == 0).all())                                # half to even
    assert bool((c["obox"].double() != torch.floor(c["prod"] + 0.5)).any()), "no tie where half-up differs"
    assert bool((c["val"] == thr).any()) and bool((c["val"][:, :-1] >= c["val"][:, 1:]).all())
    # the oracle's postprocess on probabilities whose top-k is exactly (val, idx)
    probs = torch.zeros(B, Q * K)
    probs[torch.arange(B)[:, None], c["idx"].long()] = c["val"]
    res = O.postprocess(probs.view(B, Q, K), c["boxes"], c["sizes"], top_k, thr)
    for b, (s, lab, qq, bp) in enumerate(res):
        n = int(c["count"][b])
        assert n == len(s) and 0 < n < top_k
        assert torch.equal(s, c["val"][b, :n]) and torch.equal(lab, c["labels"][b, :n].long()) and torch.equal(qq, c["queries"][b, :n].long())
        assert torch.equal(bp, c["obox"][b, :n])
    assert float(c["val"][0, int(c["count"][0])]) == thr                   # the first score left out EQUALS the threshold


@pytest.mark.parametrize("case", IC.TOPK_CASES, ids=lambda c: f"n{c[0]}")
def test_topk_reference_order(case):
    n, ld, k = case
    c = IC.topk_case(*case)
    s = c["s"]
    assert torch.equal(c["order"], torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k])
    # row 2: three positive values, then zeros of both signs straddle the cut, the lowest two indices win and the first is a -0.0
    z = s[2]
    zeros = torch.nonzero(z == 0).flatten()
    assert int((z > 0).sum()) == 3 and len(zeros) == 4 and k == 5
    assert c["order"][2, 3:].tolist() == zeros[:2].tolist()
    sign = torch.signbit(z[zeros])
    assert bool(sign[0]) and not bool(sign[1]) and bool(sign.any()) and not bool(sign.all())
    by_old_key = sorted(zeros.tolist(), key=lambda i: (bool(torch.signbit(z[i])), i))       # +0.0 ahead of -0.0: NOT the documented order
    assert by_old_key[:2] != zeros[:2].tolist()
    assert not bool(torch.signbit(c["vals"]).logical_and(c["vals"] == 0).any())
    assert ld > n and ld % 4 == 0
