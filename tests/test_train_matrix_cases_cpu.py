"""CPU checks of tests/train_matrix_cases.py (the cases of tests/test_gpu_train_matrix_ops.py): every closed-form float64 reference
against float64 torch.autograd of the same operation, the bound that makes the integer runs exact, and that every mask case holds the
rows it claims.  No GPU, no library."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import train_matrix_cases as TC
from tests.helpers import bf16_rne

# |closed form - autograd| <= 1e-12 * mag: both are float64 sums of the same terms in different orders (unit roundoff 1.1e-16, at most
# 15376 terms for the weight gradients, 257 x 32 for the attention products)
TOL = 1e-12


def close(a, b, mag):
    assert a.shape == b.shape == mag.shape, (a.shape, b.shape, mag.shape)
    return bool(((a - b).abs() <= TOL * mag + 1e-300).all())


# the 8 GFLOP shapes take seconds each in float64 on a CPU; their reference is the SAME function on a shape of the same class cut down
# in channels (the function has no shape-dependent branch), the full-size ones are compared on the GPU against the integer run
def cut(c):
    return c._replace(C=min(c.C, 16), N=min(c.N, 24)) if TC.gflop(c) > 1.0 else c


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.ALL_WGRAD, ids=TC.wid)
def test_wgrad_reference_against_autograd(case, kind):
    c = cut(case)
    pad = (c.k - 1) // 2
    d = TC.wgrad_inputs(c, kind)
    ref, mag, db, dbm = TC.wgrad_ref64(d["x"], d["dz"], c.k, c.stride)
    w = torch.zeros(c.N, c.C, c.k, c.k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c.N, dtype=torch.float64, requires_grad=True)
    F.conv2d(d["x"].double().permute(0, 3, 1, 2), w, b, stride=c.stride, padding=pad).backward(d["dz"].double().permute(0, 3, 1, 2))
    assert close(TC.nckk(ref), w.grad, TC.nckk(mag))
    assert close(db, b.grad, dbm)
    assert bool((mag >= ref.abs()).all()) and bool((dbm >= db.abs()).all())
    for t in (d["x"], d["dz"]):
        assert torch.equal(t.double(), bf16_rne(t))               # the operands hold bf16 values
    if kind == "int":
        assert float(d["x"].abs().max()) <= 2 and float(d["dz"].abs().max()) <= 2 and float(d["pre"].abs().max()) <= 8
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) + 8 < 2 ** 24


@pytest.mark.parametrize("case", TC.ALL_WGRAD, ids=TC.wid)
def test_wgrad_exact_run_bound_and_threshold_class(case):
    M = TC.pixels(case)
    assert 4 * M < 2 ** 24 and TC.exact_run_is_exact(M)
    wide = case.N % 256 == 0 and case.C % 256 == 0
    if case in TC.WGRAD_DEFAULT:
        assert wide and (TC.gflop(case) >= 8.0) == case.variant.startswith("conv_wgrad_dma"), TC.gflop(case)
        assert 7.9 <= TC.gflop(case) <= 8.2                      # the smallest shapes around the threshold
    elif case in TC.WGRAD_WIDE_SMALL:
        assert wide and TC.gflop(case) < 8.0
    else:
        assert not wide


def test_wgrad_case_claims():
    """The pixel-step counts and tile tails the notes of the small cases name."""
    steps = lambda c: -(-min(TC.pixels(c), 512) // 64)            # noqa: E731
    by = {TC.wid(c): c for c in TC.WGRAD_SMALL}
    assert TC.out_hw(by["8x5x7-c64-n64-k3s1"])[0] * TC.out_hw(by["8x5x7-c64-n64-k3s1"])[1] < 64
    assert [steps(by[k]) for k in ("1x6x8-c128-n64-k1s1", "1x10x10-c32-n64-k3s1", "1x13x13-c64-n8-k1s1")] == [1, 2, 3]
    assert 9 * by["2x9x11-c8-n64-k3s1"].C == 72 and 9 * by["2x12x12-c24-n136-k3s1"].C == 216
    assert TC.out_hw(by["3x15x17-c64-n64-k3s2"]) == (8, 9)
    assert 512 < TC.pixels(by["2x23x19-c40-n72-k3s1"]) < 1024
    # the DMA kernel's pixel ranges are 512 pixels at these sizes: the last range of the two cases that name it
    assert TC.pixels(TC.WGRAD_DEFAULT[0]) % 512 == 186 and TC.pixels(TC.WGRAD_WIDE_SMALL[1]) % 512 == 40
    # a 32-pixel step against the image: ceil(32 / W) <= H is what the DMA kernel's one-carry row update needs
    need = lambda c: -(-32 // c.W) <= c.H                          # noqa: E731
    assert [need(c) for c in TC.WGRAD_WIDE_SMALL] == [True, True, True, False, True, True]
    assert all(need(c) for c in TC.WGRAD_DEFAULT)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.LINEAR_CASES, ids=TC.lid)
def test_linear_wgrad_reference_against_autograd(case, kind):
    c = case
    d = TC.linear_inputs(c, kind)
    ref, mag, db, dbm = TC.linear_ref64(d["x"], d["dz"], c)
    w = torch.zeros(c.Np, c.Kp, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c.Np, dtype=torch.float64, requires_grad=True)
    F.linear(d["x"].double(), w, b).backward(d["dz"].double())
    assert close(ref, w.grad[:c.n_store, :c.k_store], mag) and close(db, b.grad[:c.n_store], dbm)
    assert TC.exact_run_is_exact(c.R) and c.n_store <= c.Np and c.k_store <= c.Kp and c.ld_dw >= c.k_store
    assert c.Kp % 32 == 0 and c.Np % 8 == 0


MHA_ALL = [(c, m, False, False) for c in TC.MHA_BWD_CASES for m in (False, True)] + \
          [(TC.MHA_BWD_BIG, m, True, False) for m in (False, True)] + [(TC.MHA_BWD_UNIFORM, m, False, True) for m in (False, True)]


@pytest.mark.parametrize("spec", MHA_ALL, ids=lambda s: f"{TC.mid(s[0])}{'-masked' if s[1] else ''}{'-big' if s[2] else ''}{'-uniform' if s[3] else ''}")
def test_mha_bwd_reference_against_autograd(spec):
    case, masked, big, uniform = spec
    c = TC.mha_bwd_case(case, masked, big=big, uniform=uniform)
    B, heads, Lq, Lk = case
    q, k, v = (c[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    qh, kh, vh = (t.view(B, -1, heads, 32).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(32.0)
    if masked:
        m = c["mask"].clone()
        m[m.sum(-1) == Lk] = False                                # the reference's rule, its own way: a fully masked row is cleared
        s = s.masked_fill(m[:, None], float("-inf"))
    (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, heads * 32).backward(c["do"].double())
    for n, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert close(c[n], g, c[n + "_mag"]), n
        assert bool((c[n + "_mag"] >= c[n].abs() * (1 - 1e-12)).all()), n
    assert bool(((c["p"].sum(-1) - 1).abs() < 1e-12).all())
    if big:
        assert c["smax"] > 40
    if uniform:
        assert not bool(c["k"].any()) and not bool(c["dq"].any())
        allowed = Lk - (c["mask"] & ~c["mask"].all(-1, keepdim=True)).sum(-1) if masked else torch.full((B, Lq), Lk)
        assert bool(((c["p"] > 0).sum(-1) == allowed[:, None]).all())
        share = torch.where(c["p"] > 0, c["p"] * allowed[:, None, :, None], torch.ones_like(c["p"]))
        assert bool(((share - 1).abs() < 1e-12).all())


@pytest.mark.parametrize("case", TC.MHA_BWD_CASES + [TC.MHA_BWD_BIG, TC.MHA_BWD_UNIFORM], ids=TC.mid)
def test_mask_cases_hold_the_rows_they_claim(case):
    B, heads, Lq, Lk = case
    c = TC.mha_bwd_case(case, True)
    mask, plan = c["mask"].view(B * Lq, Lk), c["plan"]
    kinds = [k for _, k in plan]
    assert kinds[:3] == ["masked", "open", "last"][:B * Lq]
    if B * Lq >= 3:
        assert set(kinds) == {"masked", "open", "last"}
    for row, kind in plan:
        if kind == "masked":
            assert bool(mask[row].all())
        elif kind == "open":
            assert not bool(mask[row].any())
        else:
            assert bool(mask[row, :Lk - 1].all()) and not bool(mask[row, Lk - 1])
            assert (Lk - 1) // 32 == (Lk + 31) // 32 - 1          # the allowed key lies in the last (partial when Lk % 32 != 0) tile
    words = TC.mask_words(c["mask"])
    assert words.shape == (B * Lq, (Lk + 31) // 32)
    bits = ((words.long().unsqueeze(-1) >> torch.arange(32)) & 1).bool().reshape(B * Lq, -1)
    assert torch.equal(bits[:, :Lk], mask) and bool(bits[:, Lk:].all())


def test_case_lists_cover_what_the_gpu_file_names():
    L = {1, 31, 32, 33, 128, 129, 256, 257}
    assert all(c.Lq in L and c.Lk in L and c.B in (1, 2) and c.heads in (1, 2, 8) for c in TC.MHA_BWD_CASES)
    pairs = {(c.Lq, c.Lk) for c in TC.MHA_BWD_CASES}
    assert (257, 33) in pairs and (33, 257) in pairs
    assert {c.Lq for c in TC.MHA_BWD_CASES} | {c.Lk for c in TC.MHA_BWD_CASES} == L
    assert {c.heads for c in TC.MHA_BWD_CASES} == {1, 2, 8} and {c.B for c in TC.MHA_BWD_CASES} == {1, 2}
