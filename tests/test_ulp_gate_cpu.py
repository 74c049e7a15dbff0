"""The per-element ulp / RNE-agreement gate of tests/helpers.py (assert_ulp_gate) on a synthetic fp64 conv: it accepts the exact
round-to-nearest-even of the reference and rejects the kernel bugs it exists to catch, each of which the old
max|got - ref| / max|ref| < 1.2e-2 gate of the conv kernel tests lets through."""
import math

import pytest
import torch

from tests.helpers import ULP_GATE_AGREE, ULP_GATE_C, assert_ulp_gate, bf16_rne, conv_ref64, ulp_of, ulp_stats

B, H, W, C, N = 2, 12, 12, 64, 64


def _bf(t):
    return bf16_rne(t.double())


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(0)
    x = _bf(torch.randn(B, H, W, C, generator=g, dtype=torch.float64) + torch.linspace(-1, 1, W, dtype=torch.float64)[None, None, :, None])
    w = _bf(torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(9 * C))
    b = torch.randn(N, generator=g).float() * 0.5
    r = _bf(torch.randn(B, H, W, N, generator=g, dtype=torch.float64))
    ref, mag = conv_ref64(x, w, b, 1, "silu", r, True)
    return x, w, b, r, ref, mag


def _rejects(got, ref, mag):
    with pytest.raises(AssertionError):
        assert_ulp_gate(got, ref, mag, "bug")


def test_bf16_rne_is_one_rounding():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, -(1.0 + 2.0 ** -8), 0.0, 3.0], dtype=torch.float64)
    assert bf16_rne(v).tolist() == [1.0, 1.0 + 2 * 2.0 ** -7, 1.0 + 2.0 ** -7, -1.0, 0.0, 3.0]   # ties to even, above a tie rounds up
    assert ulp_of(torch.tensor([1.0, 1.5, 0.75], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8]
    x = torch.randn(10000, dtype=torch.float64)
    assert ((bf16_rne(x) - x).abs() <= ulp_of(x) / 2).all()


def test_gate_accepts_exact_rne(case):
    *_, ref, mag = case
    s = assert_ulp_gate(bf16_rne(ref), ref, mag, "exact")
    assert s["agree"] == 1.0 and s["ulp_max"] <= 0.5


def test_gate_accepts_fp32_accumulation(case):
    """What a correct kernel does: fp32 sums of the bf16 products in some order, fp32 epilogue, one rounding."""
    x, w, b, r, ref, mag = case
    y32 = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding=1).permute(0, 2, 3, 1)
    y32 = torch.nn.functional.silu(y32) + r.float()
    assert_ulp_gate(bf16_rne(y32.double()), ref, mag, "fp32 accumulation")


def test_gate_rejects_truncation(case):
    *_, ref, mag = case
    m, e = torch.frexp(ref)
    got = torch.ldexp(torch.trunc(torch.ldexp(m, torch.full_like(e, 8))), e - 8)   # round toward zero
    assert ulp_stats(got, ref, mag)["agree"] < 0.7
    _rejects(got, ref, mag)


def test_gate_rejects_bf16_intermediate_before_residual(case):
    x, w, b, r, _, _ = case
    ref, mag = conv_ref64(x, w, b, 1, None, r, False)               # act(conv + b + r), residual before the activation
    z, _ = conv_ref64(x, w, b, 1, None)
    got = bf16_rne(bf16_rne(z) + r)                                   # conv + bias rounded to bf16 first, then the residual
    _rejects(got, ref, mag)


def test_gate_rejects_dropped_k_step(case):
    x, w, b, r, ref, mag = case
    w2 = w.clone()
    w2[:, 16:32, 1, 1] = 0                                            # one 16-channel k-step of the centre tap missing
    got = bf16_rne(conv_ref64(x, w2, b, 1, "silu", r, True)[0])
    _rejects(got, ref, mag)


def test_gate_rejects_tile_shifted_by_one_row(case):
    *_, ref, mag = case
    got = bf16_rne(ref).reshape(-1, N).clone()
    t = 5                                                             # rows 160..191 of the flattened M read the next row
    got[32 * t:32 * t + 32] = bf16_rne(ref).reshape(-1, N)[32 * t + 1:32 * t + 33]
    _rejects(got.reshape(ref.shape), ref, mag)


def test_gate_rejects_missing_bias_of_one_channel(case):
    x, w, b, r, ref, mag = case
    b2 = b.clone()
    b2[int(b.abs().argmax())] = 0
    got = bf16_rne(conv_ref64(x, w, b2, 1, "silu", r, True)[0])
    _rejects(got, ref, mag)


def test_gate_constants_are_tight_enough():
    """c bounds an fp32 accumulation error (a few 2^-24 of the magnitude per reduction step, far below one bf16 ulp of 2^-8), and the
    agreement floor sits well above what truncation (~0.5) reaches."""
    assert 0 < ULP_GATE_C <= 2.0 ** -12 and 0.9 <= ULP_GATE_AGREE < 1.0
