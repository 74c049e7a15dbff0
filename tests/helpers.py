"""Shared helpers for the parity tests (numpy/torch only; no product imports)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def strided_sample(t: torch.Tensor, n: int = 2048) -> np.ndarray:
    """Same sampler as scripts/make_golden.py."""
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return f[::step][:n].to(torch.float32).cpu().numpy().copy()


def rel_err(a, b) -> float:
    """max|a-b| / max|b| (b = reference)."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b) -> float:
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN, name))


# ---------------------------------------------------------------------------------------------------------------------
# Per-element gate of a bf16 (or fp32) kernel output against an fp64 reference of the same operation.
#
# Every output of the conv / pointwise kernels is an fp32 accumulation of exact bf16 products, then bias, activation and residual in
# fp32 and ONE rounding to the output type.  So |got - ref| <= 1 ulp(ref) of the output type + c * mag, where mag is the fp64 result of
# the same op on |x|, |w|, |b|, |r| (it bounds the fp32 accumulation error where terms cancel), and the fraction of outputs that equal
# the round-to-nearest-even of the fp64 reference is close to 1 (truncation gives ~0.5, a second rounding through a bf16 intermediate
# clearly less than 1).  The constants are measured on an MI355X.
ULP_GATE_C = 2.0 ** -20
ULP_GATE_AGREE = 0.995


def pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k as fp64, built from the exponent bits (exact; torch.ldexp / torch.pow with integer exponents go through a device powf)."""
    return ((k.long() + 1023) << 52).view(torch.float64)


def ulp_of(ref: torch.Tensor, mant_bits: int = 8) -> torch.Tensor:
    """Spacing of the floating-point type with `mant_bits` significand bits (bf16: 8, fp32: 24) at |ref| (fp64; subnormal spacing below
    2^-126)."""
    e = torch.frexp(ref.double().abs().clamp_min(2.0 ** -126)).exponent   # |ref| = m * 2^e, m in [0.5, 1)
    return pow2(e - mant_bits)


def bf16_rne(ref: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value, ties to even, in ONE rounding (torch's double -> bfloat16 goes through fp32), returned as fp64."""
    r = ref.double()
    u = ulp_of(r)
    return torch.round(r / u) * u        # r / u is exact (u a power of two); torch.round rounds half to even


def elem_rne(ref: torch.Tensor, dtype) -> torch.Tensor:
    """bf16_rne for either 16-bit element type: fp64 -> the nearest value of `dtype` (torch.bfloat16 or torch.float16), ties to even, in
    ONE rounding, returned as fp64.  fp16 has 11 significand bits and subnormals spaced 2^-24 below 2^-14; no input here overflows."""
    if dtype == torch.bfloat16:
        return bf16_rne(ref)
    assert dtype == torch.float16
    r = ref.double()
    e = torch.frexp(r.abs().clamp_min(2.0 ** -14)).exponent
    u = pow2(e - 11)
    return torch.round(r / u) * u


def ulp_stats(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, fp32_out: bool = False) -> dict:
    """Worst error in output ulps (over outputs with |ref| >= mag / 256), the smallest c with |got-ref| <= ulp + c*mag everywhere, and the
    RNE agreement rate (bf16 only)."""
    got, ref, mag = got.double(), ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    ulp = ulp_of(ref, 24 if fp32_out else 8)
    err = (got - ref).abs()
    finite = bool(torch.isfinite(got).all())
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    need_c = ((err - ulp).clamp_min(0) / mag.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    agree = float((got == bf16_rne(ref)).double().mean()) if not fp32_out else 1.0
    big = ref.abs() >= mag * 2.0 ** -8          # ulps are meaningful where the output does not cancel to far below its magnitude
    ulp_max = (err / ulp)[big].max().item() if bool(big.any()) else 0.0
    return {"n": err.numel(), "finite": finite, "ulp_max": ulp_max, "c_needed": need_c, "agree": agree}


def assert_ulp_gate(got, ref, mag, what="", c: float = ULP_GATE_C, agree_min: float = ULP_GATE_AGREE, fp32_out: bool = False) -> dict:
    """|got - ref| <= 1 ulp(ref) + c*mag for EVERY element and, for bf16 outputs, bit-agreement with bf16_rne(ref) >= agree_min."""
    s = ulp_stats(got, ref, mag, fp32_out)
    assert s["finite"], f"{what}: non-finite outputs"
    if s["c_needed"] > c:
        got_, ref_, mag_ = got.double(), ref.double(), mag.double()
        bad = ((got_ - ref_).abs() > ulp_of(ref_, 24 if fp32_out else 8) + c * mag_).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {s['n']} outputs outside 1 ulp + {c:.3g}*mag (needs c = {s['c_needed']:.3g}, "
                             f"{s['ulp_max']:.2f} ulp worst); first at {bad[0].tolist()}: got {got_[tuple(bad[0])].item()!r} ref {ref_[tuple(bad[0])].item()!r}")
    assert s["agree"] >= agree_min, f"{what}: only {s['agree']:.4f} of the outputs are the RNE rounding of the fp64 reference (floor {agree_min})"
    return s


def act64(y: torch.Tensor, act) -> torch.Tensor:
    """The library's activations (FX_ACT) in fp64: relu, silu, exact-erf gelu."""
    if act in (None, 0, "none"):
        return y
    if act in ("relu", 1):
        return y.clamp_min(0)
    if act in ("silu", 2):
        return y * torch.sigmoid(y)
    if act in ("gelu", 3):
        return 0.5 * y * (1 + torch.erf(y / math.sqrt(2.0)))
    raise ValueError(act)


def conv_ref64(x, w, bias=None, stride=1, act=None, residual=None, res_after=False, pool2=False):
    """fp64 reference of one fx_conv2d_nhwc_bf16 launch and its magnitude (the same op on |x|, |w|, |b|, |r|), both NHWC [B,Ho,Wo,N].
    x [B,H,W,C] and w [N,C,KH,KW] hold the bf16 values the kernel reads, bias [N] the fp32 values, residual [B,Ho,Wo,N] bf16 values.
    pool2: AvgPool2d(2, 2, ceil_mode) of x, rounded to bf16 (the MFMA operand), then the conv.  Runs on x's device (im2col + matmul)."""
    x = x.double().permute(0, 3, 1, 2)
    if pool2:
        x = bf16_rne(F.avg_pool2d(x, 2, 2, 0, ceil_mode=True))
    N, _, KH, KW = w.shape
    B, _, H, W = x.shape
    pad = (KH - 1) // 2
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    cols = F.unfold(x, (KH, KW), padding=pad, stride=stride)          # [B, C*KH*KW, Ho*Wo], k = (c, kh, kw) as w.reshape(N, -1)
    w2 = w.to(device=x.device, dtype=torch.float64).reshape(N, -1)
    y = (w2 @ cols).reshape(B, N, Ho, Wo).permute(0, 2, 3, 1)
    mag = (w2.abs() @ cols.abs()).reshape(B, N, Ho, Wo).permute(0, 2, 3, 1)
    if bias is not None:
        b = bias.to(device=x.device, dtype=torch.float64)
        y, mag = y + b, mag + b.abs()
    r = residual.to(device=x.device, dtype=torch.float64) if residual is not None else None
    if r is not None and not res_after:
        y, mag = y + r, mag + r.abs()
    y = act64(y, act)
    if r is not None and res_after:
        y, mag = y + r, mag + r.abs()
    return y, mag


def gemm_ref64(x, w, bias=None, act=None, residual=None):
    """fp64 [M,K] x [N,K]^T (+ bias, + residual before the activation) and its magnitude, on x's device."""
    x, w = x.double(), w.to(device=x.device, dtype=torch.float64)
    y, mag = x @ w.T, x.abs() @ w.abs().T
    if bias is not None:
        b = bias.to(device=x.device, dtype=torch.float64)
        y, mag = y + b, mag + b.abs()
    if residual is not None:
        r = residual.to(device=x.device, dtype=torch.float64)
        y, mag = y + r, mag + r.abs()
    return act64(y, act), mag


def frag_order(W2: torch.Tensor) -> torch.Tensor:
    """[N,K] -> MFMA fragment order [N/32][K/16][64][8] (include/focoos_amd.h, fx_conv_desc.w_frag): lane l of fragment (nb, ks) holds
    W2[nb*32 + l%32][ks*16 + (l/32)*8 .. +8].  Same dtype, contiguous."""
    N, K = W2.shape
    assert N % 32 == 0 and K % 16 == 0
    return W2.reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(N // 32, K // 16, 64, 8)


# ---------------------------------------------------------------------------------------------------------------------
# Guarded device buffers and the per-element gate of the kernels' direct tests (tests/test_gpu_train_token_ops.py,
# tests/test_gpu_infer_token_ops.py, tests/test_gpu_train_matrix_ops.py, tests/test_gpu_seg_head_ops.py).  The element type is an
# argument: nothing here reads process state.  The sentinel guards STORES; an fp32 accumulation into it (1.5e16) leaves no trace - see
# acc_buf in test_gpu_train_matrix_ops.py.
GR = 2                      # guard rows before and after every buffer
U32 = 2.0 ** -24            # unit roundoff of fp32
_SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def eps_floor(dtype):
    """(eps, floor) of ONE rounding to `dtype`: |x - round(x)| <= eps * |x| + floor.  The floor is where the relative statement ends:
    2^-25 for fp16 (half the spacing of its subnormals), 2^-126 for bf16 and fp32 (fp32 intermediates below the smallest normal may be
    flushed)."""
    return {torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 2.0 ** -126), torch.float32: (U32, 2.0 ** -126)}[dtype]


def rnd(ref, dtype):
    e, fl = eps_floor(dtype)
    return e * ref.abs() + fl


class Buf:
    """[rows][ld] device tensor of which [rows][cols] is the logical region, between GR guard rows.  With `data` it is an input (padding
    NaN; for integer types, which have none, the sentinel); without, an output (sentinel everywhere; `prefill` then sets the logical
    region, for kernels that accumulate or update in place)."""

    def __init__(self, rows, cols, ld, dtype, data=None, prefill=None, device="cuda:0"):
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        self.full = torch.empty(rows + 2 * GR, ld, dtype=dtype, device=device)
        self.sent = _SENT[self.full.element_size()]
        if data is not None:
            if dtype.is_floating_point:
                self.full.fill_(float("nan"))
            else:
                _bits(self.full).fill_(self.sent)
            self.full[GR:GR + rows, :cols] = data.reshape(rows, cols).to(device=device, dtype=dtype)
        else:
            _bits(self.full).fill_(self.sent)
            if prefill is not None:
                self.full[GR:GR + rows, :cols] = prefill.reshape(rows, cols).to(device=device, dtype=dtype)

    @property
    def ptr(self):
        return self.full[GR].data_ptr()

    def get(self):
        return self.full[GR:GR + self.rows, :self.cols].cpu()

    def assert_guards(self, written=None):
        """Everything outside the logical region - or, with `written` (bool [rows]), outside those rows of it - keeps the sentinel."""
        b = _bits(self.full).cpu().clone()
        region = b[GR:GR + self.rows, :self.cols]
        if written is None:
            region.fill_(self.sent)
        else:
            region[written] = self.sent
        assert bool((b == self.sent).all()), "a guard or an unwritten element changed"


def needed_c(got, ref, mag, dtype, extra=None):
    """Smallest c with |got - ref| <= RND(ref) (one rounding to `dtype`; or `extra`) + c * mag everywhere; inf where got is not finite."""
    got, ref, mag = got.double(), ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    assert bool(torch.isfinite(ref).all())
    err = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
    over = (err - (rnd(ref, dtype) if extra is None else extra)).clamp_min(0)
    return float((over / mag.clamp_min(1e-300)).max()) if over.numel() else 0.0


def gate(kernel, what, got, ref, mag, dtype, measured, margin, extra=None, tag=None):
    """Print the c this output needs (EXCESS <kernel> [<tag>] <c> <what>), then assert c <= margin * measured[kernel]."""
    c = needed_c(got, ref, mag, dtype, extra)
    print(f"EXCESS {kernel} {tag + ' ' if tag else ''}{c:.3e} {what}")
    assert c <= margin * measured[kernel], f"{kernel} {what}: needs c = {c:.3e}, gate {margin * measured[kernel]:.3e}"
    return c


# ---------------------------------------------------------------------------------------------------------------------
# Views of a production plan's buffers: a whole-batch _Plan (throughput lanes, forward(..., nsplit=1)) or a _MultiPlan of batch parts.
def plan_part(pl, b: int):
    """(plan that computed image b, b's index inside it)."""
    parts = getattr(pl, "parts", None)
    if not parts:
        return pl, b
    bp = parts[0].B
    return parts[b // bp], b % bp


def img_nchw(pl, name: str, b: int) -> torch.Tensor:
    """Image b's [1,C,H,W] fp32 copy of activation buffer `name`."""
    p, bl = plan_part(pl, b)
    return p.bufs[name].torch_view()[bl:bl + 1].float().cpu().permute(0, 3, 1, 2)


def img_rows(pl, name: str, b: int, rows_per_image: int) -> torch.Tensor:
    p, bl = plan_part(pl, b)
    v = p.bufs[name].torch_view().reshape(p.B, rows_per_image, -1)
    return v[bl:bl + 1].float().cpu()


def attn_from_bits(pl, b: int, Q: int, nl: int):
    """The engine's own boolean attention masks of image b, one [1,Q,Lk] tensor per decoder layer (bit set = masked)."""
    p, bl = plan_part(pl, b)
    out = []
    nlev = len(p.levels)
    for i in range(nl):
        Lk = p.levels[i % nlev]
        words = p.attn_bits[i][bl * Q:(bl + 1) * Q].cpu().numpy().view(np.uint8)
        m = np.unpackbits(words, axis=-1, bitorder="little")[:, :Lk].astype(bool)
        out.append(torch.from_numpy(m).reshape(1, Q, Lk))
    return out


def plan_variants(pl) -> dict:
    out = {}
    for m in pl.meta.values():
        out[m["variant"]] = out.get(m["variant"], 0) + 1
    return out


def _worst(worst: dict, k: str, v: float, fn=max):
    worst[k] = fn(worst.get(k, v), v)


def detr_image_check(pl, b, j, col, probs_o, boxes_o, worst, tol_score, tol_prob, tol_box, thr=0.5):
    """Stage-by-stage and final-output parity of image b (the j-th image of the oracle run) of an RT-DETR plan, with the oracle fed the
    engine's own top-300 query set; every detection the oracle puts clearly above `thr` is reported with the same (query, class), nothing
    clearly below it is."""
    for k in ("res3", "res4", "res5", "enc_s32", "enc_s16", "enc_s8"):
        e = rel_l2(img_nchw(pl, k, b), col[k][j:j + 1])
        _worst(worst, k, e)
        assert e < 2e-2, (b, k, e)
    e = rel_l2(img_rows(pl, "memory", b, plan_part(pl, b)[0].S), col["memory"][j:j + 1])
    _worst(worst, "memory", e)
    assert e < 2e-2, (b, "memory", e)
    ds = (pl.enc_scores[b].cpu() - col["enc_scores"][j]).abs().max().item()
    _worst(worst, "enc_scores", ds)
    assert ds <= tol_score, (b, ds)
    e = rel_l2(img_rows(pl, "target", b, 300), col["target"][j:j + 1])
    assert e < 3e-2, (b, "target", e)
    for i in range(6):
        e = rel_l2(img_rows(pl, f"dec{i}.out", b, 300), col[f"dec{i}_out"][j:j + 1])
        _worst(worst, f"dec{i}", e)
        assert e < 4e-2, (b, i, e)
    dp = (pl.probs[b].cpu() - probs_o[j]).abs().max().item()
    db = (pl.boxes[b].cpu() - boxes_o[j]).abs().max().item()
    _worst(worst, "dprob", dp)
    _worst(worst, "dbox", db)
    assert dp <= tol_prob and db <= tol_box, (b, dp, db)
    K = probs_o.shape[-1]
    n = int(pl.det_count[b])
    pairs = set(zip(pl.det_queries[b, :n].cpu().tolist(), pl.det_labels[b, :n].cpu().tolist()))
    flat = probs_o[j].flatten()
    for f in torch.nonzero(flat > thr + 2 * tol_prob).flatten().tolist():
        assert divmod(f, K) in pairs, (b, divmod(f, K))
    never = set(torch.nonzero(flat < thr - 2 * tol_prob).flatten().tolist())
    assert not any((q * K + c) in never for q, c in pairs)


def mask_family_check(pl, b, j, cfg, col, probs_o, stages, nl, worst):
    """Stage, decoder-layer, class-probability and mask parity of image b of a MaskFormer / BiSeNetFormer plan (oracle run of that one
    image with the engine's own attention masks)."""
    Q = int(cfg.get("num_queries", 100))
    for name in stages:
        e = rel_l2(img_nchw(pl, name, b), col[name])
        _worst(worst, name, e)
        assert e <= 2.5e-2, (b, name, e)
    for i in range(nl):
        e = rel_l2(img_rows(pl, f"dec{i}.out", b, Q), col[f"dec{i}_out"])
        _worst(worst, f"dec{i}", e)
        assert e <= 3e-2, (b, i, e)
    dp = (pl.probs[b].cpu() - probs_o[0]).abs().max().item()
    lo_o = torch.sigmoid(col["mask_logits"])[0]
    mine = pl.mask_probs[b].cpu()
    dm = (mine - lo_o).abs().mean().item()
    agree = ((mine >= 0.5) == (lo_o >= 0.5)).float().mean().item()
    _worst(worst, "dprob", dp)
    _worst(worst, "dmask_mean", dm)
    _worst(worst, "binary_agreement_min", agree, min)
    assert dp <= 3e-2 and dm <= 1e-2 and agree >= 0.99, (b, dp, dm, agree)
