"""Shared by tests/test_train_matrix_cases_cpu.py and tests/test_gpu_train_matrix_ops.py: the inputs of every case of the training
step's matrix-core kernels - the weight gradient (csrc/conv_wgrad.hip: conv_wgrad_kernel<PW>, conv_wgrad_dma_kernel<PW>) and the
attention backward (csrc/attn_bwd.hip: mha32_bwd_dq_kernel, mha32_bwd_dkv_kernel) - seeded and holding bf16 values, with the float64
closed-form reference of the operation and its float64 magnitude: the same expression with every term taken in absolute value, which
bounds the fp32 error where terms cancel.

Nothing here touches the library; the references run on whatever device their inputs live on (the CPU test runs them on the CPU and
checks them against float64 torch.autograd, the GPU test runs the large ones on the device, as helpers.conv_ref64 does)."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.helpers import gemm_ref64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(*ints):
    s = 17
    for i in ints:
        s = (s * 1000003 + int(i)) % (2 ** 31 - 1)
    return s


def bf(t):
    """Round to bf16, keep as fp32 (every value exactly representable in bf16)."""
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ weight gradient
# variant: the label fx_conv2d_wgrad_variant must give for the shape (at the default FX_WGRAD_DMA_MIN_GFLOP = 8 unless said otherwise).
WCase = namedtuple("WCase", "B H W C N k stride variant note")

PW, IM2COL, DMA_PW, DMA_3X3 = "conv_wgrad<pw>", "conv_wgrad<im2col>", "conv_wgrad_dma<pw>", "conv_wgrad_dma<3x3>"

# The 128 x 128 kernel: a K-step is 64 pixels, a tile 128 output channels x 128 columns of Ktot = k * k * C, a pixel range >= 512 pixels.
WGRAD_SMALL = [
    WCase(8, 5, 7, 64, 64, 3, 1, IM2COL, "image (35 pixels) below one K-step: `carried` false, the divisions stay; 5 steps, 8 images"),
    WCase(1, 6, 8, 128, 64, 1, 1, PW, "M = 48: one K-step, a partial one (prologue only)"),
    WCase(1, 10, 10, 32, 64, 3, 1, IM2COL, "M = 100: two K-steps (both prologue loads, no steady state); four taps per K tile"),
    WCase(1, 13, 13, 64, 8, 1, 1, PW, "M = 169: three K-steps; N = 8, one 16-byte chunk of the N tile"),
    WCase(2, 9, 11, 8, 64, 3, 1, IM2COL, "C = 8: Ktot = 72, a K tile of nine taps with a tail"),
    WCase(2, 12, 12, 24, 136, 3, 1, IM2COL, "C = 24: Ktot = 216 = two K tiles with a tail; N = 136: a second N tile of 8 channels"),
    WCase(3, 15, 17, 64, 64, 3, 2, IM2COL, "stride 2 on odd H and W (Ho x Wo = 8 x 9)"),
    WCase(2, 23, 19, 40, 72, 3, 1, IM2COL, "M = 874: two pixel ranges (atomics / two slabs), the second a partial last step"),
]

# The DMA kernel at the default threshold: the smallest shapes that cross 8 GFLOP, and one just below.
WGRAD_DEFAULT = [
    WCase(1, 42, 41, 512, 512, 3, 1, DMA_3X3, "8.13e9; last pixel range 186 pixels: 6 steps, a partial last one, not a multiple of the ring"),
    WCase(3, 99, 23, 256, 256, 3, 1, DMA_3X3, "8.06e9; W < 32 and no divisor of 32: image borders inside a step"),
    WCase(1, 124, 124, 1024, 256, 1, 1, DMA_PW, "8.06e9; pointwise, four K tiles"),
    WCase(1, 41, 41, 512, 512, 3, 1, IM2COL, "7.93e9: below the threshold, the 128 x 128 kernel"),
]

# Wide shapes far below the threshold.  `variant` is what they run on with FX_WGRAD_DMA_MIN_GFLOP=0 (the child process of the GPU
# test); at the default threshold all of them run on the 128 x 128 kernel.
WGRAD_WIDE_SMALL = [
    WCase(3, 17, 23, 256, 256, 3, 1, DMA_3X3, "rows wrap inside a 32-pixel step, pixel tail (M = 1173)"),
    WCase(1, 24, 23, 256, 256, 3, 1, DMA_3X3, "M = 552: the last range is 40 pixels, fewer steps than ring stages"),
    WCase(2, 8, 4, 256, 256, 3, 1, DMA_3X3, "a step is exactly one image (32 / W = H): the row carry wraps to the same row"),
    WCase(64, 5, 5, 256, 256, 3, 1, IM2COL, "a step is more than one image (ceil(32 / W) > H): the one-carry row update of the DMA "
                                               "kernel would leave the image, so the shape is routed to the 128 x 128 kernel"),
    WCase(2, 25, 31, 256, 512, 1, 1, DMA_PW, "pointwise, M = 1550 (tail), N = 512"),
    WCase(1, 20, 20, 512, 512, 3, 1, DMA_3X3, "two K tiles per tap, 2 x 18 tiles"),
]

ALL_WGRAD = WGRAD_SMALL + WGRAD_DEFAULT + WGRAD_WIDE_SMALL


def wid(c):
    return f"{c.B}x{c.H}x{c.W}-c{c.C}-n{c.N}-k{c.k}s{c.stride}"


def out_hw(c):
    pad = (c.k - 1) // 2
    return (c.H + 2 * pad - c.k) // c.stride + 1, (c.W + 2 * pad - c.k) // c.stride + 1


def pixels(c):
    Ho, Wo = out_hw(c)
    return c.B * Ho * Wo


def gflop(c):
    return 2.0 * pixels(c) * c.N * c.C * c.k * c.k / 1e9


def exact_run_is_exact(M):
    """Integer run: |x|, |dz| <= 2 and an integer prefill |.| <= 8, so every partial sum of a dW element is an integer of magnitude
    <= 4 M + 8 < 2^24 - exact in fp32 in any order (atomics, pixel splits, the slab sum); a dbias sum is <= 2 M + 8."""
    return 4 * M + 8 < 2 ** 24


def wgrad_inputs(c, kind):
    """x [B,H,W,C], dz [B,Ho,Wo,N] (fp32 holding bf16 values), the dW prefill [N,k,k,C], the dbias prefill [N] and the per-channel scale
    [N] of the unpack pass (powers of two: exact).  kind "int": integers in [-2, 2] (prefill in [-8, 8]); "gauss": unit normals."""
    Ho, Wo = out_hw(c)
    g = gen(_seed(c.B, c.H, c.W, c.C, c.N, c.k, c.stride, int(kind == "int")))
    if kind == "int":
        x = torch.randint(-2, 3, (c.B, c.H, c.W, c.C), generator=g).float()
        dz = torch.randint(-2, 3, (c.B, Ho, Wo, c.N), generator=g).float()
        pre = torch.randint(-8, 9, (c.N, c.k, c.k, c.C), generator=g).float()
        bpre = torch.randint(-8, 9, (c.N,), generator=g).float()
    else:
        x, dz = bf(torch.randn(c.B, c.H, c.W, c.C, generator=g)), bf(torch.randn(c.B, Ho, Wo, c.N, generator=g))
        pre, bpre = torch.randn(c.N, c.k, c.k, c.C, generator=g), torch.randn(c.N, generator=g)
    scale = 2.0 ** torch.randint(-1, 2, (c.N,), generator=g).float()
    return {"x": x, "dz": dz, "pre": pre, "bpre": bpre, "scale": scale}


def wgrad_ref64(x, dz, k, stride):
    """ref[n][kh][kw][c] = sum_m dz[m][n] * x[pix(m, kh, kw)][c] in float64 by unfold + one matmul, mag the same sum over |dz|, |x|;
    dbias[n] = sum_m dz[m][n] with magnitude sum_m |dz[m][n]|.  On x's device.  Returns (ref, mag, dbias, dbias_mag), ref [N,k,k,C]."""
    B, H, W, C = x.shape
    N = dz.shape[-1]
    pad = (k - 1) // 2
    cols = F.unfold(x.double().permute(0, 3, 1, 2), (k, k), padding=pad, stride=stride)      # [B, C*k*k, Ho*Wo], row = (c, kh, kw)
    cols = cols.permute(1, 0, 2).reshape(C * k * k, -1)                                       # [C*k*k, M]
    z = dz.to(x.device).double().reshape(-1, N)                                               # [M, N]
    assert cols.shape[1] == z.shape[0]
    shape = lambda t: t.reshape(C, k, k, N).permute(3, 1, 2, 0).contiguous()                  # noqa: E731
    return shape(cols @ z), shape(cols.abs() @ z.abs()), z.sum(0), z.abs().sum(0)


def nckk(t):
    """[N,k,k,C] -> [N,C,k,k] (the master layout fx_unpack_conv_wgrad_sum_f32 writes)."""
    return t.permute(0, 3, 1, 2).contiguous()


# fx_linear_wgrad_bias_bf16: R, Kp, Np, k_store, n_store, ld_dw, with_bias
LCase = namedtuple("LCase", "R Kp Np k_store n_store ld_dw bias note")
LINEAR_CASES = [
    LCase(600, 256, 8, 256, 4, 256, True, "bbox head: 4 of 8 output rows stored"),
    LCase(600, 256, 368, 256, 365, 256, True, "class head: 365 of 368 rows, three N tiles, two K tiles"),
    LCase(600, 32, 512, 4, 512, 4, True, "query-pos head: 4 of 32 columns stored, row stride 4"),
    LCase(600, 32, 16, 4, 12, 7, True, "ld_dw > k_store: the columns between them keep their bits"),
    LCase(600, 256, 8, 256, 4, 256, False, "dbias = None"),
]


def lid(c):
    return f"r{c.R}-k{c.k_store}of{c.Kp}-n{c.n_store}of{c.Np}-ld{c.ld_dw}{'' if c.bias else '-nobias'}"


def linear_inputs(c, kind):
    """x [R,Kp], dz [R,Np], the dW prefill [n_store,k_store] and the dbias prefill [n_store].  In train_nn.py the columns past k_store /
    n_store are zero padding; here they hold values like the others, because the entry point's contract is that ONLY the corner is
    accumulated: over zero padding a store outside the corner adds 0.0 and leaves no trace (mutation study)."""
    g = gen(_seed(c.R, c.Kp, c.Np, c.k_store, c.n_store, c.ld_dw, int(kind == "int")))
    if kind == "int":
        x, dz = torch.randint(-2, 3, (c.R, c.Kp), generator=g).float(), torch.randint(-2, 3, (c.R, c.Np), generator=g).float()
        pre, bpre = torch.randint(-8, 9, (c.n_store, c.k_store), generator=g).float(), torch.randint(-8, 9, (c.n_store,), generator=g).float()
    else:
        x, dz = bf(torch.randn(c.R, c.Kp, generator=g)), bf(torch.randn(c.R, c.Np, generator=g))
        pre, bpre = torch.randn(c.n_store, c.k_store, generator=g), torch.randn(c.n_store, generator=g)
    return {"x": x, "dz": dz, "pre": pre, "bpre": bpre}


def linear_ref64(x, dz, c):
    """dW[n][k] = sum_r dz[r][n] x[r][k] over the stored corner, dbias[n] = sum_r dz[r][n]; (ref, mag, dbias, dbias_mag)."""
    z, xx = dz.double()[:, :c.n_store], x.double()[:, :c.k_store]
    ref, mag = gemm_ref64(z.T, xx.T)                                                         # [n_store, R] x [k_store, R]^T
    return ref, mag, z.sum(0), z.abs().sum(0)


# ------------------------------------------------------------------------------------------------ attention backward
# B, heads, Lq, Lk.  Lengths from {1, 31, 32, 33, 128, 129, 256, 257}: one partial 32-row tile (1, 31, 33), the query-chunk boundary of
# the dK / dV kernel (AB_QT = 4 tiles: 128 / 129), the key-chunk boundary of the dQ kernel (AB_CT = 8 tiles: 256 / 257), a second grid
# block of either kernel (129 and up).
MCase = namedtuple("MCase", "B heads Lq Lk")
MHA_BWD_CASES = [
    MCase(2, 1, 1, 1),
    MCase(2, 2, 31, 33),
    MCase(1, 8, 32, 32),
    MCase(2, 8, 33, 257),
    MCase(2, 8, 257, 33),
    MCase(1, 2, 128, 256),
    MCase(1, 8, 129, 257),
    MCase(2, 1, 256, 129),
    MCase(1, 2, 1, 257),
    MCase(1, 1, 257, 1),
]
MHA_BWD_BIG = MCase(1, 8, 129, 257)        # scores of magnitude ~60
MHA_BWD_UNIFORM = MCase(1, 2, 129, 257)    # K = 0: uniform attention


def mid(c):
    return f"b{c.B}h{c.heads}-{c.Lq}x{c.Lk}"


def mask_plan(rows):
    """Planted mask rows (flat over batch x query): a fully masked one (attends everywhere), a fully open one, one whose only allowed
    key is the LAST key (it lies in the last, possibly partial, 32-key tile) - at the front and, where there is room, at the end."""
    plan = [(0, "masked"), (1, "open"), (2, "last")][:rows]
    if rows >= 6:
        plan += [(rows - 1, "masked"), (rows - 2, "last"), (rows - 3, "open")]
    return plan


def mha_bwd_ref64(q, k, v, do, mask, heads):
    """Closed form of the header of csrc/attn_bwd.hip in float64.  q, do [B,Lq,E], k, v [B,Lk,E], mask bool [B,Lq,Lk] (True = key not
    allowed, shared by the heads; a query whose mask forbids every key attends everywhere) or None.
    S = Q K^T / sqrt(32), P = softmax(S), dP = dO V^T, D = sum_j P dP, dS = P (dP - D), dQ = dS K / sqrt(32), dK = dS^T Q / sqrt(32),
    dV = P^T dO; the magnitudes are the same formulas on absolute values (P is positive):  dPmag = |dO| |V|^T, Dmag = sum_j P dPmag,
    dSmag = P (dPmag + Dmag), dQmag = dSmag |K| / sqrt(32), dKmag = dSmag^T |Q| / sqrt(32), dVmag = P^T |dO|."""
    B, Lq, E = q.shape
    sc = 1.0 / math.sqrt(32.0)
    split = lambda t: t.double().view(B, -1, heads, 32).transpose(1, 2)        # noqa: E731  [B, heads, L, 32]
    merge = lambda t: t.transpose(1, 2).reshape(B, -1, E)                       # noqa: E731
    qh, kh, vh, dh = split(q), split(k), split(v), split(do)
    s = qh @ kh.transpose(-1, -2) * sc
    if mask is not None:
        eff = mask & ~mask.all(-1, keepdim=True)
        s = s.masked_fill(eff[:, None], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    dp, dpm = dh @ vh.transpose(-1, -2), dh.abs() @ vh.abs().transpose(-1, -2)
    d, dm = (p * dp).sum(-1, keepdim=True), (p * dpm).sum(-1, keepdim=True)
    ds, dsm = p * (dp - d), p * (dpm + dm)
    return {"p": p, "smax": float(s[torch.isfinite(s)].abs().max()),
            "dq": merge(ds @ kh * sc), "dk": merge(ds.transpose(-1, -2) @ qh * sc), "dv": merge(p.transpose(-1, -2) @ dh),
            "dq_mag": merge(dsm @ kh.abs() * sc), "dk_mag": merge(dsm.transpose(-1, -2) @ qh.abs() * sc),
            "dv_mag": merge(p.transpose(-1, -2) @ dh.abs())}


def mha_bwd_case(c, masked, big=False, uniform=False):
    """Inputs (bf16 values), mask with its planted rows (`plan`), float64 references and magnitudes.  big: q, k scaled so that scores
    reach ~60 (the running maximum of the statistics sweep rises from tile to tile).  uniform: K = 0, so P = 1 / (allowed keys), dQ = 0
    exactly and every key and query tile carries the same share of dV."""
    B, heads, Lq, Lk = c
    E = heads * 32
    g = gen(Lq * 100003 + Lk * 101 + heads * 7 + B + int(masked) * 2 + int(big) + 4 * int(uniform))
    sc = 4.5 if big else 1.5
    q, k = bf(torch.randn(B, Lq, E, generator=g) * sc), bf(torch.randn(B, Lk, E, generator=g) * sc)
    v, do = bf(torch.randn(B, Lk, E, generator=g)), bf(torch.randn(B, Lq, E, generator=g))
    if uniform:
        k = torch.zeros_like(k)
    mask, plan = None, []
    if masked:
        mask = torch.rand(B * Lq, Lk, generator=g) < 0.5
        only_last = torch.ones(Lk, dtype=torch.bool)
        only_last[Lk - 1] = False
        plan = mask_plan(B * Lq)
        for row, kind in plan:
            mask[row] = {"masked": torch.ones(Lk, dtype=torch.bool), "open": torch.zeros(Lk, dtype=torch.bool), "last": only_last}[kind]
        mask = mask.view(B, Lq, Lk)
    out = {"B": B, "heads": heads, "Lq": Lq, "Lk": Lk, "q": q, "k": k, "v": v, "do": do, "mask": mask, "plan": plan}
    out.update(mha_bwd_ref64(q, k, v, do, mask, heads))
    return out


def mask_words(mask):
    """bool [B, Lq, Lk] -> int32 [B * Lq, ceil(Lk / 32)]: bit (key & 31) of word key / 32 set = key not allowed; bits past Lk are set."""
    B, Lq, Lk = mask.shape
    T = (Lk + 31) // 32
    m = torch.ones(B * Lq, T * 32, dtype=torch.bool)
    m[:, :Lk] = mask.reshape(B * Lq, Lk)
    w = (m.view(B * Lq, T, 32).long() << torch.arange(32)).sum(-1)      # < 2^32
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
