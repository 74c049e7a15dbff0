"""Shared by tests/test_train_norm_cases_cpu.py and tests/test_gpu_train_norm_ops.py: the inputs of every case of the train-mode BatchNorm
kernels (fx_bn_stats_bf16, fx_bn_finalize_f32, fx_bn_apply_bf16, fx_bn_bwd_stats_bf16, fx_bn_bwd_apply_bf16), the two pooling backward
kernels and the weight packers / gradient unpackers of csrc/train_conv_ops.hip, seeded and already rounded to the element type (`dtype`:
torch.bfloat16 or torch.float16) where the kernel reads the 16-bit element, with the float64 reference of the operation and its float64
magnitude `mag`: the same expression with every term taken in absolute value, which bounds the fp32 error where terms cancel.

Every BatchNorm kernel is a case ON ITS OWN: the per-channel vectors it consumes (scale, shift, mean, rstd, sums) are chosen here, not
produced by the kernel before it, so an error two kernels share cannot cancel.  The weight images are written out from the layout
comments of include/focoos_amd.h, never taken from another kernel.  Nothing here touches a GPU or the library; the CPU test checks every
reference against an independent formulation and asserts the structural properties the GPU cases rely on."""
import math

import torch

from tests.helpers import U32, act64, elem_rne, frag_order

ELEMS = {"bf16": torch.bfloat16, "fp16": torch.float16}
GRID_CAP_THREADS = 256 * 32 * 256          # a capped grid: 256 * 32 workgroups of 256 threads, one group of eight channels per thread and trip
ACTS = ("none", "relu", "silu", "gelu")
SENT16 = 0x5A5A


def gen(seed):
    return torch.Generator().manual_seed(seed)


def el(t, dtype):
    """Round to the element type, keep as fp32 (every value exactly representable in `dtype`)."""
    return t.to(dtype).float()


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    """The fp32 value a C float argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


def randint(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def first_second_trip_row(C):
    """First row of a [rows][C] matrix whose groups of eight are handled by a thread's SECOND trip through a capped grid-stride loop."""
    return GRID_CAP_THREADS // (C // 8)


# ------------------------------------------------------------------------------------------------ BatchNorm: shapes and launch rules
# (rows, C): the smallest shapes at which each thread layout and edge of bn_reduce_kernel occurs (see bn_layout / the CPU test)
BN_SHAPES = [(1, 8), (7, 24), (255, 32), (1024, 64), (1025, 64), (2049, 128), (256, 256), (257, 264), (300, 288), (513, 320), (300, 384),
             (600, 520)]
BN_KINDS = ("gauss", "mean30")
BN_CAP_SHAPE = (8200, 2048)                # 2 099 200 groups of eight > GRID_CAP_THREADS


def bn_rows_per_block(C):
    return 256 if C >= 256 else 1024


def bn_layout(C):
    """Per column block of 256 channels: (channels left, column groups, row lanes) - 32 x 8, or 4 x 64 / 8 x 32 / 16 x 16 when exactly 32 /
    64 / 128 channels are left."""
    out = []
    for blk in range(cdiv(C, 256)):
        cb = C - blk * 256
        ncg = {32: 4, 64: 8, 128: 16}.get(cb, 32)
        out.append((cb, ncg, 256 // ncg))
    return out


def bn_row_blocks(rows, C):
    return cdiv(rows, bn_rows_per_block(C))


def bn_sum_bound(rows):
    """The most c a gate of a sum of `rows` fp32 terms may allow: rows * 2^-24."""
    return rows * U32


def act_grad64(a, act):
    if act == "none":
        return torch.ones_like(a)
    if act == "relu":
        return (a > 0).double()
    if act == "silu":
        s = torch.sigmoid(a)
        return s * (1 + a * (1 - s))
    assert act == "gelu"
    return 0.5 * (1 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)


def bn_case(shape, dtype, kind, z_f32):
    """kind 'int': small integers and power-of-two vectors (every partial sum an integer multiple of 1/8 below 2^21: exact in fp32 in any
    order).  'gauss': channels with their own mean and spread; 'mean30': mean 30, sigma 0.5 (sum z^2 - mean^2 loses digits).  z is fp32
    when z_f32, else rounded to the element type; dy and the residual are always elements."""
    rows, C = shape
    g = gen(rows * 10007 + C * 13 + {"int": 0, "gauss": 1, "mean30": 2}[kind] + 5 * int(z_f32) + (100 if dtype == torch.float16 else 0))
    c = {"rows": rows, "C": C, "kind": kind}
    if kind == "int":
        c["z"], c["dy"], c["res"] = randint(-4, 4, (rows, C), g), randint(-3, 3, (rows, C), g), randint(-2, 2, (rows, C), g)
        sign = lambda: randint(0, 1, (C,), g) * 2 - 1                                           # noqa: E731
        c["scale"], c["shift"] = sign() * 2.0 ** randint(-1, 1, (C,), g), sign() * 2.0 ** randint(-1, 1, (C,), g)
        c["mean"], c["rstd"] = sign() * 2.0 ** randint(0, 1, (C,), g), 2.0 ** randint(-1, 2, (C,), g)
        c["pre"] = randint(-5, 5, (2, C), g)
    else:
        m = torch.full((C,), 30.0) if kind == "mean30" else torch.randn(C, generator=g) * 2
        sd = torch.full((C,), 0.5) if kind == "mean30" else 0.25 + 2 * torch.rand(C, generator=g)
        z = m + sd * torch.randn(rows, C, generator=g)
        c["z"] = z if z_f32 else el(z, dtype)
        c["dy"], c["res"] = el(torch.randn(rows, C, generator=g), dtype), el(torch.randn(rows, C, generator=g), dtype)
        gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
        c["mean"], c["rstd"] = m.clone(), 1.0 / sd
        c["scale"] = gamma * c["rstd"]
        c["shift"] = beta - c["mean"] * c["scale"]
        c["pre"] = torch.randn(2, C, generator=g) * 10
    c["sums"] = torch.randn(2, C, generator=g) * (0.1 * rows)            # what fx_bn_bwd_apply_bf16 is GIVEN as the reduction result
    c["acc_pre"] = torch.randn(2, C, generator=g)                        # dgamma_acc, dbeta_acc before the call
    c["inv_n"] = f32(1.0 / rows)
    return c


def bn_pre64(c, residual):
    """a = z * scale + shift (+ residual) and its magnitude."""
    z = c["z"].double()
    a, amag = z * c["scale"].double() + c["shift"].double(), (z * c["scale"].double()).abs() + c["shift"].double().abs()
    if residual:
        a, amag = a + c["res"].double(), amag + c["res"].double().abs()
    return a, amag


def relu_excluded(a, amag, act):
    """Elements whose fp64 pre-activation lies within 2^-20 of its magnitude of zero: the sign fp32 gives it is not determined."""
    return (a.abs() <= 2.0 ** -20 * amag) if act == "relu" else torch.zeros_like(a, dtype=torch.bool)


def bn_stats_ref(c):
    z, pre = c["z"].double(), c["pre"].double()
    return (torch.stack([pre[0] + z.sum(0), pre[1] + (z * z).sum(0)]),
            torch.stack([pre[0].abs() + z.abs().sum(0), pre[1].abs() + (z * z).sum(0)]))


def bn_da64(c, act, residual):
    """da = dy * act'(a); its magnitude |dy| * (|act'(a)| + |a|_mag for the smooth activations, whose slope moves with the fp32 error of
    a); the ReLU elements left out."""
    a, amag = bn_pre64(c, residual)
    gr = act_grad64(a, act)
    dy = c["dy"].double()
    smooth = amag if act in ("silu", "gelu") else 0.0
    return dy * gr, dy.abs() * (gr.abs() + smooth), relu_excluded(a, amag, act)


def bn_xhat64(c):
    return (c["z"].double() - c["mean"].double()) * c["rstd"].double()


def bn_bwd_stats_ref(c, act, residual):
    """sums[c] = pre + sum da, sums[C + c] = pre + sum da * xhat; (ref, mag, allowance for the left-out ReLU elements), each [2, C]."""
    da, damag, ex = bn_da64(c, act, residual)
    xh, pre = bn_xhat64(c), c["pre"].double()
    dyx = c["dy"].double().abs() * ex
    return (torch.stack([pre[0] + da.sum(0), pre[1] + (da * xh).sum(0)]),
            torch.stack([pre[0].abs() + damag.sum(0), pre[1].abs() + (damag * xh.abs()).sum(0)]),
            torch.stack([dyx.sum(0), (dyx * xh.abs()).sum(0)]))


def bn_apply_ref(c, act, residual, first_row=0):
    a, amag = bn_pre64(c, residual)
    return act64(a, act)[first_row:], amag[first_row:]


def bn_bwd_apply_ref(c, act, residual):
    """dz = scale * (da - sums[c] * inv_n - xhat * sums[C + c] * inv_n) with the GIVEN sums; (da, damag, dz, dzmag, left out)."""
    da, damag, ex = bn_da64(c, act, residual)
    xh, s, inv_n, sc = bn_xhat64(c), c["sums"].double(), c["inv_n"], c["scale"].double()
    dz = sc * (da - s[0] * inv_n - xh * s[1] * inv_n)
    dzmag = sc.abs() * (damag + s[0].abs() * inv_n + xh.abs() * s[1].abs() * inv_n)
    return da, damag, dz, dzmag, ex


def bn_cap_case(dtype, tail_rows):
    """The last `tail_rows` rows of the 8200 x 2048 grid-cap case, with their own per-channel vectors; the rows before them are generated
    on the device by the test (they are never compared)."""
    rows, C = BN_CAP_SHAPE
    c = bn_case((tail_rows, C), dtype, "gauss", False)
    c["inv_n"] = f32(1.0 / rows)
    return c


# ------------------------------------------------------------------------------------------------ BatchNorm finalize
FIN_C = (8, 264, 520)
FIN_N = (1, 2, 297, 1638400)
FIN_EPS, FIN_MOMENTUM = f32(1e-5), f32(0.1)
FIN_CONST, FIN_NEG, FIN_WIDE = 0, 1, 2     # planted channels


def finalize_case(C, n):
    """sums of n values per channel, as fp32.  Channel 0: a constant 1.5 (sum z^2 / n == mean^2 exactly: variance 0).  Channel 1: mean 30
    and a sum of squares eight fp32 steps BELOW n * 900: the variance is negative (-8.6e-4, far beyond eps) and must be clamped - without
    the clamp rsqrt sees a negative number.  Channel 2: mean 0.5, variance 10^4."""
    g = gen(C * 31 + n % 9973)
    m, var = torch.randn(C, generator=g) * 2, (0.25 + 2 * torch.rand(C, generator=g)) ** 2
    m[FIN_WIDE], var[FIN_WIDE] = 0.5, 1.0e4
    s0, s1 = (n * m.double()).float(), (n * (var.double() + m.double() ** 2)).float()
    s0[FIN_CONST], s1[FIN_CONST] = n * 1.5, n * 2.25
    s0[FIN_NEG] = n * 30.0
    below = torch.tensor(n * 900.0, dtype=torch.float32)
    for _ in range(8):
        below = torch.nextafter(below, torch.tensor(0.0))
    s1[FIN_NEG] = below
    return {"C": C, "n": n, "sums": torch.stack([s0, s1]), "gamma": 1 + 0.3 * torch.randn(C, generator=g), "beta": 0.2 * torch.randn(C, generator=g),
            "running_mean": torch.randn(C, generator=g), "running_var": 0.5 + torch.rand(C, generator=g), "nbt": 41}


def finalize_ref(c):
    """nn.BatchNorm2d's training step written out (F.batch_norm refuses n = 1): name -> (ref, mag).  The variance is a difference of two
    fp32 quantities of size var_mag = sum z^2 / n + mean^2, so rstd carries 0.5 * rstd^3 * var_mag next to its own size."""
    n, s, mom = float(c["n"]), c["sums"].double(), FIN_MOMENTUM
    m, q = s[0] / n, s[1] / n
    var = (q - m * m).clamp_min(0)
    var_mag = q.abs() + m * m
    r = 1.0 / torch.sqrt(var + FIN_EPS)
    r_mag = r + 0.5 * r ** 3 * var_mag
    ga, be = c["gamma"].double(), c["beta"].double()
    sc = ga * r
    unb = n / (n - 1.0) if n > 1 else 1.0
    rm, rv = c["running_mean"].double(), c["running_var"].double()
    return {"mean": (m, m.abs()), "rstd": (r, r_mag), "scale": (sc, ga.abs() * r_mag), "shift": (be - m * sc, be.abs() + m.abs() * ga.abs() * r_mag),
            "running_mean": ((1 - mom) * rm + mom * m, (1 - mom) * rm.abs() + mom * m.abs()),
            "running_var": ((1 - mom) * rv + mom * var * unb, (1 - mom) * rv.abs() + mom * var_mag * unb), "var": (var, var_mag)}


# ------------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1) backward
MP_SHAPES = [(1, 1, 1, 8), (2, 2, 2, 8), (1, 3, 5, 24), (2, 6, 6, 16), (2, 13, 15, 16), (1, 12, 16, 40)]        # B, H, W, C
MP_VARIANTS = ("relu", "const", "same", "diverging")
AP_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 8), (2, 13, 15, 24), (1, 12, 16, 16)]
POOL_CAP_SHAPE = (1, 65, 127, 2048)        # 8255 pixels x 256 groups of eight > GRID_CAP_THREADS; pixel 8192 = (row 64, column 64)
POOL_CAP_TAIL = 60                         # the reference of the tail is computed on input rows 60 .. 64: an even first row keeps the windows aligned


def mp_out(n):
    return (n - 1) // 2 + 1


def ap_out(n):
    return (n + 1) // 2


def _distinct(B, H, W, C, g, per_channel):
    """Distinct values k / 256 (k = 1 .. H * W <= 255: exact in both element types) per image plane: one permutation per group of eight
    channels (all eight alike) or one per channel."""
    n = H * W
    assert n <= 255
    x = torch.empty(B, n, C)
    for b in range(B):
        for ch in range(0, C, 1 if per_channel else 8):
            p = (torch.randperm(n, generator=g) + 1).float() / 256
            x[b, :, ch:ch + (1 if per_channel else 8)] = p[:, None]
    return x.reshape(B, H, W, C)


def maxpool_case(shape, dtype, variant):
    """x in the element type, dy integers in [-3, 3] (dx is then a sum of at most four integers: exact)."""
    B, H, W, C = shape
    g = gen(B * 1000003 + H * 10007 + W * 101 + C + MP_VARIANTS.index(variant))
    if variant == "relu":
        x = el(torch.randn(B, H, W, C, generator=g).clamp_min(0), dtype)
    elif variant == "const":
        x = torch.full((B, H, W, C), 0.75)
    else:
        x = _distinct(B, H, W, C, g, per_channel=variant == "diverging")
    return {"x": x, "dy": randint(-3, 3, (B, mp_out(H), mp_out(W), C), g)}


def maxpool_argmax(x):
    """tap (kh * 3 + kw) of the FIRST maximum of every window in kh-major scan order: a later in-bounds tap wins only if strictly greater."""
    B, H, W, C = x.shape
    Ho, Wo = mp_out(H), mp_out(W)
    xp = torch.full((B, 2 * Ho + 1, 2 * Wo + 1, C), float("-inf"), dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    arg = torch.full((B, Ho, Wo, C), -1, dtype=torch.long)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            upd = v > best
            best = torch.where(upd, v, best)
            arg = torch.where(upd, torch.full_like(arg, kh * 3 + kw), arg)
    return arg


def maxpool_bwd64(x, dy):
    """dx: every window's dy scattered onto the pixel of its first maximum, fp64."""
    B, H, W, C = x.shape
    Ho, Wo = mp_out(H), mp_out(W)
    arg = maxpool_argmax(x)
    dxp = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dxp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += dy.double() * (arg == kh * 3 + kw)
    return dxp[:, 1:H + 1, 1:W + 1]


def maxpool_paths(x):
    """(windows x groups of eight whose channels all chose one tap: the fast path; those that chose several: the mixed path)."""
    arg = maxpool_argmax(x)
    a8 = arg.reshape(*arg.shape[:3], -1, 8)
    same = (a8 == a8[..., :1]).all(-1)
    return int(same.sum()), int((~same).sum())


def avgpool_case(shape, dtype):
    B, H, W, C = shape
    return {"dp": el(torch.randn(B, ap_out(H), ap_out(W), C, generator=gen(B * 7 + H * 1009 + W * 31 + C)) * 2, dtype)}


def avgpool_bwd64(dp, H, W):
    """AvgPool2d(2, 2, 0, ceil_mode=True) backward: dx[y, x] = dp[y // 2, x // 2] / (in-bounds taps of that window)."""
    ys, xs = torch.arange(H), torch.arange(W)
    cnt_h = torch.where(2 * (ys // 2) + 1 < H, 2, 1)
    cnt_w = torch.where(2 * (xs // 2) + 1 < W, 2, 1)
    cnt = (cnt_h[:, None] * cnt_w[None, :]).double()
    return dp.double()[:, ys // 2][:, :, xs // 2] / cnt[None, :, :, None]


# ------------------------------------------------------------------------------------------------ weight images
PACK_CONV_SHAPES = [(40, 24, 3, 3), (64, 32, 3, 3), (32, 16, 1, 1), (256, 64, 1, 1), (8, 3, 7, 7), (512, 256, 3, 3)]      # N, C, KH, KW
PACK_CONV_MODES = ("both", "fwd", "dgrad")
PACK_FRAG_SHAPES = [(32, 16), (96, 48), (2048, 4608)]
PACK_LINEAR_SHAPES = [(365, 256, 368, 256), (512, 4, 512, 32), (4, 256, 16, 256)]                                       # N, K, Np, Kp
PACK_CAP_BLOCKS = 4096
PK_TILE = 2304


def packed_values(w, scale, dtype):
    """The fp32 product w * scale[n], rounded once to the element type."""
    v = w if scale is None else w * scale.reshape(-1, *([1] * (w.dim() - 1)))
    assert v.dtype == torch.float32
    return v.to(dtype)


def weights_case(N, C, KH, KW, seed=0):
    g = gen(N * 100003 + C * 1009 + KH * 31 + KW + seed)
    return {"w": torch.randn(N, C, KH, KW, generator=g) * 0.5, "scale": 0.5 + torch.rand(N, generator=g), "bias": torch.randn(N, generator=g)}


def fwd_image(v):
    """[N][C][KH][KW] -> w_fwd [N][KH][KW][C] as [N, KH * KW * C]."""
    return v.permute(0, 2, 3, 1).reshape(v.shape[0], -1)


def dgrad_image(v):
    """w_dgrad[c][kh][kw][n] = v[n][c][KH-1-kh][KW-1-kw] as [C, KH * KW * N]."""
    return v.flip(2, 3).permute(1, 2, 3, 0).reshape(v.shape[1], -1)


def frag_eligible(rows, K):
    return rows % 32 == 0 and K % 16 == 0


def pack_chunk(C, T):
    """Input channels per tile of the multi-tensor packer: <= PK_TILE (channel, tap) elements, a multiple of 8 (at least 8), or all of C."""
    return min(C, max(8, (PK_TILE // T) // 8 * 8))


def pack_blocks(N, C, KH, KW):
    """Workgroups of one entry: tiles of 8 output channels x chunks of input channels; -1 for filters of more than PK_TILE / 8 taps."""
    if KH * KW > PK_TILE // 8:
        return -1
    return cdiv(N, 8) * cdiv(C, pack_chunk(C, KH * KW))


# name, N, C, KH, KW, scale, bias, fwd frag, dgrad image, dgrad frag, ld_fwd - row length, image group
PACK_TABLE = [
    ("c3x3_256", 32, 256, 3, 3, True, False, True, True, True, 0, None),        # exactly one PK_TILE chunk
    ("c3x3_264", 16, 264, 3, 3, True, False, False, True, False, 8, None),      # second chunk 8 channels wide; ld_fwd above the row length
    ("pw_2304", 32, 2304, 1, 1, False, False, True, True, True, 0, None),       # pointwise, one chunk; no scale
    ("pw_2312", 8, 2312, 1, 1, True, False, False, False, False, 0, None),      # second chunk 8 wide; no dgrad image
    ("lin_365", 365, 256, 1, 1, False, True, False, True, False, 0, None),      # last tile: 5 output channels; n_total % 8 != 0: element dgrad stores
    ("lin_k4", 16, 4, 1, 1, False, True, False, True, False, 28, None),         # C = 4: element forward stores; Kp = 32
    ("stem7x7", 8, 3, 7, 7, True, False, False, True, False, 0, None),          # C = 3, 49 taps: element forward stores
    ("v0", 256, 64, 3, 3, True, True, True, True, True, 0, "v"),                # three masters sharing the images of 768 output channels
    ("v1", 256, 64, 3, 3, False, True, True, True, True, 0, "v"),
    ("v2", 256, 64, 3, 3, True, True, True, True, True, 0, "v"),
]


def pack_table_case(dtype):
    """Entries (dicts) and the expected images: name -> int16 bit tensor of the WHOLE image allocation, the sentinel wherever the documented
    layout writes nothing.  w_fwd row (n_offset + n) at ld_fwd, column (kh * KW + kw) * C + c; w_dgrad row c at ld_dgrad, column
    ((KH-1-kh) * KW + (KW-1-kw)) * n_total + n_offset + n; the fragment copies are frag_order of the dense [n_total][T * C] and
    [C][T * n_total] matrices; bias_out[n_offset + n] = bias[n]."""
    entries, images, first = [], {}, 0
    groups, lds = {}, {}
    for row in PACK_TABLE:
        if row[-1]:
            groups[row[-1]] = groups.get(row[-1], 0) + row[1]
    offs = {}
    for k, (name, N, C, KH, KW, has_scale, has_bias, ffrag, dimg, dfrag, ld_extra, grp) in enumerate(PACK_TABLE):
        T = KH * KW
        d = weights_case(N, C, KH, KW, seed=k)
        n_total = groups[grp] if grp else N
        n_off = offs.get(grp, 0) if grp else 0
        if grp:
            offs[grp] = n_off + N
        key = grp or name
        ld_fwd = T * C + ld_extra
        ld_dgrad = cdiv(T * n_total, 8) * 8
        v = packed_values(d["w"], d["scale"] if has_scale else None, dtype)
        e = {"name": name, "key": key, "N": N, "C": C, "KH": KH, "KW": KW, "w": d["w"], "scale": d["scale"] if has_scale else None,
             "bias": d["bias"] if has_bias else None, "fwd_frag": ffrag, "dgrad": dimg, "dgrad_frag": dfrag, "ld_fwd": ld_fwd, "ld_dgrad": ld_dgrad,
             "first_block": first, "n_offset": n_off, "n_total": n_total, "blocks": pack_blocks(N, C, KH, KW)}
        first += e["blocks"]
        entries.append(e)
        vb = v.view(torch.int16)
        img = images.setdefault(key + ".fwd", torch.full((n_total, ld_fwd), SENT16, dtype=torch.int16))
        img[n_off:n_off + N, :T * C] = fwd_image(vb)
        if ffrag:
            dense = images.setdefault(key + ".fwd_dense", torch.zeros(n_total, T * C, dtype=torch.int16))
            dense[n_off:n_off + N] = fwd_image(vb)
        if dimg:
            lds[key + ".dgrad"] = ld_dgrad
            img = images.setdefault(key + ".dgrad_rows", torch.full((C, T, n_total), SENT16, dtype=torch.int16))
            img[:, :, n_off:n_off + N] = dgrad_image(vb).view(C, T, N)
        if dfrag:
            dense = images.setdefault(key + ".dgrad_dense", torch.zeros(C, T * n_total, dtype=torch.int16))
            dense.view(C, T, n_total)[:, :, n_off:n_off + N] = dgrad_image(vb).view(C, T, N)
        if has_bias:
            b = images.setdefault(key + ".bias", torch.full((n_total,), float("nan")))
            b[n_off:n_off + N] = d["bias"]
    for k in [k for k in images if k.endswith("_rows")]:
        rows3 = images.pop(k)
        img = torch.full((rows3.shape[0], lds[k[:-5]]), SENT16, dtype=torch.int16)
        img[:, :rows3.shape[1] * rows3.shape[2]] = rows3.reshape(rows3.shape[0], -1)
        images[k[:-5]] = img
    for k in [k for k in images if k.endswith("_dense")]:
        images[k.replace("_dense", "_frag")] = frag_order(images.pop(k)).reshape(-1)
    return entries, images, first


# ------------------------------------------------------------------------------------------------ weight-gradient unpack
# N, C, KH, KW, C_eff: C % 4 != 0 under C_eff % 4 == 0 (the stem: 3 real channels of 8), a plain 3x3, and C_eff % 4 != 0 (the generic kernel)
UNPACK_SHAPES = [(16, 3, 7, 7, 8), (8, 24, 3, 3, 24), (5, 10, 3, 3, 10)]
UNPACK_SPLITS = (1, 2, 4, 5, 6, 9)


def unpack_case(shape, splits):
    """Integer partial slabs [splits][stride] in source order [n][kh][kw][c_eff], stride 12 (11 where the slab is no multiple of 4)
    above the slab with NaN in the gap and in the columns C .. C_eff of every slab; power-of-two scales; an integer dw before the call.
    The sum over the splits is exact in any order."""
    N, C, KH, KW, Ce = shape
    g = gen(N * 1009 + C * 31 + KH + Ce * 7 + splits)
    slab = N * KH * KW * Ce
    stride = slab + (12 if slab % 4 == 0 else 11)
    part = torch.full((splits, stride), float("nan"))
    data = randint(-8, 8, (splits, N, KH, KW, C), g)
    part[:, :slab].view(splits, N, KH, KW, Ce)[..., :C] = data
    return {"part": part, "stride": stride, "slab": slab, "data": data, "scale": 2.0 ** randint(-2, 2, (N,), g), "pre": randint(-9, 9, (N, C, KH, KW), g)}


def unpack_ref(c, use_scale, accumulate):
    """dw[n][c][kh][kw] (+)= scale[n] * sum_s part[s][n][kh][kw][c]."""
    ref = c["data"].double().sum(0).permute(0, 3, 1, 2)
    if use_scale:
        ref = ref * c["scale"].double().reshape(-1, 1, 1, 1)
    return ref + c["pre"].double() if accumulate else ref
