"""Shared by tests/test_seg_head_cases_cpu.py and tests/test_gpu_seg_head_ops.py: the inputs of every case of the small kernels that carry
BiSeNetFormer, the STDC stride-2 bottleneck, the classifier heads and the MaskFormer FPN (csrc/seg_ops.hip: depthwise 3x3 stride-2
conv, global mean, pooled linear, channel gate; csrc/train_seg_ops.hip: depthwise backward, row dot, vector broadcast, planes to rows;
csrc/mask_ops.hip: nearest-upsample add and its adjoint), seeded and already rounded to the element type (`dtype`: torch.bfloat16 or
torch.float16) where the kernel reads the 16-bit element, with the float64 reference of the operation and its float64 magnitude `mag`:
the same expression with every term taken in absolute value, which bounds the fp32 error where terms cancel.

The references are written out plainly (shifted slices, index maps, sums); nothing here touches a GPU or the library.  The CPU test
checks every one of them against an independent formulation (F.conv2d(groups=C) and its autograd, F.interpolate, F.linear, ...) and
asserts the structural properties the GPU cases rely on."""
import math

import torch

from tests.helpers import U32, elem_rne

ELEMS = {"bf16": torch.bfloat16, "fp16": torch.float16}
GRID_CAP_THREADS = 256 * 32 * 256          # a capped grid: 256 * 32 workgroups of 256 threads, one group of eight channels per thread and trip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def el(t, dtype):
    """Round to the element type, keep as fp32 (every value exactly representable in `dtype`)."""
    return t.to(dtype).float()


def cdiv(a, b):
    return -(-a // b)


def first_second_trip_row(C):
    """First row of a [rows][C] matrix whose groups of eight are handled by a thread's SECOND trip through a capped grid-stride loop."""
    return GRID_CAP_THREADS // (C // 8)


# ------------------------------------------------------------------------------------------------ depthwise 3x3 stride 2, pad 1
DW_SHAPES = [(1, 1, 1, 8), (2, 1, 7, 16), (2, 6, 1, 16), (1, 2, 2, 24), (2, 7, 9, 72), (1, 13, 15, 264)]      # B, H, W, C
DW_VARIANTS = ("bias", "nobias", "avg")
# P = B * Ho * Wo = 512 (one split; C = 72: the second channel group has one live lane group of eight) and 513 (two splits, per = 257)
DW_WGRAD_SHAPES = DW_SHAPES + [(2, 32, 32, 72), (1, 53, 37, 16)]
DW_CAP_SHAPE = (1, 257, 257, 2048)         # ceil(P / 512) * ceil(C / 64) = 33 * 32 > 1024: the split cap
DW_CAP_SLICE = 256                         # its reference is computed per 256-channel slice
DW_TRIP_SHAPE = (1, 181, 181, 2048)        # 91 x 91 = 8281 output pixels x 256 groups of eight > GRID_CAP_THREADS


def out_size(n):
    return (n - 1) // 2 + 1


def _padded(x):
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def _tap_views(xp, Ho, Wo):
    """(tap t = kh * 3 + kw, the [B, Ho, Wo, C] view of the padded input that tap reads)."""
    for kh in range(3):
        for kw in range(3):
            yield kh * 3 + kw, xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]


def dw_padded_reads(H, W):
    """bool [H + 2, W + 2]: the positions of the padded input (row / column 0 and H + 1 / W + 1 are padding) that some tap of dw_fwd64
    reads for some output, found by sending position indices through the very views dw_fwd64 sums."""
    idx = torch.arange((H + 2) * (W + 2)).reshape(1, H + 2, W + 2, 1)
    read = torch.zeros((H + 2) * (W + 2), dtype=torch.bool)
    for _, v in _tap_views(idx, out_size(H), out_size(W)):
        read[v.reshape(-1)] = True
    return read.reshape(H + 2, W + 2)


def dw_fwd64(x, w9, bias=None):
    """y[b,ho,wo,c] = bias[c] + sum_t w9[t][c] * x[b, 2ho-1+kh, 2wo-1+kw, c], t = kh*3+kw, zero padding: nine shifted products."""
    B, H, W, C = x.shape
    Ho, Wo = out_size(H), out_size(W)
    xp, w = _padded(x.double()), w9.double()
    ref, mag = torch.zeros(B, Ho, Wo, C, dtype=torch.float64), torch.zeros(B, Ho, Wo, C, dtype=torch.float64)
    for t, v in _tap_views(xp, Ho, Wo):
        ref += v * w[t]
        mag += v.abs() * w[t].abs()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    return ref, mag


def dw_dgrad64(dy, w9, H, W):
    """dx = the transpose of dw_fwd64 applied to dy: every tap's product scattered back onto the input pixel it read."""
    B, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (out_size(H), out_size(W))
    d, w = dy.double(), w9.double()
    ref, mag = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64), torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            ref[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += d * w[kh * 3 + kw]
            mag[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += d.abs() * w[kh * 3 + kw].abs()
    return ref[:, 1:H + 1, 1:W + 1], mag[:, 1:H + 1, 1:W + 1]


def dw_wgrad64(dy, x):
    """dw[t][c] = sum_{b,ho,wo} dy[b,ho,wo,c] * x[b, 2ho-1+kh, 2wo-1+kw, c]: nine shifted element-wise products, summed."""
    B, Ho, Wo, C = dy.shape
    xp, d = _padded(x.double()), dy.double()
    ref, mag = torch.zeros(9, C, dtype=torch.float64), torch.zeros(9, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            ref[kh * 3 + kw] = (d * v).sum((0, 1, 2))
            mag[kh * 3 + kw] = (d.abs() * v.abs()).sum((0, 1, 2))
    return ref, mag


def dw_wgrad_grid(shape):
    """(channel groups, splits, pixels per split) of the weight-gradient launch: splits = ceil(P / 512), capped at 1024 / channel groups."""
    B, H, W, C = shape
    P = B * out_size(H) * out_size(W)
    cgs = cdiv(C, 64)
    splits = cdiv(P, 512)
    if splits * cgs > 1024:
        splits = 1024 // cgs
    splits = max(splits, 1)
    return cgs, splits, cdiv(P, splits)


def dw_wgrad_ceiling(shape):
    """A lane sums ceil(per / 32) products, the tree adds 32 lanes in order, `splits` atomics land on the prefill: in units of 2^-24."""
    _, splits, per = dw_wgrad_grid(shape)
    return (cdiv(per, 32) + 32 + splits + 1) * U32


def dw_case(shape, dtype, variant="bias"):
    """x, dy in the element type; w9 [9][C] and bias [C] fp32 ('avg': the fp32 value of 1/9, no bias: AvgPool2d(3, 2, 1)); `pre` is the
    non-zero content of dw before the call (the weight gradient is added to it)."""
    B, H, W, C = shape
    g = gen(B * 1000003 + H * 10007 + W * 101 + C + DW_VARIANTS.index(variant))
    x = el(torch.randn(B, H, W, C, generator=g), dtype)
    dy = el(torch.randn(B, out_size(H), out_size(W), C, generator=g), dtype)
    w9 = torch.randn(9, C, generator=g) * 0.4
    bias = torch.randn(C, generator=g) * 0.2
    pre = torch.randn(9, C, generator=g)
    if variant == "avg":
        w9 = torch.full((9, C), 1.0 / 9.0)
    return {"x": x, "dy": dy, "w9": w9, "bias": bias if variant == "bias" else None, "pre": pre}


def dw_cap_slice(dtype, s):
    """Channels [256 s, 256 s + 256) of the split-cap case, generated and referenced on their own (the whole case is 135 M inputs)."""
    B, H, W, _ = DW_CAP_SHAPE
    g = gen(977 + s)
    x = torch.randn(B, H, W, DW_CAP_SLICE, generator=g).to(dtype)
    dy = torch.randn(B, out_size(H), out_size(W), DW_CAP_SLICE, generator=g).to(dtype)
    pre = torch.randn(9, DW_CAP_SLICE, generator=g)
    ref, mag = dw_wgrad64(dy, x)
    return {"x": x, "dy": dy, "pre": pre, "ref": ref + pre.double(), "mag": mag + pre.double().abs()}


# ------------------------------------------------------------------------------------------------ global mean
GM_P = [1, 49, 127, 128, 129, 511, 512, 513, 896, 897, 1600]
GM_C = [8, 64, 72, 520]
GM_CASES = [(P, 72) for P in GM_P] + [(513, C) for C in GM_C if C != 72]
GM_B = 2


def gm_lane_steps(P, lane):
    """(rounds of the four-way unrolled loop, tail steps) of pixel lane `lane` (0 .. 127) of global_mean_kernel."""
    p, rounds, tail = lane, 0, 0
    while p + 3 * 128 < P:
        p, rounds = p + 4 * 128, rounds + 1
    while p < P:
        p, tail = p + 128, tail + 1
    return rounds, tail


def gm_ceiling(P):
    """A lane accumulator takes ceil(ceil(P / 128) / 4) additions, two more fold the four accumulators, 128 add the lanes in order,
    one division: in units of 2^-24."""
    return (cdiv(cdiv(P, 128), 4) + 2 + 128 + 1) * U32


def global_mean_case(P, C, dtype):
    x = el(torch.randn(GM_B, P, C, generator=gen(P * 1000 + C)) * 2 + 0.3, dtype)
    return {"x": x, "ref": x.double().sum(1) / P, "mag": x.double().abs().sum(1) / P}


# ------------------------------------------------------------------------------------------------ pooled linear
PL_N = [1, 15, 16, 17, 19, 150]
PL_C = [1, 63, 64, 65, 1000]
PL_CASES = [(N, 65) for N in PL_N] + [(19, C) for C in PL_C if C != 65]
PL_B = 3
PL_ACTS = (0, 1, 4)                        # none, relu, sigmoid
PL_PLANTED = (30.0, -30.0, 95.0, -95.0)    # sigmoid pre-activations of image 0, planted through the bias


def pl_planted_rows(N):
    rows = []
    for n in (0, N - 1, N // 2, N // 3):
        if n not in rows:
            rows.append(n)
    return rows


def pl_ceiling(C):
    """A lane takes ceil(C / 64) fused multiply-adds, the butterfly 6 additions, the bias one: in units of 2^-24."""
    return (cdiv(C, 64) + 6 + 1) * U32


def pooled_linear_case(N, C, act, with_bias):
    """out[b][n] = act(bias[n] + sum_c W[n][c] in[b][c]), fp32 throughout.  `s` is the fp64 pre-activation and `mag` its magnitude
    sum|W||in| + |bias|.  Sigmoid: `sig_mag` = ref * (1 + (1 - ref) * (1 + |s|)): the exponential's relative error grows with its
    argument (the argument is scaled by log2 e in fp32 first) and reaches the output through the slope ref * (1 - ref); the addition and
    the division are relative to ref."""
    g = gen(N * 5000 + C * 3 + act + 7 * int(with_bias))
    inp, W = torch.randn(PL_B, C, generator=g), torch.randn(N, C, generator=g) / math.sqrt(C)
    bias = torch.randn(N, generator=g) if with_bias else None
    dot = inp.double() @ W.double().T
    if act == 4 and with_bias:
        for n, target in zip(pl_planted_rows(N), PL_PLANTED):
            bias[n] = float(target - dot[0, n])
    s = dot + (bias.double() if with_bias else 0.0)
    mag = inp.double().abs() @ W.double().abs().T + (bias.double().abs() if with_bias else 0.0)
    out = {"in": inp, "W": W, "bias": bias, "s": s, "mag": mag}
    if act == 0:
        out["ref"] = s
    elif act == 1:
        out["ref"] = s.clamp_min(0)
    else:
        ref = 1.0 / (1.0 + torch.exp(-s))
        out["ref"] = ref
        out["sig_mag"] = ref * (1.0 + (1.0 / (1.0 + torch.exp(s))) * (1.0 + s.abs()))
    return out


# ------------------------------------------------------------------------------------------------ channel gate
CG_SHAPE = (3, 77, 72)
CG_COMBOS = [(sa, v, m) for sa in (0, 1) for v in (0, 1) for m in (0, 1)]      # self_add, add_vec, add_map
CAP_SHAPE = (1, 8200, 2048)                # 2 099 200 groups of eight > GRID_CAP_THREADS
CG_OPS = 4                                 # x * g, + x, + add_vec, + add_map: the longest chain, four fp32 operations


def channel_gate_case(shape, dtype):
    B, P, C = shape
    g = gen(B * 100000 + P * 10 + C)
    return {"x": el(torch.randn(B, P, C, generator=g), dtype), "gate": torch.rand(B, C, generator=g),
            "add_vec": torch.randn(B, C, generator=g), "add_map": el(torch.randn(B, P, C, generator=g), dtype)}


def channel_gate_ref(c, self_add, use_vec, use_map, first_row=0):
    """y = x * gate[b][c] (+ x) (+ add_vec[b][c]) (+ add_map) for the pixel rows from `first_row` on; (ref, mag)."""
    x, gt = c["x"][:, first_row:].double(), c["gate"].double()[:, None]
    ref, mag = x * gt, x.abs() * gt.abs()
    if self_add:
        ref, mag = ref + x, mag + x.abs()
    if use_vec:
        v = c["add_vec"].double()[:, None]
        ref, mag = ref + v, mag + v.abs()
    if use_map:
        m = c["add_map"][:, first_row:].double()
        ref, mag = ref + m, mag + m.abs()
    return ref, mag


# ------------------------------------------------------------------------------------------------ row dot
RD_SHAPES = [(3, 1000, 72), (2, 33, 520), (1, 5, 8)]
RD_SCALE = 0.5


def rd_splits(P):
    return (1, 5, 7, P + 3)                # P + 3: more splits than pixels, the last ranges are empty


def rd_ceiling(P, splits):
    """A lane sums ceil(per / 32) terms, the tree adds 32 lanes in order, `splits` atomics land on the prefill, one scaling."""
    return (cdiv(cdiv(P, splits), 32) + 32 + splits + 1) * U32


def rowdot_case(shape, dtype):
    B, P, C = shape
    g = gen(B + P * 7 + C * 1009)
    return {"a": el(torch.randn(B, P, C, generator=g), dtype), "b": el(torch.randn(B, P, C, generator=g), dtype),
            "pre": torch.randn(B, C, generator=g)}


def rowdot_ref(c, second, splits):
    """out[b][c] = scale * sum_p a * (b or 1); with more than one split the result is ADDED to `pre`, with one it replaces the output."""
    a = c["a"].double()
    t = a * c["b"].double() if second else a
    ref, mag = RD_SCALE * t.sum(1), RD_SCALE * t.abs().sum(1)
    if splits > 1:
        ref, mag = ref + c["pre"].double(), mag + c["pre"].double().abs()
    return ref, mag


# ------------------------------------------------------------------------------------------------ vector broadcast
BC_SHAPES = [(3, 77, 72), CAP_SHAPE]


def bcast_case(shape, dtype):
    """y[b,p,c] = vec[b][c] * scale, scale the fp32 value of 1 / P: one fp32 multiplication and one rounding.  `prod` is the fp64
    product, `ref` [B, C] its single rounding to the element type.  The few seeded values whose fp32 product sits so close to a tie of
    either element type that rounding it again differs from rounding the fp64 product once (about one in 2^13 for fp16, more among
    its subnormals, which scale = 1 / 8200 reaches) are replaced by 1.0, whose product is exact."""
    B, P, C = shape
    vec = torch.randn(B, C, generator=gen(P + C)) * 3
    scale = float(torch.tensor(1.0 / P, dtype=torch.float32))
    p32 = vec * torch.tensor(scale, dtype=torch.float32)
    for dt in ELEMS.values():
        vec[p32.to(dt).double() != elem_rne(vec.double() * scale, dt)] = 1.0
    prod = vec.double() * scale
    return {"vec": vec, "scale": scale, "prod": prod, "ref": elem_rne(prod, dtype)}


# ------------------------------------------------------------------------------------------------ planes to rows
PR_QQP = [(1, 8), (100, 104), (100, 128), (240, 240)]      # Qp = 240: 240 * 65 * 4 = 62 400 bytes of dynamic LDS, the most the entry point takes
PR_P = [1, 63, 64, 65, 777]
PR_B = 2


def planes_case(Q, Qp, P, dtype):
    """rows[b][p][q] = planes[b][q][p] rounded once to the element type for q < Q, +0 for Q <= q < Qp."""
    planes = torch.randn(PR_B, Q, P, generator=gen(Q * 100000 + Qp * 1000 + P)) * 3
    ref = torch.zeros(PR_B, P, Qp, dtype=torch.float64)
    for q in range(Q):
        ref[:, :, q] = elem_rne(planes[:, q, :].double(), dtype)
    return {"planes": planes, "ref": ref}


# ------------------------------------------------------------------------------------------------ nearest upsample + add, adjoint
# (Hs, Ws) -> (H, W): identity, exact x2, 2 * Hs - 1, 14 -> 20 (the ratio the comment in mask_ops.hip names), unequal ratios, and 14 -> 46 /
# 26 -> 44, where the fp32 rule floor(dst * (float)in / out) and the integer floor(dst * in / out) DO disagree (dst 23: 6, not 7; dst
# 22: 12, not 13; under IEEE fp32 they agree everywhere for 14 -> 20)
UP_PAIRS = [((6, 7), (6, 7)), ((5, 6), (10, 12)), ((5, 6), (9, 11)), ((14, 14), (20, 20)), ((5, 7), (13, 9)), ((14, 26), (46, 44))]
UP_B, UP_C = 2, 72
UP_ADD_TRIP = ((46, 46), (91, 91))         # B = 1, C = 2048: 8281 output pixels x 256 groups of eight > GRID_CAP_THREADS
UP_BWD_TRIP = ((91, 91), (100, 100))       # B = 1, C = 2048: 8281 source pixels
UP_TRIP_C = 2048


def nearest_index(in_size, out_size_):
    """Source index of every output index: identity and exact x2 by shift, otherwise floor(dst * (float)in / out) in fp32, clamped."""
    dst = torch.arange(out_size_)
    if out_size_ == in_size:
        return dst
    if out_size_ == 2 * in_size:
        return dst // 2
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size_), dtype=torch.float32)
    return torch.floor(dst.to(torch.float32) * scale).long().clamp_max(in_size - 1)


def up_max_preimage(pair):
    """The most output pixels any source pixel of the pair is the nearest source of: the adjoint's longest chain of fp32 additions."""
    (Hs, Ws), (H, W) = pair
    return int(torch.bincount(nearest_index(Hs, H), minlength=Hs).max() * torch.bincount(nearest_index(Ws, W), minlength=Ws).max())


def up_candidates(s, in_size, out_size_):
    """The output indices the adjoint kernel tests for source index s."""
    return max(0, (s * out_size_) // in_size - 1), min(out_size_ - 1, cdiv((s + 1) * out_size_, in_size) + 1)


def up64(top, size):
    iy, ix = nearest_index(top.shape[1], size[0]), nearest_index(top.shape[2], size[1])
    return top.double()[:, iy][:, :, ix]


def up_bwd64(dy, src_size):
    """dtop[b,ys,xs] = sum of dy over the output pixels whose nearest source is (ys, xs)."""
    B, H, W, C = dy.shape
    Hs, Ws = src_size
    iy, ix = nearest_index(Hs, H), nearest_index(Ws, W)
    rows = torch.zeros(B, Hs, W, C, dtype=torch.float64).index_add_(1, iy, dy.double())
    return torch.zeros(B, Hs, Ws, C, dtype=torch.float64).index_add_(2, ix, rows)


def upsample_case(pair, dtype, B=UP_B, C=UP_C):
    (Hs, Ws), (H, W) = pair
    g = gen(Hs * 1000000 + Ws * 10000 + H * 100 + W)
    lat, top = el(torch.randn(B, H, W, C, generator=g), dtype), el(torch.randn(B, Hs, Ws, C, generator=g), dtype)
    dy = el(torch.randn(B, H, W, C, generator=g), dtype)
    return {"lat": lat, "top": top, "dy": dy}


def upsample_add_ref(c):
    H, W = c["lat"].shape[1:3]
    return c["lat"].double() + up64(c["top"], (H, W)), c["lat"].double().abs() + up64(c["top"].abs(), (H, W))


def upsample_bwd_ref(c):
    src = c["top"].shape[1:3]
    return up_bwd64(c["dy"], src), up_bwd64(c["dy"].abs(), src)
