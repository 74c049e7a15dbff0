"""Shared by tests/test_infer_token_cases_cpu.py and tests/test_gpu_infer_token_ops.py: the inputs of every case of the inference-side
token, pixel and selection kernels (csrc/token_ops.hip, pixel_ops.hip, select_ops.hip), seeded and already rounded to bf16 where the
kernel reads bf16, with the float64 reference of the operation and its float64 magnitude `mag`: the same expression with every term
taken in absolute value, which bounds the fp32 error where terms cancel.  Where a kernel computes a sampling COORDINATE in fp32
(deformable sampling, the bilinear resizes) the coordinate's own fp32 error moves the result by (error) x (slope of the interpolant), so
mag carries the coordinate's magnitude times the largest |value| around the taps as one more term; the docstrings say where.

Nothing here touches a GPU or the library; the CPU test checks every reference against an independent formulation."""
import math

import torch
import torch.nn.functional as F

from tests.helpers import bf16_rne

U32 = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    """Round to bf16, keep as fp32 (every value exactly representable in bf16)."""
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ add_rows
ADD_ROWS_CASES = [(37, 64, 5), (37, 64, 7), (5, 256, 5), (5, 256, 7)]        # rows, cols, y_rows


def add_rows_case(rows, cols, y_rows):
    """out[r] = x[r] + y[r % y_rows]: one fp32 addition of two bf16 values, one rounding: out = bf16_rne(fp64 sum) bit for bit (the CPU
    test asserts that every fp32 sum of the case is exact, i.e. that no second rounding exists)."""
    g = gen(rows * 1000 + cols + y_rows)
    x, y = bf(torch.randn(rows, cols, generator=g) * 2), bf(torch.randn(y_rows, cols, generator=g))
    s = x.double() + y.double()[torch.arange(rows) % y_rows]
    return {"x": x, "y": y, "sum": s, "ref": bf16_rne(s)}


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [(cols, rows, res, variant) for cols in (128, 256) for rows in (1, 4, 9) for res in (False, True) for variant in ("plain", "mean40")]


def layernorm_case(cols, rows, res, variant):
    """LayerNorm(x + residual) * gamma + beta, eps 1e-5, biased variance.  mean40: row mean 40, spread 0.5 (a one-pass E[x^2] - mean^2 in
    fp32 rounds at 1600 * 2^-24 = 1e-4 against a variance of 0.25; the kernel's two passes do not).
    mag = (|v| + mean|v|) * rstd * |gamma| + |beta|: (v - mean) with both terms in absolute value."""
    g = gen(cols * 100 + rows * 10 + int(res) + (5 if variant == "mean40" else 0))
    if variant == "mean40":
        x = torch.randn(rows, cols, generator=g) * 0.5 + 40.0
        r = torch.randn(rows, cols, generator=g) * 0.05
    else:
        x = torch.randn(rows, cols, generator=g) * 2 + 0.3
        r = torch.randn(rows, cols, generator=g)
    x, r = bf(x), (bf(r) if res else None)
    gamma, beta = torch.rand(cols, generator=g) + 0.5, torch.randn(cols, generator=g) * 0.5
    v = x.double() + (r.double() if res else 0.0)
    va = x.double().abs() + (r.double().abs() if res else 0.0)
    mean = v.mean(1, keepdim=True)
    rstd = ((v - mean).pow(2).mean(1, keepdim=True) + 1e-5).rsqrt()
    ref = (v - mean) * rstd * gamma.double() + beta.double()
    mag = (va + va.mean(1, keepdim=True)) * rstd * gamma.double().abs() + beta.double().abs()
    return {"x": x, "res": r, "gamma": gamma, "beta": beta, "ref": ref, "mag": mag}


# ------------------------------------------------------------------------------------------------ attention
# (Lq, Lk): see the table in tests/test_gpu_infer_token_ops.py
MHA_PAIRS = [(1, 1), (37, 31), (130, 32), (77, 448), (77, 449), (7, 1056)]


def mha_case(Lq, Lk, heads=8, masked=False, big=False):
    """softmax(q k^T / sqrt(32)) v per head; masked: mask[b, q, key] True = key not allowed, shared by the heads, and a query whose mask
    forbids every key attends everywhere.  big: scores of magnitude ~60 (the running-max rescale across key tiles matters).
    mag = softmax . |v| (the kernel rounds the un-normalised probabilities to bf16 for the second matrix product: c ~ 2^-9).
    Planted queries (flat over batch x query): a fully masked one, a fully open one, one whose only allowed key is the LAST key (it lies
    in the last, possibly partial, 32-key tile) - at the front and, where there is room, at the end of the query range."""
    B = 3 if Lq == 1 else 2
    g = gen(Lq * 10000 + Lk * 4 + heads + int(masked) * 2 + int(big))
    sc = 4.5 if big else 1.5
    q, k = bf(torch.randn(B, Lq, heads * 32, generator=g) * sc), bf(torch.randn(B, Lk, heads * 32, generator=g) * sc)
    v = bf(torch.randn(B, Lk, heads * 32, generator=g))
    mask = None
    if masked:
        mask = (torch.rand(B * Lq, Lk, generator=g) < 0.5)
        only_last = torch.ones(Lk, dtype=torch.bool)
        only_last[Lk - 1] = False
        plan = [(0, "masked"), (1, "open"), (2, "last")]
        if B * Lq >= 6:
            plan += [(B * Lq - 1, "masked"), (B * Lq - 2, "last"), (B * Lq - 3, "open")]
        for row, kind in plan:
            mask[row] = {"masked": torch.ones(Lk, dtype=torch.bool), "open": torch.zeros(Lk, dtype=torch.bool), "last": only_last}[kind]
        mask = mask.view(B, Lq, Lk)
    qh, kh, vh = (t.double().view(B, -1, heads, 32).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(32.0)                      # [B, heads, Lq, Lk]
    if masked:
        eff = mask & ~mask.all(-1, keepdim=True)                         # a fully masked query attends everywhere
        s = s.masked_fill(eff[:, None], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    ref = (p @ vh).transpose(1, 2).reshape(B, Lq, heads * 32)
    mag = (p @ vh.abs()).transpose(1, 2).reshape(B, Lq, heads * 32)
    return {"B": B, "q": q, "k": k, "v": v, "mask": mask, "ref": ref, "mag": mag, "smax": float(s[torch.isfinite(s)].abs().max())}


def mask_words(mask):
    """bool [B, Lq, Lk] -> int32 [B * Lq, ceil(Lk / 32)]: bit (key & 31) of word key / 32 set = key not allowed; bits past Lk are set."""
    B, Lq, Lk = mask.shape
    T = (Lk + 31) // 32
    m = torch.ones(B * Lq, T * 32, dtype=torch.bool)
    m[:, :Lk] = mask.reshape(B * Lq, Lk)
    w = (m.view(B * Lq, T, 32).long() << torch.arange(32)).sum(-1)      # < 2^32
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


# ------------------------------------------------------------------------------------------------ deformable sampling
MSDA_L3 = ((5, 7), (3, 4), (2, 2))
MSDA_L2 = ((5, 7), (3, 4))


def msda_planted(H, W):
    """(x, y) in units of the map ([0, 1] = the map): exactly 0 and 1, half a pixel outside each border, far outside, two corners."""
    return [(0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0), (-0.5 / W, 0.5), (1.0 + 0.5 / W, 0.5), (0.5, -0.5 / H), (0.5, 1.0 + 0.5 / H),
            (1e6, 0.5), (-1e6, 0.5), (0.5, 1e6), (0.5, -1e6), (0.0, 0.0), (1.0, 1.0)]


def msda_sample64(value, shapes, loc, w, loc_abs):
    """fp64 sampling: value [B, S, 8, 32], loc [B, Q, 8, L, P, 2] in map units, w [B, Q, 8, L, P].  F.grid_sample(align_corners=False,
    padding_mode="zeros") taps: ix = loc_x * W - 0.5, taps floor(ix), floor(ix) + 1, outside the map = 0.  Returns (out, mag, tap
    statistics); mag = sum_i |w_i| (sum_taps wt |v| + [sample within one pixel of the map] (W |loc_x| + H |loc_y| + 1) max_level |v|):
    the second term is the fp32 error of ix, iy times the interpolant's slope."""
    B, S, M, D = value.shape
    Q, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    v = value.double()
    out = torch.zeros(B, Q, M, D, dtype=torch.float64)
    mag = torch.zeros_like(out)
    stats = []
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, Q, M, P)
    mi = torch.arange(M).view(1, 1, M, 1).expand(B, Q, M, P)
    start = 0
    for lv, (H, W) in enumerate(shapes):
        ix, iy = loc[:, :, :, lv, :, 0].double() * W - 0.5, loc[:, :, :, lv, :, 1].double() * H - 0.5
        x0, y0 = torch.floor(ix), torch.floor(iy)
        tx, ty = ix - x0, iy - y0
        wl = w[:, :, :, lv].double()
        vmax = v[:, start:start + H * W].abs().amax(1)                   # [B, M, D]
        near = ((ix > -1) & (ix < W) & (iy > -1) & (iy < H)).double()
        coord = W * loc_abs[:, :, :, lv, :, 0].double() + H * loc_abs[:, :, :, lv, :, 1].double() + 1.0
        mag += ((wl.abs() * near * coord).sum(-1)[..., None] * vmax[:, None])
        for dy, dx, wt in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            tok = start + (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
            tv = v[bi, tok, mi]                                          # [B, Q, M, P, D]
            cw = (wl * wt * ok)[..., None]
            out += (cw * tv).sum(3)
            mag += (cw.abs() * tv.abs()).sum(3)
        stats.append({"x0": x0, "y0": y0, "H": H, "W": W})
        start += H * W
    return out.reshape(B, Q, M * D), mag.reshape(B, Q, M * D), stats


def msda_case(shapes, P, mode):
    """mode 0: loc in map units and softmaxed weights as the kernel receives them.  mode 1: raw offsets, raw logits and reference boxes
    (cx, cy, w, h); the kernel's own loc = ref_xy + off / P * ref_wh * 0.5 and softmax over the L * P logits of a head.
    B = 2, Q = 13 (26 rows: the last workgroup of four waves is partial), M = 8 heads of 32 channels."""
    B, Q, M, L = 2, 13, 8, len(shapes)
    S = sum(h * w for h, w in shapes)
    g = gen(L * 100 + P * 10 + mode)
    value = bf(torch.randn(B, S, M * 32, generator=g))
    loc = torch.rand(B, Q, M, L, P, 2, generator=g) * 1.4 - 0.2
    for lv, (H, W) in enumerate(shapes):                                 # planted points: query = plant number, head (lv + plant) % 8, point plant % P
        for n, (px, py) in enumerate(msda_planted(H, W)):
            loc[n % B, n % Q, (lv + n) % M, lv, n % P] = torch.tensor([px, py])
    logits = torch.randn(B, Q, M, L * P, generator=g) * 2
    c = {"B": B, "Q": Q, "S": S, "L": L, "P": P, "shapes": shapes, "value": value,
         "starts": [sum(h * w for h, w in shapes[:i]) for i in range(L)]}
    if mode == 0:
        w = torch.softmax(logits, -1).view(B, Q, M, L, P)                # fp32 values: what the kernel is handed
        c.update(loc=loc, attn=w)
        loc64, w64, loc_abs = loc.double(), w.double(), loc.double().abs()
    else:
        ref4 = torch.rand(B, Q, 4, generator=g) * torch.tensor([1.0, 1.0, 0.6, 0.6]) + torch.tensor([0.0, 0.0, 0.05, 0.05])
        ref4[:, 0] = torch.tensor([0.5, 0.5, 1.0, 1.0])
        r = ref4.double()[:, :, None, None, None]
        off = ((loc.double() - r[..., :2]) / (r[..., 2:] * 0.5) * P).float()     # the offsets that put the samples at (about) `loc`
        c.update(off=off, logits=logits, ref4=ref4)
        loc64 = r[..., :2] + off.double() / P * r[..., 2:] * 0.5
        loc_abs = r[..., :2].abs() + off.double().abs() / P * r[..., 2:].abs() * 0.5
        w64 = torch.softmax(logits.double(), -1).view(B, Q, M, L, P)
    c["loc64"], c["w64"] = loc64, w64
    c["ref"], c["mag"], c["stats"] = msda_sample64(value.view(B, S, M, 32), shapes, loc64, w64, loc_abs)
    return c


# ------------------------------------------------------------------------------------------------ bilinear resizes
RESIZE_SIZES = [((5, 7), (10, 14)), ((9, 9), (4, 5)), ((3, 3), (3, 3))]


def _bil_axis(n_in, n_out):
    """ATen's upsample_bilinear2d(align_corners=False) source index with the fp32 scale in / out the kernels use, evaluated in fp64."""
    scale = float(torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32))
    src = (scale * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0
    return i0, i1, 1 - l1, l1, src


def resize_ref64(x, Ho, Wo):
    """x [B, H, W, C] (fp64) -> (ref, mag) [B, Ho, Wo, C].  mag = sum_taps wt |x| + (src_h + src_w) * max |x| over the 3 x 3 surroundings of
    the four taps (the fp32 error of the source coordinate times the interpolant's slope)."""
    B, H, W, Cc = x.shape
    h0, h1, lh0, lh1, sh = _bil_axis(H, Ho)
    w0, w1, lw0, lw1, sw = _bil_axis(W, Wo)
    lh0, lh1, lw0, lw1 = lh0.view(1, Ho, 1, 1), lh1.view(1, Ho, 1, 1), lw0.view(1, 1, Wo, 1), lw1.view(1, 1, Wo, 1)

    def tap(t, hi, wi):
        return t[:, hi][:, :, wi]

    def interp(t):
        return lh0 * (lw0 * tap(t, h0, w0) + lw1 * tap(t, h0, w1)) + lh1 * (lw0 * tap(t, h1, w0) + lw1 * tap(t, h1, w1))

    a = x.abs()
    nb = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    around = torch.stack([tap(nb, hi, wi) for hi in (h0, h1) for wi in (w0, w1)]).amax(0)
    return interp(x), interp(a) + (sh.view(1, Ho, 1, 1) + sw.view(1, 1, Wo, 1)) * around


def resize_u8_case(size_in, size_out):
    (H, W), (Ho, Wo) = size_in, size_out
    x = torch.randint(0, 256, (H, W, 3), generator=gen(H * 100 + W + Ho), dtype=torch.uint8)
    x[0, 0] = 0
    x[-1, -1] = 255
    ref, mag = resize_ref64(x.double()[None], Ho, Wo)
    return {"x": x, "ref": ref[0], "mag": mag[0]}


def resize_nhwc_case(size_in, size_out, Cc, B=2):
    (H, W), (Ho, Wo) = size_in, size_out
    x = bf(torch.randn(B, H, W, Cc, generator=gen(H * 1000 + W * 10 + Cc)) * 2)
    ref, mag = resize_ref64(x.double(), Ho, Wo)
    return {"x": x, "ref": ref, "mag": mag}


# ------------------------------------------------------------------------------------------------ pools
MAXPOOL_CASES = [(1, 1, False), (1, 6, False), (5, 7, False), (6, 6, False), (5, 7, True)]     # H, W, negative values only
AVGPOOL_CASES = [(1, 1), (5, 7), (6, 6)]


def _windows(x, k, stride, pad, Ho, Wo, fill):
    """x [B, H, W, C] -> [B, Ho, Wo, C, k * k] windows, positions outside the map = fill."""
    B, H, W, Cc = x.shape
    Hp, Wp = (Ho - 1) * stride + k, (Wo - 1) * stride + k
    xp = torch.full((B, Hp, Wp, Cc), fill, dtype=x.dtype)
    hh, ww = min(H, Hp - pad), min(W, Wp - pad)
    xp[:, pad:pad + hh, pad:pad + ww] = x[:, :hh, :ww]
    return torch.stack([xp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride] for i in range(k) for j in range(k)], -1)


def maxpool_case(H, W, negative, Cc=16, B=2):
    """MaxPool2d(3, 2, 1): exact (a maximum of bf16 values).  negative: every input below zero - a padding of 0 instead of -inf would win
    at the border."""
    x = bf(torch.randn(B, H, W, Cc, generator=gen(H * 10 + W + int(negative))))
    if negative:
        x = -x.abs() - 0.125
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return {"x": x, "ref": _windows(x.double(), 3, 2, 1, Ho, Wo, float("-inf")).amax(-1)}


def avgpool_case(H, W, Cc=16, B=2):
    """AvgPool2d(2, 2, 0, ceil_mode=True): the mean over the taps inside the map.  mag = the same mean of |x|."""
    x = bf(torch.randn(B, H, W, Cc, generator=gen(H * 10 + W + 3)) * 2)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    win = _windows(x.double(), 2, 2, 0, Ho, Wo, float("nan"))
    inside = ~torch.isnan(win)
    z = torch.where(inside, win, torch.zeros_like(win))
    cnt = inside.sum(-1)
    return {"x": x, "ref": z.sum(-1) / cnt, "mag": z.abs().sum(-1) / cnt}


# ------------------------------------------------------------------------------------------------ selection
ROWMAX_COLS = [1, 63, 65, 365]


def rowmax_case(cols, rows=5, ld=368):
    x = torch.randn(rows, cols, generator=gen(cols))
    x[3] = float("-inf")
    return {"x": x, "ref": x.amax(1)}


def gather_fill_case(cols, B=3, rpb=11, k=4):
    g = gen(cols + 1)
    src = bf(torch.randn(B, rpb, cols, generator=g))
    idx = torch.randint(0, rpb, (B, k), generator=g, dtype=torch.int32)
    idx[0, 1] = idx[0, 0]                                                 # a repeated index
    idx[1] = torch.tensor([0, rpb - 1, rpb - 1, 5])
    rows_idx = torch.tensor([3, rpb - 1, 3, 0], dtype=torch.int32)       # per batch, with a repeat
    rowv = bf(torch.randn(cols, generator=g))
    gathered = src[torch.arange(B)[:, None], idx.long()]
    filled = src.clone()
    filled[:, rows_idx.long()] = rowv
    return {"src": src, "idx": idx, "rows_idx": rows_idx, "rowv": rowv, "gathered": gathered, "filled": filled}


def linear_k4_case(N, rows=3):
    """relu(b + x . w), K = 4.  mag = |b| + |x| . |w|."""
    g = gen(N)
    x, w, b = torch.rand(rows, 4, generator=g), torch.randn(N, 4, generator=g), torch.randn(N, generator=g)
    z = b.double() + x.double() @ w.double().T
    return {"x": x, "w": w, "b": b, "ref": z.clamp_min(0), "mag": b.double().abs() + x.double().abs() @ w.double().abs().T}


def inverse_sigmoid64(x, eps=1e-5):
    x = x.double().clamp(0.0, 1.0)
    return torch.log(x.clamp_min(eps) / (1 - x).clamp_min(eps))


BBOX_REF_EDGES = [0.0, 1.0, 1e-7, 1.0 - 1e-7, -0.01, 1.01, 0.5, 1e-5]


def bbox_head_case(K, mode, rows=5):
    """mode 0: u = h . w^T + b + inverse_sigmoid(ref) (clamped to [0, 1], eps 1e-5); mode 1: u = h . w^T + b + anchors[idx]; new = sigmoid(u).
    mag_u = |h| . |w|^T + |b| + |third term|; mag_new = new (1 - new) mag_u + new."""
    g = gen(K + mode)
    h = bf(torch.randn(rows, K, generator=g))
    w, b = torch.randn(4, K, generator=g) / math.sqrt(K), torch.randn(4, generator=g) * 0.1
    c = {"h": h, "w": w, "b": b}
    if mode == 0:
        ref = torch.rand(rows, 4, generator=g)
        ref.view(-1)[:len(BBOX_REF_EDGES)] = torch.tensor(BBOX_REF_EDGES)
        third = inverse_sigmoid64(ref)
        c["ref4"] = ref
    else:
        anchors = torch.randn(9, 4, generator=g) * 2
        idx = torch.tensor([8, 0, 3, 3, 7], dtype=torch.int32)[:rows]
        third = anchors.double()[idx.long()]
        c.update(anchors=anchors, idx=idx)
    u = h.double() @ w.double().T + b.double() + third
    mag_u = h.double().abs() @ w.double().abs().T + b.double().abs() + third.abs()
    new = torch.sigmoid(u)
    c.update(third=third, u=u, mag_u=mag_u, new=new, mag_new=new * (1 - new) * mag_u + new)
    return c


def head_out_case(K, rows=5, ldl=368):
    """probs = sigmoid(logits[:, :K]); boxes = (cx - w/2, cy - h/2, cx + w/2, cy + h/2).  mag: p (1 + |x|); |c| + |w| / 2."""
    g = gen(K + 77)
    logits = torch.randn(rows, K, generator=g) * 4
    logits.view(-1)[:4] = torch.tensor([0.0, 30.0, -30.0, -100.0])
    ref4 = torch.rand(rows, 4, generator=g)
    x, r = logits.double(), ref4.double()
    p = torch.sigmoid(x)
    half = 0.5 * r[:, 2:]
    boxes = torch.cat([r[:, :2] - half, r[:, :2] + half], 1)
    mag_b = torch.cat([r[:, :2].abs() + half.abs()] * 2, 1)
    return {"logits": logits, "ref4": ref4, "probs": p, "mag_p": p * (1 + x.abs()), "boxes": boxes, "mag_b": mag_b}


def postprocess_case():
    """Two images of size (H, W) = (512, 1024), Q = 6 queries, K = 5 classes, top_k = 6.  Every box coordinate is +-(j + 0.5) / size, so
    box * size is EXACTLY j + 0.5 in fp32 and in fp64: a round-half-even tie, j even and odd, one negative.  Scores are sorted
    descending and one equals the threshold (0.5, not counted: the comparison is strict)."""
    B, Q, K, top_k, thr = 2, 6, 5, 6, 0.5
    sizes = [(512, 1024), (512, 1024)]
    j = torch.tensor([[[2, 3, 100, 101], [7, 8, 9, 10], [0, 1, 510, 511], [-3, 4, 1022, 500], [-2, 5, 6, 7], [333, 222, 334, 223]],
                      [[1, 1, 2, 2], [4, 4, 5, 5], [-1, -2, 1023, 511], [20, 21, 22, 23], [41, 40, 43, 42], [0, 0, 1, 1]]], dtype=torch.float64)
    half = j + 0.5                                                       # -3 -> -2.5, -2 -> -1.5: ties on the negative side too
    div = torch.tensor([1024.0, 512.0, 1024.0, 512.0], dtype=torch.float64)
    boxes = (half / div).float()
    val = torch.tensor([[0.9, 0.8, 0.7, 0.5, 0.4, 0.3], [0.95, 0.6, 0.5, 0.5, 0.2, 0.1]])
    idx = torch.tensor([[17, 3, 29, 8, 0, 22], [25, 14, 9, 10, 5, 1]], dtype=torch.int32)   # flat query * K + class, every query of image 0 used once
    q = idx.long() // K
    prod = boxes.double()[torch.arange(B)[:, None], q] * div
    return {"B": B, "Q": Q, "K": K, "top_k": top_k, "thr": thr, "sizes": sizes, "boxes": boxes, "val": val, "idx": idx, "prod": prod,
            "labels": (idx.long() % K).int(), "queries": q.int(), "obox": torch.round(prod).int(), "count": (val > thr).sum(1).int()}


TOPK_CASES = [(700, 704, 5), (8200, 8208, 5)]        # n, ld, k; 8200 > 8192: the workspace entry point runs its two-level form


def topk_case(n, ld, k):
    """Rows: random; ties straddling the cut; signed zeros straddling the cut: 3 positive values, every other value negative, and zeros of
    both signs - the two zeros the cut admits are the two of LOWEST index, -0.0 first.  (value descending, index ascending among equals)
    treats -0.0 and +0.0 as equal; the kernel returns a selected zero as +0.0."""
    g = gen(n + k)
    s = torch.randn(3, n, generator=g)
    s[1, ::3] = s[1, 0].abs() + 1.0
    z = -torch.rand(n, generator=g) - 0.01
    z[[10, 50, n - 1]] = torch.tensor([0.5, 2.0, 1.0])
    z[[5, n - 2]] = -0.0
    z[[20, 400]] = 0.0
    s[2] = z
    v = s.numpy()
    order = torch.tensor([sorted(range(n), key=lambda i, r=r: (-float(v[r, i]), i))[:k] for r in range(3)])
    vals = s.gather(1, order)
    vals = torch.where(vals == 0, torch.zeros_like(vals), vals)          # a zero of either sign comes back as +0.0
    return {"s": s, "order": order, "vals": vals}
