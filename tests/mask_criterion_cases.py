"""Cases, float64 closed-form references and per-element magnitudes of the mask criterion kernels (csrc/mask_criterion_ops.hip), shared by
tests/test_mask_criterion_cases_cpu.py (which checks every reference against oracle/mask_criterion_oracle.py and torch.autograd) and
tests/test_gpu_mask_criterion_ops.py (which gates the kernels with them).  numpy / torch on the CPU only; nothing of the product is read.

What the references compute (all in float64)
* point sample: bilinear, zero padding; the source index of a coordinate c on an axis of `size` pixels is ((2c - 1 + 1) * size - 1) / 2
  = c * size - 0.5; taps floor(i) and floor(i) + 1 with weights 1 - frac and frac; a tap outside the plane contributes 0.
* match cost [b][q][t] = w_mask * (sum_p softplus(x) - sum_p x t) / P - w_class * prob[label_t] + w_dice * (1 - (2 sum sigma(x) t + 1) /
  (sum sigma(x) + sum t + 1)); columns t >= T of an image are 0.  prob: softmax over K + 1 logits, or sigmoid (cls_sigmoid).
* set loss: out3 = (w_ce * sum w[y] nll / sum w[y],  w_mask * sum_n (sum_p bce) / num_points / num_masks,  w_dice * sum_n dice_n /
  num_masks).  Points of pair n: of the n_over candidates the k_imp with the smallest |x|, ties to the LOWEST index (a stable sort of
  |x|), then the n_extra uniform points.
* its gradients under upstream g[0..2]: every point adds v = g1 w_mask / (num_masks num_points) * (s - t) + g2 w_dice / num_masks *
  s (1 - s) * (-2 t / D + (2 ST + 1) / D^2)  (s = sigma(x), D = sum s + sum t + 1, ST = sum s t) to its in-bounds taps with the
  sampling weights; dlogits[b,q,c] = g0 w_ce w[y] / sum w[y] * (softmax_c - [c == y]).

Magnitudes.  Every reference comes with the same expression over absolute values: |got - ref| <= RND(ref) + c * mag is the gate, c a small
multiple of 2^-24.  A sampled value x carries its own rounding (mag sum |v| weight) into everything computed from it; the derivative of
each later step is bounded (sigma' = s (1 - s), d bce / dx <= 1), so that term enters with that factor.

Coordinates.  All cases but the "free" ones draw coordinates on a dyadic grid c = m / 2^g with g + bits(largest axis) <= 24: the fp32
source index then equals the float64 one exactly (asserted on the CPU), so reference and kernel take the same taps with the same weights
and no coordinate term is needed.  The free cases use torch.rand floats; there the fp32 index is off by a few roundings of its own
magnitude, which moves a sample by (that error) x (slope of the interpolant): mag carries (|ix| + |iy| + 1) x the largest |value| in the
3 x 3 surroundings of the taps as one more term, as tests/infer_token_cases.py does for the resizes."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
CE, FOCAL, BCE, BCE_FOCAL = 0, 1, 2, 3
MPB_LDS_FLOATS = 16384      # csrc/mask_criterion_ops.hip: floats of one LDS band of the backward
MPL_THREADS = 1024          # threads (= contiguous index chunks) of the forward's selection


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def bits(n):
    return int(n).bit_length()


def grid_bits(*sizes):
    """g of the dyadic grid for axes of these sizes: g + bits(size) <= 24, at most 12."""
    return min(12, 24 - max(bits(s) for s in sizes))


def dyadic(shape, g, generator):
    """Coordinates m / 2^g, m uniform in [0, 2^g] (both ends included), as fp32 (exact)."""
    return (torch.randint(0, 2 ** g + 1, shape, generator=generator).double() / 2.0 ** g).float()


def index64(c, size):
    return c.double() * size - 0.5


def index32(c, size):
    """The kernels' fp32 operation sequence (ps_unnormalize), one rounding per operation."""
    c = c.float()
    g = 2.0 * c - 1.0
    return ((g + 1.0) * float(size) - 1.0) / 2.0


def axis_taps(c, size):
    i = index64(c, size)
    i0 = torch.floor(i)
    f = i - i0
    return i, i0.long(), 1.0 - f, f


def sample64(plane, coords, free=False):
    """plane [H, W], coords [P, 2] (x, y) -> (value, mag) [P] in float64.  mag = sum |v| weight (+ the coordinate term when `free`)."""
    plane = plane.double()
    H, W = plane.shape
    ix, x0, ex, wx = axis_taps(coords[:, 0], W)
    iy, y0, sy, ny = axis_taps(coords[:, 1], H)
    val = torch.zeros(coords.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(val)
    around = torch.zeros_like(val)
    nb = F.max_pool2d(plane.abs()[None, None], 3, 1, 1)[0, 0] if free else None
    for dy, wy in ((0, sy), (1, ny)):
        for dx, wxx in ((0, ex), (1, wx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
            v = plane[yc, xc] * ok
            val += v * (wy * wxx)
            mag += v.abs() * (wy * wxx)
            if free:
                around = torch.maximum(around, nb[yc, xc] * ok)
    if free:
        mag = mag + (ix.abs() + iy.abs() + 1.0) * around
    return val, mag


def scatter64(h, w, coords, v, weighted=True):
    """Transpose of sample64: [h * w] plane with v added to the in-bounds taps of every point (`weighted` False: v itself to each tap)."""
    out = torch.zeros(h * w, dtype=torch.float64)
    _, x0, ex, wx = axis_taps(coords[:, 0], w)
    _, y0, sy, ny = axis_taps(coords[:, 1], h)
    for dy, wy in ((0, sy), (1, ny)):
        for dx, wxx in ((0, ex), (1, wx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            out.index_add_(0, (yy * w + xx)[ok], (v * (wy * wxx) if weighted else v)[ok])
    return out


def main_tap(h, w, coords):
    """(flat pixel, weight) of the in-bounds tap with the largest weight of every point (a coordinate in [0, 1] always has one >= 1/4)."""
    _, x0, ex, wx = axis_taps(coords[:, 0], w)
    _, y0, sy, ny = axis_taps(coords[:, 1], h)
    best_w = torch.full((coords.shape[0],), -1.0, dtype=torch.float64)
    best_p = torch.zeros(coords.shape[0], dtype=torch.long)
    for dy, wy in ((0, sy), (1, ny)):
        for dx, wxx in ((0, ex), (1, wx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            wt = torch.where(ok, wy * wxx, torch.full_like(wy, -1.0))
            better = wt > best_w
            best_w = torch.where(better, wt, best_w)
            best_p = torch.where(better, yy * w + xx, best_p)
    return best_p, best_w


# ------------------------------------------------------------------------------------------------ point sample
PS_PLANES = [(1, 1), (13, 17), (64, 32)]
PS_POINTS = [1, 255, 256, 257]      # one partial workgroup, one short of / exactly / one past a 256-thread workgroup
PS_SOURCES, PS_COORD_SETS = 6, 5


def point_sample_case(H, W, P, u8, free=False):
    """PS_SOURCES source planes, PS_COORD_SETS coordinate sets of P points.  The first points of every set are c = 0, c = 1 (all four taps
    half or fully outside), the mixed corners and c = 0.5 (an exact pixel centre on odd axes)."""
    g = gen(H * 100003 + W * 1009 + P * 7 + int(u8) + 2 * int(free))
    if u8:
        src = torch.randint(0, 256, (PS_SOURCES, H, W), generator=g, dtype=torch.uint8)
        src.view(-1)[0] = 255
    else:
        src = torch.randn(PS_SOURCES, H, W, generator=g) * 3.0
    gb = grid_bits(H, W)
    coords = torch.rand(PS_COORD_SETS, P, 2, generator=g) if free else dyadic((PS_COORD_SETS, P, 2), gb, g)
    special = torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.5, 0.5]])
    n = min(P, special.shape[0])
    coords[:, :n] = special[:n]
    return {"src": src, "coords": coords, "H": H, "W": W, "P": P, "u8": u8, "free": free, "g": gb}


def point_sample_ref(c, src_index, coord_index):
    """(ref, mag) [R, P] of fx_point_sample_f32 on the case with the two index vectors (lists of ints)."""
    out = [sample64(c["src"][s], c["coords"][k], c["free"]) for s, k in zip(src_index, coord_index)]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def pixel_centres(H, W):
    """Coordinates of every pixel centre of an [H, W] plane in row-major order (exact in fp32 when H and W are powers of two)."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return torch.stack([(xs.reshape(-1) + 0.5) / W, (ys.reshape(-1) + 0.5) / H], dim=1).float()


# ------------------------------------------------------------------------------------------------ match cost
# (Q, target counts per image, P, K).  Q: one query, exactly / one past / not a multiple of the 16-query tile.  Counts: an image without
# targets next to 21 (two target blocks) and 40 (three); few targets; exactly the 64 the tiled kernel holds in registers; 65 (zero workspace,
# the untiled kernel).  P: one point, below / at / above one 64-point tile, 777 (slices with tails).  K + 1 = 2, 65 (a wave and one), 151.
MATCH_CASES = [
    (1, (3, 5), 1, 1), (16, (3, 5), 63, 64), (17, (3, 5), 64, 150), (37, (3, 5), 65, 64), (16, (3, 5), 777, 1),
    (37, (0, 21, 40), 1, 64), (17, (0, 21, 40), 63, 150), (1, (0, 21, 40), 64, 1), (16, (0, 21, 40), 65, 150), (37, (0, 21, 40), 777, 64),
    (17, (64,), 1, 150), (37, (64,), 63, 1), (16, (64,), 64, 64), (1, (64,), 65, 64), (17, (64,), 777, 1),
    (16, (65,), 1, 64), (1, (65,), 63, 150), (37, (65,), 64, 1), (17, (65,), 65, 150), (16, (65,), 777, 64),
]
MATCH_W = (2.0, 5.0, 3.0)    # w_class, w_mask, w_dice: distinct


def match_id(c):
    Q, counts, P, K = c
    return f"Q{Q}-T{'_'.join(map(str, counts))}-P{P}-K{K}"


def mmc_splits(B, Q):
    s = (512 + B * ((Q + 15) // 16) - 1) // (B * ((Q + 15) // 16))
    return max(1, min(16, s))


@functools.lru_cache(maxsize=None)
def match_case(case):
    Q, counts, P, K = case
    B, n = len(counts), sum(counts)
    g = gen(Q * 7919 + P * 31 + K + n)
    logits = torch.randn(B, Q, K + 1, generator=g) * 2.0
    pred = torch.randn(B * Q, P, generator=g) * 3.0
    tgt = (torch.rand(n, P, generator=g) > 0.6).float()
    frac = torch.rand(n, P, generator=g) < 0.2
    tgt = torch.where(frac, torch.randint(0, 5, (n, P), generator=g).float() / 4.0, tgt)       # sampled target values lie in [0, 1]
    labels = torch.randint(0, K, (n,), generator=g, dtype=torch.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return {"B": B, "Q": Q, "P": P, "K": K, "counts": counts, "Tmax": max(counts), "logits": logits, "pred": pred, "tgt": tgt, "labels": labels,
            "offsets": torch.from_numpy(off)}


def match_cost_ref(c, cls_sigmoid, w=MATCH_W):
    """(ref, mag) [B, Q, Tmax].  The mask term is a difference of two sums, so its magnitude is (sum softplus + sum |x t|) / P."""
    w_class, w_mask, w_dice = w
    B, Q, P, Tmax = c["B"], c["Q"], c["P"], c["Tmax"]
    ref = torch.zeros(B, Q, Tmax, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    lg = c["logits"].double()
    prob = torch.sigmoid(lg) if cls_sigmoid else torch.softmax(lg, -1)
    off = c["offsets"].tolist()
    for b in range(B):
        t0, t1 = off[b], off[b + 1]
        if t1 == t0:
            continue
        x = c["pred"][b * Q:(b + 1) * Q].double()            # [Q, P]
        t = c["tgt"][t0:t1].double()                         # [T, P]
        sp = F.softplus(x).sum(-1, keepdim=True)
        s = torch.sigmoid(x)
        pr = prob[b][:, c["labels"][t0:t1].long()]
        ratio = (2.0 * (s @ t.T) + 1.0) / (s.sum(-1, keepdim=True) + t.sum(-1)[None] + 1.0)
        ref[b, :, :t1 - t0] = w_mask * (sp - x @ t.T) / P - w_class * pr + w_dice * (1.0 - ratio)
        mag[b, :, :t1 - t0] = w_mask * (sp + x.abs() @ t.T) / P + w_class * pr + w_dice * (1.0 + ratio)
    return ref, mag


# ------------------------------------------------------------------------------------------------ set loss and its gradients
def bands(h, w):
    """(band_rows, number of bands, rows of the last band) of the LDS backward; None when w > MPB_LDS_FLOATS (the atomic form runs)."""
    if w > MPB_LDS_FLOATS:
        return None
    br = min(h, MPB_LDS_FLOATS // w)
    nb = (h + br - 1) // br
    return br, nb, h - (nb - 1) * br


# name: h, w, B, Q, counts, K, num_points, n_over, n_extra, u8 targets, free coordinates, seed.  H x W = 4 x (h x w).
#   one-pair       sum_T = 1: out3 is one pair; B x Q = 5 rows, K + 1 = 65
#   three-images   sum_T = 9 over B = 3, the middle image empty, indices permuted within each image; 21 rows, K + 1 = 151
#   two-bands      130 x 127: band_rows = 129, a second band of one row; B x Q = 7 rows
#   three-bands    200 x 200: bands of 81, 81 and 38 rows
#   row-bands      3 x 16384: band_rows = 1, the two tap rows of every point fall into different bands; 64 KiB of LDS
#   too-wide       2 x 16385: w > MPB_LDS_FLOATS, the atomic kernel in the default process
#   free           torch.rand coordinates (seed 0: selection margin 3.8 x the required 16 x bound, and of the seeds tried the one whose
#                  weakest point stands highest above the dmasks gate)
#   many-targets   65 targets in one image (the lane loop over the matches runs twice), small planes; one row with logits near 60
SET_CASES = {
    "one-pair":     (40, 48, 1, 5, (1,), 64, 112, 336, 28, False, False, 0),
    "three-images": (40, 48, 3, 7, (5, 0, 4), 150, 112, 336, 28, True, False, 0),
    "two-bands":    (130, 127, 1, 7, (2,), 64, 1000, 3000, 250, True, False, 0),
    "three-bands":  (200, 200, 2, 3, (1, 2), 20, 341, 1023, 86, False, False, 0),
    "row-bands":    (3, 16384, 1, 2, (1,), 64, 112, 336, 28, True, False, 0),
    "too-wide":     (2, 16385, 1, 2, (2,), 20, 112, 336, 28, False, False, 0),
    "free":         (40, 48, 2, 5, (2, 3), 64, 112, 336, 28, False, True, 0),
    "many-targets": (5, 6, 2, 70, (65, 2), 64, 16, 48, 4, True, False, 0),
}
SET_W = (2.0, 5.0, 3.0)                 # w_ce, w_mask, w_dice
GRADS = {"all": (0.5, 1.25, 0.75), "no-dice": (0.5, 1.25, 0.0), "no-bce": (0.5, 0.0, 0.75)}
EOS = 0.1


def _matches(B, Q, counts, g):
    """pred_idx (distinct within an image) and tgt_idx (a permutation of the image's targets), both in a shuffled order."""
    pi, ti = [], []
    for b in range(B):
        pi.append(torch.randperm(Q, generator=g)[:counts[b]])
        ti.append(torch.randperm(counts[b], generator=g))
    return torch.cat(pi).int(), torch.cat(ti).int()


def target_classes(B, Q, K, labels, off, pred_idx, tgt_idx):
    y = torch.full((B, Q), K, dtype=torch.long)
    for b in range(B):
        for i in range(off[b], off[b + 1]):
            y[b, int(pred_idx[i])] = int(labels[off[b] + int(tgt_idx[i])])
    return y


def set_loss_ref(c, grads=None):
    """out3 with magnitudes; with `grads` also dmasks [B*Q, h*w], dlogits [B*Q, K+1], their magnitudes and, per point, the pixel of its
    main tap and its contribution there.  Stores into c["sel"] the selected candidate indices of every pair (index order)."""
    B, Q, K, h, w, H, W = c["B"], c["Q"], c["K"], c["h"], c["w"], c["H"], c["W"]
    w_ce, w_mask, w_dice = c["weights"]
    P, n_over, n_extra, k_imp, free = c["num_points"], c["n_over"], c["n_extra"], c["k_imp"], c["free"]
    off = c["offsets"].tolist()
    nm = c["num_masks"]
    # ---- class part
    lg = c["logits"].double().reshape(B * Q, K + 1)
    y = target_classes(B, Q, K, c["labels"], off, c["pred_idx"], c["tgt_idx"]).reshape(-1)
    wy = torch.where(y == K, torch.full_like(lg[:, 0], c["eos"]), torch.ones_like(lg[:, 0]))
    mx = lg.max(-1).values
    lse = torch.log(torch.exp(lg - mx[:, None]).sum(-1))
    ly = lg.gather(1, y[:, None])[:, 0]
    nll = (mx + lse) - ly
    out = {"y": y, "out3": torch.zeros(3, dtype=torch.float64), "out3_mag": torch.zeros(3, dtype=torch.float64)}
    out["out3"][0] = w_ce * (wy * nll).sum() / wy.sum()
    out["out3_mag"][0] = w_ce * (wy * (mx.abs() + lse.abs() + ly.abs())).sum() / wy.sum()
    if grads is not None:
        g0, g1, g2 = grads
        p = torch.softmax(lg, -1)
        hot = F.one_hot(y, K + 1).double()
        coef = (g0 * w_ce * wy / wy.sum())[:, None]
        out["dlogits"], out["dlogits_mag"] = coef * (p - hot), coef.abs() * (p + hot)
        out["dmasks"] = torch.zeros(B * Q, h * w, dtype=torch.float64)
        out["dmasks_mag"] = torch.zeros_like(out["dmasks"])
        out["points"] = []
        c_bce, c_dice = w_mask / (nm * P), w_dice / nm
    # ---- mask part, pair by pair
    sel_all, gaps, lm, ld, lm_mag, ld_mag = [], [], 0.0, 0.0, 0.0, 0.0
    n = 0
    for b in range(B):
        for i in range(off[b], off[b + 1]):
            q = int(c["pred_idx"][i])
            pm = c["pred_masks"][b * Q + q].reshape(h, w)
            tm = c["tgt_masks"][off[b] + int(c["tgt_idx"][i])].reshape(H, W)
            pts = []
            if k_imp > 0:
                ro = c["rand_over"][n]
                xo, xo_mag = sample64(pm, ro, free)
                order = torch.sort(xo.abs(), stable=True).indices
                sel = torch.sort(order[:k_imp]).values
                sel_all.append(sel)
                if k_imp < n_over:
                    s_abs = xo.abs()[order]
                    gaps.append((float(s_abs[k_imp] - s_abs[k_imp - 1]), float(xo_mag.max())))
                pts.append(ro[sel])
            else:
                sel_all.append(torch.zeros(0, dtype=torch.long))
            if n_extra > 0:
                pts.append(c["rand_extra"][n])
            pts = torch.cat(pts)
            x, xm = sample64(pm, pts, free)
            t, tmg = sample64(tm, pts, free)
            s = torch.sigmoid(x)
            bce = x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))
            ST, SS, TT = (s * t).sum(), s.sum(), t.sum()
            D = SS + TT + 1.0
            lm += float(bce.sum()) / P
            ld += float(1.0 - (2.0 * ST + 1.0) / D)
            lm_mag += float((x.clamp_min(0) + x.abs() * tmg + torch.log1p(torch.exp(-x.abs())) + xm).sum()) / P
            ld_mag += float(1.0 + (2.0 * ST + 1.0) / D + 2.0 * (xm / 4.0 + tmg).sum() / D)
            if grads is not None:
                da, db = -2.0 / D, (2.0 * ST + 1.0) / (D * D)
                v = g1 * c_bce * (s - t) + g2 * c_dice * (s * (1.0 - s)) * (da * t + db)
                # d s / dx = s (1 - s) and |d (s (1 - s)) / dx| <= s (1 - s): the error of x (its rounding xm, and |x| + 2 roundings of
                # exp(-x)) enters with that factor, so mag shrinks with the gradient where the sigmoid saturates
                ds = s * (1.0 - s)
                # 1 - s is exact for s >= 1/2 but inherits the rounding of s, an absolute s * 2^-24 that is large against 1 - s where the
                # sigmoid saturates: the s * s term
                vm = abs(g1 * c_bce) * (s + tmg + ds * (xm + 2.0)) + abs(g2 * c_dice) * (ds * (xm + 3.0) + s * s) * (abs(da) * tmg + db)
                out["dmasks"][b * Q + q] = scatter64(h, w, pts, v)
                out["dmasks_mag"][b * Q + q] = scatter64(h, w, pts, vm)
                if free:     # the tap weights themselves move with the coordinate
                    ixy = index64(pts[:, 0], w).abs() + index64(pts[:, 1], h).abs() + 1.0
                    out["dmasks_mag"][b * Q + q] += scatter64(h, w, pts, v.abs() * ixy, weighted=False)
                pix, wt = main_tap(h, w, pts)
                out["points"].append((b * Q + q, pix, v.abs() * wt))
            n += 1
    out["out3"][1], out["out3"][2] = w_mask * lm / nm, w_dice * ld / nm
    out["out3_mag"][1], out["out3_mag"][2] = w_mask * lm_mag / nm, w_dice * ld_mag / nm
    out["sel"], out["gaps"] = sel_all, gaps
    return out


@functools.lru_cache(maxsize=None)
def set_case(name, seed=None):
    h, w, B, Q, counts, K, P, n_over, n_extra, u8, free, seed0 = SET_CASES[name]
    seed = seed0 if seed is None else seed
    g = gen(seed * 1000 + sum(ord(ch) for ch in name))
    H, W = 4 * h, 4 * w
    n = sum(counts)
    gb = grid_bits(H, W)
    logits = torch.randn(B, Q, K + 1, generator=g) * 2.0
    if name == "many-targets":
        logits[0, 3] = torch.randn(K + 1, generator=g) * 2.0 + 58.0          # large logits near 60 in one row
    pred = torch.randn(B * Q, h * w, generator=g) * 3.0
    if u8:
        tgt = (torch.rand(n, H * W, generator=g) > 0.5).to(torch.uint8)
    else:
        tgt = torch.randint(0, 5, (n, H * W), generator=g).float() / 4.0
    labels = torch.randint(0, K, (n,), generator=g, dtype=torch.int32)
    pred_idx, tgt_idx = _matches(B, Q, counts, g)
    if free:
        ro, re = torch.rand(n, n_over, 2, generator=g), torch.rand(n, n_extra, 2, generator=g)
    else:
        ro, re = dyadic((n, n_over, 2), gb, g), dyadic((n, n_extra, 2), gb, g)
        sp = torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0], [0.5, 0.5]])
        re[:, :min(4, n_extra)] = sp[:min(4, n_extra)]                            # the extra points are always used
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    c = {"name": name, "h": h, "w": w, "H": H, "W": W, "B": B, "Q": Q, "K": K, "counts": counts, "sum_T": n, "num_points": P, "n_over": n_over,
         "n_extra": n_extra, "k_imp": P - n_extra, "u8": u8, "free": free, "g": gb, "logits": logits, "pred_masks": pred, "tgt_masks": tgt,
         "labels": labels, "offsets": off, "pred_idx": pred_idx, "tgt_idx": tgt_idx, "rand_over": ro, "rand_extra": re, "weights": SET_W,
         "eos": EOS, "num_masks": float(n) + 0.5, "exact": False}
    return c


@functools.lru_cache(maxsize=None)
def set_ref(name, grads_key=None):
    return set_loss_ref(set_case(name), None if grads_key is None else GRADS[grads_key])


def matched_rows(c):
    off = c["offsets"].tolist()
    rows = torch.zeros(c["B"] * c["Q"], dtype=torch.bool)
    for b in range(c["B"]):
        for i in range(off[b], off[b + 1]):
            rows[b * c["Q"] + int(c["pred_idx"][i])] = True
    return rows


# ------------------------------------------------------------------------------------------------ the selection run
# 64 x 32 planes, values multiples of 1/8, every candidate at the centre of its own pixel: x IS the plane value (exact in fp32), so the
# selected set is a matter of keys and ranks alone.  40 candidates with |x| = 1.5 (mixed signs) are planted so that exactly `need` of
# them are selected: 17 where k_imp allows, all that fit otherwise.  Ten of them are consecutive in index order from an odd index, so
# with chunks of two (n_over > 1024) they share chunks and straddle chunk boundaries; the others are spread.  Targets are constant over
# 4 x 4 blocks and binary, so t is 0 or 1 exactly, s - t is never 0 and every selected point leaves a nonzero gradient in its pixel.
SEL_H, SEL_W = 64, 32
SEL_N_OVER = [300, 1024, 1025, 1500]
SEL_K_IMP = [1, 100, "all", 0]
SEL_TIES, SEL_TIE_ABS, SEL_NEED = 40, 1.5, 17


def sel_id(n_over, k):
    return f"n{n_over}-k{k}"


@functools.lru_cache(maxsize=None)
def selection_case(n_over, k):
    k_imp = n_over if k == "all" else int(k)
    n_extra = 16 if k_imp == 0 else 5
    P = k_imp + n_extra
    B, Q, K, n = 1, 3, 4, 2
    h, w, H, W = SEL_H, SEL_W, 4 * SEL_H, 4 * SEL_W
    g = gen(n_over * 13 + k_imp)
    need = min(SEL_NEED, k_imp)
    n_below = k_imp - need if k_imp < n_over else 0
    centres = pixel_centres(h, w)
    pred = torch.zeros(B * Q, h * w)
    tgt = torch.zeros(n, H, W)
    ro = torch.zeros(n, n_over, 2)
    re = torch.zeros(n, n_extra, 2)
    pred_idx, tgt_idx = torch.tensor([2, 0], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    tie_index = []
    for pair in range(n):
        pix = torch.randperm(h * w, generator=g)
        cand, extra = pix[:n_over], pix[n_over:n_over + n_extra]
        start = 2 * int(torch.randint(10, (n_over - 20) // 2, (1,), generator=g)) + 1                 # odd
        run = torch.arange(start, start + 10)
        rest = torch.tensor([i for i in torch.randperm(n_over, generator=g).tolist() if i < start or i >= start + 10][:SEL_TIES - 10])
        ties = torch.sort(torch.cat([run, rest])).values
        other = torch.tensor([i for i in torch.randperm(n_over, generator=g).tolist() if i not in set(ties.tolist())])
        below, above = other[:n_below], other[n_below:]
        a = torch.zeros(n_over)
        a[ties] = SEL_TIE_ABS
        a[below] = torch.randint(0, 12, (below.numel(),), generator=g).float() / 8.0                # 0 .. 1.375, zeros of both signs among them
        a[above] = torch.randint(13, 65, (above.numel(),), generator=g).float() / 8.0               # 1.625 .. 8
        sign = torch.where(torch.rand(n_over, generator=g) < 0.5, -1.0, 1.0)
        plane = torch.randint(-64, 65, (h * w,), generator=g).float() / 8.0
        plane[cand] = a * sign
        pred[int(pred_idx[pair])] = plane
        small = (torch.rand(h, w, generator=g) > 0.5).float()
        tgt[int(tgt_idx[pair])] = small.repeat_interleave(4, 0).repeat_interleave(4, 1)
        ro[pair], re[pair] = centres[cand], centres[extra]
        tie_index.append(ties)
    pred[1] = float("nan")                                                                           # the unmatched query's plane is never read
    logits = torch.randn(B, Q, K + 1, generator=g)
    c = {"name": sel_id(n_over, k), "h": h, "w": w, "H": H, "W": W, "B": B, "Q": Q, "K": K, "counts": (n,), "sum_T": n, "num_points": P,
         "n_over": n_over, "n_extra": n_extra, "k_imp": k_imp, "u8": False, "free": False, "g": 0, "logits": logits, "pred_masks": pred,
         "tgt_masks": tgt.reshape(n, H * W), "labels": torch.tensor([1, 3], dtype=torch.int32), "offsets": torch.tensor([0, n], dtype=torch.int32),
         "pred_idx": pred_idx, "tgt_idx": tgt_idx, "rand_over": ro, "rand_extra": re, "weights": SET_W, "eos": EOS, "num_masks": 2.0,
         "exact": True, "ties": tie_index, "need": need if k_imp < n_over else None, "n_below": n_below,
         "chunk": (n_over + MPL_THREADS - 1) // MPL_THREADS}
    return c


SEL_GRADS = (0.5, 1.0, 0.0)      # no dice term: v = g1 c_bce (s - t), never 0


@functools.lru_cache(maxsize=None)
def selection_ref(n_over, k):
    c = dict(selection_case(n_over, k))
    c["pred_masks"] = torch.nan_to_num(c["pred_masks"], nan=0.0)
    return set_loss_ref(c, SEL_GRADS)


def expected_pixels(c, ref):
    """bool [B*Q, h*w]: the pixels of the reference's selected candidates and of the extra points."""
    out = torch.zeros(c["B"] * c["Q"], c["h"] * c["w"], dtype=torch.bool)
    for n in range(c["sum_T"]):
        row = int(c["pred_idx"][n])          # B = 1
        pts = torch.cat([c["rand_over"][n][ref["sel"][n]], c["rand_extra"][n]])
        pix, wt = main_tap(c["h"], c["w"], pts)
        assert bool((wt == 1.0).all())
        out[row, pix] = True
    return out


def point_gate_ratio(ref, cgate):
    """Largest (one fp32 rounding + cgate * mag at a point's main tap) / (that point's own contribution there) over the points of a case:
    below 1, a dropped or extra point cannot pass the dmasks gate."""
    bound = 2.0 ** -24 * ref["dmasks"].abs() + 2.0 ** -126 + cgate * ref["dmasks_mag"]
    return max(float((bound[row, pix] / contrib).max()) for row, pix, contrib in ref["points"])
