"""Seeded cases and float64 references for the direct tests of the deformable-attention training kernels, their prelude and the fused
AdamW step of csrc/train_ops.hip (tests/test_gpu_msda_train_ops.py; pinned without a GPU by tests/test_msda_train_cases_cpu.py).
No GPU and no library here: numpy / torch on the CPU only.

The core reference is written from the DEFINITION of the reference function - F.grid_sample, bilinear, zeros padding,
align_corners=False - not from the kernels' make_taps: the pixel coordinate of a location is ix = loc_x * W - 0.5, iy = loc_y * H - 0.5,
the four pixels around it carry the weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty, a pixel outside the map counts as 0.

Magnitudes.  With every output comes `mag`: the same sum with every term in absolute value, plus a POSITION term.  fp32 carries ix with an
absolute error proportional to W * 2^-24, and so the bilinear weights.  The kernels evaluate
    gx = 2 lx - 1;   ix = ((gx + 1) W - 1) / 2
with one rounding (u = 2^-24 relative) per operation: u |gx| on gx, u |gx + 1| more on gx + 1, both times W, u |gx + 1| W for the product,
u |2 ix| for the subtraction, and an exact halving:
    |d ix| <= u/2 (W (|gx| + 2 |gx + 1|) + 2 |ix|) <= u (W (1/2 + 3 |lx|) + |lx| W + 1/2) <= u W (1/2 + 4 |lx| + 1 / (2 W)).
tx = ix - floor(ix) is exact.  For |lx| <= 1.25 (asserted for every point that has a pixel inside the map) that is below POS * W * u with
POS = 6.  An output that depends on ix through s (the sampled value) therefore moves by up to POS * u * W * |ds/dix|; the position term of
its magnitude is POS * aw * (W |ds/dix|_abs + H |ds/diy|_abs), so that |got - ref| <= c * mag can hold with c of the order of u.  For the
location gradient ds/dix depends on ty only: its position term is POS * H * (|v00| + |v01| + |v10| + |v11|), and likewise for y; for the
value gradient the weight of a tap moves by POS * u * (W wy + H wx).

Rules the inputs follow, so that the float64 reference alone decides the answer:
* random sampling points are NUDGED at construction (never left out): the float64 pixel coordinate of every point stays at least 2^-10
  pixel away from every grid line, where the derivative of bilinear sampling jumps and fp32 could floor to the other pixel;
* points meant to sit on pixel centres or grid lines use power-of-two level sizes and dyadic locations, so that every fp32 step of the
  coordinate arithmetic is exact;
* values and output gradients are multiples of 1/16 below 4: they are the same number in fp32, bfloat16 and IEEE half, so ONE case and
  one reference serve the fp32 and the element-typed operands of both libraries;
* exact runs: values small integers, attn powers of two, tx, ty in {0, 1/4, 1/2, 3/4}, grad_out in {-1, 0, 1}: every product and partial
  sum is a dyadic far below 2^24 (and the binned value gradient has at most 8 significant bits), so fp32 in any order gives the float64
  bits.

Which case is for which edge: CORE_CASES below."""
import functools
import math

import numpy as np
import torch

from tests.helpers import pow2

M, D = 8, 32
CH = M * D
U32 = 2.0 ** -24
POS = 6.0                    # see above
LOC_BOUND = 1.25             # |loc| of every point that has a pixel inside the map
GRID_DIST = 2.0 ** -10       # distance every random point keeps from the grid lines
MS_PIX, MS_MAXL, MS_HOT, LDS_BYTES = 3200, 8, 96, 160 * 1024
PRODUCTION = [[80, 80], [40, 40], [20, 20]]
CROWD_COUNTS = (95, 96, 97, 111, 112, 113, 128, 129)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the slab form's host arithmetic, restated
def slab_smem(P, Q, go16):
    """Dynamic LDS of msda_bwd_value_kernel: MS_PIX counters, 8 wave totals, 2 ints, 512 partial sums, the set-aside list (padded so the
    entries start on 16 bytes), Q*P*4 8-byte entries, Q grad_out rows of 32."""
    fixed = MS_PIX + 8 + 2 + 512
    hot = (fixed + (Q * P * 4 // MS_HOT + 2) + 3) // 4 * 4 - fixed
    return (fixed + hot) * 4 + Q * P * 4 * 8 + Q * 32 * (2 if go16 else 4)


def slab_supported(shapes, P, Q, Mh, go16):
    L = len(shapes)
    if Mh != 8 or L < 1 or L > MS_MAXL or P < 1 or Q < 1 or Q >= 1 << 24:
        return False
    if any(h < 1 or w < 1 or w > MS_PIX for h, w in shapes):
        return False
    return slab_smem(P, Q, go16) <= LDS_BYTES


def q_max(P, go16):
    q = 1
    while slab_smem(P, q + 1, go16) <= LDS_BYTES:
        q += 1
    return q


def slab_rows(H, W):
    """(rows per slab, number of slabs, rows of the last slab) of one level."""
    rows = min(MS_PIX // W, H)
    n = (H + rows - 1) // rows
    return rows, n, H - (n - 1) * rows


def level_starts(shapes):
    out, acc = [], 0
    for h, w in shapes:
        out.append(acc)
        acc += h * w
    return out, acc


# ------------------------------------------------------------------------------------------------ coordinates
def pix64(loc, shapes):
    """float64 pixel coordinates [B,Q,M,L,P,2] of fp32 locations."""
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    return loc.double() * wh - 0.5


def pix32(loc, shapes):
    """The kernels' coordinate formula, every step rounded to fp32 (numpy float32 arithmetic): ((2 l - 1 + 1) * W - 1) * 0.5."""
    l32 = loc.numpy().astype(np.float32)
    wh = np.array([[w, h] for h, w in shapes], dtype=np.float32)[None, None, None, :, None, :]
    one, two, half = np.float32(1), np.float32(2), np.float32(0.5)
    g = two * l32 - one
    return torch.from_numpy((((g + one) * wh - one) * half).astype(np.float32))


def nudge(loc, shapes):
    """Move every point whose float64 pixel coordinate lies within 2^-9 of a grid line by 3 * 2^-9 pixel (then 2^-8 .. 2^-7 away), in
    fp32; deterministic, and no point is dropped."""
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    for _ in range(2):
        ix = pix64(loc, shapes)
        near = (ix - torch.round(ix)).abs() < 2.0 ** -9
        loc = torch.where(near, (loc.double() + 3 * 2.0 ** -9 / wh), loc.double()).float()
    return loc


def has_inside_tap(loc, shapes):
    """bool [B,Q,M,L,P]: at least one of the four pixels lies in the map."""
    ix = pix64(loc, shapes)
    x0, y0 = torch.floor(ix[..., 0]), torch.floor(ix[..., 1])
    W = torch.tensor([w for _, w in shapes], dtype=torch.float64)[None, None, None, :, None]
    H = torch.tensor([h for h, _ in shapes], dtype=torch.float64)[None, None, None, :, None]
    return (x0 >= -1) & (x0 <= W - 1) & (y0 >= -1) & (y0 <= H - 1)


# ------------------------------------------------------------------------------------------------ core cases
def _sixteenths(shape, g, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 16


def _softmax_attn(B, Q, L, P, g):
    return torch.softmax(torch.randn(B, Q, M, L * P, generator=g), -1).view(B, Q, M, L, P).float()


def _case(name, shapes, B, Q, P, loc, attn, value, go, exact=False, random=True):
    starts, S = level_starts(shapes)
    assert value.shape == (B, S, CH) and loc.shape == (B, Q, M, len(shapes), P, 2) and attn.shape == loc.shape[:-1] and go.shape == (B, Q, CH)
    return {"name": name, "shapes": [list(s) for s in shapes], "starts": starts, "S": S, "B": B, "Q": Q, "L": len(shapes), "P": P, "loc": loc.float().contiguous(),
            "attn": attn.float().contiguous(), "value": value.float().contiguous(), "go": go.float().contiguous(), "exact": exact, "random": random}


def _random_case(name, shapes, B, Q, P, seed, plant=None):
    g = gen(seed)
    L = len(shapes)
    _, S = level_starts(shapes)
    loc = torch.rand(B, Q, M, L, P, 2, generator=g) * 1.3 - 0.15
    if plant is not None:
        loc = plant(loc)
    loc = nudge(loc.float(), shapes)
    return _case(name, shapes, B, Q, P, loc, _softmax_attn(B, Q, L, P, g), _sixteenths((B, S, CH), g, 63), _sixteenths((B, Q, CH), g, 31))


def _plant_rows(level, H, rows):
    """Queries 0 .. len(rows)-1, point 0 of `level`: iy = row + 0.3, so that y0 = row and y0 + 1 = row + 1."""
    def f(loc):
        for q, r in enumerate(rows):
            loc[:, q, :, level, 0, 1] = (r + 0.8) / H
        return loc
    return f


def _edges_case():
    """One 4 x 4 level, P = 1, 21 queries (every head the same point): the four corners half outside = locations exactly 0.0 and 1.0, the
    four edges half outside, all four pixels outside on each side, far outside (-3, 5), exact pixel centres (inner, last column / row)."""
    pts = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.4), (1.0, 0.4), (0.4, 0.0), (0.4, 1.0), (-0.3, 0.5), (1.3, 0.5), (0.5, -0.3), (0.5, 1.3),
           (-3.0, 5.0), (5.0, -3.0), (0.125, 0.125), (0.875, 0.875), (0.375, 0.625), (0.875, 0.125), (0.25, 0.5), (0.5, 0.75), (0.3, 0.7)]
    Q = len(pts)
    g = gen(404)
    loc = torch.tensor(pts, dtype=torch.float32)[None, :, None, None, None, :].expand(1, Q, M, 1, 1, 2).contiguous()
    attn = torch.rand(1, Q, M, 1, 1, generator=g) + 0.25
    return _case("edges", [[4, 4]], 1, Q, 1, loc, attn, _sixteenths((1, 16, CH), g, 63), _sixteenths((1, Q, CH), g, 31), random=False)


EDGE_CENTRES = {14: (0, 0), 15: (3, 3), 16: (1, 2), 17: (3, 0)}       # query -> (x0, y0) with tx = ty = 0
EDGE_LINES = {18: (0.5, 1.5), 19: (1.5, 2.5)}                        # query -> (ix, iy): loc = k / W, half way between two centres


def _exact_case(name, shapes, Q, P, seed):
    """Dyadic points on power-of-two levels: ix = x0 + tx with x0 in [-1, W - 1] (borders included) and tx in {0, 1/4, 1/2, 3/4}."""
    g = gen(seed)
    L = len(shapes)
    _, S = level_starts(shapes)
    loc = torch.empty(1, Q, M, L, P, 2)
    for l, (h, w) in enumerate(shapes):
        assert h & (h - 1) == 0 and w & (w - 1) == 0
        for k, n in ((0, w), (1, h)):
            x0 = torch.randint(-1, n, (1, Q, M, P), generator=g).float()
            t = torch.randint(0, 4, (1, Q, M, P), generator=g).float() / 4
            loc[:, :, :, l, :, k] = (x0 + t + 0.5) / n
    attn = 2.0 ** -torch.randint(0, 2, (1, Q, M, L, P), generator=g).float()
    value = torch.randint(-3, 4, (1, S, CH), generator=g).float()
    go = torch.randint(-1, 2, (1, Q, CH), generator=g).float()
    return _case(name, shapes, 1, Q, P, loc, attn, value, go, exact=True, random=False)


CROWD_Q, CROWD_SIDE = 224, 16


def crowd_targets(h):
    """Head h: pixel (x, y) -> number of points put on its centre.  Eight targets four pixels apart (a centre point files an entry - three
    of them of weight 0 - under (x, y), (x+1, y), (x, y+1) and (x+1, y+1), so each count occurs on four pixels); the list rotates with
    the head."""
    cells = [(1 + 4 * (i % 4), 1 + 4 * (i // 4)) for i in range(8)]
    return {cells[i]: CROWD_COUNTS[(i + h) % 8] for i in range(8)}


def _crowd_case():
    """Exact run of the set-aside path: one 16 x 16 level, Q = 224, P = 4 (896 points per head), 881 of them on eight pixel centres with
    exactly 95, 96, 97, 111, 112, 113, 128 and 129 points, the other 15 on the centre of pixel (13, 13); attn = 1, grad_out in {-1, 0, 1}:
    the value gradient of a target pixel is an integer of at most 129, exact in fp32 and in both 16-bit types.  Q * 8 = 1792 > 512: four
    staging passes of the grad_out rows.  Two batches."""
    g = gen(129)
    B, Q, P, n = 2, CROWD_Q, 4, CROWD_SIDE
    loc = torch.empty(B, Q, M, 1, P, 2)
    for h in range(M):
        cells = []
        for (x, y), k in crowd_targets(h).items():
            cells += [(x, y)] * k
        cells += [(13, 13)] * (Q * P - len(cells))
        c = torch.tensor(cells, dtype=torch.float32)
        for b in range(B):
            perm = torch.randperm(Q * P, generator=g)
            loc[b, :, h, 0] = ((c[perm] + 0.5) / n).view(Q, P, 2)
    attn = torch.ones(B, Q, M, 1, P)
    value = torch.randint(-3, 4, (B, n * n, CH), generator=g).float()
    go = torch.randint(-1, 2, (B, Q, CH), generator=g).float()
    return _case("crowd", [[n, n]], B, Q, P, loc, attn, value, go, exact=True, random=False)


def _qmax_case(go16):
    Q = q_max(4, go16)
    return _random_case(f"qmax_go{'16' if go16 else '32'}", [[4, 4], [2, 2]], 1, Q, 4, 700 + int(go16))


# name -> (builder, what the case is for)
CORE_CASES = {
    "l1p1": (lambda: _random_case("l1p1", [[2, 2]], 1, 1, 1, 11), "B*Q = 1 (one wave of a block of four), L = 1, P = 1, a 2 x 2 level"),
    "l3p3": (lambda: _random_case("l3p3", [[1, 1], [1, 9], [7, 1]], 1, 15, 3, 12), "B*Q = 15 (tail block of three waves), L = 3, P = 3 (the point split falls back to 1), "
             "levels 1 x 1, 1 x W, H x 1"),
    "l8p4": (lambda: _random_case("l8p4", [[16, 16], [8, 8], [4, 4], [2, 2], [1, 1], [3, 400], [5, 7], [2, 2]], 1, 67, 4, 13), "B*Q = 64 + 3, L = MS_MAXL = 8, P = 4, "
             "a power-of-two pyramid, 3 x 400, Q * 8 = 536 > 512: two staging passes"),
    "prod": (lambda: _random_case("prod", PRODUCTION, 2, 40, 4, 14, _plant_rows(0, 80, [39, 39, 39])), "the production pyramid once, two batches; 80 x 80 = two slabs of 40 rows, "
             "planted points with y0 = 39, y0 + 1 = 40 in different slabs"),
    "slabs": (lambda: _random_case("slabs", [[100, 33], [2, 3200]], 1, 67, 4, 15, lambda loc: _plant_rows(1, 2, [0, 0])(_plant_rows(0, 100, [95, 95, 95])(loc))),
              "H = 100, W = 33: 96 rows per slab, a last slab of 4 rows; W = MS_PIX = 3200, H = 2: one row per slab; points with y0 and y0 + 1 in "
              "different slabs on both levels; most pixels without a tap"),
    "edges": (_edges_case, "positions: corners and edges half outside, 0.0 and 1.0 exactly, all pixels outside, far outside, pixel centres, grid lines"),
    "exact": (lambda: _exact_case("exact", [[16, 16], [8, 8]], 15, 4, 21), "exact run, P = 4, two levels"),
    "exact3": (lambda: _exact_case("exact3", [[8, 8], [4, 4], [16, 16]], 15, 3, 22), "exact run, P = 3, three levels"),
    "crowd": (_crowd_case, "exact run of the set-aside path: pixels with 95 .. 129 entries, several set-aside pixels in one slab"),
    "qmax_go16": (lambda: _qmax_case(True), "the largest Q the slab form admits at P = 4 with 16-bit grad_out"),
    "qmax_go32": (lambda: _qmax_case(False), "the same with fp32 grad_out"),
}
EXACT_CASES = ("exact", "exact3", "crowd")
GATED_CASES = ("l1p1", "l3p3", "l8p4", "prod", "slabs", "edges")
QMAX_CASES = ("qmax_go16", "qmax_go32")


@functools.lru_cache(maxsize=None)
def core_case(name):
    return CORE_CASES[name][0]()


def core_ref_tensors(value, shapes, loc, attn, go):
    """float64: dict of out, grad_value [B,S,256], grad_loc, grad_attn, each with its `_mag`, and counts int64 [B,M,S] (every in-range tap,
    weight 0 included, as the binning kernel counts them)."""
    B, S, _ = value.shape
    _, Q, _, L, P, _ = loc.shape
    starts, S_ = level_starts(shapes)
    assert S == S_
    v4, g4 = value.double().view(B, S, M, D), go.double().view(B, Q, M, 1, D)
    ga = g4.abs()
    pix = pix64(loc, shapes)
    aw_all = attn.double()
    out, out_mag = torch.zeros(B, Q, M, D, dtype=torch.float64), torch.zeros(B, Q, M, D, dtype=torch.float64)
    gv, gv_mag = torch.zeros(B * S * M, D, dtype=torch.float64), torch.zeros(B * S * M, D, dtype=torch.float64)
    cnt = torch.zeros(B * M * S, dtype=torch.int64)
    g_attn, g_attn_mag = torch.zeros(B, Q, M, L, P, dtype=torch.float64), torch.zeros(B, Q, M, L, P, dtype=torch.float64)
    g_loc, g_loc_mag = torch.zeros(B, Q, M, L, P, 2, dtype=torch.float64), torch.zeros(B, Q, M, L, P, 2, dtype=torch.float64)
    bi = torch.arange(B)[:, None, None, None]
    hi = torch.arange(M)[None, None, :, None]
    for l, (H, W) in enumerate(shapes):
        ix, iy = pix[:, :, :, l, :, 0], pix[:, :, :, l, :, 1]                # [B,Q,M,P]
        x0, y0 = torch.floor(ix), torch.floor(iy)
        tx, ty = ix - x0, iy - y0
        a = aw_all[:, :, :, l]
        vs, idxs, oks = [], [], []
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            idx = torch.where(ok, starts[l] + yy * W + xx, torch.zeros_like(xx)).long()
            vs.append(v4[bi, idx, hi] * ok[..., None])
            idxs.append(idx)
            oks.append(ok)
        wx, wy = (1 - tx, tx, 1 - tx, tx), (1 - ty, 1 - ty, ty, ty)
        v00, v01, v10, v11 = vs
        e = lambda t: t[..., None]                                            # noqa: E731
        s = sum(e(wx[k] * wy[k]) * vs[k] for k in range(4))
        s_abs = sum(e(wx[k] * wy[k]) * vs[k].abs() for k in range(4))
        dsx = (v01 - v00) * e(1 - ty) + (v11 - v10) * e(ty)
        dsy = (v10 - v00) * e(1 - tx) + (v11 - v01) * e(tx)
        dsx_abs = (v01.abs() + v00.abs()) * e(1 - ty) + (v11.abs() + v10.abs()) * e(ty)
        dsy_abs = (v10.abs() + v00.abs()) * e(1 - tx) + (v11.abs() + v01.abs()) * e(tx)
        d2 = v00.abs() + v01.abs() + v10.abs() + v11.abs()
        s_mag = s_abs + POS * (W * dsx_abs + H * dsy_abs)
        out += (e(a) * s).sum(3)
        out_mag += (e(a) * s_mag).sum(3)
        g_attn[:, :, :, l] = (g4 * s).sum(-1)
        g_attn_mag[:, :, :, l] = (ga * s_mag).sum(-1)
        g_loc[:, :, :, l, :, 0] = a * W * (g4 * dsx).sum(-1)
        g_loc[:, :, :, l, :, 1] = a * H * (g4 * dsy).sum(-1)
        g_loc_mag[:, :, :, l, :, 0] = a * W * (ga * (dsx_abs + POS * H * d2)).sum(-1)
        g_loc_mag[:, :, :, l, :, 1] = a * H * (ga * (dsy_abs + POS * W * d2)).sum(-1)
        for k in range(4):
            ok = oks[k].reshape(-1)
            lin = ((bi * S + idxs[k]) * M + hi).reshape(-1)[ok]
            w = (a * wx[k] * wy[k]).reshape(-1)[ok]
            wm = (a * (wx[k] * wy[k] + POS * (W * wy[k] + H * wx[k]))).reshape(-1)[ok]
            gq = g4.expand(B, Q, M, P, D).reshape(-1, D)[ok]
            gv.index_add_(0, lin, w[:, None] * gq)
            gv_mag.index_add_(0, lin, wm[:, None] * gq.abs())
            clin = ((bi * M + hi) * S + idxs[k]).reshape(-1)[ok]
            cnt.index_add_(0, clin, torch.ones_like(clin))
    return {"out": out.view(B, Q, CH), "out_mag": out_mag.view(B, Q, CH), "grad_value": gv.view(B, S, CH), "grad_value_mag": gv_mag.view(B, S, CH),
            "grad_loc": g_loc, "grad_loc_mag": g_loc_mag, "grad_attn": g_attn, "grad_attn_mag": g_attn_mag, "counts": cnt.view(B, M, S)}


@functools.lru_cache(maxsize=None)
def core_ref(name):
    c = core_case(name)
    return core_ref_tensors(c["value"], c["shapes"], c["loc"], c["attn"], c["go"])


def pixel_terms(c, r):
    """int64 [B,S,256]: the number of terms of each element of the value gradient = its pixel's tap count (per head)."""
    return r["counts"].permute(0, 2, 1).repeat_interleave(D, dim=2).contiguous()


def half_step(x, dtype):
    """Half the spacing of `dtype` (torch.bfloat16 / torch.float16) at |x| (fp64): the most ONE rounding to it can move a value of that
    size; tests.helpers.elem_rne moves nothing further (CPU test)."""
    mant, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.frexp(x.double().abs().clamp_min(2.0 ** emin)).exponent
    return pow2(e - mant - 1)


# ------------------------------------------------------------------------------------------------ prelude
# (BQ, M, L, P): BQ * M in {8, 264}, M in {1, 8}, (L, P) in {(1, 1), (3, 4), (8, 3)}
PREP_SHAPES = [(1, 8, 1, 1), (33, 8, 3, 4), (264, 1, 8, 3), (8, 1, 3, 4)]
PREP_EQUAL_ROW, PREP_SPREAD_ROW, PREP_ZERO_WH_ROW = 0, 1, 2            # rows (queries) with equal logits, logits over +-80, ref_wh = 0; where BQ >= 3


@functools.lru_cache(maxsize=None)
def prep_case(shape):
    """off, logit multiples of 1/16 (integers in the spread row): the same numbers in both 16-bit types."""
    BQ, Mh, L, P = shape
    g = gen(1000 + BQ + 7 * L)
    LP = L * P
    off = _sixteenths((BQ, Mh * LP * 2), g, 127)
    logit = _sixteenths((BQ, Mh * LP), g, 63)
    ref = torch.cat([torch.rand(BQ, 2, generator=g), torch.rand(BQ, 2, generator=g) * 0.4 + 0.02], -1)
    if BQ >= 3:
        logit[PREP_EQUAL_ROW] = 1.5
        logit[PREP_SPREAD_ROW] = torch.linspace(-80, 80, LP).round().repeat(Mh)      # +-80 inside every (query, head)
        ref[PREP_ZERO_WH_ROW, 2:] = 0
    gl = torch.randn(BQ, Mh, LP, 2, generator=g)
    ga = torch.randn(BQ, Mh, LP, generator=g)
    aw = torch.softmax(torch.randn(BQ, Mh, LP, generator=g), -1)         # the backward is a case of its own: aw is an input
    return {"BQ": BQ, "M": Mh, "L": L, "P": P, "off": off, "logit": logit, "ref": ref.float(), "grad_loc": gl.float(), "grad_attn": ga.float(), "aw": aw.float()}


def prep_fwd_ref(c):
    """(loc [BQ,M,LP,2], mag), (aw [BQ,M,LP], mag) in float64."""
    BQ, Mh, LP, P = c["BQ"], c["M"], c["L"] * c["P"], c["P"]
    off = c["off"].double().view(BQ, Mh, LP, 2)
    ref = c["ref"].double()
    step = off / P * ref[:, None, None, 2:] * 0.5
    loc = ref[:, None, None, :2] + step
    x = c["logit"].double().view(BQ, Mh, LP)
    ex = torch.exp(x - x.max(-1, keepdim=True).values)
    aw = ex / ex.sum(-1, keepdim=True)
    return (loc, ref[:, None, None, :2].abs() + step.abs()), (aw, aw * (1 + aw.sum(-1, keepdim=True)))


def prep_bwd_ref(c):
    """(grad_off [BQ, M*LP*2], mag), (grad_logit [BQ, M*LP], mag) in float64 from the case's own aw."""
    BQ, Mh, LP, P = c["BQ"], c["M"], c["L"] * c["P"], c["P"]
    aw, ga, gl = c["aw"].double(), c["grad_attn"].double(), c["grad_loc"].double()
    ref = c["ref"].double()
    dot = (aw * ga).sum(-1, keepdim=True)
    g_logit = aw * (ga - dot)
    g_logit_mag = aw * (ga.abs() + (aw * ga.abs()).sum(-1, keepdim=True))
    g_off = gl * ref[:, None, None, 2:] * 0.5 / P
    return (g_off.reshape(BQ, -1), g_off.abs().reshape(BQ, -1)), (g_logit.reshape(BQ, -1), g_logit_mag.reshape(BQ, -1))


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_CHUNK = 65536
# (numel, lr, weight_decay) of the tensors of ONE flat buffer: 1 element, around the 256 threads of a workgroup, around one chunk;
# one tensor with lr = 0 (parameters unchanged, moments updated), one without weight decay
ADAMW_TENSORS = [(1, 1e-3, 1e-2), (255, 1e-4, 1e-4), (256, 0.0, 1e-2), (257, 1e-3, 0.0), (65535, 1e-4, 1e-4), (65536, 1e-5, 5e-2), (65537, 1e-3, 1e-2)]
ADAMW_BETAS, ADAMW_EPS = (0.9, 0.999), 1e-8
# (max_grad_norm, norm of the gradient, step): no clipping at all (the max_grad_norm <= 0 branch), below and above the bound, late steps
ADAMW_RUNS = [(0.0, 5.0, 1), (0.1, 0.05, 2), (0.1, 5.0, 10000), (0.1, 5.0, 1), (0.0, 0.05, 10000)]


def adamw_chunks(tensors=ADAMW_TENSORS, chunk=ADAMW_CHUNK):
    """(start, len, lr, wd) lists as FlatAdamW cuts them."""
    cs, cl, clr, cwd, o = [], [], [], [], 0
    for n, lr, wd in tensors:
        for c0 in range(0, n, chunk):
            cs.append(o + c0)
            cl.append(min(chunk, n - c0))
            clr.append(lr)
            cwd.append(wd)
        o += n
    return cs, cl, clr, cwd


@functools.lru_cache(maxsize=None)
def adamw_case(run):
    max_norm, norm, step = ADAMW_RUNS[run]
    g = gen(2000 + run)
    n = sum(t[0] for t in ADAMW_TENSORS)
    grad = torch.randn(n, generator=g)
    grad = (grad * (norm / float(grad.double().norm()))).float()
    p = torch.randn(n, generator=g)
    first = step == 1
    m = torch.zeros(n) if first else torch.randn(n, generator=g) * 1e-3
    v = torch.zeros(n) if first else torch.rand(n, generator=g) * 1e-5
    return {"p": p, "g": grad, "m": m, "v": v, "step": step, "max_norm": max_norm, "numel": n}


def f32(x):
    """The fp32 value the C ABI carries for a Python float, as a Python float."""
    return float(np.float32(x))


def adamw_ref(p, g, m, v, step, lr, wd, max_norm, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """One step of torch.nn.utils.clip_grad_norm_(max_norm) + torch.optim.AdamW in float64: (p, m, v, total_norm), and the magnitudes of
    p, m, v.  lr, wd: per-element float64 tensors; every hyper-parameter is the fp32 value the entry point receives (beta2 = 0.999f is
    the beta the step runs with: 1 - beta2 is formed from it)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    b1, b2, eps, mx = f32(betas[0]), f32(betas[1]), f32(eps), f32(max_norm)
    norm = float(g.pow(2).sum().sqrt())
    clip = min(1.0, mx / (norm + f32(1e-6))) if mx > 0 else 1.0
    gc = g * clip
    p1 = p * (1 - lr * wd)
    m1 = b1 * m + (1 - b1) * gc
    v1 = b2 * v + (1 - b2) * gc * gc
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    upd = lr / bc1 * m1 / denom
    mags = (p.abs() * (1 + lr * wd) + upd.abs(), b1 * m.abs() + (1 - b1) * gc.abs(), b2 * v + (1 - b2) * gc * gc)
    return p1 - upd, m1, v1, norm, mags


def adamw_per_element():
    lr = torch.cat([torch.full((n,), f32(a), dtype=torch.float64) for n, a, _ in ADAMW_TENSORS])
    wd = torch.cat([torch.full((n,), f32(w), dtype=torch.float64) for n, _, w in ADAMW_TENSORS])
    return lr, wd
