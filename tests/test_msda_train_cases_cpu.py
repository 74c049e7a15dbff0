"""tests/msda_train_cases.py without a GPU: the float64 references the GPU tests of the deformable-attention training kernels, their
prelude and the fused AdamW step gate against are checked here against INDEPENDENT formulations (the oracle's restatement of the
reference function under float64 autograd, the reference's golden output, torch's softmax / AdamW / clip_grad_norm_ in float64), and
every structural property the GPU cases rely on is asserted on the cases themselves: the distance of the random points from the grid
lines and the agreement of the fp32 floor with the float64 one, the exact dyadic coordinates of the planted points, the tap counts of the
crowded pixels, slab counts and rows per slab, points that straddle a slab boundary, the exactness of the exact runs in fp32 and in both
16-bit types, the chunk table of the optimiser."""
import numpy as np
import pytest
import torch

from oracle import detr_oracle as O
from tests import msda_train_cases as MC
from tests._cases import MSDA_SHAPES, msda_case_inputs
from tests.helpers import elem_rne, load_golden

DTYPES = [torch.bfloat16, torch.float16]
TIGHT = 1e-11


def close(a, b, tol=TIGHT):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(((a - b).abs() <= tol * (1 + b.abs())).all()), float((a - b).abs().max())


def oracle_grads(c):
    B, S = c["B"], c["S"]
    v = c["value"].double().view(B, S, MC.M, MC.D).requires_grad_()
    lc, aw = c["loc"].double().requires_grad_(), c["attn"].double().requires_grad_()
    out = O.ms_deform_attn_core(v, c["shapes"], lc, aw)
    out.backward(c["go"].double())
    return out.detach(), v.grad.reshape(B, S, MC.CH), lc.grad, aw.grad


@pytest.mark.parametrize("name", ["l1p1", "l3p3", "l8p4", "prod", "edges", "exact", "exact3", "crowd", "qmax_go32"])
def test_core_reference_vs_oracle_autograd(name):
    """out, grad_value, grad_loc, grad_attn of the written-out reference = float64 autograd through F.grid_sample (oracle.detr_oracle),
    also on pixel centres and grid lines (both take the floor's side of the jump) and outside the map."""
    c, r = MC.core_case(name), MC.core_ref(name)
    out, gv, gl, ga = oracle_grads(c)
    close(r["out"], out)
    close(r["grad_value"], gv)
    close(r["grad_loc"], gl, 1e-10)
    close(r["grad_attn"], ga)
    for k in ("out", "grad_value", "grad_loc", "grad_attn"):
        assert bool((r[k + "_mag"] >= r[k].abs() * (1 - 1e-12)).all()), k


def test_core_reference_vs_golden():
    value, loc, w = (torch.from_numpy(a) for a in msda_case_inputs())
    gold = torch.from_numpy(load_golden("msda_core.npz")["out"]).double()
    B, S = value.shape[:2]
    r = MC.core_ref_tensors(value.reshape(B, S, MC.CH), MSDA_SHAPES, loc, w, torch.zeros(B, loc.shape[1], MC.CH))
    assert float((r["out"] - gold).abs().max()) <= 2e-6 * float(gold.abs().max())          # the golden file holds an fp32 result


@pytest.mark.parametrize("name", list(MC.CORE_CASES))
def test_points_keep_clear_of_the_grid_lines_and_floor_alike(name):
    """Every point of every case: the fp32 evaluation of the kernels' coordinate formula floors to the pixel float64 floors to.  Random
    cases: the float64 coordinate is at least 2^-10 from every grid line.  Points with a pixel inside the map lie within |loc| <= 1.25
    (the bound behind POS).  Values and gradients are the same numbers in both 16-bit types."""
    c = MC.core_case(name)
    p64, p32 = MC.pix64(c["loc"], c["shapes"]), MC.pix32(c["loc"], c["shapes"])
    assert torch.equal(torch.floor(p64), torch.floor(p32.double()))
    if c["random"]:
        assert float((p64 - torch.round(p64)).abs().min()) >= MC.GRID_DIST
    inside = MC.has_inside_tap(c["loc"], c["shapes"])
    assert float(c["loc"].abs().amax(-1)[inside].max()) <= MC.LOC_BOUND
    for dt in DTYPES:
        assert torch.equal(c["value"], c["value"].to(dt).float()) and torch.equal(c["go"], c["go"].to(dt).float())
    assert c["S"] == sum(h * w for h, w in c["shapes"]) and len(MC.CORE_CASES[name][1]) > 0


def test_geometry_of_the_case_list():
    cs = {n: MC.core_case(n) for n in MC.CORE_CASES}
    assert {cs[n]["B"] * cs[n]["Q"] for n in ("l1p1", "l3p3", "l8p4")} == {1, 15, 67}
    assert {cs[n]["L"] for n in ("l1p1", "l3p3", "l8p4")} == {1, 3, MC.MS_MAXL} and {cs[n]["P"] for n in ("l1p1", "l3p3", "l8p4")} == {1, 3, 4}
    shapes = [tuple(s) for n in cs for s in cs[n]["shapes"]]
    for want in ((1, 1), (1, 9), (7, 1), (2, 2), (3, 400), (100, 33), (2, 3200), (80, 80), (40, 40), (20, 20)):
        assert want in shapes, want
    assert cs["prod"]["shapes"] == MC.PRODUCTION and cs["l8p4"]["shapes"][:5] == [[16, 16], [8, 8], [4, 4], [2, 2], [1, 1]]
    assert cs["l8p4"]["Q"] * 8 > 512 and cs["crowd"]["Q"] * 8 > 512                      # more than one staging pass of the grad_out rows
    # slabs: 80 x 80 two of 40 rows; 100 x 33 one of 96 and a short one of 4; 2 x 3200 one row per slab
    assert MC.slab_rows(80, 80) == (40, 2, 40) and MC.slab_rows(100, 33) == (96, 2, 4) and MC.slab_rows(2, 3200) == (1, 2, 1)
    assert MC.slab_rows(16, 16) == (16, 1, 16) and MC.slab_rows(3, 400) == (3, 1, 3)


def _y0_in_map(c, level, q, H, W):
    p = MC.pix64(c["loc"], c["shapes"])[:, q, :, level, 0]
    x0, y0 = torch.floor(p[..., 0]), torch.floor(p[..., 1])
    return y0[(x0 >= 0) & (x0 < W - 1)]


def test_points_straddle_the_slab_boundaries():
    """prod: y0 = 39 / 40 on 80 x 80.  slabs: y0 = 95 / 96 on 100 x 33 and 0 / 1 on 2 x 3200, each with both columns inside the map."""
    for name, level, H, W, row in (("prod", 0, 80, 80, 39), ("slabs", 0, 100, 33, 95), ("slabs", 1, 2, 3200, 0)):
        c = MC.core_case(name)
        rows, _, _ = MC.slab_rows(H, W)
        assert (row + 1) % rows == 0
        y0 = torch.cat([_y0_in_map(c, level, q, H, W) for q in range(2)])
        assert y0.numel() > 0 and bool((y0 == row).all()), (name, level)
    r = MC.core_ref("slabs")
    assert float((r["counts"] == 0).double().mean()) > 0.5                              # most pixels get no tap at all


def test_edges_case_positions():
    """The planted points of `edges`: tx, ty exactly 0 on the centres, exactly 1/2 on the grid lines, in fp32 as in float64; every
    corner / edge point has pixels on both sides of the border; the outside points have none inside."""
    c = MC.core_case("edges")
    p64, p32 = MC.pix64(c["loc"], c["shapes"])[0, :, 0, 0, 0], MC.pix32(c["loc"], c["shapes"])[0, :, 0, 0, 0].double()
    assert torch.equal(p64, p32)                                                        # a 4 x 4 level: every step is exact here even for 0.4 * 4
    for q, (x, y) in MC.EDGE_CENTRES.items():
        assert p32[q].tolist() == [float(x), float(y)]
    for q, xy in MC.EDGE_LINES.items():
        assert p32[q].tolist() == list(xy)
    inside = MC.has_inside_tap(c["loc"], c["shapes"])[0, :, 0, 0, 0]
    assert inside[:8].all() and not inside[8:14].any() and inside[14:].all()
    n_in = MC.core_ref("edges")["counts"].sum().item() // MC.M
    x0, y0 = torch.floor(p64[:, 0]), torch.floor(p64[:, 1])
    taps = sum(int(0 <= x0[q] + dx < 4 and 0 <= y0[q] + dy < 4) for q in range(c["Q"]) for dx in (0, 1) for dy in (0, 1))
    assert n_in == taps and [int(0 <= x0[q] + dx < 4 and 0 <= y0[q] + dy < 4) for q in range(4) for dx in (0, 1) for dy in (0, 1)].count(1) == 4
    assert c["loc"][0, :4, 0, 0, 0].flatten().tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("name", MC.EXACT_CASES)
def test_exact_runs_are_exact(name):
    """tx, ty in {0, 1/4, 1/2, 3/4} in fp32; every output of the float64 reference is an fp32 number (so is every partial sum: all terms
    are multiples of 2^-9 and the sum of their absolute values stays below 2^12); the value gradient is a number of both 16-bit types."""
    c, r = MC.core_case(name), MC.core_ref(name)
    p32 = MC.pix32(c["loc"], c["shapes"]).double()
    assert torch.equal(p32, MC.pix64(c["loc"], c["shapes"]))
    t = p32 - torch.floor(p32)
    assert bool(((t * 4) == torch.round(t * 4)).all())
    lg = torch.log2(c["attn"].double())
    assert torch.equal(lg, torch.round(lg)) and torch.equal(c["value"], torch.round(c["value"])) and torch.equal(c["go"], torch.round(c["go"]))
    assert set(c["go"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    for k in ("out", "grad_value", "grad_loc", "grad_attn"):
        assert torch.equal(r[k], r[k].float().double()), k
        assert torch.equal(r[k] * 512, torch.round(r[k] * 512)), k
    # sum of |terms| WITHOUT the position term: mag with POS = 0 is bounded by mag itself / the exact sum of absolute values
    B, S = c["B"], c["S"]
    absr = MC.core_ref_tensors(c["value"].abs(), c["shapes"], c["loc"], c["attn"], c["go"].abs())
    assert float(absr["out"].max()) < 2 ** 12 and float(absr["grad_value"].max()) < 2 ** 12 and float(absr["grad_attn"].max()) < 2 ** 12
    assert float(absr["grad_loc_mag"].max()) < 2 ** 20                                  # multiples of 1/4 times aw * W: far below 2^24 ulps
    for dt in DTYPES:
        assert torch.equal(elem_rne(r["grad_value"], dt), r["grad_value"]), dt


def test_crowd_counts():
    """The reference tap counter on the crowd case: every head and batch has pixels with exactly 95, 96, 97, 111, 112, 113, 128 and 129
    entries (four of each), seven of the eight counts are set aside (>= MS_HOT) in the single slab, pixel (13, 13) carries the other 15
    points, and 220 of the 256 pixels carry nothing."""
    c, r = MC.core_case("crowd"), MC.core_ref("crowd")
    n = MC.CROWD_SIDE
    assert MC.slab_rows(n, n)[1] == 1 and sum(MC.CROWD_COUNTS) + 15 == c["Q"] * c["P"]
    for b in range(c["B"]):
        for h in range(MC.M):
            cnt = r["counts"][b, h].view(n, n)
            for (x, y), k in MC.crowd_targets(h).items():
                assert [int(cnt[y + dy, x + dx]) for dy in (0, 1) for dx in (0, 1)] == [k] * 4
            vals = sorted(cnt[cnt > 0].tolist())
            assert vals == sorted([15] * 4 + [k for k in MC.CROWD_COUNTS for _ in range(4)])
            assert int((cnt >= MC.MS_HOT).sum()) == 28 and int((cnt == 0).sum()) == 220
    assert len({tuple(sorted(MC.crowd_targets(h).items())) for h in range(MC.M)}) == MC.M


def test_slab_formula_and_q_max():
    """The restated LDS formula: entries and grad_out rows start on 16 bytes, Q_max sits on the 160 KiB edge for either grad_out type."""
    for go16 in (True, False):
        q = MC.q_max(4, go16)
        assert MC.slab_smem(4, q, go16) <= MC.LDS_BYTES < MC.slab_smem(4, q + 1, go16)
        assert MC.slab_supported([[4, 4], [2, 2]], 4, q, 8, go16) and not MC.slab_supported([[4, 4], [2, 2]], 4, q + 1, 8, go16)
        assert MC.core_case("qmax_go16" if go16 else "qmax_go32")["Q"] == q
    assert MC.q_max(4, True) > MC.q_max(4, False) > 512
    assert not MC.slab_supported([[1, 1]] * 9, 4, 8, 8, True) and not MC.slab_supported([[1, 3201]], 4, 8, 8, True) and not MC.slab_supported([[1, 1]], 4, 8, 4, True)
    for Q in (1, 23, 24, 300, 577):
        fixed = 3200 + 8 + 2 + 512
        assert (MC.slab_smem(4, Q, False) - Q * 16 * 8 - Q * 128) % 16 == 0 and MC.slab_smem(4, Q, False) - Q * 16 * 8 - Q * 128 >= (fixed + Q * 16 // 96 + 2) * 4


def test_half_step_bounds_one_rounding():
    x = torch.cat([torch.randn(4096, generator=MC.gen(5)).double() * 3, torch.tensor([0.0, 1.0, 2.0 ** -20, 255.0, 257.0, 1e-7])])
    for dt in DTYPES:
        d = (elem_rne(x, dt) - x).abs()
        assert bool((d <= MC.half_step(x, dt)).all()) and float((d / MC.half_step(x, dt)).max()) > 0.9


# ------------------------------------------------------------------------------------------------ prelude
@pytest.mark.parametrize("shape", MC.PREP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prelude_reference_vs_torch_autograd(shape):
    c = MC.prep_case(shape)
    BQ, Mh, L, P = shape
    LP = L * P
    assert BQ * Mh in (8, 264) and Mh in (1, 8) and (L, P) in ((1, 1), (3, 4), (8, 3))
    for dt in DTYPES:
        assert torch.equal(c["off"], c["off"].to(dt).float()) and torch.equal(c["logit"], c["logit"].to(dt).float())
    off, lg = c["off"].double().requires_grad_(), c["logit"].double().requires_grad_()
    ref = c["ref"].double()
    aw = torch.softmax(lg.view(BQ, Mh, LP), -1)
    loc = ref[:, None, None, :2] + off.view(BQ, Mh, LP, 2) / P * ref[:, None, None, 2:] * 0.5
    (l_ref, l_mag), (a_ref, a_mag) = MC.prep_fwd_ref(c)
    close(l_ref, loc.detach())
    close(a_ref, aw.detach())
    assert bool((l_mag >= l_ref.abs() * (1 - 1e-12)).all()) and bool((a_mag >= a_ref).all())
    # the backward case has its own aw (an fp32 softmax: its rows sum to 1 within 1e-7): differentiate softmax at logits that produce it
    lg2 = torch.log(c["aw"].double()).requires_grad_()
    aw2 = torch.softmax(lg2, -1)
    close(aw2.detach(), c["aw"].double(), 1e-6)
    (aw2 * c["grad_attn"].double()).sum().backward()
    (loc * c["grad_loc"].double()).sum().backward()
    (go_ref, go_mag), (gg_ref, gg_mag) = MC.prep_bwd_ref(c)
    close(gg_ref, lg2.grad.reshape(BQ, -1), 1e-6)
    close(go_ref, off.grad)
    assert bool((gg_mag >= gg_ref.abs() * (1 - 1e-12)).all()) and bool((go_mag >= go_ref.abs()).all())
    if BQ >= 3:
        assert float(c["logit"][MC.PREP_EQUAL_ROW].std()) == 0 and float(c["logit"][MC.PREP_SPREAD_ROW].max() - c["logit"][MC.PREP_SPREAD_ROW].min()) == 160
        assert float(a_ref[MC.PREP_SPREAD_ROW].min()) < 2.0 ** -149                    # below the smallest fp32 subnormal: exp underflows
        assert bool((c["ref"][MC.PREP_ZERO_WH_ROW, 2:] == 0).all()) and bool((l_ref[MC.PREP_ZERO_WH_ROW] == ref[MC.PREP_ZERO_WH_ROW, None, None, :2]).all())
        close(a_ref[MC.PREP_EQUAL_ROW], torch.full_like(a_ref[MC.PREP_EQUAL_ROW], 1.0 / LP))


# ------------------------------------------------------------------------------------------------ AdamW
def test_adamw_chunk_table():
    cs, cl, clr, cwd = MC.adamw_chunks()
    sizes = [t[0] for t in MC.ADAMW_TENSORS]
    assert sizes == [1, 255, 256, 257, 65535, 65536, 65537] and MC.ADAMW_CHUNK == 65536
    assert cl == [1, 255, 256, 257, 65535, 65536, 65536, 1] and cs == [0, 1, 256, 512, 769, 66304, 131840, 197376] and sum(cl) == sum(sizes)
    assert clr[2] == 0.0 and cwd[3] == 0.0 and len(clr) == len(cwd) == 8
    assert {r[0] for r in MC.ADAMW_RUNS} == {0.0, 0.1} and {r[2] for r in MC.ADAMW_RUNS} == {1, 2, 10000}
    assert any(r[0] == 0.1 and r[1] < 0.1 for r in MC.ADAMW_RUNS) and any(r[0] == 0.1 and r[1] > 0.1 for r in MC.ADAMW_RUNS)


@pytest.mark.parametrize("run", range(len(MC.ADAMW_RUNS)))
def test_adamw_reference_vs_torch(run):
    """adamw_ref = clip_grad_norm_ + torch.optim.AdamW in float64, one step from given (p, g, m, v, step), with the fp32-rounded
    hyper-parameters the entry point receives."""
    c = MC.adamw_case(run)
    lr, wd = MC.adamw_per_element()
    p1, m1, v1, norm, mags = MC.adamw_ref(c["p"], c["g"], c["m"], c["v"], c["step"], lr, wd, c["max_norm"])
    assert abs(norm - MC.ADAMW_RUNS[run][1]) <= 1e-6 * norm
    params, o = [], 0
    for n, _, _ in MC.ADAMW_TENSORS:
        params.append(torch.nn.Parameter(c["p"][o:o + n].double().clone()))
        params[-1].grad = c["g"][o:o + n].double().clone()
        o += n
    b1, b2 = MC.f32(MC.ADAMW_BETAS[0]), MC.f32(MC.ADAMW_BETAS[1])
    opt = torch.optim.AdamW([{"params": [p], "lr": MC.f32(t[1]), "weight_decay": MC.f32(t[2])} for p, t in zip(params, MC.ADAMW_TENSORS)], betas=(b1, b2),
                            eps=MC.f32(MC.ADAMW_EPS))
    o = 0
    for p, (n, _, _) in zip(params, MC.ADAMW_TENSORS):
        opt.state[p] = {"step": torch.tensor(float(c["step"] - 1)), "exp_avg": c["m"][o:o + n].double().clone(), "exp_avg_sq": c["v"][o:o + n].double().clone()}
        o += n
    if c["max_norm"] > 0:
        total = torch.nn.utils.clip_grad_norm_(params, MC.f32(c["max_norm"]))
        assert abs(float(total) - norm) <= 1e-12 * norm
    opt.step()
    close(p1, torch.cat([p.detach() for p in params]), 1e-10)
    close(m1, torch.cat([opt.state[p]["exp_avg"] for p in params]), 1e-10)
    close(v1, torch.cat([opt.state[p]["exp_avg_sq"] for p in params]), 1e-10)
    lr0 = slice(256, 512)
    assert torch.equal(p1[lr0], c["p"][lr0].double()) and not torch.equal(m1[lr0], c["m"][lr0].double())          # lr = 0: parameters unchanged, moments updated
    assert bool((mags[0] >= p1.abs() * (1 - 1e-12)).all()) and bool((mags[1] >= m1.abs() * (1 - 1e-12)).all()) and bool((mags[2] >= v1 * (1 - 1e-12)).all())
    assert np.isfinite(norm)
