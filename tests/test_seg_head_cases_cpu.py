"""tests/seg_head_cases.py without a GPU: every float64 reference the GPU tests of the segmentation-head pooling, gate and depthwise
kernels gate against is checked here against an INDEPENDENT formulation of the same operation (torch's own operators in float64 and
their autograd), so a reference cannot be wrong unnoticed; and the properties the GPU cases rely on (which windows cross a border,
which pixel lanes enter the unrolled loop, where the launch rule splits, which products round once, where a second trip begins) are
asserted on the cases themselves."""
import pytest
import torch
import torch.nn.functional as F

from tests import seg_head_cases as SC
from tests.helpers import U32, bf16_rne, elem_rne

TIGHT = 1e-12
DTYPES = [torch.bfloat16, torch.float16]


def close(a, b, tol=TIGHT):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(((a - b).abs() <= tol * (1 + b.abs())).all()), float((a - b).abs().max())


def is_elem(t, dtype):
    return torch.equal(t, t.to(dtype).float())


def nchw(t):
    return t.double().permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def w_conv(w9):
    """[9][C] tap-major -> the [C, 1, 3, 3] weight of F.conv2d(groups=C)."""
    return w9.double().T.reshape(-1, 1, 3, 3)


def test_elem_rne_is_one_rounding():
    """elem_rne against torch's own conversion on values fp32 holds exactly (one rounding either way), incl. ties and fp16 subnormals."""
    g = SC.gen(1)
    v = torch.cat([torch.randn(4096, generator=g) * 3, torch.randn(512, generator=g) * 1e-6,
                   torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 0.0])])
    for dt in DTYPES:
        assert torch.equal(elem_rne(v.double(), dt), v.to(dt).double())
    assert torch.equal(elem_rne(v.double(), torch.bfloat16), bf16_rne(v.double()))


# ------------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("variant", SC.DW_VARIANTS)
@pytest.mark.parametrize("shape", SC.DW_WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv_references(shape, variant):
    """Forward vs F.conv2d(groups=C) (and F.avg_pool2d for the 1/9 weights), dgrad and wgrad vs its autograd, all in fp64; mag is the same
    operator on absolute values."""
    B, H, W, C = shape
    for dt in DTYPES:
        c = SC.dw_case(shape, dt, variant)
        assert is_elem(c["x"], dt) and is_elem(c["dy"], dt) and (c["bias"] is None) == (variant != "bias")
        assert bool((c["pre"] != 0).all())
        x = nchw(c["x"]).requires_grad_(True)
        w = w_conv(c["w9"]).requires_grad_(True)
        bias = c["bias"].double() if c["bias"] is not None else None
        y = F.conv2d(x, w, bias, stride=2, padding=1, groups=C)
        ref, mag = SC.dw_fwd64(c["x"], c["w9"], c["bias"])
        close(ref, nhwc(y.detach()))
        close(mag, nhwc(F.conv2d(nchw(c["x"]).abs(), w_conv(c["w9"]).abs(), bias.abs() if bias is not None else None, stride=2, padding=1, groups=C)))
        if variant == "avg":
            close(ref, nhwc(F.avg_pool2d(nchw(c["x"]), 3, 2, 1)), 1e-7)        # the weights are the fp32 value of 1/9
        assert tuple(y.shape[2:]) == (SC.out_size(H), SC.out_size(W))
        y.backward(nchw(c["dy"]))
        dx, dx_mag = SC.dw_dgrad64(c["dy"], c["w9"], H, W)
        close(dx, nhwc(x.grad))
        dw, dw_mag = SC.dw_wgrad64(c["dy"], c["x"])
        close(dw, w.grad.reshape(C, 9).T, 1e-11)
        xa = nchw(c["x"]).abs().requires_grad_(True)
        wa = w_conv(c["w9"]).abs().requires_grad_(True)
        F.conv2d(xa, wa, None, stride=2, padding=1, groups=C).backward(nchw(c["dy"]).abs())
        close(dx_mag, nhwc(xa.grad))
        close(dw_mag, wa.grad.reshape(C, 9).T, 1e-11)


def test_dwconv_shapes_cross_every_border_they_have():
    """Top and left padding are read by output row / column 0 of every shape; the bottom (right) padding only where H (W) is odd - with an
    even size the last window ends on the last input row, which then has ONE contributing window where an odd size gives it two rows
    of taps.  Both parities occur on both axes, so the dgrad's last row / column is checked with one and with two contributing windows.
    The reads are those of the reference itself: position indices sent through the views dw_fwd64 sums (dw_padded_reads)."""
    for B, H, W, C in SC.DW_SHAPES:
        read = SC.dw_padded_reads(H, W)                                   # [H + 2, W + 2]; rows / columns 0 and H + 1 / W + 1 are padding
        assert bool(read[0, 1:W + 1].any()) and bool(read[1:H + 1, 0].any()), "no window crosses the top / left border"
        assert bool(read[H, 1:W + 1].all()) and bool(read[1:H + 1, W].all()), "the last input row / column is not read"
        assert bool(read[1:H + 1, 1:W + 1].all()), "an input pixel no window reads"
        assert bool(read[H + 1, 1:W + 1].any()) == (H % 2 == 1), "the bottom border is crossed exactly where H is odd"
        assert bool(read[1:H + 1, W + 1].any()) == (W % 2 == 1), "the right border is crossed exactly where W is odd"
        assert bool(read[0, 0])                                            # output (0, 0) crosses two borders at once
    four = [s for s in SC.DW_SHAPES if bool(SC.dw_padded_reads(s[1], s[2])[s[1] + 1, s[2] + 1])]
    assert len(four) >= 3 and (1, 1, 1, 8) in four                       # the last output crosses bottom AND right: all four borders in one shape
    assert {H % 2 for _, H, _, _ in SC.DW_SHAPES} == {0, 1} and {W % 2 for _, _, W, _ in SC.DW_SHAPES} == {0, 1}
    assert any(C % 64 for _, _, _, C in SC.DW_SHAPES) and any(C > 256 for _, _, _, C in SC.DW_SHAPES)


def test_dwconv_wgrad_launch_rule():
    """The boundaries of the weight-gradient grid rule the cases sit on."""
    assert SC.dw_wgrad_grid((2, 32, 32, 72)) == (2, 1, 512)              # P = 512: one split; C = 72: 8 live channels in the second group
    assert SC.dw_wgrad_grid((1, 53, 37, 16)) == (1, 2, 257)              # P = 513: two splits of 257 and 256
    B, H, W, C = SC.DW_CAP_SHAPE
    P = B * SC.out_size(H) * SC.out_size(W)
    assert SC.cdiv(P, 512) * SC.cdiv(C, 64) > 1024                       # past the cap ...
    assert SC.dw_wgrad_grid(SC.DW_CAP_SHAPE) == (32, 32, 521)            # ... so 1024 / 32 splits of 521 pixels
    for s in SC.DW_SHAPES:
        assert SC.dw_wgrad_grid(s)[1] == 1
    assert C % SC.DW_CAP_SLICE == 0


def test_dwconv_cap_slice_reference():
    """One 256-channel slice of the split-cap case: its nine-shifted-products reference vs the autograd of F.conv2d on 16 of its channels."""
    c = SC.dw_cap_slice(torch.bfloat16, 3)
    assert c["x"].dtype == torch.bfloat16 and c["x"].shape == (1, 257, 257, 256) and c["dy"].shape == (1, 129, 129, 256)
    sel = slice(100, 116)
    x = nchw(c["x"][..., sel])
    w = torch.zeros(16, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=2, padding=1, groups=16).backward(nchw(c["dy"][..., sel]))
    close(c["ref"][:, sel], w.grad.reshape(16, 9).T + c["pre"][:, sel].double(), 1e-10)
    assert bool((c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all())


def test_dwconv_second_trip_arithmetic_and_row_windows():
    """Where the second trips of the capped depthwise grids begin, and that a reference computed on a window of rows equals those rows
    of the whole reference (what the GPU test does for the one large shape)."""
    B, H, W, C = SC.DW_TRIP_SHAPE
    Ho, Wo = SC.out_size(H), SC.out_size(W)
    assert (Ho, Wo) == (91, 91) and B * Ho * Wo * (C // 8) > SC.GRID_CAP_THREADS
    first = SC.first_second_trip_row(C)
    assert first == 8192 and divmod(first, Wo) == (90, 2)                # forward: output pixel (90, 2) on; rows 89 and 90 are compared
    assert divmod(first, W) == (45, 47)                                  # dgrad: input pixel (45, 47) on; rows 45, 179, 180 are compared
    assert (179 * W) // first == 3                                       # the last two input rows are fourth trips
    c = SC.dw_case((1, 13, 15, 264), torch.bfloat16)
    full, _ = SC.dw_fwd64(c["x"], c["w9"], c["bias"])
    tail, _ = SC.dw_fwd64(c["x"][:, 8:], c["w9"], c["bias"])             # input rows from the even row 2k = 8 on: outputs k + 1 .. are complete
    close(tail[:, 1:], full[:, 5:])
    dfull, _ = SC.dw_dgrad64(c["dy"], c["w9"], 13, 15)
    dwin, _ = SC.dw_dgrad64(c["dy"][:, 2:4], c["w9"], 3, 15)             # dy rows k .. k + 1 = 2, 3: input rows 2k .. 2k + 2 are complete
    close(dwin, dfull[:, 4:7])
    dtail, _ = SC.dw_dgrad64(c["dy"][:, 4:], c["w9"], 5, 15)
    close(dtail, dfull[:, 8:])


# ------------------------------------------------------------------------------------------------ global mean
def test_global_mean_cases():
    assert {P for P, C in SC.GM_CASES if C == 72} == set(SC.GM_P) and {C for P, C in SC.GM_CASES if P == 513} == set(SC.GM_C)
    for P, C in SC.GM_CASES:
        for dt in DTYPES:
            c = SC.global_mean_case(P, C, dt)
            assert is_elem(c["x"], dt)
            close(c["ref"], F.adaptive_avg_pool2d(c["x"].double().permute(0, 2, 1).reshape(SC.GM_B, C, P, 1), 1).reshape(SC.GM_B, C))
            close(c["mag"], c["x"].double().abs().mean(1))


def test_global_mean_loop_structure():
    """Which P enter the four-way unrolled loop (p + 3 * 128 < P) and how many tail steps follow.  At P = 897 pixel lane 0 makes a
    second unrolled round (512 + 384 < 897) and no tail step, while lanes 1 .. 127 make one round and all THREE tail steps; at P = 896
    lane 0 does: either way the third tail step runs."""
    steps = SC.gm_lane_steps
    for P in (1, 49, 127, 128, 129):
        assert all(steps(P, l)[0] == 0 for l in range(128))
    assert steps(1, 0) == (0, 1) and steps(1, 1) == (0, 0) and steps(128, 127) == (0, 1) and steps(129, 0) == (0, 2)
    assert steps(511, 0) == (1, 0) and steps(511, 126) == (1, 0) and steps(511, 127) == (0, 3)
    assert steps(512, 0) == (1, 0) and steps(512, 127) == (1, 0)
    assert steps(513, 0) == (1, 1) and steps(513, 1) == (1, 0)
    assert steps(896, 0) == (1, 3) and steps(896, 127) == (1, 3)
    assert steps(897, 0) == (2, 0) and all(steps(897, l) == (1, 3) for l in range(1, 128))
    assert steps(1600, 0) == (3, 1) and steps(1600, 63) == (3, 1) and steps(1600, 64) == (3, 0)
    for P in SC.GM_P:                                                     # every pixel is read exactly once
        assert sum(4 * r + t for r, t in (steps(P, l) for l in range(128))) == P
    assert any(C % 64 for _, C in SC.GM_CASES) and any(C > 64 and C % 64 == 8 for _, C in SC.GM_CASES)      # a partial 64-channel group


# ------------------------------------------------------------------------------------------------ pooled linear
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("act", SC.PL_ACTS)
def test_pooled_linear_references(act, with_bias):
    assert {N for N, C in SC.PL_CASES if C == 65} == set(SC.PL_N) and {C for N, C in SC.PL_CASES if N == 19} == set(SC.PL_C)
    fn = {0: lambda t: t, 1: F.relu, 4: torch.sigmoid}[act]
    for N, C in SC.PL_CASES:
        c = SC.pooled_linear_case(N, C, act, with_bias)
        bias = c["bias"].double() if with_bias else None
        assert (c["bias"] is None) == (not with_bias) and c["in"].dtype == c["W"].dtype == torch.float32
        close(c["s"], F.linear(c["in"].double(), c["W"].double(), bias))
        close(c["ref"], fn(F.linear(c["in"].double(), c["W"].double(), bias)))
        close(c["mag"], F.linear(c["in"].double().abs(), c["W"].double().abs(), bias.abs() if with_bias else None))
        if act == 4:
            assert bool(torch.isfinite(c["ref"]).all()) and bool((c["sig_mag"] >= c["ref"]).all()) and bool((c["sig_mag"] <= c["ref"] * 100).all())
        if act == 4 and with_bias:
            rows = SC.pl_planted_rows(N)
            assert rows[0] == 0 and (N == 1 or rows[1] == N - 1)         # the last row lies in the last, possibly partial, block of 16
            if N >= 4:
                assert len(rows) == 4
            for n, target in zip(rows, SC.PL_PLANTED):
                assert abs(float(c["s"][0, n]) - target) <= 1e-5, (N, C, n)
                want = 1.0 if target > 0 else 0.0
                assert abs(float(c["ref"][0, n]) - want) < 1e-12


def test_pooled_linear_block_boundaries():
    """N = 15, 17, 19, 150 end inside a block of 16 output rows (the n_end clamp), 16 on its edge; C = 63, 65, 1000 are no multiple of the
    64 lanes, C = 1 leaves 63 lanes idle."""
    assert [N % 16 for N in SC.PL_N] == [1, 15, 0, 1, 3, 6] and [C % 64 for C in SC.PL_C] == [1, 63, 0, 1, 40]


# ------------------------------------------------------------------------------------------------ channel gate, row dot
def test_channel_gate_references():
    assert len(set(SC.CG_COMBOS)) == 8
    for dt in DTYPES:
        c = SC.channel_gate_case(SC.CG_SHAPE, dt)
        assert is_elem(c["x"], dt) and is_elem(c["add_map"], dt)
        x, g, v, m = c["x"].double(), c["gate"].double(), c["add_vec"].double(), c["add_map"].double()
        for sa, uv, um in SC.CG_COMBOS:
            ref, mag = SC.channel_gate_ref(c, sa, uv, um)
            want = torch.einsum("bpc,bc->bpc", x, g + (1.0 if sa else 0.0))
            want = want + (v.unsqueeze(1).expand_as(x) if uv else 0.0) + (m if um else 0.0)
            close(ref, want)
            assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
            tail, _ = SC.channel_gate_ref(c, sa, uv, um, first_row=70)
            close(tail, want[:, 70:])


def test_grid_cap_arithmetic():
    B, P, C = SC.CAP_SHAPE
    assert B * P * (C // 8) == 2099200 > SC.GRID_CAP_THREADS == 2097152
    assert SC.first_second_trip_row(C) == 8192 < P                       # rows 8192 .. 8199 are second trips
    for (src, dst), n in ((SC.UP_ADD_TRIP, 1), (SC.UP_BWD_TRIP, 0)):
        size = (dst, src)[1 - n]
        assert size[0] * size[1] * (SC.UP_TRIP_C // 8) > SC.GRID_CAP_THREADS and SC.first_second_trip_row(SC.UP_TRIP_C) < size[0] * size[1]


def test_rowdot_references():
    for shape in SC.RD_SHAPES:
        B, P, C = shape
        assert P + 3 <= 1024 and len(set(SC.rd_splits(P))) == 4
        for dt in DTYPES:
            c = SC.rowdot_case(shape, dt)
            assert is_elem(c["a"], dt) and is_elem(c["b"], dt) and bool((c["pre"] != 0).all())
            for second in (True, False):
                want = 0.5 * (torch.einsum("bpc,bpc->bc", c["a"].double(), c["b"].double()) if second else c["a"].double().transpose(1, 2).sum(-1))
                ref, mag = SC.rowdot_ref(c, second, 1)
                close(ref, want, 1e-11)
                ref5, mag5 = SC.rowdot_ref(c, second, 5)
                close(ref5, want + c["pre"].double(), 1e-11)
                close(mag5, mag + c["pre"].double().abs())
    assert SC.cdiv(5, 8) == 1 and 8 > 5                                  # splits = P + 3 = 8 at P = 5: ranges 5, 6, 7 are empty


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape", SC.BC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bcast_reference_is_one_rounding(shape):
    """The kernel rounds twice (fp64 product -> fp32 -> element); for the seeded values that equals the single rounding of the fp64
    product, so bit equality with `ref` is the right demand."""
    for dt in DTYPES:
        c = SC.bcast_case(shape, dt)
        assert c["scale"] == float(torch.tensor(1.0 / shape[1], dtype=torch.float32))
        assert int((c["vec"] == 1.0).sum()) <= 4                          # the replaced values: a handful
        p32 = c["vec"] * torch.tensor(c["scale"], dtype=torch.float32)    # torch's fp32 multiplication
        assert torch.equal(p32.double(), c["prod"].float().double())      # = the fp32 rounding of the fp64 product
        assert torch.equal(p32.to(dt).double(), c["ref"]), "a product of this case rounds differently through fp32"


def test_planes_to_rows_references():
    assert max(Qp for _, Qp in SC.PR_QQP) * 65 * 4 == 62400
    for Q, Qp in SC.PR_QQP:
        assert Qp % 8 == 0 and Q <= Qp <= 240
        for P in SC.PR_P:
            for dt in DTYPES:
                c = SC.planes_case(Q, Qp, P, dt)
                want = torch.zeros(SC.PR_B, P, Qp, dtype=dt)
                want[:, :, :Q] = c["planes"].transpose(1, 2).to(dt)
                assert torch.equal(c["ref"], want.double())
                assert bool((c["ref"][:, :, Q:] == 0).all())


# ------------------------------------------------------------------------------------------------ nearest upsample
ALL_UP = SC.UP_PAIRS + [SC.UP_ADD_TRIP, SC.UP_BWD_TRIP]


@pytest.mark.parametrize("pair", ALL_UP, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_nearest_index_is_atens_and_preimages_lie_in_the_searched_window(pair):
    (Hs, Ws), (H, W) = pair
    for in_size, out in ((Hs, H), (Ws, W)):
        idx = SC.nearest_index(in_size, out)
        src = torch.arange(in_size, dtype=torch.float64).reshape(1, 1, in_size, 1)
        for dt in (torch.float64, torch.float32):
            assert torch.equal(F.interpolate(src.to(dt), size=(out, 1), mode="nearest").reshape(-1).long(), idx)
        assert bool((idx[1:] >= idx[:-1]).all())
        for s in range(in_size):
            lo, hi = SC.up_candidates(s, in_size, out)
            pre = (idx == s).nonzero().flatten()
            assert pre.numel() == 0 or (lo <= int(pre[0]) and int(pre[-1]) <= hi), (in_size, out, s)
    assert 1 <= SC.up_max_preimage(pair) <= 8


def test_upsample_longest_chains():
    assert [SC.up_max_preimage(p) for p in SC.UP_PAIRS] == [1, 4, 4, 4, 6, 8] and SC.up_max_preimage(SC.UP_BWD_TRIP) == 4


def test_nearest_index_float_rule_differs_from_integer_floor():
    """14 -> 46 and 26 -> 44 hold an output index whose fp32 source index is one below the integer floor; 14 -> 20 holds none."""
    assert int(SC.nearest_index(14, 46)[23]) == 6 and (23 * 14) // 46 == 7
    assert int(SC.nearest_index(26, 44)[22]) == 12 and (22 * 26) // 44 == 13
    assert SC.nearest_index(14, 20).tolist() == [(d * 14) // 20 for d in range(20)]
    assert ((14, 26), (46, 44)) in SC.UP_PAIRS and ((14, 14), (20, 20)) in SC.UP_PAIRS


@pytest.mark.parametrize("pair", SC.UP_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_upsample_references(pair):
    (Hs, Ws), (H, W) = pair
    for dt in DTYPES:
        c = SC.upsample_case(pair, dt)
        assert all(is_elem(c[k], dt) for k in ("lat", "top", "dy"))
        top = nchw(c["top"]).requires_grad_(True)
        up = F.interpolate(top, size=(H, W), mode="nearest")
        ref, mag = SC.upsample_add_ref(c)
        close(ref, c["lat"].double() + nhwc(up.detach()))
        close(mag, c["lat"].double().abs() + nhwc(F.interpolate(nchw(c["top"]).abs(), size=(H, W), mode="nearest")))
        s = ref.float().double()                                          # one fp32 addition: within 2^-24 |ref| of the fp64 sum
        assert bool(((s - ref).abs() <= U32 * ref.abs()).all())
        up.backward(nchw(c["dy"]))
        bref, bmag = SC.upsample_bwd_ref(c)
        close(bref, nhwc(top.grad))
        assert bool((bmag >= bref.abs() * (1 - 1e-12)).all())
        lhs = (SC.up64(c["top"], (H, W)) * c["dy"].double()).sum()       # <up(t), dy> == <t, bwd(dy)>
        rhs = (c["top"].double() * bref).sum()
        assert abs(float(lhs - rhs)) <= 1e-10 * float((c["top"].double().abs() * bmag).sum())
