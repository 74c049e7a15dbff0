"""tests/train_norm_cases.py without a GPU: every float64 reference the GPU tests of the BatchNorm, pooling-backward, weight-packing and
gradient-unpacking kernels gate against is checked here against an INDEPENDENT formulation of the same operation (torch's own operators
in float64 and their autograd), so a reference cannot be wrong unnoticed; and the properties the GPU cases rely on (which lane layout a
shape selects, how many row blocks feed the atomics, the ties and the fast / mixed path content of the max-pool inputs, the share of
ReLU elements left out, where a second trip begins, the chunk and tile counts of the pack table) are asserted on the cases themselves."""
import pytest
import torch
import torch.nn.functional as F

from tests import train_norm_cases as NC
from tests.helpers import act64, elem_rne, frag_order

TIGHT = 1e-11
DTYPES = [torch.bfloat16, torch.float16]
ACT_FN = {"none": lambda a: a, "relu": F.relu, "silu": F.silu, "gelu": F.gelu}


def close(a, b, tol=TIGHT):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(((a - b).abs() <= tol * (1 + b.abs())).all()), float((a - b).abs().max())


def is_elem(t, dtype):
    return torch.equal(t, t.to(dtype).float())


def sid(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------------------ BatchNorm
def test_bn_shapes_reach_every_layout_and_edge():
    """What each (rows, C) is in the list for."""
    lay = {s: NC.bn_layout(s[1]) for s in NC.BN_SHAPES}
    blocks = {s: NC.bn_row_blocks(*s) for s in NC.BN_SHAPES}
    assert lay[(1, 8)] == [(8, 32, 8)] and lay[(7, 24)] == [(24, 32, 8)]                  # 32 x 8 lanes, most without a channel; 7 rows < 8 row lanes
    assert lay[(255, 32)] == [(32, 4, 64)] and 255 % 64 != 0 and 255 // 64 == 3           # 4 x 64: row lane 63 has one row fewer
    assert lay[(1024, 64)] == [(64, 8, 32)] and blocks[(1024, 64)] == 1                   # rows == BN_ROWS: exactly one row block
    assert blocks[(1025, 64)] == 2 and 1025 - 1024 == 1                                   # the second row block holds one row
    assert lay[(2049, 128)] == [(128, 16, 16)] and blocks[(2049, 128)] == 3
    assert NC.bn_rows_per_block(255) == 1024 and NC.bn_rows_per_block(256) == 256         # BN_ROWS changes at C = 256
    assert lay[(256, 256)] == [(256, 32, 8)] and blocks[(256, 256)] == 1                  # rows == BN_ROWS at the wide setting
    assert lay[(257, 264)] == [(264, 32, 8), (8, 32, 8)] and blocks[(257, 264)] == 2      # second column block: 8 channels; rows == BN_ROWS + 1
    assert lay[(300, 288)][1] == (32, 4, 64)                                              # second column block in the 32-channel form
    assert lay[(513, 320)][1] == (64, 8, 32) and blocks[(513, 320)] == 3                  # the 64-channel form
    assert lay[(300, 384)][1] == (128, 16, 16)                                            # the 128-channel form
    assert lay[(600, 520)] == [(520, 32, 8), (264, 32, 8), (8, 32, 8)]
    # a row block with no row for some lanes: 300 - 256 = 44 rows for the 64 row lanes of the 32-channel form
    assert 300 - 256 < lay[(300, 288)][1][2]
    rows, C = NC.BN_CAP_SHAPE
    assert rows * C // 8 > NC.GRID_CAP_THREADS and NC.first_second_trip_row(C) == 8192 < rows


def bn_autograd(c, act, residual, gamma_like=False):
    """act(F.batch_norm(z, training=True) [+ res]) in fp64 with the batch's own statistics; returns y, dz, dgamma, dbeta and the statistics."""
    z = c["z"].double().requires_grad_(True)
    C = z.shape[1]
    gamma, beta = (1 + 0.1 * torch.arange(C).double()).requires_grad_(True), (0.05 * torch.arange(C).double() - 0.3).requires_grad_(True)
    y = F.batch_norm(z, None, None, gamma, beta, True, 0.1, NC.FIN_EPS)
    if residual:
        y = y + c["res"].double()
    y = ACT_FN[act](y)
    y.backward(c["dy"].double())
    return y.detach(), z.grad, gamma.grad, beta.grad, gamma.detach(), beta.detach()


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", NC.ACTS)
@pytest.mark.parametrize("shape", [(7, 24), (255, 32), (257, 264)], ids=sid)
def test_bn_references_against_autograd(shape, act, residual):
    """The four isolated references, CHAINED here with the statistics of the batch itself, reproduce fp64 autograd of
    act(F.batch_norm(z, training=True) [+ res]): forward output, dz, dgamma, dbeta."""
    c = NC.bn_case(shape, torch.bfloat16, "gauss", True)
    rows, C = shape
    y, dz, dgamma, dbeta, gamma, beta = bn_autograd(c, act, residual)
    c["pre"] = torch.zeros(2, C, dtype=torch.float64)
    s, _ = NC.bn_stats_ref(c)
    mean = s[0] / rows
    var = s[1] / rows - mean * mean
    close(var, c["z"].double().var(0, unbiased=False), 1e-9)
    rstd = 1 / torch.sqrt(var + NC.FIN_EPS)
    c.update(mean=mean, rstd=rstd, scale=gamma * rstd, shift=beta - mean * gamma * rstd, inv_n=1.0 / rows)
    close(NC.bn_apply_ref(c, act, residual)[0], y, 1e-9)
    b, bmag, extra = NC.bn_bwd_stats_ref(c, act, residual)
    close(b[0], dbeta, 1e-9)
    close(b[1], dgamma, 1e-8)
    assert bool((bmag >= b.abs() - 1e-9).all()) and bool((extra == 0).all())
    c["sums"] = b
    da, damag, dz_ref, dzmag, ex = NC.bn_bwd_apply_ref(c, act, residual)
    close(dz_ref, dz, 1e-8)
    assert bool((damag >= da.abs()).all()) and bool((dzmag >= dz_ref.abs() - 1e-12).all()) and not bool(ex.any())


@pytest.mark.parametrize("act", NC.ACTS)
def test_act_grad_is_the_derivative(act):
    a = torch.linspace(-6, 6, 4001, dtype=torch.float64)
    a = a[a != 0].clone().requires_grad_(True)
    act64(a, act).sum().backward()
    close(NC.act_grad64(a.detach(), act), a.grad)


@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=sid)
def test_bn_cases_are_what_they_claim(shape):
    """Elements are elements, the integer run is exact in fp32 in any order, mags dominate, and the ReLU exclusion is empty for the small
    cases and at most 0.1 % of any case."""
    rows, C = shape
    for dt in DTYPES:
        for z_f32 in (False, True):
            c = NC.bn_case(shape, dt, "int", z_f32)
            for k in ("z", "dy", "res", "pre"):
                assert torch.equal(c[k], c[k].round()) and is_elem(c[k], dt)
            for k in ("scale", "shift", "mean", "rstd"):
                assert bool((torch.frexp(c[k].abs()).mantissa == 0.5).all())                # powers of two
            for act in ("none", "relu"):
                for residual in (False, True):
                    ref, mag, extra = NC.bn_bwd_stats_ref(c, act, residual)
                    assert bool((extra == 0).all()) or act == "relu"
                    assert torch.equal(ref * 8, (ref * 8).round()) and float(mag.max()) * 8 < 2.0 ** 24       # every partial sum: a multiple of 1/8 below 2^21
                    assert torch.equal(ref.float().double(), ref)
            ref, mag = NC.bn_stats_ref(c)
            assert torch.equal(ref, ref.round()) and float(mag.max()) < 2.0 ** 24
            for kind in NC.BN_KINDS:
                c = NC.bn_case(shape, dt, kind, z_f32)
                assert is_elem(c["dy"], dt) and is_elem(c["res"], dt) and (z_f32 or is_elem(c["z"], dt))
                assert z_f32 == (not is_elem(c["z"], dt)) or rows * C < 64
                assert bool((c["rstd"] > 0).all()) and bool((c["pre"] != 0).all()) and bool((c["acc_pre"] != 0).all())
                if kind == "mean30":
                    assert abs(float(c["z"].mean()) - 30) < 0.5
                for residual in (False, True):
                    _, _, ex = NC.bn_da64(c, "relu", residual)
                    assert int(ex.sum()) <= 1e-3 * ex.numel(), (kind, z_f32, residual, int(ex.sum()))
                    assert rows * C > 1000 or int(ex.sum()) == 0          # |a|_mag reaches ~120 at mean 30: a handful of elements of the larger cases


def test_bn_cap_tail_is_second_trip():
    c = NC.bn_cap_case(torch.bfloat16, 9)
    assert c["z"].shape == (9, 2048) and NC.BN_CAP_SHAPE[0] - 9 == NC.first_second_trip_row(2048) - 1
    for residual in (False, True):
        assert int(NC.bn_da64(c, "relu", residual)[2].sum()) <= 1e-3 * 9 * 2048


@pytest.mark.parametrize("n", NC.FIN_N)
@pytest.mark.parametrize("C", NC.FIN_C)
def test_finalize_reference(C, n):
    """Against nn.BatchNorm2d semantics rebuilt from data for n >= 2 (two-valued data with the same sums reproduce mean and variance), and
    the planted channels: variance exactly 0, variance negative before the clamp in fp64 AND in IEEE fp32, one wide channel."""
    c = NC.finalize_case(C, n)
    r = NC.finalize_ref(c)
    s = c["sums"]
    assert s.dtype == torch.float32
    q32, m32 = s[1] / n, s[0] / n
    assert float(q32[NC.FIN_CONST] - m32[NC.FIN_CONST] ** 2) == 0.0 and float(r["var"][0][NC.FIN_CONST]) == 0.0
    raw = s[1].double() / n - (s[0].double() / n) ** 2
    assert float(raw[NC.FIN_NEG]) < -10 * NC.FIN_EPS and float(q32[NC.FIN_NEG] - m32[NC.FIN_NEG] ** 2) < -10 * NC.FIN_EPS
    assert float(r["var"][0][NC.FIN_NEG]) == 0.0 and abs(float(r["rstd"][0][NC.FIN_NEG]) - NC.FIN_EPS ** -0.5) < 1e-9
    assert abs(float(r["var"][0][NC.FIN_WIDE]) - 1e4) < 1
    keep = torch.ones(C, dtype=torch.bool)
    keep[NC.FIN_NEG] = False
    assert bool((raw[keep] >= -1e-6 * r["var"][1][keep]).all())
    if n >= 2:
        # data with exactly these sums: n - 1 values a and one value b per channel is overkill; two moments suffice for F.batch_norm on
        # the pair (m - d, m + d) repeated, d = sqrt(var): mean m, biased variance d^2
        m, var = r["mean"][0][keep], r["var"][0][keep]
        x = torch.stack([m - var.sqrt(), m + var.sqrt()])
        rm, rv = c["running_mean"].double()[keep].clone(), c["running_var"].double()[keep].clone()
        ga, be = c["gamma"].double()[keep], c["beta"].double()[keep]
        y = F.batch_norm(x, rm, rv, ga, be, True, NC.FIN_MOMENTUM, NC.FIN_EPS)
        close(x[1] * r["scale"][0][keep] + r["shift"][0][keep], y[1], 1e-9)
        close(r["running_mean"][0][keep], rm, 1e-9)
        # F.batch_norm's unbiased factor is that of ITS two samples (2); the reference's is n / (n - 1)
        close((r["running_var"][0][keep] - (1 - NC.FIN_MOMENTUM) * c["running_var"].double()[keep]) / (n / (n - 1.0)), (rv - (1 - NC.FIN_MOMENTUM) * c["running_var"].double()[keep]) / 2.0, 1e-8)
    else:
        close(r["running_var"][0], (1 - NC.FIN_MOMENTUM) * c["running_var"].double() + NC.FIN_MOMENTUM * r["var"][0])     # factor 1 at n = 1
    for k, (ref, mag) in r.items():
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all()), k


# ------------------------------------------------------------------------------------------------ pooling backward
@pytest.mark.parametrize("variant", NC.MP_VARIANTS)
@pytest.mark.parametrize("shape", NC.MP_SHAPES, ids=sid)
def test_maxpool_reference_and_paths(shape, variant):
    """The first-maximum scatter vs autograd of F.max_pool2d(3, 2, 1) in fp64 (where maxima are unique the two must agree; where they tie,
    ATen's CPU kernel keeps the first in scan order too), and the content each variant is there for."""
    B, H, W, C = shape
    for dt in DTYPES:
        c = NC.maxpool_case(shape, dt, variant)
        assert is_elem(c["x"], dt) and torch.equal(c["dy"], c["dy"].round()) and float(c["dy"].abs().max()) <= 3
        x = c["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
        y = F.max_pool2d(x, 3, 2, 1)
        assert tuple(y.shape[2:]) == (NC.mp_out(H), NC.mp_out(W))
        y.backward(c["dy"].double().permute(0, 3, 1, 2))
        ref = NC.maxpool_bwd64(c["x"], c["dy"])
        close(ref, x.grad.permute(0, 2, 3, 1))
        assert torch.equal(ref, ref.round()) and is_elem(ref.float(), dt)
        arg = NC.maxpool_argmax(c["x"])
        fast, mixed = NC.maxpool_paths(c["x"])
        if variant == "relu" and H * W > 4:
            xp = F.pad(c["x"].permute(0, 3, 1, 2), (1, 1, 1, 1), value=-1.0)
            win = F.unfold(xp, 3, stride=2).reshape(B, C, 9, -1)
            assert int(((win == win.max(2, keepdim=True).values).sum(2) > 1).sum()) > 0          # windows with a tied maximum
        if variant == "const":
            # every window is one tie: the first in-bounds tap wins - tap 4 (the centre) for window (0, 0), 3 along the top, 1 along the left, 0 inside
            assert int(arg[0, 0, 0, 0]) == 4 and mixed == 0
            if NC.mp_out(H) > 1 and NC.mp_out(W) > 1:
                assert int(arg[0, 0, 1, 0]) == 3 and int(arg[0, 1, 0, 0]) == 1 and int(arg[0, 1, 1, 0]) == 0
        if variant == "same":
            assert mixed == 0 and fast == arg.numel() // 8
        if variant == "diverging" and H * W > 1:
            assert mixed > 0
            if H * W > 4:
                a8 = arg.reshape(-1, 8)
                assert max(len(set(r.tolist())) for r in a8) >= 4 and mixed > fast


def test_pool_cap_tail():
    B, H, W, C = NC.POOL_CAP_SHAPE
    assert B * H * W * C // 8 > NC.GRID_CAP_THREADS
    first = NC.GRID_CAP_THREADS // (C // 8)
    assert divmod(first, W) == (64, 64) and H - 1 == 64                  # the second trips begin inside the last input row
    assert NC.POOL_CAP_TAIL % 2 == 0 and NC.POOL_CAP_TAIL <= 62
    # a window's argmax depends on the rows 2 ho - 1 .. 2 ho + 1: rows 63 and 64 of dx on windows 31 and 32, hence on input rows 61 .. 64
    x = torch.randn(1, 9, 6, 8, generator=NC.gen(3))
    dy = NC.randint(-3, 3, (1, 5, 3, 8), NC.gen(4))
    full = NC.maxpool_bwd64(x, dy)
    tail = NC.maxpool_bwd64(x[:, 4:], dy[:, 2:])                         # an even first row: the windows of the tail are windows of the whole
    assert torch.equal(full[:, 7:], tail[:, 3:])
    dp = torch.randn(1, 5, 3, 8, generator=NC.gen(5))
    assert torch.equal(NC.avgpool_bwd64(dp, 9, 6)[:, 6:], NC.avgpool_bwd64(dp[:, 3:], 3, 6))


@pytest.mark.parametrize("shape", NC.AP_SHAPES, ids=sid)
def test_avgpool_reference(shape):
    """vs autograd of F.avg_pool2d(2, 2, 0, ceil_mode=True); dp / 1, 2 or 4 is exact for normal values, so rounding the reference changes nothing
    but fp16 values that fall below its normal range."""
    B, H, W, C = shape
    for dt in DTYPES:
        c = NC.avgpool_case(shape, dt)
        x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        y = F.avg_pool2d(x, 2, 2, 0, ceil_mode=True)
        assert tuple(y.shape[2:]) == (NC.ap_out(H), NC.ap_out(W))
        y.backward(c["dp"].double().permute(0, 3, 1, 2))
        ref = NC.avgpool_bwd64(c["dp"], H, W)
        close(ref, x.grad.permute(0, 2, 3, 1))
        normal = ref.abs() >= (2.0 ** -14 if dt == torch.float16 else 2.0 ** -126)
        assert torch.equal(elem_rne(ref, dt)[normal], ref[normal])


# ------------------------------------------------------------------------------------------------ weight images
@pytest.mark.parametrize("shape", [s for s in NC.PACK_CONV_SHAPES if s[0] * s[1] < 10000], ids=sid)
def test_conv_images_convolve(shape):
    """F.conv2d with the packed forward image equals the conv with the (rounded, scaled) master weights, and the stride-1 'same' conv of dz
    with the flipped-transposed image equals its input gradient."""
    N, C, KH, KW = shape
    d = NC.weights_case(N, C, KH, KW)
    v = NC.packed_values(d["w"], d["scale"], torch.bfloat16)
    assert torch.equal(v.float(), (d["w"] * d["scale"][:, None, None, None]).to(torch.bfloat16).float())
    pad = (KH - 1) // 2
    x = torch.randn(2, C, 9, 8, dtype=torch.float64, generator=NC.gen(1)).requires_grad_(True)
    y = F.conv2d(x, v.double(), padding=pad)
    w_fwd = NC.fwd_image(v).double().reshape(N, KH, KW, C).permute(0, 3, 1, 2)
    close(F.conv2d(x.detach(), w_fwd, padding=pad), y.detach())
    dz = torch.randn(y.shape, dtype=torch.float64, generator=NC.gen(2))
    y.backward(dz)
    w_dg = NC.dgrad_image(v).double().reshape(C, KH, KW, N).permute(0, 3, 1, 2)
    close(F.conv2d(dz, w_dg, padding=pad), x.grad)


def test_frag_order_is_the_documented_permutation():
    W2 = torch.arange(64 * 48).reshape(64, 48)
    fr = frag_order(W2)
    for nb, ks, lane, j in [(0, 0, 0, 0), (1, 2, 37, 5), (0, 1, 63, 7), (1, 0, 31, 3)]:
        assert int(fr[nb, ks, lane, j]) == int(W2[nb * 32 + lane % 32, ks * 16 + (lane // 32) * 8 + j])


def test_pack_cases_cross_their_caps():
    N, C, KH, KW = NC.PACK_CONV_SHAPES[-1]
    assert N * C * KH * KW == 1179648 > NC.PACK_CAP_BLOCKS * 256 and N * C * KH * KW // 8 <= NC.PACK_CAP_BLOCKS * 256
    r, K = NC.PACK_FRAG_SHAPES[-1]
    assert r * K // 8 > NC.PACK_CAP_BLOCKS * 256
    assert [NC.frag_eligible(s[0], s[1] * s[2] * s[3]) and NC.frag_eligible(s[1], s[0] * s[2] * s[3]) for s in NC.PACK_CONV_SHAPES] == \
        [False, True, False, True, False, True]


def test_pack_table_layout():
    """Chunk and tile counts, the shared image, and every image element written exactly once or never."""
    entries, images, total = NC.pack_table_case(torch.bfloat16)
    by = {e["name"]: e for e in entries}
    assert NC.pack_chunk(256, 9) == 256 and by["c3x3_256"]["blocks"] == 4                         # exactly one chunk, 4 tiles
    assert NC.pack_chunk(264, 9) == 256 and by["c3x3_264"]["blocks"] == 2 * 2 and 264 - 256 == 8
    assert NC.pack_chunk(2304, 1) == 2304 and by["pw_2304"]["blocks"] == 4
    assert NC.pack_chunk(2312, 1) == 2304 and by["pw_2312"]["blocks"] == 2 and 2312 - 2304 == 8
    assert by["lin_365"]["blocks"] == 46 and 365 - 45 * 8 == 5 and by["lin_365"]["n_total"] % 8 != 0 and by["lin_365"]["ld_dgrad"] == 368
    assert by["lin_k4"]["C"] % 8 != 0 and by["lin_k4"]["ld_fwd"] == 32
    assert NC.pack_chunk(3, 49) == 3 and by["stem7x7"]["ld_fwd"] == 147 and by["stem7x7"]["ld_dgrad"] == 392
    assert [by[k]["n_offset"] for k in ("v0", "v1", "v2")] == [0, 256, 512] and all(by[k]["n_total"] == 768 for k in ("v0", "v1", "v2"))
    assert by["c3x3_264"]["ld_fwd"] > 9 * 264
    assert [e["first_block"] for e in entries] == [sum(x["blocks"] for x in entries[:i]) for i in range(len(entries))] and total == sum(e["blocks"] for e in entries)
    assert any(e["scale"] is None for e in entries) and any(not e["dgrad"] for e in entries) and any(not e["fwd_frag"] for e in entries)
    assert NC.pack_blocks(8, 8, 17, 17) == -1 and NC.pack_blocks(8, 8, 16, 18) == 1 and NC.pack_blocks(8, 16, 16, 18) == 2
    # the shared images are complete, the padded ones keep their sentinel exactly where no (row, column) is addressed
    assert not bool((images["v.fwd"] == NC.SENT16).all(1).any()) and images["v.fwd"].shape == (768, 576)
    assert images["v.dgrad"].shape == (64, 9 * 768) and images["v.fwd_frag"].numel() == 768 * 576 and images["v.dgrad_frag"].numel() == 64 * 9 * 768
    assert bool((images["c3x3_264.fwd"][:, 9 * 264:] == NC.SENT16).all()) and bool((images["lin_365.dgrad"][:, 365:] == NC.SENT16).all())
    assert not bool(torch.isnan(images["v.bias"]).any())
    # one element followed by hand through the documented index formula: entry v1, n = 3, c = 5, kh = 0, kw = 2
    e = by["v1"]
    v = NC.packed_values(e["w"], None, torch.bfloat16).view(torch.int16)
    assert int(images["v.fwd"][256 + 3, (0 * 3 + 2) * 64 + 5]) == int(v[3, 5, 0, 2])
    assert int(images["v.dgrad"][5, ((2 - 0) * 3 + (2 - 2)) * 768 + 256 + 3]) == int(v[3, 5, 0, 2])


@pytest.mark.parametrize("splits", NC.UNPACK_SPLITS)
@pytest.mark.parametrize("shape", NC.UNPACK_SHAPES, ids=sid)
def test_unpack_reference(shape, splits):
    N, C, KH, KW, Ce = shape
    c = NC.unpack_case(shape, splits)
    assert c["stride"] > c["slab"] and (c["stride"] % 4 == 0) == (Ce % 4 == 0)
    slabs = c["part"][:, :c["slab"]].reshape(splits, N, KH, KW, Ce)
    assert bool(torch.isnan(c["part"][:, c["slab"]:]).all()) and (Ce == C or bool(torch.isnan(slabs[..., C:]).all()))
    assert not bool(torch.isnan(slabs[..., :C]).any())
    ref = NC.unpack_ref(c, True, True)
    want = torch.einsum("snhwc,n->nchw", slabs[..., :C].double(), c["scale"].double()) + c["pre"].double()
    assert torch.equal(ref, want) and torch.equal(ref.float().double(), ref)
    assert (shape[1] % 4 != 0 and shape[4] % 4 == 0) == (shape == NC.UNPACK_SHAPES[0]) and NC.UNPACK_SHAPES[2][4] % 4 != 0
    # splits 1: no sum; 2, 4: remainder loop only; 5: one unrolled round, no remainder; 6: one round + 1; 9: two rounds, no remainder
    rounds = (max(splits - 1, 0)) // 4
    assert (rounds, splits - 1 - 4 * rounds) == {1: (0, 0), 2: (0, 1), 4: (0, 3), 5: (1, 0), 6: (1, 1), 9: (2, 0)}[splits]
