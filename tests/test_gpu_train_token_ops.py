"""The small training-side kernels, called directly on a real MI355X under BOTH element types (libfocoos_amd.so = bfloat16,
libfocoos_amd_fp16.so = IEEE half): csrc/train_token_ops.hip (LayerNorm backward, activation forward / backward, column sum, bilinear
resize backward, VFL loss + gradient, row scatter, fp32 -> element cast) and the helpers of csrc/train_conv_ops.hip (ReLU backward with
a second gradient, zero insertion, image normalisation).  The fp32-output depthwise conv is in tests/test_gpu_bf.py.

Rules every case follows
* Reference: the same operation in torch on the CPU in float64 (autograd where a gradient is checked) on the identical inputs, already
  rounded to the element type.
* Guards: every device buffer sits inside GR guard rows on either side and has a leading dimension above its column count.  Outputs are
  prefilled with a sentinel bit pattern and everything outside the written region must keep it bit for bit; the padding of inputs is
  NaN, so a read outside the logical region poisons the result.
* Exact where the arithmetic allows (small-integer sums, copies, casts, one fp32 operation chain without a contraction): bit equality.
* Otherwise, element by element (never "of the maximum"):  |got - ref| <= RND(ref) + c * mag.
    RND(ref) = eps * |ref| + floor is ONE rounding to the element type: eps = 2^-8 (bf16) or 2^-11 (fp16); floor is where the relative
    statement ends: 2^-25 for fp16 (half the spacing of its subnormals), 2^-126 for bf16 (fp32 intermediates below the smallest
    normal may be flushed).
    mag is the fp64 value of the same expression with every term taken in absolute value (it bounds the fp32 error where terms cancel).
    c is the kernel's fp32-arithmetic slack: MEASURED[kernel] is the largest c any case of that kernel needed on an MI355X (over both
    element types), the gate is MARGIN = 4 times that (the fast-math intrinsics' error varies with the argument).  Every test prints
    the c it needs before it asserts, and its docstring carries the figure.
* fp32 sums formed by n sequential fp32 additions are additionally allowed n * 2^-24 * (sum of the |terms|)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FX_ACT, FocoosAmdError, check  # noqa: E402
from tests import helpers  # noqa: E402
from tests.helpers import U32, Buf, _bits, act64  # noqa: E402

DEV = "cuda:0"
MARGIN = 4.0
# largest c = (|got - ref| - RND(ref)) / mag over all cases of the kernel and both element types, measured on an MI355X
MEASURED = {
    "layernorm_bwd.dx": 3.664e-09,
    "layernorm_bwd.dgamma": 3.627e-08,
    "act_fwd": 1.437e-08,
    "act_bwd": 1.387e-08,
    "resize_bwd": 6.771e-07,
    "vfl.loss": 0.0,
    "vfl.dlogits": 4.656e-14,
}


@pytest.fixture(params=["bf16", "fp16"], autouse=True)
def elem(request):
    prev = _lib.set_compute_dtype(request.param)
    yield request.param
    _lib.set_compute_dtype(prev)


@pytest.fixture
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def adt():
    return _lib.act_dtype()


def rnd(ref):
    return helpers.rnd(ref, adt())


def gate(kernel, what, got, ref, mag, extra=None):
    helpers.gate(kernel, what, got, ref, mag, adt(), MEASURED, MARGIN, extra=extra, tag=_lib.compute_dtype())


def rounded(t):
    return t.to(adt())


def plant(t, values):
    """Write `values` into t (flattened, cyclically when t is shorter) at evenly spread positions."""
    f = t.reshape(-1)
    n = f.numel()
    for k, v in enumerate(values):
        f[(k * max(1, n // len(values))) % n] = v
    return t


# ------------------------------------------------------------------------------------------------ 1. LayerNorm backward
def ln_grid(rows):
    """fx_layernorm_bwd_bf16's documented grid rule: ~64 rows per workgroup, at least min(ceil(rows / 4), 64) workgroups, at most 1024;
    a workgroup is 4 waves, a wave walks rows wave, wave + 4 * grid, ..."""
    grid = (rows + 63) // 64
    if grid < 64:
        grid = min((rows + 3) // 4, 64)
    return min(grid, 1024)


def ln_inputs(rows, cols, variant, seed):
    g = torch.Generator().manual_seed(seed)
    if variant == "mean30":
        x = torch.randn(rows, cols, generator=g) * 0.5 + 30.0
    else:
        x = torch.randn(rows, cols, generator=g) * 2 + 0.3
    if rows >= 3:
        x[rows // 2] = 1.5                                   # one constant row: variance 0
    dy = torch.randn(rows, cols, generator=g)
    gamma = torch.rand(cols, generator=g) + 0.5
    return rounded(x), rounded(dy), gamma


def ln_ref(x, dy, gamma):
    """fp64 autograd of F.layer_norm and the magnitudes of the gates."""
    cols = x.shape[1]
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros(cols, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xr, (cols,), gr, br, 1e-5).backward(dy.double())
    xd, d = x.double(), dy.double()
    mu = xd.mean(1, keepdim=True)
    rstd = (xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xh = (xd - mu) * rstd
    gv = d * gamma.double()
    # fp32 error of (x - mean) relative to the row's sigma: the conditioning of xhat (4800 at mean 30, sigma 0.5 would be 60)
    cond = 1.0 + xd.abs().amax(1, keepdim=True) * rstd
    mag_dx = rstd * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True)) * cond
    return {"dx": xr.grad, "dgamma": gr.grad, "dbeta": br.grad, "mag_dx": mag_dx, "abs_dgamma": (d * xh).abs().sum(0),
            "mag_dgamma": ((d * xh).abs() * cond).sum(0), "abs_dbeta": d.abs().sum(0)}


def ln_run(lib, x, dy, gamma, strided, pre_g=None, pre_b=None, null_g=False, null_b=False):
    rows, cols = x.shape
    ldx, lddy, lddx = (cols + 8, cols + 4, cols + 12) if strided else (cols, cols, cols)
    xb, dyb = Buf(rows, cols, ldx, adt(), data=x), Buf(rows, cols, lddy, adt(), data=dy)
    dxb = Buf(rows, cols, lddx, adt())
    gm = gamma.to(DEV)
    dgb = Buf(1, cols, cols + 8, torch.float32, prefill=pre_g if pre_g is not None else torch.zeros(cols))
    dbb = Buf(1, cols, cols + 8, torch.float32, prefill=pre_b if pre_b is not None else torch.zeros(cols))
    check(lib.fx_layernorm_bwd_bf16(dyb.ptr, lddy, xb.ptr, ldx, gm.data_ptr(), dxb.ptr, lddx, None if null_g else dgb.ptr,
                                    None if null_b else dbb.ptr, rows, cols, stream()), "fx_layernorm_bwd_bf16")
    torch.cuda.synchronize()
    for b in (dxb, dgb, dbb):
        b.assert_guards()
    return dxb.get(), dgb.get()[0], dbb.get()[0]


@pytest.mark.parametrize("variant", ["plain", "mean30"])
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("rows", [1, 3, 150, 257, 1000, 4801])
@pytest.mark.parametrize("cols", [256, 128])
def test_layernorm_bwd(lib, cols, rows, strided, variant):
    """dx, dgamma, dbeta of fx_layernorm_bwd_bf16 vs fp64 autograd of F.layer_norm(eps=1e-5); dgamma / dbeta are accumulated onto
    non-zero values.  rows: 1, 3 (fewer rows than waves), 150 (every wave at most one row), 257 (one wave makes a second trip),
    1000 (3 and 4 trips), 4801 (16 trips, ragged end).
    dx: RND + c * mag, mag = rstd * (|g| + mean|g| + |xhat| mean|g xhat|) * (1 + max|x| rstd).
    dgamma: rows * 2^-24 * (sum_r |dy xhat| + |prefill|) + c * sum_r |dy xhat| (1 + max|x| rstd); dbeta: rows * 2^-24 * (sum|dy| + |prefill|).
    Measured c: dx 3.66e-09 (gate 1.47e-08), at 256 x 4801 bf16; dgamma 3.63e-08 (gate 1.45e-07), at 128 x 1 fp16."""
    grid = ln_grid(rows)
    if rows >= 257:
        assert rows > 4 * grid, "this case is meant to make waves walk more than one row"
    if rows == 257:
        assert grid == 64 and rows - 4 * grid == 1          # exactly one wave makes a second trip
    if rows == 4801:
        assert grid == 76 and -(-rows // (4 * grid)) == 16   # 16 trips, the last one ragged
    x, dy, gamma = ln_inputs(rows, cols, variant, 1000 * cols + rows)
    g = torch.Generator().manual_seed(7)
    pre_g, pre_b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    dx, dg, db = ln_run(lib, x, dy, gamma, strided, pre_g, pre_b)
    r = ln_ref(x, dy, gamma)
    gate("layernorm_bwd.dx", f"{cols}x{rows} {variant}", dx, r["dx"], r["mag_dx"])
    gate("layernorm_bwd.dgamma", f"{cols}x{rows} {variant}", dg, pre_g.double() + r["dgamma"], r["mag_dgamma"] + pre_g.double().abs(),
         extra=rows * U32 * (r["abs_dgamma"] + pre_g.double().abs()))
    assert bool(((db.double() - (pre_b.double() + r["dbeta"])).abs() <= rows * U32 * (r["abs_dbeta"] + pre_b.double().abs())).all())


@pytest.mark.parametrize("null", ["dgamma", "dbeta", "both"])
@pytest.mark.parametrize("cols", [256, 128])
def test_layernorm_bwd_null_parameter_gradients(lib, cols, null):
    """A null dgamma and / or dbeta: dx and the other gradient are unchanged (same gates as test_layernorm_bwd), the buffer that was
    not passed keeps its prefill."""
    rows = 257
    x, dy, gamma = ln_inputs(rows, cols, "plain", cols + 1)
    pre = torch.full((cols,), 0.75)
    dx, dg, db = ln_run(lib, x, dy, gamma, True, pre, pre, null_g=null in ("dgamma", "both"), null_b=null in ("dbeta", "both"))
    r = ln_ref(x, dy, gamma)
    gate("layernorm_bwd.dx", f"null {null}", dx, r["dx"], r["mag_dx"])
    if null in ("dgamma", "both"):
        assert torch.equal(dg, pre)
    else:
        gate("layernorm_bwd.dgamma", f"null {null}", dg, 0.75 + r["dgamma"], r["mag_dgamma"] + 0.75, extra=rows * U32 * (r["abs_dgamma"] + 0.75))
    if null in ("dbeta", "both"):
        assert torch.equal(db, pre)
    else:
        assert bool(((db.double() - (0.75 + r["dbeta"])).abs() <= rows * U32 * (r["abs_dbeta"] + 0.75)).all())


@pytest.mark.parametrize("cols", [256, 128])
def test_layernorm_bwd_dbeta_exact_on_integers(lib, cols):
    """Integer dy in [-4, 4] over 1000 rows (3 and 4 trips per wave): every partial sum is an exact fp32 integer, so dbeta = prefill +
    sum(dy) bit for bit whatever the order of the waves' and workgroups' additions - a dropped or doubled row shows."""
    rows = 1000
    x, _, gamma = ln_inputs(rows, cols, "plain", 5)
    g = torch.Generator().manual_seed(cols)
    dy = torch.randint(-4, 5, (rows, cols), generator=g).float()
    pre = torch.full((cols,), 3.0)
    _, _, db = ln_run(lib, x, rounded(dy), gamma, False, None, pre)
    assert torch.equal(db, 3.0 + dy.sum(0))


@pytest.mark.parametrize("cols", [64, 512])
def test_layernorm_bwd_unsupported_width(lib, cols):
    x, dy, gamma = ln_inputs(8, cols, "plain", 1)
    with pytest.raises(FocoosAmdError, match="unsupported"):
        ln_run(lib, x, dy, gamma, False)


# ------------------------------------------------------------------------------------------------ 2. activations
def act_grad64(z, act):
    """d act / dz in fp64 and the same expression with every term in absolute value."""
    one = torch.ones_like(z)
    if act == "relu":
        g = (z > 0).double()
        return g, g
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s)), s * (1 + z.abs() * (1 - s))
    if act == "gelu":
        erf = torch.erf(z / math.sqrt(2.0))
        pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        return 0.5 * (1 + erf) + z * pdf, 0.5 * (1 + erf.abs()) + z.abs() * pdf
    return one, one


def act_mag64(z, act):
    if act == "gelu":
        return 0.5 * z.abs() * (1 + torch.erf(z / math.sqrt(2.0)).abs())
    return act64(z, act).abs()


def act_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    big = torch.finfo(adt()).max
    z = plant(torch.randn(rows, cols, generator=g) * 3, [1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, 0.0, -0.0, big, -big])
    return rounded(z), rounded(torch.randn(rows, cols, generator=g))


# rows * cols / 8 = 1, 255, 257, 3000 groups of eight (cols = 8); 255, 3000 (cols = 24); 128, 256, 2944 (cols = 1024)
ACT_SHAPES = [(1, 8), (255, 8), (257, 8), (3000, 8), (85, 24), (1000, 24), (1, 1024), (2, 1024), (23, 1024)]


@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu"])
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_act_fwd_bwd(lib, shape, act):
    """fx_act_fwd_bf16 / fx_act_bwd_bf16 vs the fp64 activation (tests/helpers.act64) and its fp64 derivative, with +-0, +-1e-3, +-20,
    +-100 and the largest finite element value planted: finite wherever the reference is, none / relu exact, ReLU' (0) = 0.
    silu / gelu: RND + c * mag (mag: every term of the expression in absolute value).  Measured c: forward 1.44e-08 (gate 5.75e-08), backward
    1.39e-08 (gate 5.55e-08), both on GELU (1 + erf cancels for z < 0); SiLU needs 0."""
    rows, cols = shape
    ld = cols + 8
    z, dy = act_inputs(rows, cols, rows * cols + FX_ACT[act])
    zb, dyb = Buf(rows, cols, ld, adt(), data=z), Buf(rows, cols, ld, adt(), data=dy)
    yb, dzb = Buf(rows, cols, ld, adt()), Buf(rows, cols, ld, adt())
    check(lib.fx_act_fwd_bf16(zb.ptr, ld, yb.ptr, ld, rows, cols, FX_ACT[act], stream()), "fx_act_fwd_bf16")
    check(lib.fx_act_bwd_bf16(dyb.ptr, ld, zb.ptr, ld, dzb.ptr, ld, rows, cols, FX_ACT[act], stream()), "fx_act_bwd_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    dzb.assert_guards()
    z64, dy64 = z.double(), dy.double()
    y_ref = act64(z64, act)
    gr, gr_abs = act_grad64(z64, act)
    y, dz = yb.get(), dzb.get()
    if act in ("none", "relu"):
        assert bool((y.double() == y_ref).all()) and bool((dz.double() == dy64 * gr).all())
        if act == "relu":
            assert bool((dz[z == 0] == 0).all())            # +0 and -0 are planted
    else:
        gate("act_fwd", f"{act} {rows}x{cols}", y, y_ref, act_mag64(z64, act))
        gate("act_bwd", f"{act} {rows}x{cols}", dz, dy64 * gr, dy64.abs() * gr_abs)


CAP_ROWS, CAP_COLS = 8200, 2048                       # 2 099 200 groups of eight > the 256 * 32 * 256 = 2 097 152 threads of a capped grid
CAP_FIRST_ROW = 256 * 32 * 256 // (CAP_COLS // 8)     # 8192: first row handled by a thread's second trip through the grid-stride loop


def test_grid_cap_act_bwd(lib):
    """fx_act_bwd_bf16 (SiLU) past the grid cap: the last 8 rows are second trips through the grid-stride loop.  Gate of act_bwd."""
    assert CAP_ROWS * CAP_COLS // 8 > 256 * 32 * 256 and CAP_FIRST_ROW < CAP_ROWS
    ld = CAP_COLS + 8
    g = torch.Generator().manual_seed(11)
    z, dy = rounded(torch.randn(CAP_ROWS, CAP_COLS, generator=g) * 3), rounded(torch.randn(CAP_ROWS, CAP_COLS, generator=g))
    zb, dyb, dzb = Buf(CAP_ROWS, CAP_COLS, ld, adt(), data=z), Buf(CAP_ROWS, CAP_COLS, ld, adt(), data=dy), Buf(CAP_ROWS, CAP_COLS, ld, adt())
    check(lib.fx_act_bwd_bf16(dyb.ptr, ld, zb.ptr, ld, dzb.ptr, ld, CAP_ROWS, CAP_COLS, FX_ACT["silu"], stream()), "fx_act_bwd_bf16")
    torch.cuda.synchronize()
    dzb.assert_guards()
    gr, gr_abs = act_grad64(z.double(), "silu")
    ref, mag, dz = dy.double() * gr, dy.double().abs() * gr_abs, dzb.get()
    gate("act_bwd", "grid cap, second trip", dz[CAP_FIRST_ROW:], ref[CAP_FIRST_ROW:], mag[CAP_FIRST_ROW:])
    gate("act_bwd", "grid cap, all", dz, ref, mag)


def test_grid_cap_relu_bwd(lib):
    """fx_relu_bwd_bf16 with a second upstream gradient past the grid cap.  (dy + dy2) is one fp32 addition, the mask exact, then one
    rounding: |got - ref| <= RND(ref) + 2^-24 |ref|, no measured slack."""
    ld = CAP_COLS + 8
    g = torch.Generator().manual_seed(12)
    dy, dy2 = (rounded(torch.randn(CAP_ROWS, CAP_COLS, generator=g)) for _ in range(2))
    y = rounded(torch.randn(CAP_ROWS, CAP_COLS, generator=g).clamp_min(0))
    bufs = [Buf(CAP_ROWS, CAP_COLS, ld, adt(), data=t) for t in (dy, dy2, y)]
    dzb = Buf(CAP_ROWS, CAP_COLS, ld, adt())
    check(lib.fx_relu_bwd_bf16(bufs[0].ptr, ld, bufs[1].ptr, ld, bufs[2].ptr, ld, dzb.ptr, ld, CAP_ROWS, CAP_COLS, 1, stream()), "fx_relu_bwd_bf16")
    torch.cuda.synchronize()
    dzb.assert_guards()
    ref = (dy.double() + dy2.double()) * (y.double() > 0)
    ok = (dzb.get().double() - ref).abs() <= rnd(ref) + U32 * ref.abs()
    assert bool(ok[CAP_FIRST_ROW:].all()), "second trip"
    assert bool(ok.all())


def _same_bits_or_nan(got, ref):
    nan = torch.isnan(ref)
    return bool((torch.isnan(got) == nan).all()) and bool((_bits(got)[~nan] == _bits(ref)[~nan]).all())


def test_grid_cap_cast(lib):
    """fx_cast_f32_bf16 of 8 * 2 099 200 values: bit-identical to torch's own conversion, the second-trip tail checked on its own."""
    n = CAP_ROWS * CAP_COLS
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, generator=g) * 50
    xb, yb = Buf(1, n, n + 8, torch.float32, data=x), Buf(1, n, n + 8, adt())
    check(lib.fx_cast_f32_bf16(xb.ptr, yb.ptr, n, stream()), "fx_cast_f32_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    got, ref = yb.get()[0], x.to(adt())
    assert _same_bits_or_nan(got[8 * 256 * 32 * 256:], ref[8 * 256 * 32 * 256:]), "second trip"
    assert _same_bits_or_nan(got, ref)


# ------------------------------------------------------------------------------------------------ 3. column sum
@pytest.mark.parametrize("cols", [8, 256, 264, 368, 1024])
@pytest.mark.parametrize("rows", [1, 7, 255, 256, 257, 1000])
def test_colsum_exact_on_integers(lib, rows, cols):
    """Integer x in [-8, 8]: out = prefill + column sums, bit for bit (row tails below 8 and 256, column tails below 256, ldx > cols)."""
    g = torch.Generator().manual_seed(rows * 2000 + cols)
    x = torch.randint(-8, 9, (rows, cols), generator=g).float()
    pre = torch.randint(-5, 6, (cols,), generator=g).float()
    xb, ob = Buf(rows, cols, cols + 8, adt(), data=rounded(x)), Buf(1, cols, cols + 8, torch.float32, prefill=pre)
    check(lib.fx_colsum_bf16(xb.ptr, cols + 8, ob.ptr, rows, cols, stream()), "fx_colsum_bf16")
    torch.cuda.synchronize()
    ob.assert_guards()
    assert torch.equal(ob.get()[0], pre + x.sum(0))


def test_colsum_random(lib):
    """Random x: |out - (prefill + sum)| <= rows * 2^-24 * (sum|x| + |prefill|) per column (the additions' roundings alone)."""
    rows, cols = 1000, 264
    g = torch.Generator().manual_seed(3)
    x, pre = rounded(torch.randn(rows, cols, generator=g) * 2), torch.randn(cols, generator=g)
    xb, ob = Buf(rows, cols, cols + 8, adt(), data=x), Buf(1, cols, cols + 8, torch.float32, prefill=pre)
    check(lib.fx_colsum_bf16(xb.ptr, cols + 8, ob.ptr, rows, cols, stream()), "fx_colsum_bf16")
    torch.cuda.synchronize()
    ob.assert_guards()
    ref = pre.double() + x.double().sum(0)
    assert bool(((ob.get()[0].double() - ref).abs() <= rows * U32 * (x.double().abs().sum(0) + pre.double().abs())).all())


# ------------------------------------------------------------------------------------------------ 4. bilinear resize backward
RESIZE_SHAPES = [((4, 4), (32, 32)), ((32, 32), (4, 4)), ((16, 20), (5, 7)), ((5, 7), (16, 20)), ((1, 9), (6, 9)), ((9, 1), (9, 5)),
                 ((6, 10), (1, 1)), ((3, 50), (50, 3)), ((11, 13), (11, 13)), ((10, 12), (20, 24)), ((20, 24), (10, 12)), ((7, 9), (13, 17))]


def resize_bwd_ref(dy, H, W):
    """fp64 autograd of F.interpolate(bilinear, align_corners=False); dy [B, Ho, Wo, C] -> dx [B, H, W, C]."""
    B, Ho, Wo, Cc = dy.shape
    x = torch.zeros(B, Cc, H, W, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False).backward(dy.double().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1)


def resize_bwd_run(lib, dy, H, W):
    B, Ho, Wo, Cc = dy.shape
    dyb, dxb = Buf(B * Ho * Wo, Cc, Cc + 8, adt(), data=dy), Buf(B * H * W, Cc, Cc + 16, adt())
    check(lib.fx_resize_bilinear_bwd_nhwc_bf16(dyb.ptr, Cc + 8, dxb.ptr, Cc + 16, B, H, W, Cc, Ho, Wo, stream()), "fx_resize_bilinear_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    dxb.assert_guards()
    return dxb.get().reshape(B, H, W, Cc)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Cc", [8, 64])
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_bilinear_bwd(lib, shape, Cc, B):
    """fx_resize_bilinear_bwd_nhwc_bf16 vs fp64 autograd of F.interpolate at strong up / down scales, single rows and columns, a 1x1
    output, transposed aspect ratios and the identity (bit-exact).
    Random dy: RND + c * mag, mag = the adjoint applied to |dy| (the weights are non-negative).  Measured c: 6.77e-07 (gate 2.71e-06), at 7x9 -> 13x17 (fp32 source coordinates).
    One-hot dy: every (image, channel) plane has ONE output pixel set, at positions spread over the output incl. its corners, so one
    launch probes up to 128 output pixels.  Every input pixel the reference reaches must be non-zero (a bil_range one pixel short loses
    exactly such a tap).  The converse holds up to fp32 coordinates: where (dst + 0.5) * in / out - 0.5 is an integer n (7 -> 13 at
    dst 6, 9 -> 17 at dst 8) fp32 may land a few ulp above n and give tap n + 1 a weight of a few 2^-24 * n where fp64 has exactly 0;
    an input pixel the reference does not reach may therefore hold at most 8 * 2^-24 * max(H, W) * |dy| (a genuinely wrong tap weighs
    >= 1 / (2 * max(Ho, Wo)) >= 1e-2)."""
    (H, W), (Ho, Wo) = shape
    g = torch.Generator().manual_seed(H * 1000 + Wo * 10 + B)
    dy = rounded(torch.randn(B, Ho, Wo, Cc, generator=g))
    dx = resize_bwd_run(lib, dy, H, W)
    if (H, W) == (Ho, Wo):
        assert torch.equal(_bits(dx), _bits(dy))
    gate("resize_bwd", f"{H}x{W}->{Ho}x{Wo}", dx, resize_bwd_ref(dy, H, W), resize_bwd_ref(dy.abs(), H, W))
    # one output pixel per (image, channel) plane
    k = torch.arange(B * Cc)
    pix = (k * 37) % (Ho * Wo)
    pix[-1] = Ho * Wo - 1
    hot = torch.zeros(B * Cc, Ho * Wo)
    hot[k, pix] = 1.5
    hot = rounded(hot.reshape(B, Cc, Ho, Wo).permute(0, 2, 3, 1).contiguous())
    dx, ref = resize_bwd_run(lib, hot, H, W), resize_bwd_ref(hot, H, W)
    assert bool((dx[ref != 0] != 0).all()), "an input pixel the reference reaches got nothing: bil_range too short"
    assert bool((dx[ref == 0].double().abs() <= 8 * U32 * max(H, W) * 1.5).all()), "an input pixel outside the reference's taps was written"
    gate("resize_bwd", f"{H}x{W}->{Ho}x{Wo} one-hot", dx[ref != 0], ref[ref != 0], ref[ref != 0].abs())


# ------------------------------------------------------------------------------------------------ 5. VFL loss + gradient
def vfl_inputs(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    logits = rounded(plant(torch.randn(rows, K, generator=g) * 3, [30.0, -30.0, 0.0]))
    cls = torch.full((rows,), K, dtype=torch.int32)                    # K = no object
    pos = torch.arange(0, rows, 7)
    cls[pos] = ((pos * 13) % K).int()
    cls[0] = 0
    if rows > 1:
        cls[rows - 1] = K - 1
    score = torch.rand(rows, generator=g)
    p = torch.nonzero(cls < K).flatten()
    score[p[0]] = 1.0
    if len(p) > 1:
        score[p[1]] = 0.0
    return logits, cls, score


def vfl_ref(logits, cls, score, alpha, gamma, scale):
    """The per-element formula of loss_labels_vfl (oracle/criterion_oracle.py: weight = alpha * sigmoid^gamma * (1 - onehot) + target score,
    sigmoid detached; weighted BCE with logits) in fp64, summed and scaled; autograd for d loss / d logits."""
    rows, K = logits.shape
    x = logits.double().requires_grad_(True)
    pos = torch.nonzero(cls < K).flatten()
    onehot = torch.zeros(rows, K, dtype=torch.float64)
    onehot[pos, cls[pos].long()] = 1.0
    t = onehot * score.double().unsqueeze(1)
    p = torch.sigmoid(x).detach()
    w = alpha * p.pow(gamma) * (1 - onehot) + t
    el = F.binary_cross_entropy_with_logits(x, t, weight=w, reduction="none")
    (el.sum() * scale).backward()
    return {"loss": float(el.detach().sum() * scale), "abs": float(el.detach().abs().sum() * scale), "d": x.grad, "mag_d": w * (p + t) * scale, "p": p}


@pytest.mark.parametrize("ag", [(0.75, 2.0), (0.25, 1.5)], ids=["a.75g2", "a.25g1.5"])
@pytest.mark.parametrize("lddl_pad", [0, 5])
@pytest.mark.parametrize("ld_pad", [0, 3])
@pytest.mark.parametrize("rows", [1, 300, 1201])
@pytest.mark.parametrize("K", [1, 80, 365])
def test_vfl_loss(lib, K, rows, ld_pad, lddl_pad, ag):
    """fx_vfl_loss_bf16 vs the fp64 per-element formula of loss_labels_vfl and its autograd: positives on classes 0 .. K-1, no-object
    rows, scores exactly 0 and 1, logits +-30 and 0, odd K and leading dimensions (2-byte stores), scale = 1/7, loss accumulated onto
    2.5, and the same loss with dlogits = NULL.
    loss: rows * K * 2^-24 * (sum|w bce| * scale + 2.5) + c * (sum|w bce| * scale + 2.5); dlogits: RND + c * w (p + t) scale; a no-object
    row's gradient is alpha * p^gamma * p * scale under the same gate.  Measured c: loss 0, dlogits 4.66e-14 (gate 1.86e-13).  Both gates are in effect 'no slack': the loss must hold the summation
    term alone and dlogits the rounding bound alone on these seeded inputs (__expf / __powf / __logf stay inside one rounding of the
    element type here); a toolchain that moves one intrinsic by an ulp at the bottom of a binade can trip it without a kernel fault -
    then re-measure, as the file's header says, rather than widen by hand."""
    alpha, gamma = ag
    scale = float(torch.tensor(1.0 / 7.0, dtype=torch.float32))        # the fp32 value the kernel receives
    ld, lddl = K + ld_pad, K + lddl_pad
    logits, cls, score = vfl_inputs(rows, K, K * 10000 + rows)
    lb, db = Buf(rows, K, ld, adt(), data=logits), Buf(rows, K, lddl, adt())
    cd, sd = cls.to(DEV), score.to(DEV)
    losses = []
    for dl in (db.ptr, None):
        lo = Buf(1, 1, 8, torch.float32, prefill=torch.tensor([2.5]))
        check(lib.fx_vfl_loss_bf16(lb.ptr, ld, cd.data_ptr(), sd.data_ptr(), alpha, gamma, scale, lo.ptr, dl, lddl, rows, K, stream()), "fx_vfl_loss_bf16")
        torch.cuda.synchronize()
        lo.assert_guards()
        losses.append(lo.get().reshape(()))
    db.assert_guards()
    r = vfl_ref(logits, cls, score, alpha, gamma, scale)
    what = f"K{K} rows{rows} ld+{ld_pad} lddl+{lddl_pad} a{alpha} g{gamma}"
    mag = torch.tensor(r["abs"] + 2.5, dtype=torch.float64)
    for lo in losses:
        gate("vfl.loss", what, lo, torch.tensor(2.5 + r["loss"], dtype=torch.float64), mag, extra=rows * K * U32 * mag)
    d = db.get()
    gate("vfl.dlogits", what, d, r["d"], r["mag_d"])
    noobj = cls == K
    if bool(noobj.any()):
        p = r["p"][noobj]
        gate("vfl.dlogits", what + " no-object rows", d[noobj], alpha * p.pow(gamma) * p * scale, alpha * p.pow(gamma) * p * scale)


# ------------------------------------------------------------------------------------------------ 6. bit-exact copies and casts
def cast_specials():
    dt = adt()
    fi = torch.finfo(dt)
    bits = torch.tensor([0x3C00, 0x3C01, 0x3C02, 0x3C03, 0x0400, 0x0401, 0x4711, 0x4712, 0x0001, 0x0002], dtype=torch.int16)
    lo, hi = bits.view(dt).float(), (bits + 1).view(dt).float()
    ties = (lo + hi) / 2                                                 # exactly half way between two neighbours, even and odd lower ones
    assert bool((ties != lo).all() and (ties != hi).all())
    f32 = torch.finfo(torch.float32)
    sp = [0.0, -0.0, float("inf"), -float("inf"), float("nan")]
    sp += ties.tolist() + (-ties).tolist()
    # the tie between the largest finite value and "the next one" rounds to infinity (even), the fp32 value just below it does not
    top = torch.tensor([0x7F7F8000], dtype=torch.int32).view(torch.float32) if dt == torch.bfloat16 else torch.tensor([65520.0])
    below = torch.nextafter(top, torch.zeros(1))
    sp += [f32.max, -f32.max, fi.max, -fi.max, float(top), -float(top), float(below), -float(below)]
    sp += [fi.smallest_normal / 2, fi.smallest_normal / 3, -fi.smallest_normal / 5, fi.smallest_normal * 2.0 ** -8,            # element-type subnormals
           f32.smallest_normal / 2, -f32.smallest_normal / 3, 1.4e-45, -1.4e-45]                                                # fp32 subnormals
    return torch.tensor(sp, dtype=torch.float64).float()


@pytest.mark.parametrize("n", [8, 2040, 2056])
def test_cast_f32_matches_torch(lib, n):
    """fx_cast_f32_bf16 vs torch's own .to(element type), bit for bit (NaN: NaN-ness): round-to-nearest-even ties of both parities, +-0,
    +-inf, NaN, subnormals of the element type and of fp32, values that round up to infinity.  With n = 8 the first 8 specials fit;
    a second call at n = 8 casts ties."""
    g = torch.Generator().manual_seed(n)
    sp = cast_specials()
    for first in (0, 5):
        x = torch.randn(n, generator=g) * 100
        k = min(n, len(sp) - first)
        x[:k] = sp[first:first + k]
        xb, yb = Buf(1, n, n + 8, torch.float32, data=x), Buf(1, n, n + 8, adt())
        check(lib.fx_cast_f32_bf16(xb.ptr, yb.ptr, n, stream()), "fx_cast_f32_bf16")
        torch.cuda.synchronize()
        yb.assert_guards()
        assert _same_bits_or_nan(yb.get()[0], x.to(adt()))


@pytest.mark.parametrize("cols", [8, 256])
@pytest.mark.parametrize("k", [1, 17, 50])
def test_scatter_rows(lib, k, cols):
    """dsrc[b, idx[b, j]] = dout[b, j] bit for bit; rows that no index names keep the sentinel."""
    B, rpb = 3, 50
    g = torch.Generator().manual_seed(k * cols)
    dout = rounded(torch.randn(B * k, cols, generator=g))
    idx = torch.stack([torch.randperm(rpb, generator=g)[:k] for _ in range(B)]).int()
    ob, sb = Buf(B * k, cols, cols + 8, adt(), data=dout), Buf(B * rpb, cols, cols + 16, adt())
    idd = idx.to(DEV)
    check(lib.fx_scatter_rows_bf16(ob.ptr, cols + 8, idd.data_ptr(), k, sb.ptr, cols + 16, rpb, B, cols, stream()), "fx_scatter_rows_bf16")
    torch.cuda.synchronize()
    rows = (torch.arange(B).unsqueeze(1) * rpb + idx.long()).flatten()
    written = torch.zeros(B * rpb, dtype=torch.bool)
    written[rows] = True
    sb.assert_guards(written)
    assert torch.equal(_bits(sb.get()[rows]), _bits(dout))


@pytest.mark.parametrize("Cc", [8, 40])
@pytest.mark.parametrize("dims", [(5, 7, 9, 13), (5, 7, 10, 14), (5, 7, 10, 13), (1, 1, 1, 1), (1, 1, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_zero_insert2(lib, dims, Cc):
    """u[b, 2 ho, 2 wo] = dz[b, ho, wo], +0 elsewhere, vs a torch strided assignment, bit for bit."""
    Ho, Wo, H, W = dims
    B = 2
    g = torch.Generator().manual_seed(H * W + Cc)
    dz = rounded(torch.randn(B, Ho, Wo, Cc, generator=g))
    zb, ub = Buf(B * Ho * Wo, Cc, Cc + 8, adt(), data=dz), Buf(B * H * W, Cc, Cc + 16, adt())
    check(lib.fx_zero_insert2_nhwc_bf16(zb.ptr, Cc + 8, ub.ptr, Cc + 16, B, Ho, Wo, H, W, Cc, stream()), "fx_zero_insert2_nhwc_bf16")
    torch.cuda.synchronize()
    ub.assert_guards()
    ref = torch.zeros(B, H, W, Cc, dtype=adt())
    ref[:, 0:2 * Ho:2, 0:2 * Wo:2] = dz
    assert torch.equal(_bits(ub.get().reshape(B, H, W, Cc)), _bits(ref))


@pytest.mark.parametrize("pixels", [1, 255, 257, 70001])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_normalize_pad8(lib, kind, pixels):
    """((raw - mean) * inv_std) in fp32 in that order (no addition follows the multiplication: nothing to contract), rounded once to the
    element type: bit for bit; channels 3..7 are +0.
    70001 fp32 pixels are 210 003 distinct values: enough to meet the roughly 1 in 10^4 for which rounding the exact product once to
    fp16 differs from rounding it to fp32 first (the fp16 build used to do the former for channel 2 alone)."""
    g = torch.Generator().manual_seed(pixels)
    if kind == "u8":
        img = torch.randint(0, 256, (pixels, 3), generator=g).to(torch.uint8)
        img_d = img.to(DEV)
    else:
        img = torch.rand(pixels, 3, generator=g) * 255
        ib = Buf(pixels, 3, 3, torch.float32, data=img)
    mean = torch.tensor([123.675, 116.28, 103.53])
    inv_std = 1.0 / torch.tensor([58.395, 57.12, 57.375])
    md, sd = mean.to(DEV), inv_std.to(DEV)
    ob = Buf(pixels, 8, 8, adt())
    check(lib.fx_normalize_pad8(img_d.data_ptr() if kind == "u8" else ib.ptr, int(kind == "f32"), md.data_ptr(), sd.data_ptr(), ob.ptr, pixels,
                                stream()), "fx_normalize_pad8")
    torch.cuda.synchronize()
    ob.assert_guards()
    ref = torch.zeros(pixels, 8, dtype=adt())
    ref[:, :3] = ((img.float() - mean) * inv_std).to(adt())
    assert torch.equal(_bits(ob.get()), _bits(ref))
