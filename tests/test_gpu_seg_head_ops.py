"""The small kernels that carry BiSeNetFormer, the STDC stride-2 bottleneck, the classifier heads and the MaskFormer FPN, called directly
through the C ABI on a real MI355X under BOTH element types (libfocoos_amd.so = bfloat16, libfocoos_amd_fp16.so = IEEE half):
csrc/seg_ops.hip (depthwise 3x3 stride-2 conv with element and fp32 output, global mean, pooled linear, channel gate),
csrc/train_seg_ops.hip (depthwise backward, row dot, vector broadcast, planes to rows) and the two nearest-upsample kernels of
csrc/mask_ops.hip.  Inputs, float64 references and magnitudes come from tests/seg_head_cases.py, which tests/test_seg_head_cases_cpu.py
pins against independent formulations.

Rules every case follows (those of tests/test_gpu_train_token_ops.py)
* Every device buffer is a helpers.Buf: guard rows on either side, a leading dimension above its column count, inputs padded with NaN,
  outputs prefilled with a sentinel that everything outside the written region must keep bit for bit.  fp32 outputs a kernel ADDS to
  lie in the corner of a region of 1.0s instead (acc_buf): an addition to the 1.5e16 the sentinel reads as leaves no trace.
* Exact where the arithmetic is one fp32 operation and one rounding for the seeded inputs (vector broadcast, planes to rows): bit
  equality with the single rounding of the fp64 value.
* Otherwise, per element:  |got - ref| <= RND(ref) + c * mag.  RND(ref) is one rounding to the output type, mag the fp64 value of the
  same expression with every term in absolute value.
  - DERIVED c where the chain is a fixed number of fp32 operations: c = (operations in the longest chain) * 2^-24, counted in the
    docstring of the test.
  - MEASURED c where the order of summation is the runtime's or a fast-math intrinsic is involved: MEASURED[kernel] is the largest c
    any case needed on an MI355X over both element types (printed as EXCESS ...), the gate is MARGIN = 4 times that, and the recorded
    figure must lie below the derived worst case of EVERY case it gates (the `ceiling` each test asserts): a kernel that needs more
    than its ceiling is a finding, not a number to record.
* Run twice, identical bits: global mean, row dot with one split, depthwise forward and dgrad, both upsample kernels, vector broadcast,
  planes to rows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FocoosAmdError, check  # noqa: E402
from tests import helpers  # noqa: E402
from tests import seg_head_cases as SC  # noqa: E402
from tests.helpers import U32, Buf, _bits, elem_rne, needed_c  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
MARGIN = 4.0
# largest c = (|got - ref| - RND(ref)) / mag over all cases of the kernel and both element types, measured on an MI355X
MEASURED = {
    "global_mean": 3.221e-08,
    "pooled_linear": 5.086e-08,
    "pooled_linear.sigmoid": 2.615e-09,
    "rowdot": 1.643e-07,
    "dw_wgrad": 1.560e-07,
}


# The yardstick of the __expf intrinsic: what the activation forward (x / (1 + __expf(-x)), tests/test_gpu_train_token_ops.py) needs.
ACT_FWD_C = 1.437e-08


@pytest.fixture(params=["bf16", "fp16"])
def elem(request):
    prev = _lib.set_compute_dtype(request.param)
    yield request.param
    _lib.set_compute_dtype(prev)


@pytest.fixture
def lib(elem):
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture
def lib32():
    """fx_pooled_linear_f32 reads no 16-bit data: one library is enough."""
    assert torch.cuda.is_available()
    return _lib.load("bf16")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def adt():
    return _lib.act_dtype()


def tag():
    return _lib.compute_dtype()


def sid(s):
    return "x".join(map(str, s))


def rows_buf(t, ld, dtype=None):
    """[..., C] values as a [rows][ld] input Buf."""
    Cc = t.shape[-1]
    return Buf(t.numel() // Cc, Cc, ld, dtype or adt(), data=t)


def derived(kernel, what, got, ref, mag, dtype, ops, extra=None):
    """Print the c this output needs, then assert c <= ops * 2^-24 (the derived slack of a chain of `ops` fp32 operations)."""
    c = needed_c(got, ref, mag, dtype, extra)
    print(f"EXCESS {kernel} {tag()} {c:.3e} {what} (derived {ops} * 2^-24 = {ops * U32:.3e})")
    assert c <= ops * U32, f"{kernel} {what}: needs c = {c:.3e}, derived {ops} * 2^-24 = {ops * U32:.3e}"


def measured(kernel, what, got, ref, mag, dtype, ceiling, extra=None):
    """The measured gate; the recorded figure itself must lie below this case's derived worst case."""
    assert MEASURED[kernel] <= ceiling, f"{kernel} {what}: recorded {MEASURED[kernel]:.3e} above the derived ceiling {ceiling:.3e}"
    return helpers.gate(kernel, what, got, ref, mag, dtype, MEASURED, MARGIN, extra=extra, tag=tag())


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def untouched(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.assert_guards(written=torch.zeros(b.rows, dtype=torch.bool))


def refused(rc, what):
    with pytest.raises(FocoosAmdError, match="invalid argument"):
        check(rc, what)
        pytest.fail(f"{what}: accepted")


NEIGHBOUR = 1.0


def acc_buf(pre, rows, cols):
    """An ACCUMULATED fp32 output as it lies in a flat gradient buffer: `pre` in the corner of a [rows][cols] region whose other elements
    hold 1.0 (see the header)."""
    full = torch.full((rows, cols), NEIGHBOUR)
    full[:pre.shape[0], :pre.shape[1]] = pre
    return Buf(rows, cols, cols, F32, prefill=full)


def acc_get(buf, rows, cols):
    buf.assert_guards()
    got = buf.get()
    rest = got.clone()
    rest[:rows, :cols] = NEIGHBOUR
    assert bool((rest == NEIGHBOUR).all()), "an element outside the accumulated corner changed"
    return got[:rows, :cols].contiguous()


# ------------------------------------------------------------------------------------------------ 1. depthwise 3x3 stride 2: forward
def dw_fwd_run(lib, c, f32out, ldx, ldy):
    B, H, W, Cc = c["x"].shape
    Ho, Wo = SC.out_size(H), SC.out_size(W)
    xb = rows_buf(c["x"], ldx)
    wd = c["w9"].to(DEV)
    bd = c["bias"].to(DEV) if c["bias"] is not None else None
    fn = lib.fx_dwconv3x3s2_nhwc_f32out if f32out else lib.fx_dwconv3x3s2_nhwc_bf16
    outs = []
    for _ in range(2):
        yb = Buf(B * Ho * Wo, Cc, ldy, F32 if f32out else adt())
        check(fn(xb.ptr, ldx, wd.data_ptr(), bd.data_ptr() if bd is not None else None, yb.ptr, ldy, B, H, W, Cc, stream()), "fx_dwconv3x3s2")
        torch.cuda.synchronize()
        yb.assert_guards()
        outs.append(yb.get())
    assert same_bits(outs[0], outs[1]), "two runs differ"
    return outs[0].reshape(B, Ho, Wo, Cc)


@pytest.mark.parametrize("variant", SC.DW_VARIANTS)
@pytest.mark.parametrize("shape", SC.DW_SHAPES, ids=sid)
def test_dwconv_forward(lib, shape, variant):
    """fx_dwconv3x3s2_nhwc_bf16 and fx_dwconv3x3s2_nhwc_f32out with bias, with a NULL bias and with the 1/9 weights of AvgPool2d(3, 2, 1),
    ldx = C + 8 and ldy = C + 16 (channel slices of a concat buffer).  Nine fused multiply-adds onto the bias: 10 fp32 operations with the
    conversion of the bias counted, so c = 10 * 2^-24 on mag = conv(|x|, |w|) + |bias|; the element output adds its one rounding."""
    Cc = shape[3]
    c = SC.dw_case(shape, adt(), variant)
    ref, mag = SC.dw_fwd64(c["x"], c["w9"], c["bias"])
    what = f"{sid(shape)} {variant}"
    derived("dwconv.elem", what, dw_fwd_run(lib, c, False, Cc + 8, Cc + 16), ref, mag, adt(), 10)
    derived("dwconv.f32out", what, dw_fwd_run(lib, c, True, Cc + 8, Cc + 8), ref, mag, F32, 10, extra=0.0)


# ------------------------------------------------------------------------------------------------ 2. depthwise backward
def dw_bwd_run(lib, c, want_dx, want_dw, pre=None):
    """(dx or None, dw or None); the output that is not asked for is passed as NULL together with the operand only it reads."""
    B, H, W, Cc = c["x"].shape
    ldx, lddy, lddx = Cc + 8, Cc + 16, Cc + 24
    dyb, xb = rows_buf(c["dy"], lddy), rows_buf(c["x"], ldx)
    wd = c["w9"].to(DEV)
    dxb = Buf(B * H * W, Cc, lddx, adt())
    dwb = acc_buf(c["pre"] if pre is None else pre, 10, Cc)
    check(lib.fx_dwconv3x3s2_bwd_nhwc_bf16(dyb.ptr, lddy, xb.ptr if want_dw else None, ldx if want_dw else 0, wd.data_ptr() if want_dx else None,
                                           dxb.ptr if want_dx else None, lddx if want_dx else 0, dwb.ptr if want_dw else None, B, H, W, Cc, stream()),
          "fx_dwconv3x3s2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    if want_dx:
        dxb.assert_guards()
    else:
        untouched(dxb)
    dw = acc_get(dwb, 9, Cc)
    if not want_dw:
        assert torch.equal(dw, c["pre"])
    return (dxb.get().reshape(B, H, W, Cc) if want_dx else None), (dw if want_dw else None)


@pytest.mark.parametrize("mode", ["dx", "dw", "both"])
@pytest.mark.parametrize("shape", SC.DW_WGRAD_SHAPES, ids=sid)
def test_dwconv_backward(lib, shape, mode):
    """fx_dwconv3x3s2_bwd_nhwc_bf16 called for dx only (x = NULL; the 1/9 weights: AvgPool2d's backward), for dw only (dx = w = NULL) and
    for both, vs the fp64 transpose / weight gradient of the forward reference.
    dgrad: an input pixel has at most 2 x 2 contributing windows (odd row and column), so 4 fused multiply-adds: c = 4 * 2^-24 on
    mag = dgrad(|dy|, |w|); even and odd H / W give the last row / column one and two windows.  Run twice, identical bits.
    wgrad: added to a non-zero dw; measured c on mag = sum|dy||x| + |prefill|, ceiling (ceil(per / 32) + 32 + splits + 1) * 2^-24: a lane's
    sequential sum, the 32-lane tree, one atomic per split, the prefill.  Shapes: P = 512 (one split, C = 72: one live lane group in the
    second channel group), P = 513 (two splits, per = 257).
    Measured c: 1.56e-07 (gate 6.24e-07), at 1 x 13 x 15 x 264 fp16; the smallest ceiling of a case here is 35 * 2^-24 = 2.09e-06."""
    B, H, W, Cc = shape
    want_dx, want_dw = mode != "dw", mode != "dx"
    c = SC.dw_case(shape, adt(), "avg" if mode == "dx" else "bias")
    dx, dw = dw_bwd_run(lib, c, want_dx, want_dw)
    if want_dx:
        ref, mag = SC.dw_dgrad64(c["dy"], c["w9"], H, W)
        derived("dwconv.dgrad", f"{sid(shape)} {mode}", dx, ref, mag, adt(), 4)
        dx2, _ = dw_bwd_run(lib, c, True, False)
        assert same_bits(dx, dx2), "two runs differ"
    if want_dw:
        ref, mag = SC.dw_wgrad64(c["dy"], c["x"])
        measured("dw_wgrad", f"{sid(shape)} {mode}", dw, ref + c["pre"].double(), mag + c["pre"].double().abs(), F32, SC.dw_wgrad_ceiling(shape))


def test_dwconv_wgrad_split_cap(lib):
    """The weight gradient past the split cap: C = 2048, 257 x 257 -> ceil(16641 / 512) * 32 = 1056 > 1024 workgroups, so 32 splits of 521
    pixels.  The one large input of this file (135 M elements): generated, uploaded and referenced per 256-channel slice (nine shifted
    products each); 3.4 s per element type, most of it the random numbers.  Gate of dw_wgrad (this case needs 1e-08), ceiling
    (17 + 32 + 32 + 1) * 2^-24 = 4.89e-06."""
    B, H, W, Cc = SC.DW_CAP_SHAPE
    Ho, Wo = SC.out_size(H), SC.out_size(W)
    assert SC.dw_wgrad_grid(SC.DW_CAP_SHAPE) == (32, 32, 521)
    ldx, lddy = Cc + 8, Cc + 16
    nan = torch.full((1, 1), float("nan"))                            # a slice that is not uploaded below poisons the result
    xb, dyb = Buf(B * H * W, Cc, ldx, adt(), data=nan.expand(B * H * W, Cc)), Buf(B * Ho * Wo, Cc, lddy, adt(), data=nan.expand(B * Ho * Wo, Cc))
    pre, refs, mags = [], [], []
    for s in range(Cc // SC.DW_CAP_SLICE):
        c = SC.dw_cap_slice(adt(), s)
        cols = slice(s * SC.DW_CAP_SLICE, (s + 1) * SC.DW_CAP_SLICE)
        xb.full[helpers.GR:helpers.GR + xb.rows, cols] = c["x"].reshape(-1, SC.DW_CAP_SLICE).to(DEV)
        dyb.full[helpers.GR:helpers.GR + dyb.rows, cols] = c["dy"].reshape(-1, SC.DW_CAP_SLICE).to(DEV)
        pre.append(c["pre"]), refs.append(c["ref"]), mags.append(c["mag"])
    dwb = acc_buf(torch.cat(pre, 1), 10, Cc)
    check(lib.fx_dwconv3x3s2_bwd_nhwc_bf16(dyb.ptr, lddy, xb.ptr, ldx, None, None, 0, dwb.ptr, B, H, W, Cc, stream()), "fx_dwconv3x3s2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    measured("dw_wgrad", "split cap", acc_get(dwb, 9, Cc), torch.cat(refs, 1), torch.cat(mags, 1), F32, SC.dw_wgrad_ceiling(SC.DW_CAP_SHAPE))


def test_dwconv_second_trips(lib):
    """Both forward entry points (element and fp32 output: each has its own capped launch, and the fp32 store is two 16-byte stores) and the
    dgrad past the grid cap: C = 2048, 181 x 181 -> 91 x 91.  Forward: 8281 output pixels x 256 groups of eight; the first
    second-trip group is output pixel 8192 = (row 90, column 2), so output rows 89 and 90 are compared in full.  dgrad: 32761 input
    pixels; input pixel 8192 = (row 45, column 47) starts the second trips and the last two input rows are fourth trips: rows 45, 179
    and 180 are compared in full.  The inputs are generated on the device; only the rows those outputs read come back (input rows 176 ..
    180 and dy rows 22, 23, 88 .. 90), and the reference is computed on these windows, which start on an even input row so that the
    windows' own outputs keep their alignment (pinned in the CPU test).  Derived gates of the forward and the dgrad."""
    B, H, W, Cc = SC.DW_TRIP_SHAPE
    Ho, Wo = SC.out_size(H), SC.out_size(W)
    g = torch.Generator(device=DEV).manual_seed(181)
    ldx, ldy = Cc + 8, Cc + 16
    xb = Buf(H * W, Cc, ldx, adt(), data=torch.randn(H * W, Cc, device=DEV, generator=g))
    dyb = Buf(Ho * Wo, Cc, ldy, adt(), data=torch.randn(Ho * Wo, Cc, device=DEV, generator=g))
    c = SC.dw_case((1, 1, 1, Cc), adt())
    wd, bd = c["w9"].to(DEV), c["bias"].to(DEV)
    yb, dxb, yfb = Buf(Ho * Wo, Cc, ldy, adt()), Buf(H * W, Cc, ldx, adt()), Buf(Ho * Wo, Cc, Cc + 8, F32)
    check(lib.fx_dwconv3x3s2_nhwc_bf16(xb.ptr, ldx, wd.data_ptr(), bd.data_ptr(), yb.ptr, ldy, B, H, W, Cc, stream()), "fx_dwconv3x3s2_nhwc_bf16")
    check(lib.fx_dwconv3x3s2_nhwc_f32out(xb.ptr, ldx, wd.data_ptr(), bd.data_ptr(), yfb.ptr, Cc + 8, B, H, W, Cc, stream()), "fx_dwconv3x3s2_nhwc_f32out")
    check(lib.fx_dwconv3x3s2_bwd_nhwc_bf16(dyb.ptr, ldy, None, 0, wd.data_ptr(), dxb.ptr, ldx, None, B, H, W, Cc, stream()), "fx_dwconv3x3s2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    yfb.assert_guards()
    dxb.assert_guards()
    x_tail = xb.full[helpers.GR + 176 * W:helpers.GR + H * W, :Cc].cpu().float().reshape(1, 5, W, Cc)
    ref, mag = SC.dw_fwd64(x_tail, c["w9"], c["bias"])
    got = yb.full[helpers.GR + 89 * Wo:helpers.GR + 91 * Wo, :Cc].cpu().reshape(1, 2, Wo, Cc)
    derived("dwconv.elem", "second trip, output rows 89, 90", got, ref[:, 1:], mag[:, 1:], adt(), 10)
    got = yfb.full[helpers.GR + 89 * Wo:helpers.GR + 91 * Wo, :Cc].cpu().reshape(1, 2, Wo, Cc)
    derived("dwconv.f32out", "second trip, output rows 89, 90", got, ref[:, 1:], mag[:, 1:], F32, 10, extra=0.0)

    def dy_rows(lo, hi):
        return dyb.full[helpers.GR + lo * Wo:helpers.GR + hi * Wo, :Cc].cpu().float().reshape(1, hi - lo, Wo, Cc)

    def dx_rows(lo, hi):
        return dxb.full[helpers.GR + lo * W:helpers.GR + hi * W, :Cc].cpu().reshape(1, hi - lo, W, Cc)

    ref, mag = SC.dw_dgrad64(dy_rows(22, 24), c["w9"], 3, W)                     # input rows 44, 45, 46
    derived("dwconv.dgrad", "second trip, input row 45", dx_rows(45, 46), ref[:, 1:2], mag[:, 1:2], adt(), 4)
    ref, mag = SC.dw_dgrad64(dy_rows(88, 91), c["w9"], 5, W)                     # input rows 176 .. 180
    derived("dwconv.dgrad", "fourth trip, input rows 179, 180", dx_rows(179, 181), ref[:, 3:], mag[:, 3:], adt(), 4)


# ------------------------------------------------------------------------------------------------ 3. global mean
@pytest.mark.parametrize("case", SC.GM_CASES, ids=lambda c: f"P{c[0]}-C{c[1]}")
def test_global_mean(lib, case):
    """fx_global_mean_nhwc_bf16 vs the fp64 mean, B = 2, ldx = C + 8, ldo = C + 3.  P around 128 (one pixel per lane), around 512 (one
    unrolled round), 896 / 897 (one round and all three tail steps: for lane 0 at 896, for lanes 1 .. 127 at 897), 1600 (production);
    C = 8 (one lane group), 64, 72 and 520 (a partial 64-channel group).  Measured c on mag = mean|x|, ceiling
    (ceil(ceil(P / 128) / 4) + 2 + 128 + 1) * 2^-24: a lane accumulator's sequential additions, the fold of the four accumulators, the
    128 lanes in order, the division.  Run twice, identical bits.
    Measured c: 3.22e-08 (gate 1.29e-07), at P = 1600, C = 72 fp16; the smallest ceiling (P = 1) is 132 * 2^-24 = 7.87e-06."""
    P, Cc = case
    c = SC.global_mean_case(P, Cc, adt())
    ldx, ldo = Cc + 8, Cc + 3
    xb = Buf(SC.GM_B * P, Cc, ldx, adt(), data=c["x"])
    outs = []
    for _ in range(2):
        ob = Buf(SC.GM_B, Cc, ldo, F32)
        check(lib.fx_global_mean_nhwc_bf16(xb.ptr, ldx, ob.ptr, ldo, SC.GM_B, P, Cc, stream()), "fx_global_mean_nhwc_bf16")
        torch.cuda.synchronize()
        ob.assert_guards()
        outs.append(ob.get())
    assert same_bits(outs[0], outs[1]), "two runs differ"
    measured("global_mean", f"P{P} C{Cc}", outs[0], c["ref"], c["mag"], F32, SC.gm_ceiling(P))


# ------------------------------------------------------------------------------------------------ 4. pooled linear
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", SC.PL_ACTS, ids=["none", "relu", "sigmoid"])
@pytest.mark.parametrize("case", SC.PL_CASES, ids=lambda c: f"N{c[0]}-C{c[1]}")
def test_pooled_linear(lib32, case, act, with_bias):
    """fx_pooled_linear_f32 vs fp64 F.linear semantics, B = 3, ldi = C + 1, ldo = N + 1: N on both sides of the 16 output rows of a
    workgroup (the n_end clamp) and C on both sides of the 64 lanes.  none / relu: measured c on mag = sum|W||in| + |bias|, ceiling
    (ceil(C / 64) + 6 + 1) * 2^-24: a lane's fused multiply-adds, the butterfly, the bias.  sigmoid: the linear part's gate times the
    slope bound 1/4, plus the measured term of 1 / (1 + __expf(-s)) on sig_mag = ref * (1 + (1 - ref) * (1 + |s|)) (see
    seg_head_cases.pooled_linear_case); with pre-activations of +-30 and +-95 planted through the bias the output must be finite and
    inside the gate at 1 or 0 (__expf(95) overflows to inf -> exactly 0; RND's floor of 2^-126 covers the 5e-42 of the reference).
    Measured c: linear 5.09e-08 (gate 2.03e-07), at N = 150, C = 65 with ReLU and bias; the smallest ceiling (C = 1 .. 64) is 8 * 2^-24 =
    4.77e-07.  Sigmoid term: measured as what the output needs on sig_mag beyond one fp32 rounding and the linear term at its RECORDED
    size (recorded * mag / 4, no margin - next to the margined term it would read 0 and leave the intrinsic no margin at all): 2.62e-09,
    at N = 19, C = 1 without bias, below act_fwd's 1.4e-08 for the same __expf.  The gate margins both: RND + 4 * linear * mag / 4 +
    4 * 2.62e-09 * sig_mag."""
    N, Cc = case
    c = SC.pooled_linear_case(N, Cc, act, with_bias)
    ldi, ldo = Cc + 1, N + 1
    ib, ob = Buf(SC.PL_B, Cc, ldi, F32, data=c["in"]), Buf(SC.PL_B, N, ldo, F32)
    wb = Buf(N, Cc, Cc, F32, data=c["W"])
    bb = Buf(1, N, N + 3, F32, data=c["bias"]) if with_bias else None
    check(lib32.fx_pooled_linear_f32(ib.ptr, ldi, wb.ptr, bb.ptr if with_bias else None, act, ob.ptr, ldo, SC.PL_B, Cc, N, stream()), "fx_pooled_linear_f32")
    torch.cuda.synchronize()
    ob.assert_guards()
    got = ob.get()
    what = f"N{N} C{Cc} act{act} {'bias' if with_bias else 'nobias'}"
    if act != 4:
        measured("pooled_linear", what, got, c["ref"], c["mag"], F32, SC.pl_ceiling(Cc))
        return
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all()) and bool((got <= 1).all())
    assert MEASURED["pooled_linear"] <= SC.pl_ceiling(Cc)
    lin = MEASURED["pooled_linear"] * 0.25 * c["mag"]
    c_sig = needed_c(got, c["ref"], c["sig_mag"], F32, extra=helpers.rnd(c["ref"], F32) + lin)       # measured next to the UNMARGINED linear term
    print(f"EXCESS pooled_linear.sigmoid {c_sig:.3e} {what}")
    assert MEASURED["pooled_linear.sigmoid"] <= 10 * ACT_FWD_C, "an order of magnitude above the yardstick: explain it first"
    c_gate = needed_c(got, c["ref"], c["sig_mag"], F32, extra=helpers.rnd(c["ref"], F32) + MARGIN * lin)
    allowed = MARGIN * MEASURED["pooled_linear.sigmoid"]
    assert c_gate <= allowed, f"pooled_linear.sigmoid {what}: needs c = {c_gate:.3e} beyond the linear allowance, gate {allowed:.3e}"
    if with_bias:
        for n, target in zip(SC.pl_planted_rows(N), SC.PL_PLANTED):
            assert abs(float(got[0, n]) - (1.0 if target > 0 else 0.0)) <= 1e-12, (n, target, float(got[0, n]))


# ------------------------------------------------------------------------------------------------ 5. channel gate
def cg_run(lib, c, shape, combo, first_row=0):
    B, P, Cc = shape
    sa, uv, um = combo
    ldx, ldg, ldv, ldm, ldy = Cc + 8, Cc + 1, Cc + 3, Cc + 16, Cc + 24
    xb, gb = Buf(B * P, Cc, ldx, adt(), data=c["x"]), Buf(B, Cc, ldg, F32, data=c["gate"])
    vb, mb = Buf(B, Cc, ldv, F32, data=c["add_vec"]), Buf(B * P, Cc, ldm, adt(), data=c["add_map"])
    yb = Buf(B * P, Cc, ldy, adt())
    check(lib.fx_channel_gate_nhwc_bf16(xb.ptr, ldx, gb.ptr, ldg, sa, vb.ptr if uv else None, ldv if uv else 0, mb.ptr if um else None,
                                        ldm if um else 0, yb.ptr, ldy, B, P, Cc, stream()), "fx_channel_gate_nhwc_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    return yb.get().reshape(B, P, Cc)[:, first_row:]


@pytest.mark.parametrize("combo", SC.CG_COMBOS, ids=lambda c: f"self{c[0]}-vec{c[1]}-map{c[2]}")
def test_channel_gate(lib, combo):
    """fx_channel_gate_nhwc_bf16 with every combination of self_add, add_vec and add_map, (B, P, C) = (3, 77, 72), five distinct leading
    dimensions; an operand that is not used is passed as NULL with ld 0.  x * g, + x, + add_vec, + add_map is at most 4 fp32
    operations (contracted or not), then one rounding: c = 4 * 2^-24 on mag = |x||g| + |x| + |add_vec| + |add_map|."""
    c = SC.channel_gate_case(SC.CG_SHAPE, adt())
    ref, mag = SC.channel_gate_ref(c, *combo)
    derived("channel_gate", f"self{combo[0]} vec{combo[1]} map{combo[2]}", cg_run(lib, c, SC.CG_SHAPE, combo), ref, mag, adt(), SC.CG_OPS)


def test_channel_gate_second_trip(lib):
    """(1, 8200, 2048): 2 099 200 groups of eight > 2 097 152 threads; rows 8192 .. 8199 are second trips.  Those and row 8191 are compared
    in full, with all three additions on; derived gate of the channel gate."""
    first = SC.first_second_trip_row(SC.CAP_SHAPE[2]) - 1
    c = SC.channel_gate_case(SC.CAP_SHAPE, adt())
    ref, mag = SC.channel_gate_ref(c, 1, 1, 1, first_row=first)
    got = cg_run(lib, c, SC.CAP_SHAPE, (1, 1, 1), first_row=first)
    assert got.shape[1] == 9
    derived("channel_gate", "second trip", got, ref, mag, adt(), SC.CG_OPS)


# ------------------------------------------------------------------------------------------------ 6. row dot
@pytest.mark.parametrize("second", [True, False], ids=["a.b", "a"])
@pytest.mark.parametrize("shape", SC.RD_SHAPES, ids=sid)
def test_rowdot(lib, shape, second):
    """fx_rowdot_nhwc_bf16 with and without the second operand, scale 0.5, lda = C + 8, ldb = C + 16, ldo = C + 3, splits 1, 5, 7 and
    P + 3 (more ranges than pixels).  One split REPLACES the output (a sentinel-filled Buf: every sentinel of the logical region must be
    gone and every other kept; run twice, identical bits); more splits ADD to a non-zero prefill in a region of 1.0s.  Measured c on
    mag = 0.5 * sum|a||b| + |prefill|, ceiling (ceil(per / 32) + 32 + splits + 1) * 2^-24.
    Measured c: 1.64e-07 (gate 6.57e-07), at 3 x 1000 x 72 with both operands and 1003 splits, fp16 (the atomics' order varies: 1.2e-07
    in another run); the smallest ceiling (P = 5, one split) is 35 * 2^-24 = 2.09e-06."""
    B, P, Cc = shape
    c = SC.rowdot_case(shape, adt())
    lda, ldb, ldo = Cc + 8, Cc + 16, Cc + 3
    ab, bb = Buf(B * P, Cc, lda, adt(), data=c["a"]), Buf(B * P, Cc, ldb, adt(), data=c["b"])

    def call(out_ptr, splits):
        check(lib.fx_rowdot_nhwc_bf16(ab.ptr, lda, bb.ptr if second else None, ldb if second else 0, SC.RD_SCALE, out_ptr, ldo, B, P, Cc, splits, stream()),
              "fx_rowdot_nhwc_bf16")
        torch.cuda.synchronize()

    for splits in SC.rd_splits(P):
        ref, mag = SC.rowdot_ref(c, second, splits)
        what = f"{sid(shape)} {'a.b' if second else 'a'} splits{splits}"
        if splits == 1:
            outs = []
            for _ in range(2):
                ob = Buf(B, Cc, ldo, F32)
                call(ob.ptr, 1)
                ob.assert_guards()
                outs.append(ob.get())
            assert same_bits(outs[0], outs[1]), "two runs differ"
            got = outs[0]
        else:
            ob = acc_buf(c["pre"], B, ldo)
            call(ob.ptr, splits)
            got = acc_get(ob, B, Cc)
        measured("rowdot", what, got, ref, mag, F32, SC.rd_ceiling(P, splits))


# ------------------------------------------------------------------------------------------------ 7. exact: vector broadcast, planes to rows
@pytest.mark.parametrize("shape", SC.BC_SHAPES, ids=sid)
def test_bcast_vec(lib, shape):
    """fx_bcast_vec_nhwc_bf16, ldv = C + 3, ldy = C + 8: every row of an image is the single rounding of vec * scale, bit for bit (the
    CPU test shows that rounding through fp32 changes nothing for these values).  (1, 8200, 2048) is past the grid cap: rows 8192 on are
    second trips, and all 8200 rows are compared.  Run twice, identical bits."""
    B, P, Cc = shape
    c = SC.bcast_case(shape, adt())
    ldv, ldy = Cc + 3, Cc + 8
    vb = Buf(B, Cc, ldv, F32, data=c["vec"])
    outs = []
    for _ in range(2):
        yb = Buf(B * P, Cc, ldy, adt())
        check(lib.fx_bcast_vec_nhwc_bf16(vb.ptr, ldv, c["scale"], yb.ptr, ldy, B, P, Cc, stream()), "fx_bcast_vec_nhwc_bf16")
        torch.cuda.synchronize()
        yb.assert_guards()
        outs.append(yb.get())
    assert same_bits(outs[0], outs[1]), "two runs differ"
    got = outs[0].reshape(B, P, Cc)
    want = c["ref"].to(adt())
    assert torch.equal(want.double(), c["ref"])
    if P > SC.first_second_trip_row(Cc):
        assert same_bits(got[:, SC.first_second_trip_row(Cc):], want[:, None].expand(B, P, Cc)[:, SC.first_second_trip_row(Cc):].contiguous()), "second trip"
    assert same_bits(got, want[:, None].expand(B, P, Cc).contiguous())


@pytest.mark.parametrize("P", SC.PR_P)
@pytest.mark.parametrize("qqp", SC.PR_QQP, ids=lambda q: f"Q{q[0]}-Qp{q[1]}")
def test_planes_to_rows(lib, qqp, P):
    """fx_planes_to_rows_bf16, B = 2, ld_rows = Qp + 8: rows[b][p][q] is the single rounding of planes[b][q][p], bit for bit; the padding
    columns Q .. Qp are +0 and the columns Qp .. ld_rows keep the sentinel.  P on both sides of the 64-pixel tile, Qp up to the 240 whose
    62 400 bytes of dynamic LDS are the most the entry point takes.  Run twice, identical bits."""
    Q, Qp = qqp
    c = SC.planes_case(Q, Qp, P, adt())
    ld = Qp + 8
    pb = Buf(SC.PR_B * Q, P, P, F32, data=c["planes"])
    outs = []
    for _ in range(2):
        rb = Buf(SC.PR_B * P, Qp, ld, adt())
        check(lib.fx_planes_to_rows_bf16(pb.ptr, Q, P, rb.ptr, ld, Qp, SC.PR_B, stream()), "fx_planes_to_rows_bf16")
        torch.cuda.synchronize()
        rb.assert_guards()
        outs.append(rb.get())
    assert same_bits(outs[0], outs[1]), "two runs differ"
    want = c["ref"].to(adt())
    assert torch.equal(want.double(), c["ref"])
    assert same_bits(outs[0].reshape(SC.PR_B, P, Qp), want)
    assert bool((_bits(outs[0])[:, Q:] == 0).all()), "a padding column is not +0"


# ------------------------------------------------------------------------------------------------ 8. nearest upsample + add, adjoint
def up_run(lib, c):
    B, H, W, Cc = c["lat"].shape
    Hs, Ws = c["top"].shape[1:3]
    ldl, ldt, ldo = Cc + 8, Cc + 16, Cc + 24
    lb, tb, dyb = rows_buf(c["lat"], ldl), rows_buf(c["top"], ldt), rows_buf(c["dy"], ldl)
    adds, bwds = [], []
    for _ in range(2):
        ob, db = Buf(B * H * W, Cc, ldo, adt()), Buf(B * Hs * Ws, Cc, ldt, adt())
        check(lib.fx_upsample_nearest_add_nhwc_bf16(lb.ptr, ldl, tb.ptr, ldt, ob.ptr, ldo, B, H, W, Hs, Ws, Cc, stream()), "fx_upsample_nearest_add_nhwc_bf16")
        check(lib.fx_upsample_nearest_bwd_nhwc_bf16(dyb.ptr, ldl, db.ptr, ldt, B, H, W, Hs, Ws, Cc, stream()), "fx_upsample_nearest_bwd_nhwc_bf16")
        torch.cuda.synchronize()
        ob.assert_guards()
        db.assert_guards()
        adds.append(ob.get()), bwds.append(db.get())
    assert same_bits(adds[0], adds[1]) and same_bits(bwds[0], bwds[1]), "two runs differ"
    return adds[0].reshape(B, H, W, Cc), bwds[0].reshape(B, Hs, Ws, Cc)


def up_check(lib, c, what, ops):
    got, dgot = up_run(lib, c)
    ref, mag = SC.upsample_add_ref(c)
    derived("upsample_add", what, got, ref, mag, adt(), 1)
    bref, bmag = SC.upsample_bwd_ref(c)
    derived("upsample_bwd", what, dgot, bref, bmag, adt(), ops)
    # <up(t), dy> == <t, bwd(dy)>, with the kernel's own bwd(dy): off by at most the sum of |t| times the per-element gate
    H, W = c["lat"].shape[1:3]
    t = c["top"].double()
    lhs = float((SC.up64(c["top"], (H, W)) * c["dy"].double()).sum())
    rhs = float((t * dgot.double()).sum())
    bound = float((t.abs() * (helpers.rnd(bref, adt()) + ops * U32 * bmag)).sum())
    print(f"ADJOINT {what} {tag()} |lhs - rhs| = {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("pair", SC.UP_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_upsample_nearest_add_and_adjoint(lib, pair):
    """fx_upsample_nearest_add_nhwc_bf16 and fx_upsample_nearest_bwd_nhwc_bf16 at the identity, exact x2, 2 Hs - 1, 14 -> 20, (5, 7) ->
    (13, 9) and (14, 26) -> (46, 44), where ATen's fp32 index rule and the integer floor disagree (CPU test); B = 2, C = 72, three
    distinct leading dimensions.
    Forward: one fp32 addition, one rounding: c = 1 * 2^-24 on mag = |lateral| + |top|.  Adjoint vs the fp64 transpose of the index map
    (= autograd of F.interpolate, CPU test): a source pixel sums the output pixels of its pre-image, so c = (largest pre-image of the
    pair) * 2^-24 fp32 additions - 1, 4, 4, 4, 6 and 8 for the six pairs - on mag = bwd(|dy|); and the inner-product identity
    <up(t), dy> == <t, bwd(dy)> in fp64 to the same gate.  Both run twice, identical bits."""
    up_check(lib, SC.upsample_case(pair, adt()), f"{pair[0]}->{pair[1]}", SC.up_max_preimage(pair))


@pytest.mark.parametrize("which", ["add", "bwd"])
def test_upsample_nearest_second_trip(lib, which):
    """B = 1, C = 2048.  add: (46, 46) -> (91, 91), 8281 output pixels; bwd: (91, 91) -> (100, 100), 8281 source pixels: pixel 8192 =
    (row 90, column 2) starts the second trips of the capped grid either way.  Everything is compared (the same gates), the rows from
    89 on also on their own."""
    pair = SC.UP_ADD_TRIP if which == "add" else SC.UP_BWD_TRIP
    c = SC.upsample_case(pair, adt(), B=1, C=SC.UP_TRIP_C)
    got, dgot = up_run(lib, c)
    if which == "add":
        ref, mag = SC.upsample_add_ref(c)
        derived("upsample_add", "second trip rows", got[:, 89:], ref[:, 89:], mag[:, 89:], adt(), 1)
        derived("upsample_add", "second trip case", got, ref, mag, adt(), 1)
    else:
        ref, mag = SC.upsample_bwd_ref(c)
        derived("upsample_bwd", "second trip rows", dgot[:, 89:], ref[:, 89:], mag[:, 89:], adt(), SC.up_max_preimage(pair))
        derived("upsample_bwd", "second trip case", dgot, ref, mag, adt(), SC.up_max_preimage(pair))


# ------------------------------------------------------------------------------------------------ 9. refusals
def run_refusals(name, call, bad, outs):
    """Every call of `bad` (name -> keyword overrides of a valid call) must return the invalid-argument code without touching an output;
    the valid call is then accepted."""
    for what, kw in bad.items():
        refused(call(**kw), f"{name}: {what}")
    untouched(*outs)
    check(call(), f"{name}: valid call")
    torch.cuda.synchronize()
    for b in outs:
        b.assert_guards()


def test_dwconv_forward_refusals(lib):
    """C % 8, ld < C, ld % 8, misaligned x / y / w, NULL x / w / y - for both forward entry points."""
    B, H, W, Cc = 1, 5, 5, 16
    c = SC.dw_case((B, H, W, Cc), adt())
    xb, wb = rows_buf(c["x"], 24), Buf(9, Cc, Cc, F32, data=c["w9"])
    for fn, odt in ((lib.fx_dwconv3x3s2_nhwc_bf16, adt()), (lib.fx_dwconv3x3s2_nhwc_f32out, F32)):
        yb = Buf(9, Cc, 24, odt)

        def call(x=xb.ptr, ldx=24, w=wb.ptr, y=yb.ptr, ldy=24, Cc=Cc):
            return fn(x, ldx, w, None, y, ldy, B, H, W, Cc, stream())

        bad = {"C % 8": {"Cc": 12}, "ldx < C": {"ldx": 8}, "ldy < C": {"ldy": 8}, "ldx % 8": {"ldx": 20}, "ldy % 8": {"ldy": 20},
               "x misaligned": {"x": xb.ptr + 2}, "y misaligned": {"y": yb.ptr + 4}, "w misaligned": {"w": wb.ptr + 4},
               "x NULL": {"x": None}, "w NULL": {"w": None}, "y NULL": {"y": None}}
        run_refusals("fx_dwconv3x3s2", call, bad, [yb])


def test_dwconv_backward_refusals(lib):
    """dy: NULL, lddy < C, lddy % 8, misaligned, C % 8; dx asked without w, with lddx < C, lddx % 8, misaligned; dw asked without x, with
    ldx < C, ldx % 8, misaligned x."""
    B, H, W, Cc = 1, 5, 5, 16
    c = SC.dw_case((B, H, W, Cc), adt())
    xb, dyb, wb = rows_buf(c["x"], 24), rows_buf(c["dy"], 24), Buf(9, Cc, Cc, F32, data=c["w9"])
    dxb, dwb = Buf(25, Cc, 24, adt()), Buf(9, Cc, Cc, F32)

    def call(dy=dyb.ptr, lddy=24, x=xb.ptr, ldx=24, w=wb.ptr, dx=dxb.ptr, lddx=24, dw=None, Cc=Cc):
        return lib.fx_dwconv3x3s2_bwd_nhwc_bf16(dy, lddy, x, ldx, w, dx, lddx, dw, B, H, W, Cc, stream())

    bad = {"dy NULL": {"dy": None}, "lddy < C": {"lddy": 8}, "lddy % 8": {"lddy": 20}, "dy misaligned": {"dy": dyb.ptr + 2}, "C % 8": {"Cc": 12},
           "dx without w": {"w": None}, "lddx < C": {"lddx": 8}, "lddx % 8": {"lddx": 20}, "dx misaligned": {"dx": dxb.ptr + 2},
           "dw without x": {"dw": dwb.ptr, "x": None}, "ldx < C": {"dw": dwb.ptr, "ldx": 8}, "ldx % 8": {"dw": dwb.ptr, "ldx": 20},
           "x misaligned": {"dw": dwb.ptr, "x": xb.ptr + 2}}
    run_refusals("fx_dwconv3x3s2_bwd_nhwc_bf16", call, bad, [dxb])
    untouched(dwb)


def test_global_mean_and_pooled_linear_refusals(lib):
    """global mean: C % 8, ldx < C, ldx % 8, ldo < C, misaligned x, NULL x / out.  pooled linear: ldi < C, ldo < N, NULL in / W / out, an
    unknown act (2 = SiLU and 3 = GELU are activations of the library, not of this entry point)."""
    B, P, Cc = 2, 9, 16
    c = SC.global_mean_case(P, Cc, adt())
    xb = Buf(B * P, Cc, 24, adt(), data=c["x"][:, :, :Cc])
    ob = Buf(B, Cc, 19, F32)

    def call(x=xb.ptr, ldx=24, out=ob.ptr, ldo=19, Cc=Cc):
        return lib.fx_global_mean_nhwc_bf16(x, ldx, out, ldo, B, P, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "ldx < C": {"ldx": 8}, "ldx % 8": {"ldx": 20}, "ldo < C": {"ldo": 15}, "x misaligned": {"x": xb.ptr + 2},
           "x NULL": {"x": None}, "out NULL": {"out": None}}
    run_refusals("fx_global_mean_nhwc_bf16", call, bad, [ob])

    N = 5
    p = SC.pooled_linear_case(N, Cc, 0, False)
    ib, wb, lb = Buf(SC.PL_B, Cc, 17, F32, data=p["in"]), Buf(N, Cc, Cc, F32, data=p["W"]), Buf(SC.PL_B, N, 6, F32)

    def call_pl(inp=ib.ptr, ldi=17, w=wb.ptr, act=0, out=lb.ptr, ldo=6):
        return lib.fx_pooled_linear_f32(inp, ldi, w, None, act, out, ldo, SC.PL_B, Cc, N, stream())

    bad = {"ldi < C": {"ldi": 15}, "ldo < N": {"ldo": 4}, "in NULL": {"inp": None}, "W NULL": {"w": None}, "out NULL": {"out": None},
           "act 2": {"act": 2}, "act 3": {"act": 3}, "act 5": {"act": 5}, "act -1": {"act": -1}}
    run_refusals("fx_pooled_linear_f32", call_pl, bad, [lb])


def test_channel_gate_refusals(lib):
    """C % 8, each of the five leading dimensions below C, each 16-bit one no multiple of 8, NULL x / gate / y.  ldv and ldm count only with
    their operand: without it any value is accepted."""
    shape = (2, 5, 16)
    B, P, Cc = shape
    c = SC.channel_gate_case(shape, adt())
    xb, gb = Buf(B * P, Cc, 24, adt(), data=c["x"]), Buf(B, Cc, 17, F32, data=c["gate"])
    vb, mb = Buf(B, Cc, 19, F32, data=c["add_vec"]), Buf(B * P, Cc, 32, adt(), data=c["add_map"])
    yb = Buf(B * P, Cc, 40, adt())

    def call(x=xb.ptr, ldx=24, g=gb.ptr, ldg=17, v=vb.ptr, ldv=19, m=mb.ptr, ldm=32, y=yb.ptr, ldy=40, Cc=Cc):
        return lib.fx_channel_gate_nhwc_bf16(x, ldx, g, ldg, 1, v, ldv, m, ldm, y, ldy, B, P, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "ldx < C": {"ldx": 8}, "ldy < C": {"ldy": 8}, "ldg < C": {"ldg": 15}, "ldv < C": {"ldv": 15}, "ldm < C": {"ldm": 8},
           "ldx % 8": {"ldx": 20}, "ldy % 8": {"ldy": 20}, "ldm % 8": {"ldm": 20}, "x NULL": {"x": None}, "gate NULL": {"g": None}, "y NULL": {"y": None}}
    run_refusals("fx_channel_gate_nhwc_bf16", call, bad, [yb])
    check(call(v=None, ldv=0, m=None, ldm=3), "unused leading dimensions")
    torch.cuda.synchronize()
    yb.assert_guards()


def test_rowdot_bcast_planes_refusals(lib):
    """row dot: C % 8, lda < C, lda % 8, ldo < C, misaligned a, NULL a / out, ldb < C, ldb % 8, misaligned b, splits 0 and 1025.
    broadcast: C % 8, ldv < C, ldy < C, ldy % 8, misaligned y, NULL vec / y.  planes to rows: Qp < Q, Qp % 8, Qp > 240, ld_rows < Qp,
    ld_rows % 8, misaligned rows, NULL planes / rows."""
    shape = (2, 9, 16)
    B, P, Cc = shape
    c = SC.rowdot_case(shape, adt())
    ab, bb, ob = Buf(B * P, Cc, 24, adt(), data=c["a"]), Buf(B * P, Cc, 32, adt(), data=c["b"]), Buf(B, Cc, 19, F32)

    def call(a=ab.ptr, lda=24, b=bb.ptr, ldb=32, out=ob.ptr, ldo=19, Cc=Cc, splits=1):
        return lib.fx_rowdot_nhwc_bf16(a, lda, b, ldb, 0.5, out, ldo, B, P, Cc, splits, stream())

    bad = {"C % 8": {"Cc": 12}, "lda < C": {"lda": 8}, "lda % 8": {"lda": 20}, "ldo < C": {"ldo": 15}, "a misaligned": {"a": ab.ptr + 2},
           "a NULL": {"a": None}, "out NULL": {"out": None}, "ldb < C": {"ldb": 8}, "ldb % 8": {"ldb": 20}, "b misaligned": {"b": bb.ptr + 2},
           "splits 0": {"splits": 0}, "splits 1025": {"splits": 1025}}
    run_refusals("fx_rowdot_nhwc_bf16", call, bad, [ob])

    vb, yb = Buf(B, Cc, 19, F32, data=c["pre"]), Buf(B * P, Cc, 24, adt())

    def call_bc(vec=vb.ptr, ldv=19, y=yb.ptr, ldy=24, Cc=Cc):
        return lib.fx_bcast_vec_nhwc_bf16(vec, ldv, 0.25, y, ldy, B, P, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "ldv < C": {"ldv": 15}, "ldy < C": {"ldy": 8}, "ldy % 8": {"ldy": 20}, "y misaligned": {"y": yb.ptr + 2},
           "vec NULL": {"vec": None}, "y NULL": {"y": None}}
    run_refusals("fx_bcast_vec_nhwc_bf16", call_bc, bad, [yb])

    Q, Qp, Pp = 10, 16, 9
    p = SC.planes_case(Q, Qp, Pp, adt())
    pb, rb = Buf(SC.PR_B * Q, Pp, Pp, F32, data=p["planes"]), Buf(SC.PR_B * Pp, 248, 256, adt())

    def call_pr(planes=pb.ptr, rows=rb.ptr, ld=256, Qp=Qp):
        return lib.fx_planes_to_rows_bf16(planes, Q, Pp, rows, ld, Qp, SC.PR_B, stream())

    bad = {"Qp < Q": {"Qp": 8}, "Qp % 8": {"Qp": 12}, "Qp > 240": {"Qp": 248}, "ld_rows < Qp": {"ld": 8}, "ld_rows % 8": {"ld": 20},
           "rows misaligned": {"rows": rb.ptr + 2}, "planes NULL": {"planes": None}, "rows NULL": {"rows": None}}
    for what, kw in bad.items():
        refused(call_pr(**kw), f"fx_planes_to_rows_bf16: {what}")
    untouched(rb)
    check(call_pr(), "fx_planes_to_rows_bf16: valid call")
    torch.cuda.synchronize()
    every = _bits(rb.full).cpu().clone()                                # the whole allocation: guard rows, all 256 columns
    stored = every[helpers.GR:helpers.GR + rb.rows, :Qp].clone()
    every[helpers.GR:helpers.GR + rb.rows, :Qp] = rb.sent
    assert bool((every == rb.sent).all()), "the valid call wrote outside its Qp columns"
    assert torch.equal(stored.reshape(SC.PR_B, Pp, Qp), _bits(p["ref"].to(adt())))


def test_upsample_refusals(lib):
    """Both nearest-upsample entry points: C % 8, every leading dimension below C and no multiple of 8, every pointer NULL, a size of 0."""
    pair = ((3, 4), (6, 8))
    c = SC.upsample_case(pair, adt(), B=1, C=16)
    lb, tb, dyb = rows_buf(c["lat"], 24), rows_buf(c["top"], 32), rows_buf(c["dy"], 24)
    ob, db = Buf(48, 16, 40, adt()), Buf(12, 16, 32, adt())

    def call(lat=lb.ptr, ldl=24, top=tb.ptr, ldt=32, out=ob.ptr, ldo=40, Cc=16, Hs=3):
        return lib.fx_upsample_nearest_add_nhwc_bf16(lat, ldl, top, ldt, out, ldo, 1, 6, 8, Hs, 4, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "ldl < C": {"ldl": 8}, "ldt < C": {"ldt": 8}, "ldo < C": {"ldo": 8}, "ldl % 8": {"ldl": 20}, "ldt % 8": {"ldt": 20},
           "ldo % 8": {"ldo": 20}, "lateral NULL": {"lat": None}, "top NULL": {"top": None}, "out NULL": {"out": None}, "Hs 0": {"Hs": 0}}
    run_refusals("fx_upsample_nearest_add_nhwc_bf16", call, bad, [ob])

    def call_b(dy=dyb.ptr, lddy=24, dtop=db.ptr, lddt=32, Cc=16, Hs=3):
        return lib.fx_upsample_nearest_bwd_nhwc_bf16(dy, lddy, dtop, lddt, 1, 6, 8, Hs, 4, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "lddy < C": {"lddy": 8}, "lddt < C": {"lddt": 8}, "lddy % 8": {"lddy": 20}, "lddt % 8": {"lddt": 20},
           "dy NULL": {"dy": None}, "dtop NULL": {"dtop": None}, "Hs 0": {"Hs": 0}}
    run_refusals("fx_upsample_nearest_bwd_nhwc_bf16", call_b, bad, [db])
