"""The kernels of csrc/train_conv_ops.hip that every training step runs around every convolution, called directly through the C ABI on a
real MI355X under BOTH element types (libfocoos_amd.so = bfloat16, libfocoos_amd_fp16.so = IEEE half): train-mode BatchNorm
(fx_bn_stats_bf16, fx_bn_finalize_f32, fx_bn_apply_bf16, fx_bn_bwd_stats_bf16, fx_bn_bwd_apply_bf16), the pooling backward kernels
(fx_maxpool3x3s2_bwd_nhwc_bf16, fx_avgpool2x2_bwd_nhwc_bf16), the weight packers (fx_pack_conv_weights_f32, fx_pack_frag_bf16,
fx_pack_linear_weights_f32, fx_pack_weights_many_f32, fx_pack_entry_blocks) and the weight-gradient unpackers
(fx_unpack_conv_wgrad_f32, fx_unpack_conv_wgrad_sum_f32, fused and with FX_UNPACK_FUSED=0).  Inputs, float64 references and magnitudes
come from tests/train_norm_cases.py, which tests/test_train_norm_cases_cpu.py pins against independent formulations.

Rules every case follows (those of tests/test_gpu_train_token_ops.py)
* Every BatchNorm kernel is tested ON ITS OWN: the per-channel vectors it reads are inputs of the case, not outputs of the kernel before.
* Every activation buffer is a helpers.Buf: guard rows on either side, a leading dimension above its column count and distinct per
  operand, inputs padded with NaN, outputs prefilled with a sentinel that everything outside the written region must keep bit for bit.
  fp32 outputs a kernel ADDS to (sums, dgamma_acc, dbeta_acc) lie in the corner of a region of 1.0s with a non-zero prefill (acc_buf):
  an addition to the 1.5e16 the sentinel reads as leaves no trace.  Weight images lie between 64 sentinel elements and are compared
  over the WHOLE allocation: padding rows and columns must keep the sentinel.
* Exact, bit for bit: the integer runs of the two reductions (every partial sum is an integer multiple of 1/8 below 2^21, so any order
  of the atomics gives the same bits), both pooling backward kernels, every weight image, every unpacked gradient, prefill + sums.
* Otherwise, per element:  |got - ref| <= RND(ref) + c * mag, RND(ref) one rounding to the output type, mag the fp64 value of the same
  expression with every term in absolute value.  MEASURED[kernel.output] is the largest c any case of that output needed on an MI355X
  AGAINST THE FP64 REFERENCE over both element types (printed as EXCESS ...), the gate is MARGIN = 4 times that: the order of the atomics
  and the fast-math intrinsics of the activation gradients vary.  No gate of an n-term fp32 sum (n = rows) exceeds
  n * 2^-24: sum_gate holds each case to min(MARGIN * MEASURED, n * 2^-24) and asserts what the case needs against n * 2^-24.
* ReLU: elements whose fp64 pre-activation lies within 2^-20 of its magnitude of zero are left out of the backward gates (the sign fp32
  gives them is not determined); at most 0.1 % of a case, asserted here and in the CPU test."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FX_ACT, FocoosAmdError, FxPackEntry, check  # noqa: E402
from tests import helpers  # noqa: E402
from tests import train_norm_cases as NC  # noqa: E402
from tests.helpers import GR, ROOT, U32, Buf, _bits, elem_rne, frag_order  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
MARGIN = 4.0
# largest c = (|got - ref| - RND(ref)) / mag over all cases of the output and both element types, measured on an MI355X
MEASURED = {
    "bn_stats.sum": 1.829e-07,
    "bn_stats.sumsq": 3.435e-07,
    "bn_bwd_stats.dbeta": 2.513e-08,
    "bn_bwd_stats.dgamma": 9.388e-08,
    "bn_apply.y": 1.473e-08,
    "bn_bwd_apply.da": 1.901e-08,
    "bn_bwd_apply.dz": 4.318e-08,
    "bn_finalize.mean": 0.0,
    "bn_finalize.rstd": 6.098e-08,
    "bn_finalize.scale": 6.111e-08,
    "bn_finalize.shift": 6.204e-08,
    "bn_finalize.running_mean": 6.750e-08,
    "bn_finalize.running_var": 5.365e-08,
}
SUM_KEYS = ("bn_stats.sum", "bn_stats.sumsq", "bn_bwd_stats.dbeta", "bn_bwd_stats.dgamma")
RES = [False, True]


@pytest.fixture(params=["bf16", "fp16"])
def elem(request):
    prev = _lib.set_compute_dtype(request.param)
    yield request.param
    _lib.set_compute_dtype(prev)


@pytest.fixture
def lib(elem):
    assert torch.cuda.is_available()
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def adt():
    return _lib.act_dtype()


def tag():
    return _lib.compute_dtype()


def sid(s):
    return "x".join(map(str, s))


def gate(key, what, got, ref, mag, dtype, extra=None):
    return helpers.gate(key, what, got, ref, mag, dtype, MEASURED, MARGIN, extra=extra, tag=tag())


def sum_gate(key, what, got, ref, mag, rows, allowance=None):
    """helpers.gate for an n-term fp32 sum (n = rows): MARGIN * MEASURED[key], but never above n * 2^-24 - the small cases are held to
    their own bound, which the largest recorded figure (from a case of a thousand rows) exceeds.  What the case NEEDS is then compared
    with n * 2^-24 once more, from the row count alone."""
    bound = NC.bn_sum_bound(rows)
    capped = {key: min(MEASURED[key], bound / MARGIN)}
    extra = helpers.rnd(ref, F32) + (allowance if allowance is not None else 0.0)
    c = helpers.gate(key, f"{what} (n * 2^-24 = {bound:.3e})", got, ref, mag, F32, capped, MARGIN, extra=extra, tag=tag())
    assert c <= rows * U32, f"{key} {what}: a sum of {rows} terms needs c = {c:.3e} > {rows} * 2^-24"


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


def run_refusals(name, call, bad, outs):
    """Every call of `bad` (name -> keyword overrides of a valid call) must return the invalid-argument code without touching an output;
    the valid call is then accepted."""
    for what, kw in bad.items():
        refused(call(**kw), f"{name}: {what}")
    untouched(*outs)
    check(call(), f"{name}: valid call")
    torch.cuda.synchronize()


NEIGHBOUR = 1.0


def acc_buf(pre, rows, cols):
    """An ACCUMULATED fp32 output as it lies in a flat buffer: `pre` in the corner of a [rows][cols] region whose other elements hold 1.0."""
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


def vec(t):
    """A per-channel fp32 input vector (any number of rows of it, contiguous: sums is [2][C])."""
    n = t.numel()
    return Buf(1, n, n + 8, F32, data=t.reshape(1, n))


def mask_out(got, ref, ex):
    """`got` with the left-out elements set to the reference."""
    got = got.double().clone()
    got[ex] = ref[ex]
    return got


def check_cap(ex):
    assert int(ex.sum()) <= 1e-3 * ex.numel(), f"{int(ex.sum())} of {ex.numel()} ReLU elements left out: above 0.1 %"


# ------------------------------------------------------------------------------------------------ 1. BatchNorm statistics
def bn_bufs(c, z_f32):
    rows, Cc = c["rows"], c["C"]
    ld = {"z": Cc + 8, "dy": Cc + 16, "res": Cc + 24, "y": Cc + 32, "da": Cc + 40, "dz": Cc + 48}
    return ld, Buf(rows, Cc, ld["z"], F32 if z_f32 else adt(), data=c["z"]), Buf(rows, Cc, ld["dy"], adt(), data=c["dy"]), Buf(rows, Cc, ld["res"], adt(), data=c["res"])


@pytest.mark.parametrize("z_f32", [0, 1], ids=["z_elem", "z_f32"])
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=sid)
def test_bn_stats(lib, shape, z_f32):
    """fx_bn_stats_bf16: sums[c] += sum z, sums[C + c] += sum z^2 into a non-zero prefill, ldz = C + 8.  Integer run: bit equality with
    the fp64 sums.  Gaussian and mean-30 runs: measured c on mag = |prefill| + sum|z| (sum z^2), never above rows * 2^-24."""
    rows, Cc = shape
    for kind in ("int",) + NC.BN_KINDS:
        c = NC.bn_case(shape, adt(), kind, bool(z_f32))
        ld, zb, _, _ = bn_bufs(c, z_f32)
        sb = acc_buf(c["pre"].reshape(1, -1), 3, 2 * Cc + 8)
        check(lib.fx_bn_stats_bf16(zb.ptr, ld["z"], z_f32, sb.ptr, rows, Cc, stream()), "fx_bn_stats_bf16")
        torch.cuda.synchronize()
        got = acc_get(sb, 1, 2 * Cc).reshape(2, Cc)
        ref, mag = NC.bn_stats_ref(c)
        if kind == "int":
            assert torch.equal(got.double(), ref), f"integer run {sid(shape)}: {int((got.double() != ref).sum())} sums differ"
        else:
            sum_gate("bn_stats.sum", f"{sid(shape)} {kind} z_f32={z_f32}", got[0], ref[0], mag[0], rows)
            sum_gate("bn_stats.sumsq", f"{sid(shape)} {kind} z_f32={z_f32}", got[1], ref[1], mag[1], rows)


def bwd_stats_run(lib, c, z_f32, act, residual):
    rows, Cc = c["rows"], c["C"]
    ld, zb, dyb, rb = bn_bufs(c, z_f32)
    vs = [vec(c[k]) for k in ("scale", "shift", "mean", "rstd")]
    sb = acc_buf(c["pre"].reshape(1, -1), 3, 2 * Cc + 8)
    check(lib.fx_bn_bwd_stats_bf16(dyb.ptr, ld["dy"], zb.ptr, ld["z"], z_f32, rb.ptr if residual else None, ld["res"] if residual else 0, vs[0].ptr,
                                   vs[1].ptr, vs[2].ptr, vs[3].ptr, FX_ACT[act], sb.ptr, rows, Cc, stream()), "fx_bn_bwd_stats_bf16")
    torch.cuda.synchronize()
    return acc_get(sb, 1, 2 * Cc).reshape(2, Cc)


@pytest.mark.parametrize("z_f32", [0, 1], ids=["z_elem", "z_f32"])
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=sid)
def test_bn_bwd_stats(lib, shape, z_f32):
    """fx_bn_bwd_stats_bf16 with test-chosen scale, shift, mean, rstd: sums[c] += sum da, sums[C + c] += sum da * xhat.  Integer run (none,
    ReLU; power-of-two vectors): bit equality.  Gaussian and mean-30 runs with the four activations, with and without a residual:
    measured c on mag = |prefill| + sum |dy| (|act'| + |a|_mag) (|xhat|), never above rows * 2^-24; the ReLU elements left out
    enter as an allowance of |dy| (|xhat|) each."""
    rows, _ = shape
    for act in ("none", "relu"):
        for residual in RES:
            c = NC.bn_case(shape, adt(), "int", bool(z_f32))
            ref, _, allowance = NC.bn_bwd_stats_ref(c, act, residual)
            got = bwd_stats_run(lib, c, z_f32, act, residual)
            assert torch.equal(got.double(), ref), f"integer run {sid(shape)} {act} res={residual}: {int((got.double() != ref).sum())} sums differ"
    for kind in NC.BN_KINDS:
        c = NC.bn_case(shape, adt(), kind, bool(z_f32))
        for act in NC.ACTS:
            for residual in RES:
                ref, mag, allowance = NC.bn_bwd_stats_ref(c, act, residual)
                check_cap(NC.bn_da64(c, act, residual)[2])
                got = bwd_stats_run(lib, c, z_f32, act, residual)
                what = f"{sid(shape)} {kind} z_f32={z_f32} {act} res={int(residual)}"
                sum_gate("bn_bwd_stats.dbeta", what, got[0], ref[0], mag[0], rows, allowance[0])
                sum_gate("bn_bwd_stats.dgamma", what, got[1], ref[1], mag[1], rows, allowance[1])


def test_sum_records_below_the_bound_of_their_case():
    """Each recorded c of a sum was measured at a case of at least 255 rows and lies below that case's n * 2^-24."""
    at_rows = {"bn_stats.sum": 1024, "bn_stats.sumsq": 1024, "bn_bwd_stats.dbeta": 7, "bn_bwd_stats.dgamma": 255}
    assert set(at_rows) == set(SUM_KEYS)
    for key, rows in at_rows.items():
        assert (rows, ) in [(s[0], ) for s in NC.BN_SHAPES] and MEASURED[key] <= rows * U32, key


# ------------------------------------------------------------------------------------------------ 2. BatchNorm apply, backward apply
def apply_run(lib, c, z_f32, act, residual):
    rows, Cc = c["rows"], c["C"]
    ld, zb, _, rb = bn_bufs(c, z_f32)
    sc, sh = vec(c["scale"]), vec(c["shift"])
    yb = Buf(rows, Cc, ld["y"], adt())
    check(lib.fx_bn_apply_bf16(zb.ptr, ld["z"], z_f32, sc.ptr, sh.ptr, rb.ptr if residual else None, ld["res"] if residual else 0, FX_ACT[act], yb.ptr,
                               ld["y"], rows, Cc, stream()), "fx_bn_apply_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    return yb.get()


@pytest.mark.parametrize("z_f32", [0, 1], ids=["z_elem", "z_f32"])
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=sid)
def test_bn_apply(lib, shape, z_f32):
    """fx_bn_apply_bf16: y = act(z * scale + shift [+ residual]) with test-chosen scale and shift, four activations, with and without a
    residual, Gaussian and mean-30 inputs; measured c on mag = |z scale| + |shift| + |residual| (every activation has slope <= 1.13).
    The ReLU forward is continuous: no element is left out."""
    for kind in NC.BN_KINDS:
        c = NC.bn_case(shape, adt(), kind, bool(z_f32))
        for act in NC.ACTS:
            for residual in RES:
                ref, mag = NC.bn_apply_ref(c, act, residual)
                gate("bn_apply.y", f"{sid(shape)} {kind} z_f32={z_f32} {act} res={int(residual)}", apply_run(lib, c, z_f32, act, residual), ref, mag, adt())


def bwd_apply_run(lib, c, z_f32, act, residual, with_da, with_acc, first_row=0):
    """(da or None, dz, dgamma_acc, dbeta_acc or None)."""
    rows, Cc = c["rows"], c["C"]
    ld, zb, dyb, rb = bn_bufs(c, z_f32)
    vs = [vec(c[k]) for k in ("scale", "shift", "mean", "rstd", "sums")]
    dab, dzb = Buf(rows, Cc, ld["da"], adt()), Buf(rows, Cc, ld["dz"], adt())
    ga, ba = acc_buf(c["acc_pre"][0:1], 3, Cc + 8), acc_buf(c["acc_pre"][1:2], 3, Cc + 8)
    check(lib.fx_bn_bwd_apply_bf16(dyb.ptr, ld["dy"], zb.ptr, ld["z"], z_f32, rb.ptr if residual else None, ld["res"] if residual else 0, vs[0].ptr,
                                   vs[1].ptr, vs[2].ptr, vs[3].ptr, FX_ACT[act], vs[4].ptr, c["inv_n"], dab.ptr if with_da else None,
                                   ld["da"] if with_da else 0, dzb.ptr, ld["dz"], rows, Cc, ga.ptr if with_acc else None, ba.ptr if with_acc else None,
                                   stream()), "fx_bn_bwd_apply_bf16")
    torch.cuda.synchronize()
    dzb.assert_guards()
    if with_da:
        dab.assert_guards()
    else:
        untouched(dab)
    dg, db = acc_get(ga, 1, Cc), acc_get(ba, 1, Cc)
    if not with_acc:
        assert torch.equal(dg, c["acc_pre"][0:1]) and torch.equal(db, c["acc_pre"][1:2])
    return (dab.get() if with_da else None), dzb.get(), (dg[0] if with_acc else None), (db[0] if with_acc else None)


@pytest.mark.parametrize("z_f32", [0, 1], ids=["z_elem", "z_f32"])
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=sid)
def test_bn_bwd_apply(lib, shape, z_f32):
    """fx_bn_bwd_apply_bf16 with test-chosen vectors and GIVEN sums: dz = scale * (da - sums[c] / n - xhat * sums[C + c] / n), da_out NULL
    and present with and without a residual, dgamma_acc / dbeta_acc NULL and present (both alternate over the cases): present, they must hold
    prefill + sums in ONE fp32 addition, bit for bit - also for C > 256, where more than one workgroup runs.  Measured c of dz on
    mag = |scale| (|da|_mag + |sums[c]| / n + |xhat| |sums[C + c]| / n), of da on |dy| (|act'| + |a|_mag)."""
    for ki, kind in enumerate(NC.BN_KINDS):
        c = NC.bn_case(shape, adt(), kind, bool(z_f32))
        for ai, act in enumerate(NC.ACTS):
            for residual in RES:
                # every (act, residual) pair sees da_out and the accumulators NULL and present over the two kinds, in both pairings over the activations
                with_da, with_acc = (ki + int(residual)) % 2 == 0, (ki + ai + int(residual)) % 2 == 0
                da_ref, da_mag, dz_ref, dz_mag, ex = NC.bn_bwd_apply_ref(c, act, residual)
                check_cap(ex)
                da, dz, dg, db = bwd_apply_run(lib, c, z_f32, act, residual, with_da, with_acc)
                what = f"{sid(shape)} {kind} z_f32={z_f32} {act} res={int(residual)}"
                gate("bn_bwd_apply.dz", what, mask_out(dz, dz_ref, ex), dz_ref, dz_mag, adt())
                if with_da:
                    gate("bn_bwd_apply.da", what, mask_out(da, da_ref, ex), da_ref, da_mag, adt())
                if with_acc:
                    assert same_bits(dg, c["acc_pre"][0] + c["sums"][1]), f"{what}: dgamma_acc is not prefill + sums[C + c] in one addition"
                    assert same_bits(db, c["acc_pre"][1] + c["sums"][0]), f"{what}: dbeta_acc is not prefill + sums[c] in one addition"


def cap_bufs(c, names):
    """Device buffers of the 8200 x 2048 case: Gaussian rows generated on the device, the case's rows at the end."""
    rows, Cc = NC.BN_CAP_SHAPE
    tail = c["rows"]
    g = torch.Generator(device=DEV).manual_seed(8200)
    out = []
    for i, k in enumerate(names):
        b = Buf(rows, Cc, Cc + 8 * (i + 1), adt(), data=torch.randn(rows, Cc, device=DEV, generator=g))
        b.full[GR + rows - tail:GR + rows, :Cc] = c[k].to(device=DEV, dtype=adt())
        out.append(b)
    return out


def test_bn_apply_second_trip(lib):
    """fx_bn_apply_bf16 past the grid cap: 8200 x 2048 = 2 099 200 groups of eight > 2 097 152 threads; rows 8192 .. 8199 are second trips.
    Those and row 8191 are gated on their own (SiLU, residual); the gate of bn_apply.y."""
    rows, Cc = NC.BN_CAP_SHAPE
    c = NC.bn_cap_case(adt(), 9)
    assert rows - 9 == NC.first_second_trip_row(Cc) - 1
    zb, rb = cap_bufs(c, ("z", "res"))
    sc, sh = vec(c["scale"]), vec(c["shift"])
    yb = Buf(rows, Cc, Cc + 32, adt())
    check(lib.fx_bn_apply_bf16(zb.ptr, zb.ld, 0, sc.ptr, sh.ptr, rb.ptr, rb.ld, FX_ACT["silu"], yb.ptr, yb.ld, rows, Cc, stream()), "fx_bn_apply_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    ref, mag = NC.bn_apply_ref(c, "silu", True)
    gate("bn_apply.y", "second trip", yb.full[GR + rows - 9:GR + rows, :Cc].cpu(), ref, mag, adt())
    assert bool(torch.isfinite(yb.full[GR:GR + rows, :Cc].float()).all())


def test_bn_bwd_apply_second_trip(lib):
    """fx_bn_bwd_apply_bf16 past the grid cap, the same shape: GELU, residual, da_out and the accumulators present (2048 channels: the
    accumulation must still happen once); rows 8191 .. 8199 gated on their own."""
    rows, Cc = NC.BN_CAP_SHAPE
    c = NC.bn_cap_case(adt(), 9)
    dyb, zb, rb = cap_bufs(c, ("dy", "z", "res"))
    vs = [vec(c[k]) for k in ("scale", "shift", "mean", "rstd", "sums")]
    dab, dzb = Buf(rows, Cc, Cc + 40, adt()), Buf(rows, Cc, Cc + 48, adt())
    ga, ba = acc_buf(c["acc_pre"][0:1], 3, Cc + 8), acc_buf(c["acc_pre"][1:2], 3, Cc + 8)
    check(lib.fx_bn_bwd_apply_bf16(dyb.ptr, dyb.ld, zb.ptr, zb.ld, 0, rb.ptr, rb.ld, vs[0].ptr, vs[1].ptr, vs[2].ptr, vs[3].ptr, FX_ACT["gelu"], vs[4].ptr,
                                   c["inv_n"], dab.ptr, dab.ld, dzb.ptr, dzb.ld, rows, Cc, ga.ptr, ba.ptr, stream()), "fx_bn_bwd_apply_bf16")
    torch.cuda.synchronize()
    dab.assert_guards()
    dzb.assert_guards()
    da_ref, da_mag, dz_ref, dz_mag, _ = NC.bn_bwd_apply_ref(c, "gelu", True)
    gate("bn_bwd_apply.dz", "second trip", dzb.full[GR + rows - 9:GR + rows, :Cc].cpu(), dz_ref, dz_mag, adt())
    gate("bn_bwd_apply.da", "second trip", dab.full[GR + rows - 9:GR + rows, :Cc].cpu(), da_ref, da_mag, adt())
    assert same_bits(acc_get(ga, 1, Cc)[0], c["acc_pre"][0] + c["sums"][1]) and same_bits(acc_get(ba, 1, Cc)[0], c["acc_pre"][1] + c["sums"][0])


# ------------------------------------------------------------------------------------------------ 3. BatchNorm finalize
SENT64 = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("form", ["full", "no_running", "no_nbt"])
@pytest.mark.parametrize("n", NC.FIN_N)
@pytest.mark.parametrize("Cc", NC.FIN_C)
def test_bn_finalize(lib, Cc, n, form):
    """fx_bn_finalize_f32 (fp32 throughout: one library's result is the other's) at C = 8, 264, 520 (one and three workgroups) and
    n = 1, 2, 297, 1 638 400 with the planted channels: variance exactly 0, variance negative before the clamp (rstd must be finite and
    1 / sqrt(eps)), variance 10^4.  mean, rstd, scale, shift, the running statistics (momentum 0.1, unbiased factor n / (n - 1), 1 at
    n = 1) vs the fp64 reference, measured c; num_batches_tracked rises by exactly 1 whatever the number of workgroups; the NULL
    running-statistics form and the NULL num_batches_tracked form leave what they do not have untouched."""
    c = NC.finalize_case(Cc, n)
    ref = NC.finalize_ref(c)
    sb, ga, be = vec(c["sums"]), vec(c["gamma"]), vec(c["beta"])
    outs = {k: Buf(1, Cc, Cc + 8, F32) for k in ("mean", "rstd", "scale", "shift")}
    rm, rv = Buf(1, Cc, Cc + 8, F32, prefill=c["running_mean"].reshape(1, -1)), Buf(1, Cc, Cc + 8, F32, prefill=c["running_var"].reshape(1, -1))
    nbt = torch.tensor([SENT64, c["nbt"], SENT64], dtype=torch.int64, device=DEV)
    run, cnt = form != "no_running", form != "no_nbt"
    check(lib.fx_bn_finalize_f32(sb.ptr, float(n), ga.ptr, be.ptr, NC.FIN_EPS, NC.FIN_MOMENTUM, rm.ptr if run else None, rv.ptr if run else None,
                                 nbt[1:].data_ptr() if cnt else None, outs["mean"].ptr, outs["rstd"].ptr, outs["scale"].ptr, outs["shift"].ptr, Cc,
                                 stream()), "fx_bn_finalize_f32")
    torch.cuda.synchronize()
    assert nbt.cpu().tolist() == [SENT64, c["nbt"] + (1 if cnt else 0), SENT64]
    what = f"C{Cc} n{n} {form}"
    for k, b in outs.items():
        b.assert_guards()
        gate("bn_finalize." + k, what, b.get()[0], ref[k][0], ref[k][1], F32)
    got_r = outs["rstd"].get()[0]
    assert bool(torch.isfinite(got_r).all()) and abs(float(got_r[NC.FIN_NEG]) - NC.FIN_EPS ** -0.5) <= 1e-3
    for k, b in (("running_mean", rm), ("running_var", rv)):
        b.assert_guards()
        if run:
            gate("bn_finalize." + k, what, b.get()[0], ref[k][0], ref[k][1], F32)
        else:
            assert torch.equal(b.get()[0], c[k])


# ------------------------------------------------------------------------------------------------ 4. pooling backward
def maxpool_run(lib, x, dy, shape, device_inputs=False):
    B, H, W, Cc = shape
    Ho, Wo = NC.mp_out(H), NC.mp_out(W)
    xb, dyb = Buf(B * H * W, Cc, Cc + 8, adt(), data=x), Buf(B * Ho * Wo, Cc, Cc + 16, adt(), data=dy)
    dxb = Buf(B * H * W, Cc, Cc + 24, adt())
    nws = B * Ho * Wo * Cc
    ws = torch.full((nws + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    check(lib.fx_maxpool3x3s2_bwd_nhwc_bf16(xb.ptr, Cc + 8, dyb.ptr, Cc + 16, dxb.ptr, Cc + 24, B, H, W, Cc, ws.data_ptr(), stream()), "fx_maxpool3x3s2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    dxb.assert_guards()
    assert bool((ws[nws:] == 0x5A).all()) and bool((ws[:nws] <= 8).all()), "the arg-max workspace: a byte past its end changed or a tap above 8"
    return xb, dyb, dxb


@pytest.mark.parametrize("variant", NC.MP_VARIANTS)
@pytest.mark.parametrize("shape", NC.MP_SHAPES, ids=sid)
def test_maxpool_bwd(lib, shape, variant):
    """fx_maxpool3x3s2_bwd_nhwc_bf16 vs the fp64 first-maximum scatter, bit for bit (dy holds integers: dx is a sum of at most four):
    post-ReLU inputs (ties at zero), a constant input (every window one tie: the first in-bounds tap wins), all eight channels of a
    group peaking at one pixel (fast path only) and each channel on its own (mixed path); H and W of 1 and 2; ldx = C + 8, lddy = C + 16,
    lddx = C + 24; the byte after the arg-max workspace keeps its value."""
    B, H, W, Cc = shape
    c = NC.maxpool_case(shape, adt(), variant)
    _, _, dxb = maxpool_run(lib, c["x"], c["dy"], shape)
    want = NC.maxpool_bwd64(c["x"], c["dy"]).to(adt()).reshape(B * H * W, Cc)
    got = dxb.get()
    assert same_bits(got, want), f"{int((got.float() != want.float()).sum())} of {got.numel()} elements differ"


@pytest.mark.parametrize("shape", NC.AP_SHAPES, ids=sid)
def test_avgpool_bwd(lib, shape):
    """fx_avgpool2x2_bwd_nhwc_bf16 vs dp / (in-bounds taps), bit for bit with the single rounding of the fp64 value (the product with 1,
    1/2 or 1/4 is exact in fp32); odd H and W (windows of two and one tap), H = W = 1; lddp = C + 8, lddx = C + 16."""
    B, H, W, Cc = shape
    c = NC.avgpool_case(shape, adt())
    pb = Buf(B * NC.ap_out(H) * NC.ap_out(W), Cc, Cc + 8, adt(), data=c["dp"])
    dxb = Buf(B * H * W, Cc, Cc + 16, adt())
    check(lib.fx_avgpool2x2_bwd_nhwc_bf16(pb.ptr, Cc + 8, dxb.ptr, Cc + 16, B, H, W, Cc, stream()), "fx_avgpool2x2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    dxb.assert_guards()
    want = elem_rne(NC.avgpool_bwd64(c["dp"], H, W), adt())
    assert torch.equal(want.to(adt()).double(), want)
    assert same_bits(dxb.get(), want.to(adt()).reshape(B * H * W, Cc))


def test_pool_bwd_second_trips(lib):
    """Both pooling backward entries past the grid cap: 1 x 65 x 127 x 2048, 8255 input pixels x 256 groups of eight; pixel 8192 =
    (row 64, column 64) starts the second trips.  Inputs are generated on the device; input rows 60 .. 64 and the output-gradient rows
    that reach dx rows 63 and 64 come back, and those two rows are compared bit for bit (an even first row keeps the windows aligned:
    CPU test)."""
    B, H, W, Cc = NC.POOL_CAP_SHAPE
    Ho, Wo, t0 = NC.mp_out(H), NC.mp_out(W), NC.POOL_CAP_TAIL
    g = torch.Generator(device=DEV).manual_seed(65)
    x = torch.randn(H * W, Cc, device=DEV, generator=g).clamp_min(0)
    dy = torch.randint(-3, 4, (Ho * Wo, Cc), device=DEV, generator=g).float()
    xb, dyb, dxb = maxpool_run(lib, x, dy, NC.POOL_CAP_SHAPE)
    x_tail = xb.full[GR + t0 * W:GR + H * W, :Cc].cpu().float().reshape(1, H - t0, W, Cc)
    dy_tail = dyb.full[GR + (t0 // 2) * Wo:GR + Ho * Wo, :Cc].cpu().float().reshape(1, Ho - t0 // 2, Wo, Cc)
    want = NC.maxpool_bwd64(x_tail, dy_tail)[:, 63 - t0:].to(adt()).reshape(2 * W, Cc)
    assert same_bits(dxb.full[GR + 63 * W:GR + 65 * W, :Cc].cpu(), want), "max pool, dx rows 63 and 64"

    Hp, Wp = NC.ap_out(H), NC.ap_out(W)
    pb = Buf(Hp * Wp, Cc, Cc + 8, adt(), data=torch.randn(Hp * Wp, Cc, device=DEV, generator=g) * 2)
    axb = Buf(H * W, Cc, Cc + 16, adt())
    check(lib.fx_avgpool2x2_bwd_nhwc_bf16(pb.ptr, Cc + 8, axb.ptr, Cc + 16, B, H, W, Cc, stream()), "fx_avgpool2x2_bwd_nhwc_bf16")
    torch.cuda.synchronize()
    axb.assert_guards()
    dp_tail = pb.full[GR + 31 * Wp:GR + Hp * Wp, :Cc].cpu().float().reshape(1, 2, Wp, Cc)         # pooled rows 31 and 32 = input rows 62 .. 64
    want = elem_rne(NC.avgpool_bwd64(dp_tail, 3, W), adt())[:, 1:].to(adt()).reshape(2 * W, Cc)
    assert same_bits(axb.full[GR + 63 * W:GR + 65 * W, :Cc].cpu(), want), "average pool, dx rows 63 and 64"


# ------------------------------------------------------------------------------------------------ 5. weight images
PADE = 64                                  # sentinel elements on either side of an image (128 / 256 bytes: keeps the 16-byte alignment)
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}


class Image:
    """A device allocation of `numel` elements between PADE sentinel elements on either side, the image itself prefilled with the
    sentinel too; `check(expected)` compares the WHOLE allocation bit for bit (expected: the image's bits, the sentinel where nothing is
    to be written)."""

    def __init__(self, numel, dtype):
        self.numel = numel
        self.full = torch.empty(numel + 2 * PADE, dtype=dtype, device=DEV)
        self.sent = SENT[self.full.element_size()]
        _bits(self.full).fill_(self.sent)

    @property
    def ptr(self):
        return self.full.data_ptr() + PADE * self.full.element_size()

    def check(self, expected, what):
        want = torch.full((self.numel + 2 * PADE,), self.sent, dtype=_bits(self.full).dtype)
        want[PADE:PADE + self.numel] = expected.reshape(-1)
        got = _bits(self.full).cpu()
        assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} elements differ (first at {int((got != want).nonzero()[0]) - PADE})"

    def untouched(self, what):
        self.check(torch.full((self.numel,), self.sent, dtype=_bits(self.full).dtype), what)


def bits16(t):
    return t.contiguous().view(torch.int16)


def padded_rows(img_bits, rows_total):
    """The image followed by sentinel rows up to rows_total."""
    out = torch.full((rows_total, img_bits.shape[1]), NC.SENT16, dtype=torch.int16)
    out[:img_bits.shape[0]] = img_bits
    return out


@pytest.mark.parametrize("use_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("mode", NC.PACK_CONV_MODES)
@pytest.mark.parametrize("shape", NC.PACK_CONV_SHAPES, ids=sid)
def test_pack_conv_weights(lib, shape, mode, use_scale):
    """fx_pack_conv_weights_f32 vs the documented layouts, bit for bit: w_fwd [N][KH][KW][C], w_dgrad[c][kh][kw][n] = the flipped,
    transposed filter, each the fp32 product w * scale[n] rounded once; forward only, dgrad only and both; with the fragment-order
    copies wherever the shape admits them (N and C multiples of 32: 64x32x3x3, 256x64x1x1, 512x256x3x3 - the last 1 179 648 elements,
    past the 4096-workgroup cap of the element kernel).  The 8 rows after N (C) of the padded images keep their sentinel."""
    N, Cc, KH, KW = shape
    T = KH * KW
    d = NC.weights_case(N, Cc, KH, KW)
    v = bits16(NC.packed_values(d["w"], d["scale"] if use_scale else None, adt()))
    fwd, dg = NC.fwd_image(v), NC.dgrad_image(v)
    want_f, want_d = mode != "dgrad", mode != "fwd"
    wd, sd = d["w"].to(DEV), d["scale"].to(DEV)
    f_img, d_img = Image((N + 8) * T * Cc, adt()), Image((Cc + 8) * T * N, adt())
    ff = Image(N * T * Cc, adt()) if want_f and NC.frag_eligible(N, T * Cc) else None
    df = Image(N * T * Cc, adt()) if want_d and NC.frag_eligible(Cc, T * N) else None
    check(lib.fx_pack_conv_weights_f32(wd.data_ptr(), sd.data_ptr() if use_scale else None, f_img.ptr if want_f else None, d_img.ptr if want_d else None,
                                       ff.ptr if ff else None, df.ptr if df else None, N, Cc, KH, KW, stream()), "fx_pack_conv_weights_f32")
    torch.cuda.synchronize()
    if want_f:
        f_img.check(padded_rows(fwd, N + 8), "w_fwd")
    else:
        f_img.untouched("w_fwd (NULL)")
    if want_d:
        d_img.check(padded_rows(dg, Cc + 8), "w_dgrad")
    else:
        d_img.untouched("w_dgrad (NULL)")
    if ff:
        ff.check(frag_order(fwd), "w_fwd_frag")
    if df:
        df.check(frag_order(dg), "w_dgrad_frag")
    if mode == "both":
        assert (ff is not None and df is not None) == (shape in (NC.PACK_CONV_SHAPES[1], NC.PACK_CONV_SHAPES[3], NC.PACK_CONV_SHAPES[5]))


@pytest.mark.parametrize("shape", NC.PACK_FRAG_SHAPES, ids=sid)
def test_pack_frag(lib, shape):
    """fx_pack_frag_bf16 vs the documented permutation of 16-byte pieces; 2048 x 4608 is past the 4096-workgroup cap."""
    rows, K = shape
    w = bits16(torch.randn(rows, K, generator=NC.gen(rows + K)).to(adt()))
    src, dst = Image(rows * K, adt()), Image(rows * K, adt())
    _bits(src.full)[PADE:PADE + rows * K] = w.reshape(-1).to(DEV)
    check(lib.fx_pack_frag_bf16(src.ptr, dst.ptr, rows, K, stream()), "fx_pack_frag_bf16")
    torch.cuda.synchronize()
    dst.check(frag_order(w), "frag")
    src.check(w, "the source image")


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", NC.PACK_LINEAR_SHAPES, ids=sid)
def test_pack_linear_weights(lib, shape, with_bias):
    """fx_pack_linear_weights_f32: w_fwd [Np][Kp] row n, w_t [Kp][Np] row k, bias into its padded vector; everything outside the N x K
    (K x N, N) corner keeps the sentinel."""
    N, K, Np, Kp = shape
    d = NC.weights_case(N, K, 1, 1)
    v = bits16(d["w"].reshape(N, K).to(adt()))
    wd, bd = d["w"].to(DEV), d["bias"].to(DEV)
    f_img, t_img, b_img = Image(Np * Kp, adt()), Image(Kp * Np, adt()), Image(Np, F32)
    check(lib.fx_pack_linear_weights_f32(wd.data_ptr(), bd.data_ptr() if with_bias else None, f_img.ptr, t_img.ptr, b_img.ptr if with_bias else None, N, K, Np,
                                         Kp, stream()), "fx_pack_linear_weights_f32")
    torch.cuda.synchronize()
    want = torch.full((Np, Kp), NC.SENT16, dtype=torch.int16)
    want[:N, :K] = v
    f_img.check(want, "w_fwd")
    want = torch.full((Kp, Np), NC.SENT16, dtype=torch.int16)
    want[:K, :N] = v.T
    t_img.check(want, "w_t")
    want = torch.full((Np,), SENT[4], dtype=torch.int32)
    if with_bias:
        want[:N] = d["bias"].view(torch.int32)
    b_img.check(want, "bias_out")


def test_pack_weights_many(lib):
    """fx_pack_weights_many_f32 over ONE table (train_norm_cases.PACK_TABLE) vs images written out from the documented index formulas - not
    vs the per-layer packers: 3x3 with C = 256 (one PK_TILE chunk) and C = 264 (a second chunk of 8 channels, ld_fwd above the row
    length), pointwise with C = 2304 and 2312, N = 365 (a last tile of 5 output channels, element dgrad stores), K = 4 and 7x7 with
    C = 3 (element forward stores), three masters sharing the images of 768 output channels, NULL fragment pointers, a NULL w_dgrad,
    NULL scales, bias outputs.  fx_pack_entry_blocks returns the workgroups the layout predicts, and -1 beyond 288 taps."""
    entries, images, total = NC.pack_table_case(adt())
    dev, keep = {}, []
    for k, img in images.items():
        dev[k] = Image(img.numel(), F32 if k.endswith(".bias") else adt())
    arr = (FxPackEntry * len(entries))()

    def up(t):
        keep.append(t.to(DEV))
        return keep[-1].data_ptr()

    for a, e in zip(arr, entries):
        assert lib.fx_pack_entry_blocks(e["N"], e["C"], e["KH"], e["KW"]) == e["blocks"] > 0, e["name"]
        key = e["key"]
        a.w, a.scale, a.bias = up(e["w"]), (up(e["scale"]) if e["scale"] is not None else None), (up(e["bias"]) if e["bias"] is not None else None)
        a.w_fwd, a.w_dgrad = dev[key + ".fwd"].ptr, (dev[key + ".dgrad"].ptr if e["dgrad"] else None)
        a.w_fwd_frag, a.w_dgrad_frag = (dev[key + ".fwd_frag"].ptr if e["fwd_frag"] else None), (dev[key + ".dgrad_frag"].ptr if e["dgrad_frag"] else None)
        a.bias_out = dev[key + ".bias"].ptr if e["bias"] is not None else None
        a.N, a.C, a.KH, a.KW, a.ld_fwd, a.ld_dgrad = e["N"], e["C"], e["KH"], e["KW"], e["ld_fwd"], e["ld_dgrad"]
        a.first_block, a.n_offset, a.n_total, a.reserved = e["first_block"], e["n_offset"], e["n_total"], 0
    assert lib.fx_pack_entry_blocks(8, 8, 17, 17) == -1 and lib.fx_pack_entry_blocks(8, 16, 16, 18) == NC.pack_blocks(8, 16, 16, 18) == 2
    assert lib.fx_pack_entry_blocks(0, 8, 1, 1) == -1
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    check(lib.fx_pack_weights_many_f32(table.data_ptr(), len(entries), total, stream()), "fx_pack_weights_many_f32")
    torch.cuda.synchronize()
    for k, img in images.items():
        dev[k].check(img.view(torch.int32) if k.endswith(".bias") else img, k)


# ------------------------------------------------------------------------------------------------ 6. weight-gradient unpack
@pytest.mark.parametrize("splits", NC.UNPACK_SPLITS)
@pytest.mark.parametrize("shape", NC.UNPACK_SHAPES, ids=sid)
def test_unpack_wgrad(lib, shape, splits):
    """fx_unpack_conv_wgrad_sum_f32 (and, for one split, fx_unpack_conv_wgrad_f32) vs dw[n][c][kh][kw] (+)= scale[n] * sum over the splits,
    exact (integer slabs, power-of-two scales): accumulate 0 and 1, scale NULL and present; split_stride above the slab with NaN in the
    gap; C = 3 in C_eff = 8 with NaN in the padded columns of every slab (they may be read, they must not reach dw); C_eff = 10 takes
    the generic kernel; splits 2, 4 run only the remainder loop of the 4-way unrolled sum, 5 and 9 only whole rounds, 6 both.  The
    partial slabs are uploaded anew for every call: with FX_UNPACK_FUSED=0 slab_sum_kernel overwrites slab 0."""
    N, Cc, KH, KW, Ce = shape
    T = KH * KW
    c = NC.unpack_case(shape, splits)
    sd = c["scale"].to(DEV)
    for accumulate in (0, 1):
        for use_scale in (False, True):
            entries = ["sum"] + (["plain"] if splits == 1 else [])
            for entry in entries:
                part = c["part"].to(DEV)
                out = Buf(N, Cc * T, Cc * T, F32, prefill=c["pre"].reshape(N, -1) if accumulate else None)
                if entry == "sum":
                    rc = lib.fx_unpack_conv_wgrad_sum_f32(part.data_ptr(), c["stride"], splits, sd.data_ptr() if use_scale else None, out.ptr, N, Cc, KH, KW, Ce,
                                                          accumulate, stream())
                else:
                    rc = lib.fx_unpack_conv_wgrad_f32(part.data_ptr(), sd.data_ptr() if use_scale else None, out.ptr, N, Cc, KH, KW, Ce, accumulate, stream())
                check(rc, "fx_unpack_conv_wgrad")
                torch.cuda.synchronize()
                out.assert_guards()
                got = out.get().reshape(N, Cc, KH, KW)
                ref = NC.unpack_ref(c, use_scale, accumulate)
                assert torch.equal(got.double(), ref), f"{entry} accumulate={accumulate} scale={use_scale}: {int((got.double() != ref).sum())} of {ref.numel()} differ"
                assert bool(torch.isnan(part[:, c["slab"]:]).all()), "the gap between the slabs was written"


def test_unpack_wgrad_unfused():
    """test_unpack_wgrad again in ONE fresh process with FX_UNPACK_FUSED=0: slab_sum_kernel, then unpack_conv_wgrad_kernel on slab 0."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_train_norm_ops.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_unpack_wgrad and not unfused"],
                       cwd=ROOT, env=dict(os.environ, FX_UNPACK_FUSED="0"), capture_output=True, text=True, timeout=300)
    tail = r.stdout[-2000:] + r.stderr[-500:]
    assert r.returncode == 0, tail
    summary = r.stdout.strip().splitlines()[-1]
    n = 2 * len(NC.UNPACK_SHAPES) * len(NC.UNPACK_SPLITS)
    assert re.search(rf"\b{n} passed\b", summary) and "skipped" not in summary and "failed" not in summary, tail


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_bn_refusals(lib):
    """The five BatchNorm entry points: C % 8, every leading dimension below C and no multiple of 8, every required pointer NULL, rows 0,
    n <= 0, exactly one of dgamma_acc / dbeta_acc, exactly one of running_mean / running_var.  Nothing may be written."""
    c = NC.bn_case((7, 24), adt(), "gauss", False)
    rows, Cc = 7, 24
    ld, zb, dyb, rb = bn_bufs(c, 0)
    vs = {k: vec(c[k]) for k in ("scale", "shift", "mean", "rstd", "sums")}
    sums_out = Buf(1, 2 * Cc, 2 * Cc + 8, F32)

    def stats(z=zb.ptr, ldz=ld["z"], sums=sums_out.ptr, rows=rows, Cc=Cc):
        return lib.fx_bn_stats_bf16(z, ldz, 0, sums, rows, Cc, stream())

    bad = {"C % 8": {"Cc": 20}, "ldz < C": {"ldz": 16}, "ldz % 8": {"ldz": 28}, "z NULL": {"z": None}, "sums NULL": {"sums": None}, "rows 0": {"rows": 0}}
    for what, kw in bad.items():
        refused(stats(**kw), f"fx_bn_stats_bf16: {what}")
    untouched(sums_out)

    def bstats(dy=dyb.ptr, lddy=ld["dy"], z=zb.ptr, ldz=ld["z"], res=rb.ptr, ldr=ld["res"], scale=vs["scale"].ptr, shift=vs["shift"].ptr, mean=vs["mean"].ptr,
               rstd=vs["rstd"].ptr, sums=sums_out.ptr, rows=rows, Cc=Cc):
        return lib.fx_bn_bwd_stats_bf16(dy, lddy, z, ldz, 0, res, ldr, scale, shift, mean, rstd, 1, sums, rows, Cc, stream())

    bad = {"C % 8": {"Cc": 20}, "ldz < C": {"ldz": 16}, "ldz % 8": {"ldz": 28}, "lddy < C": {"lddy": 16}, "lddy % 8": {"lddy": 28}, "ldr < C": {"ldr": 16},
           "ldr % 8": {"ldr": 28}, "dy NULL": {"dy": None}, "z NULL": {"z": None}, "scale NULL": {"scale": None}, "shift NULL": {"shift": None},
           "mean NULL": {"mean": None}, "rstd NULL": {"rstd": None}, "sums NULL": {"sums": None}, "rows 0": {"rows": 0}}
    for what, kw in bad.items():
        refused(bstats(**kw), f"fx_bn_bwd_stats_bf16: {what}")
    untouched(sums_out)

    yb = Buf(rows, Cc, ld["y"], adt())

    def apply(z=zb.ptr, ldz=ld["z"], scale=vs["scale"].ptr, shift=vs["shift"].ptr, res=rb.ptr, ldr=ld["res"], y=yb.ptr, ldy=ld["y"], rows=rows, Cc=Cc):
        return lib.fx_bn_apply_bf16(z, ldz, 0, scale, shift, res, ldr, 1, y, ldy, rows, Cc, stream())

    bad = {"C % 8": {"Cc": 20}, "ldz < C": {"ldz": 16}, "ldz % 8": {"ldz": 28}, "ldy < C": {"ldy": 16}, "ldy % 8": {"ldy": 28}, "ldr < C": {"ldr": 16},
           "ldr % 8": {"ldr": 28}, "z NULL": {"z": None}, "scale NULL": {"scale": None}, "shift NULL": {"shift": None}, "y NULL": {"y": None}, "rows 0": {"rows": 0}}
    run_refusals("fx_bn_apply_bf16", apply, bad, [yb])
    yb.assert_guards()

    dab, dzb = Buf(rows, Cc, ld["da"], adt()), Buf(rows, Cc, ld["dz"], adt())
    ga, ba = Buf(1, Cc, Cc + 8, F32), Buf(1, Cc, Cc + 8, F32)

    def bapply(dy=dyb.ptr, lddy=ld["dy"], z=zb.ptr, ldz=ld["z"], res=rb.ptr, ldr=ld["res"], scale=vs["scale"].ptr, shift=vs["shift"].ptr, mean=vs["mean"].ptr,
               rstd=vs["rstd"].ptr, sums=vs["sums"].ptr, da=dab.ptr, ldda=ld["da"], dz=dzb.ptr, lddz=ld["dz"], rows=rows, Cc=Cc, dg=None, db=None):
        return lib.fx_bn_bwd_apply_bf16(dy, lddy, z, ldz, 0, res, ldr, scale, shift, mean, rstd, 1, sums, c["inv_n"], da, ldda, dz, lddz, rows, Cc, dg, db,
                                        stream())

    bad = {"C % 8": {"Cc": 20}, "ldz < C": {"ldz": 16}, "ldz % 8": {"ldz": 28}, "lddy < C": {"lddy": 16}, "lddy % 8": {"lddy": 28}, "ldr < C": {"ldr": 16},
           "ldr % 8": {"ldr": 28}, "lddz < C": {"lddz": 16}, "lddz % 8": {"lddz": 28}, "ldda < C": {"ldda": 16}, "ldda % 8": {"ldda": 28},
           "dy NULL": {"dy": None}, "z NULL": {"z": None}, "scale NULL": {"scale": None}, "shift NULL": {"shift": None}, "mean NULL": {"mean": None},
           "rstd NULL": {"rstd": None}, "sums NULL": {"sums": None}, "dz NULL": {"dz": None}, "rows 0": {"rows": 0},
           "dgamma_acc alone": {"dg": ga.ptr}, "dbeta_acc alone": {"db": ba.ptr}}
    run_refusals("fx_bn_bwd_apply_bf16", bapply, bad, [dab, dzb, ga, ba])
    untouched(ga, ba)

    f = NC.finalize_case(8, 2)
    fs, fg, fb = vec(f["sums"]), vec(f["gamma"]), vec(f["beta"])
    fo = [Buf(1, 8, 16, F32) for _ in range(4)]
    rm, rv = Buf(1, 8, 16, F32, prefill=f["running_mean"].reshape(1, -1)), Buf(1, 8, 16, F32, prefill=f["running_var"].reshape(1, -1))

    def fin(sums=fs.ptr, n=2.0, gamma=fg.ptr, beta=fb.ptr, rmean=None, rvar=None, mean=fo[0].ptr, rstd=fo[1].ptr, scale=fo[2].ptr, shift=fo[3].ptr, Cc=8):
        return lib.fx_bn_finalize_f32(sums, n, gamma, beta, NC.FIN_EPS, NC.FIN_MOMENTUM, rmean, rvar, None, mean, rstd, scale, shift, Cc, stream())

    bad = {"sums NULL": {"sums": None}, "gamma NULL": {"gamma": None}, "beta NULL": {"beta": None}, "mean NULL": {"mean": None}, "rstd NULL": {"rstd": None},
           "scale NULL": {"scale": None}, "shift NULL": {"shift": None}, "C 0": {"Cc": 0}, "n 0": {"n": 0.0}, "n -1": {"n": -1.0},
           "running_mean alone": {"rmean": rm.ptr}, "running_var alone": {"rvar": rv.ptr}}
    for what, kw in bad.items():
        refused(fin(**kw), f"fx_bn_finalize_f32: {what}")
    untouched(*fo)
    torch.cuda.synchronize()
    assert torch.equal(rm.get()[0], f["running_mean"]) and torch.equal(rv.get()[0], f["running_var"])


def test_pool_refusals(lib):
    """Both pooling backward entries: C % 8, every leading dimension below C and no multiple of 8, every pointer NULL, a size of 0, a
    workspace that is not 8-byte aligned."""
    shape = (1, 5, 6, 16)
    B, H, W, Cc = shape
    c = NC.maxpool_case(shape, adt(), "relu")
    xb, dyb, dxb = Buf(30, Cc, 24, adt(), data=c["x"]), Buf(9, Cc, 32, adt(), data=c["dy"]), Buf(30, Cc, 40, adt())
    ws = torch.full((9 * Cc + 64,), 0x5A, dtype=torch.uint8, device=DEV)

    def mp(x=xb.ptr, ldx=24, dy=dyb.ptr, lddy=32, dx=dxb.ptr, lddx=40, H=H, Cc=Cc, w=ws.data_ptr()):
        return lib.fx_maxpool3x3s2_bwd_nhwc_bf16(x, ldx, dy, lddy, dx, lddx, B, H, W, Cc, w, stream())

    bad = {"C % 8": {"Cc": 12}, "ldx < C": {"ldx": 8}, "lddy < C": {"lddy": 8}, "lddx < C": {"lddx": 8}, "ldx % 8": {"ldx": 20}, "lddy % 8": {"lddy": 20},
           "lddx % 8": {"lddx": 20}, "x NULL": {"x": None}, "dy NULL": {"dy": None}, "dx NULL": {"dx": None}, "workspace NULL": {"w": None}, "H 0": {"H": 0},
           "workspace misaligned": {"w": ws.data_ptr() + 4}}
    for what, kw in bad.items():
        refused(mp(**kw), f"fx_maxpool3x3s2_bwd_nhwc_bf16: {what}")
    untouched(dxb)
    assert bool((ws == 0x5A).all())

    a = NC.avgpool_case(shape, adt())
    pb, adx = Buf(9, Cc, 24, adt(), data=a["dp"]), Buf(30, Cc, 32, adt())

    def ap(dp=pb.ptr, lddp=24, dx=adx.ptr, lddx=32, H=H, Cc=Cc):
        return lib.fx_avgpool2x2_bwd_nhwc_bf16(dp, lddp, dx, lddx, B, H, W, Cc, stream())

    bad = {"C % 8": {"Cc": 12}, "lddp < C": {"lddp": 8}, "lddx < C": {"lddx": 8}, "lddp % 8": {"lddp": 20}, "lddx % 8": {"lddx": 20}, "dp NULL": {"dp": None},
           "dx NULL": {"dx": None}, "H 0": {"H": 0}}
    run_refusals("fx_avgpool2x2_bwd_nhwc_bf16", ap, bad, [adx])
    adx.assert_guards()


def test_pack_and_unpack_refusals(lib):
    """fx_pack_conv_weights_f32: w NULL, both images NULL, a size of 0, a fragment copy without its image or with N % 32 (C % 32) != 0.
    fx_pack_frag_bf16: rows % 32, K % 16, a NULL or misaligned pointer.  fx_pack_linear_weights_f32: Np < N, Kp < K, a NULL pointer,
    bias_out without bias.  fx_pack_weights_many_f32: a NULL table, no entries, no workgroups.  Both unpack entries: a NULL pointer,
    C_eff < C, a size of 0, splits 0, split_stride below the slab."""
    N, Cc, KH, KW = 32, 32, 3, 3
    d = NC.weights_case(N, Cc, KH, KW)
    wd = d["w"].to(DEV)
    n = N * Cc * 9
    imgs = [Image(n, adt()) for _ in range(4)]

    def pc(w=wd.data_ptr(), f=imgs[0].ptr, dgr=imgs[1].ptr, ff=imgs[2].ptr, df=imgs[3].ptr, N=N, Cc=Cc, KH=KH):
        return lib.fx_pack_conv_weights_f32(w, None, f, dgr, ff, df, N, Cc, KH, KW, stream())

    bad = {"w NULL": {"w": None}, "no image": {"f": None, "dgr": None, "ff": None, "df": None}, "N 0": {"N": 0}, "KH 0": {"KH": 0},
           "fwd frag without w_fwd": {"f": None}, "dgrad frag without w_dgrad": {"dgr": None}, "fwd frag, N % 32": {"N": 24, "df": None},
           "dgrad frag, C % 32": {"Cc": 24, "ff": None}, "fwd frag misaligned": {"ff": imgs[2].ptr + 2}}
    for what, kw in bad.items():
        refused(pc(**kw), f"fx_pack_conv_weights_f32: {what}")
    torch.cuda.synchronize()
    for i in imgs:
        i.untouched("fx_pack_conv_weights_f32 refusals")

    def pf(src=imgs[0].ptr, dst=imgs[1].ptr, rows=32, K=32):
        return lib.fx_pack_frag_bf16(src, dst, rows, K, stream())

    bad = {"rows % 32": {"rows": 24}, "K % 16": {"K": 24}, "src NULL": {"src": None}, "frag NULL": {"dst": None}, "src misaligned": {"src": imgs[0].ptr + 2},
           "frag misaligned": {"dst": imgs[1].ptr + 2}, "rows 0": {"rows": 0}}
    for what, kw in bad.items():
        refused(pf(**kw), f"fx_pack_frag_bf16: {what}")

    bd = d["bias"].to(DEV)
    bo = Image(64, F32)

    def plin(w=wd.data_ptr(), bias=bd.data_ptr(), f=imgs[0].ptr, t=imgs[1].ptr, b=bo.ptr, N=32, K=32, Np=40, Kp=48):
        return lib.fx_pack_linear_weights_f32(w, bias, f, t, b, N, K, Np, Kp, stream())

    bad = {"Np < N": {"Np": 24}, "Kp < K": {"Kp": 24}, "w NULL": {"w": None}, "w_fwd NULL": {"f": None}, "w_t NULL": {"t": None}, "bias_out without bias": {"bias": None},
           "N 0": {"N": 0}}
    for what, kw in bad.items():
        refused(plin(**kw), f"fx_pack_linear_weights_f32: {what}")
    table = torch.zeros(FxPackEntryBytes, dtype=torch.uint8, device=DEV)
    for what, args in {"table NULL": (None, 1, 1), "no entries": (table.data_ptr(), 0, 1), "no workgroups": (table.data_ptr(), 1, 0)}.items():
        refused(lib.fx_pack_weights_many_f32(*args, stream()), f"fx_pack_weights_many_f32: {what}")
    torch.cuda.synchronize()
    for i in imgs + [bo]:
        i.untouched("pack refusals")

    shape = NC.UNPACK_SHAPES[1]
    Nn, Cu, KHu, KWu, Ce = shape
    u = NC.unpack_case(shape, 2)
    part = u["part"].to(DEV)
    out = Buf(Nn, Cu * 9, Cu * 9, F32)

    def us(p=part.data_ptr(), stride=u["stride"], splits=2, dw=out.ptr, N=Nn, Cc=Cu, Ce=Ce):
        return lib.fx_unpack_conv_wgrad_sum_f32(p, stride, splits, None, dw, N, Cc, KHu, KWu, Ce, 0, stream())

    bad = {"partials NULL": {"p": None}, "dw NULL": {"dw": None}, "C_eff < C": {"Ce": Cu - 8, "stride": u["stride"]}, "N 0": {"N": 0}, "splits 0": {"splits": 0},
           "split_stride below the slab": {"stride": u["slab"] - 4}}
    run_refusals("fx_unpack_conv_wgrad_sum_f32", us, bad, [out])
    out2 = Buf(Nn, Cu * 9, Cu * 9, F32)

    def up(p=part.data_ptr(), dw=out2.ptr, N=Nn, Ce=Ce):
        return lib.fx_unpack_conv_wgrad_f32(p, None, dw, N, Cu, KHu, KWu, Ce, 0, stream())

    bad = {"dw_eff NULL": {"p": None}, "dw NULL": {"dw": None}, "C_eff < C": {"Ce": Cu - 8}, "N 0": {"N": 0}}
    run_refusals("fx_unpack_conv_wgrad_f32", up, bad, [out2])


FxPackEntryBytes = C.sizeof(FxPackEntry)
