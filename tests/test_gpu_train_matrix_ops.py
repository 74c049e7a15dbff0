"""The training step's matrix-core kernels, called directly on a real MI355X: the weight gradient (csrc/conv_wgrad.hip:
conv_wgrad_kernel<PW> behind fx_conv2d_wgrad_nhwc_bf16 / _bias / _partial and fx_linear_wgrad_bias_bf16, conv_wgrad_dma_kernel<PW>
behind the partial-slab entry of wide layers, both followed by fx_unpack_conv_wgrad_sum_f32) and the attention backward
(csrc/attn_bwd.hip: mha32_bwd_dq_kernel and mha32_bwd_dkv_kernel behind fx_mha_masked_bwd_bf16 / fx_mha_bwd_bf16).  The cases, their
float64 references and magnitudes are built by tests/train_matrix_cases.py (checked on the CPU by test_train_matrix_cases_cpu.py).

Rules every case follows
* Views and guards: every operand is a column slice of a wider buffer (distinct leading dimensions, the dz slice at a non-zero column)
  between guard rows; outputs are prefilled with a sentinel bit pattern and everything outside the written region must keep it; the
  padding of inputs is NaN, so a read outside the logical region poisons the result.  Outputs that are ACCUMULATED (dW, dbias) are
  followed by neighbours holding 1.0 in front of the guard rows: an fp32 add does not change the sentinel's bits.
* Variant: every weight-gradient case names the kernel it expects and asserts it with fx_conv2d_wgrad_variant before it runs.
* Exact run: x and dz are integers in [-2, 2] (dW prefilled with integers), so every partial sum is an integer below 2^24 - exact in
  fp32 in any order - and dW / dbias equal the float64 reference bit for bit: a dropped, doubled or misplaced pixel, tap or tile shows.
* Gaussian run: |got - ref| <= c * mag element by element; mag is the same sum over absolute values; c = MARGIN * MEASURED[kernel form]
  (MEASURED: the largest c any case of that form needed on an MI355X; the order of the atomics varies from run to run, hence the
  margin).  No gate may exceed M * 2^-24, the worst case of an fp32 sum of M products (asserted per case).
* Attention backward: |got - ref| <= RND(ref) (one rounding to bf16) + c * mag; the probabilities and dS enter the second MFMA as bf16,
  so c is a few 2^-8 of the magnitude.
Every gate prints the c it needs before it asserts (EXCESS lines, pytest -s)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FocoosAmdError, check  # noqa: E402
from tests import helpers  # noqa: E402
from tests import train_matrix_cases as TC  # noqa: E402
from tests.helpers import U32, Buf, _bits  # noqa: E402

DEV = "cuda:0"
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
MARGIN = 4.0
# largest c over all cases of the kernel form, measured on an MI355X against the float64 reference
MEASURED = {
    "wgrad.pw": 7.268e-08,
    "wgrad.im2col": 1.638e-07,
    "wgrad_dma.pw": 4.105e-08,
    "wgrad_dma.3x3": 1.638e-07,
    "wgrad.dbias": 1.200e-08,
    "mha_bwd.dq": 5.410e-04,
    "mha_bwd.dk": 1.216e-03,
    "mha_bwd.dv": 3.164e-03,
    "mha_bwd_masked.dq": 5.199e-04,
    "mha_bwd_masked.dk": 8.704e-04,
    "mha_bwd_masked.dv": 3.196e-03,
}
FORM = {TC.PW: "wgrad.pw", TC.IM2COL: "wgrad.im2col", TC.DMA_PW: "wgrad_dma.pw", TC.DMA_3X3: "wgrad_dma.3x3"}
# fx_tune reads FX_WGRAD_DMA_MIN_GFLOP once per process: the wide-but-small cases reach the DMA kernel only in a process started with 0
DMA0 = os.environ.get("FX_WGRAD_DMA_MIN_GFLOP") == "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load("bf16")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def view(data, off, ld):
    """[rows][cols] values as the column slice [off, off + cols) of a [rows][ld] buffer (NaN in every other column, guard rows around):
    (buffer, pointer of the slice)."""
    rows, cols = data.shape
    full = torch.full((rows, off + cols), float("nan"))
    full[:, off:] = data
    b = Buf(rows, off + cols, ld, BF, data=full)
    return b, b.ptr + 2 * off


NEIGHBOUR = 1.0


def acc_buf(pre, rows, cols):
    """An ACCUMULATED fp32 output as it lies in a flat gradient buffer: `pre` in the corner of a [rows][cols] region whose other elements
    - the neighbouring parameters' gradients - hold 1.0.  The sentinel cannot guard an accumulation: as fp32 it is 1.5e16, and an atomic
    add of a gradient-sized value leaves its bits unchanged."""
    full = torch.full((rows, cols), NEIGHBOUR)
    full[:pre.shape[0], :pre.shape[1]] = pre
    return Buf(rows, cols, cols, F32, prefill=full)


def acc_get(buf, rows, cols):
    """The corner of an acc_buf; every neighbour still holds 1.0 and the guard rows their sentinel."""
    buf.assert_guards()
    got = buf.get()
    rest = got.clone()
    rest[:rows, :cols] = NEIGHBOUR
    assert bool((rest == NEIGHBOUR).all()), "an element outside the stored corner changed"
    return got[:rows, :cols].contiguous()


def compare(kernel, what, kind, got, ref, mag, M):
    """Integer run: bit equality with the float64 reference (an integer, or half of one after the power-of-two scale).  Gaussian run:
    the per-element gate, which must itself lie below the worst case M * 2^-24 of an fp32 sum of M terms."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if kind == "int":
        bad = (got.double() != ref).nonzero()
        assert bad.shape[0] == 0, (f"{kernel} {what}: {bad.shape[0]} of {ref.numel()} elements differ from the exact integer result; first at "
                                   f"{bad[0].tolist()}: got {got[tuple(bad[0])].item()!r} ref {ref[tuple(bad[0])].item()!r}")
    else:
        assert MARGIN * MEASURED[kernel] <= M * U32, f"{kernel}: gate {MARGIN * MEASURED[kernel]:.3e} above the fp32 worst case {M * U32:.3e}"
        helpers.gate(kernel, what, got, ref, mag, F32, MEASURED, MARGIN, extra=0.0)


# ------------------------------------------------------------------------------------------------ weight gradient
class Wgrad:
    """One weight-gradient case on the device: operands as views, the float64 reference (computed on the device), the three entries."""

    def __init__(self, lib, c, kind):
        self.lib, self.c, self.kind = lib, c, kind
        self.M, self.Ktot = TC.pixels(c), c.k * c.k * c.C
        assert TC.exact_run_is_exact(self.M)
        d = self.d = TC.wgrad_inputs(c, kind)
        self.ldx, self.lddz = c.C + 40, c.N + 24
        assert self.ldx != self.lddz
        self.xb, self.xp = view(d["x"].reshape(-1, c.C), 8, self.ldx)
        self.zb, self.zp = view(d["dz"].reshape(-1, c.N), 16, self.lddz)          # a non-zero column, as a group's slice in train_nn.py
        self.ref, self.mag, self.db, self.dbm = (t.cpu() for t in TC.wgrad_ref64(d["x"].to(DEV), d["dz"].to(DEV), c.k, c.stride))
        Ho, Wo = TC.out_hw(c)
        self.geom = (c.B, c.H, c.W, c.C, Ho, Wo, c.N, c.k, c.k, c.stride, (c.k - 1) // 2)

    def variant(self):
        Ho, Wo = TC.out_hw(self.c)
        out = C.create_string_buffer(64)
        check(self.lib.fx_conv2d_wgrad_variant(self.c.B, Ho, Wo, self.c.C, self.c.N, self.c.k, self.c.k, self.c.stride, (self.c.k - 1) // 2, out, 64))
        return out.value.decode()

    def atomic(self, with_bias):
        """fx_conv2d_wgrad_nhwc_bf16 / fx_conv2d_wgrad_bias_nhwc_bf16: fp32 atomics into a prefilled dW (always the 128 x 128 kernel)."""
        c, d = self.c, self.d
        form = "wgrad.pw" if c.k == 1 else "wgrad.im2col"
        dwb = acc_buf(d["pre"].reshape(c.N, self.Ktot), c.N + 8, self.Ktot)
        if with_bias:
            bb = acc_buf(d["bpre"].view(1, -1), 1, c.N + 8)
            check(self.lib.fx_conv2d_wgrad_bias_nhwc_bf16(self.xp, self.ldx, self.zp, self.lddz, dwb.ptr, bb.ptr, *self.geom, stream()), "wgrad_bias")
        else:
            check(self.lib.fx_conv2d_wgrad_nhwc_bf16(self.xp, self.ldx, self.zp, self.lddz, dwb.ptr, *self.geom, stream()), "wgrad")
        torch.cuda.synchronize()
        what = f"{TC.wid(c)} {'bias' if with_bias else 'atomic'}"
        compare(form, what, self.kind, acc_get(dwb, c.N, self.Ktot).reshape(self.ref.shape), self.ref + d["pre"].double(), self.mag + d["pre"].double().abs(), self.M)
        if with_bias:
            compare("wgrad.dbias", what, self.kind, acc_get(bb, 1, c.N).reshape(-1), self.db + d["bpre"].double(), self.dbm + d["bpre"].double().abs(), self.M)

    def partial(self, form):
        """fx_conv2d_wgrad_partial_nhwc_bf16 into slabs whose stride exceeds N * Ktot (the gaps keep their bits), then
        fx_unpack_conv_wgrad_sum_f32 (sum of the slabs x a power-of-two scale, accumulated into a prefilled [N][C][KH][KW] master)."""
        c, d = self.c, self.d
        Ho, Wo = TC.out_hw(c)
        S = self.lib.fx_conv2d_wgrad_splits(c.B, Ho, Wo, c.C, c.N, c.k, c.k)
        assert S >= 1
        slab, stride = c.N * self.Ktot, c.N * self.Ktot + 64
        pb = Buf(S, slab, stride, F32)
        check(self.lib.fx_conv2d_wgrad_partial_nhwc_bf16(self.xp, self.ldx, self.zp, self.lddz, pb.ptr, stride, S, *self.geom, stream()), "wgrad_partial")
        sb = Buf(1, c.N, c.N + 8, F32, data=d["scale"])
        ob = Buf(c.N, self.Ktot, self.Ktot, F32, prefill=TC.nckk(d["pre"]))
        check(self.lib.fx_unpack_conv_wgrad_sum_f32(pb.ptr, stride, S, sb.ptr, ob.ptr, c.N, c.C, c.k, c.k, c.C, 1, stream()), "unpack_sum")
        torch.cuda.synchronize()
        pb.assert_guards()
        ob.assert_guards()
        sc = d["scale"].double().view(-1, 1, 1, 1)
        pre = TC.nckk(d["pre"]).double()
        compare(form, f"{TC.wid(c)} partial S={S}", self.kind, ob.get().reshape(pre.shape), TC.nckk(self.ref) * sc + pre, TC.nckk(self.mag) * sc + pre.abs(),
                self.M)
        return S


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.WGRAD_SMALL, ids=TC.wid)
def test_wgrad_small(lib, case, kind):
    """conv_wgrad_kernel<PW> through its three conv entries at the sizes where its pipeline, tiles and index carry change path (the notes
    of TC.WGRAD_SMALL).  The bias entry runs on every case: 2x12x12-c24-n136 has two N tiles and two K tiles, and only the kt == 0
    workgroups may add to dbias - an integer dbias that came out doubled is a bit mismatch.
    Measured c: see MEASURED (wgrad.pw, wgrad.im2col, wgrad.dbias)."""
    w = Wgrad(lib, case, kind)
    assert w.variant() == case.variant
    w.atomic(False)
    w.atomic(True)
    S = w.partial(FORM[case.variant])
    assert S == (2 if w.M > 512 else 1)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.WGRAD_DEFAULT, ids=TC.wid)
def test_wgrad_at_the_default_threshold(lib, case, kind):
    """The partial-slab entry at the smallest wide shapes that cross FX_WGRAD_DMA_MIN_GFLOP = 8 (conv_wgrad_dma_kernel<PW> with its 4-stage
    LDS-DMA ring, source-side swizzle and counted waits, 3x3 and pointwise) and one just below (the 128 x 128 kernel).
    Measured c: see MEASURED (wgrad_dma.3x3, wgrad_dma.pw, wgrad.im2col)."""
    w = Wgrad(lib, case, kind)
    assert w.variant() == case.variant
    assert (TC.gflop(case) >= 8.0) == case.variant.startswith("conv_wgrad_dma")
    w.partial(FORM[case.variant])


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.WGRAD_WIDE_SMALL, ids=TC.wid)
def test_wgrad_wide_small(lib, case, kind):
    """Wide layers (N, C multiples of 256) at small sizes.  In a process started with FX_WGRAD_DMA_MIN_GFLOP=0 (the child of the test
    below) they run on the DMA kernel - all but 64x5x5, whose images are smaller than a 32-pixel step's row advance and which is routed to
    the 128 x 128 kernel on the wide class's split plan; at the default threshold all run on the 128 x 128 kernel."""
    w = Wgrad(lib, case, kind)
    expect = case.variant if DMA0 else TC.IM2COL if case.k == 3 else TC.PW
    assert w.variant() == expect
    w.partial(FORM[expect])


def test_wgrad_wide_small_on_the_dma_kernel():
    """test_wgrad_wide_small again in ONE fresh process with FX_WGRAD_DMA_MIN_GFLOP=0: every case asserts its conv_wgrad_dma<...> variant
    (64x5x5: conv_wgrad<im2col>) and runs both the exact and the Gaussian run."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_train_matrix_ops.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_wgrad_wide_small and not on_the_dma_kernel"],
                       cwd=ROOT, env=dict(os.environ, FX_WGRAD_DMA_MIN_GFLOP="0"), capture_output=True, text=True, timeout=300)
    tail = r.stdout[-2000:] + r.stderr[-500:]
    assert r.returncode == 0, tail
    summary = r.stdout.strip().splitlines()[-1]
    assert re.search(rf"\b{2 * len(TC.WGRAD_WIDE_SMALL)} passed\b", summary) and "skipped" not in summary and "failed" not in summary, tail


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", TC.LINEAR_CASES, ids=TC.lid)
def test_linear_wgrad(lib, case, kind):
    """fx_linear_wgrad_bias_bf16 at the three production shapes (R = 600 rows) and with ld_dw > k_store: ONLY the n_store x k_store corner
    of dW and the first n_store bias gradients are accumulated - the kernel writes straight into master gradients, so the rows from
    n_store to Np, the columns from k_store to ld_dw and dbias[n_store:] (neighbours holding 1.0, see acc_buf) must keep their bits.  The
    padding columns of x and dz hold values, not zeros, so that a store outside the corner is not an add of 0.0.
    Measured c: see MEASURED (wgrad.pw, wgrad.dbias)."""
    c = case
    d = TC.linear_inputs(c, kind)
    assert TC.exact_run_is_exact(c.R)
    xb, xp = view(d["x"], 8, c.Kp + 40)
    zb, zp = view(d["dz"], 16, c.Np + 24)
    ref, mag, db, dbm = TC.linear_ref64(d["x"], d["dz"], c)
    dwb = acc_buf(d["pre"], c.Np, c.ld_dw)                      # Np rows: a row past n_store lands on a neighbour, not outside the buffer
    bb = acc_buf(d["bpre"].view(1, -1), 1, c.Np)
    check(lib.fx_linear_wgrad_bias_bf16(xp, c.Kp + 40, zp, c.Np + 24, dwb.ptr, c.ld_dw, bb.ptr if c.bias else None, c.R, c.Kp, c.Np, c.k_store, c.n_store,
                                        stream()), "fx_linear_wgrad_bias_bf16")
    torch.cuda.synchronize()
    compare("wgrad.pw", TC.lid(c), kind, acc_get(dwb, c.n_store, c.k_store), ref + d["pre"].double(), mag + d["pre"].double().abs(), c.R)
    got_b = acc_get(bb, 1, c.n_store).reshape(-1)
    if c.bias:
        compare("wgrad.dbias", TC.lid(c), kind, got_b, db + d["bpre"].double(), dbm + d["bpre"].double().abs(), c.R)
    else:
        assert torch.equal(got_b, d["bpre"])


# ------------------------------------------------------------------------------------------------ attention backward
def mha_bwd_run(lib, c, layout, entry="masked"):
    """layout "fused": q | k | v are column slices of ONE buffer with leading dimension 3 * heads * 32, dO / dQ / dK / dV have four more
    leading dimensions; "separate": seven buffers, seven leading dimensions.  The outputs are views with ld > heads * 32, the workspace is
    exactly fx_mha_bwd_workspace_bytes with guards behind it, the mask rows are one word longer than needed.
    entry "masked": fx_mha_masked_bwd_bf16 (null mask for an unmasked case); "plain": fx_mha_bwd_bf16 with o = None.
    Returns (dq, dk, dv) as bf16 [B, L, E] on the CPU."""
    B, heads, Lq, Lk = c["B"], c["heads"], c["Lq"], c["Lk"]
    E = heads * 32
    if layout == "fused":
        rows = B * max(Lq, Lk)
        data = torch.full((rows, 3 * E), float("nan"))
        data[:B * Lq, :E], data[:B * Lk, E:2 * E], data[:B * Lk, 2 * E:] = c["q"].reshape(-1, E), c["k"].reshape(-1, E), c["v"].reshape(-1, E)
        pk = Buf(rows, 3 * E, 3 * E, BF, data=data)
        (qp, ldq), (kp, ldk), (vp, ldv) = (pk.ptr, 3 * E), (pk.ptr + 2 * E, 3 * E), (pk.ptr + 4 * E, 3 * E)
    else:
        qb, kb, vb = Buf(B * Lq, E, E + 40, BF, data=c["q"]), Buf(B * Lk, E, E + 48, BF, data=c["k"]), Buf(B * Lk, E, E + 56, BF, data=c["v"])
        (qp, ldq), (kp, ldk), (vp, ldv) = (qb.ptr, E + 40), (kb.ptr, E + 48), (vb.ptr, E + 56)
    dob = Buf(B * Lq, E, E + 8, BF, data=c["do"])
    dqb, dkb, dvb = Buf(B * Lq, E, E + 16, BF), Buf(B * Lk, E, E + 24, BF), Buf(B * Lk, E, E + 32, BF)
    T = (Lk + 31) // 32
    mb = Buf(B * Lq, T, T + 1, I32, data=TC.mask_words(c["mask"])) if c["mask"] is not None else None
    nws = lib.fx_mha_bwd_workspace_bytes(B, Lq, Lk, heads)
    assert nws == 12 * B * heads * Lq
    wsb = Buf(1, nws // 4, nws // 4 + 8, F32)
    if entry == "plain":
        assert mb is None
        check(lib.fx_mha_bwd_bf16(qp, ldq, kp, ldk, vp, ldv, None, 0, dob.ptr, E + 8, dqb.ptr, E + 16, dkb.ptr, E + 24, dvb.ptr, E + 32, B, Lq, Lk, heads,
                                  wsb.ptr, nws, stream()), "fx_mha_bwd_bf16")
    else:
        check(lib.fx_mha_masked_bwd_bf16(qp, ldq, kp, ldk, vp, ldv, dob.ptr, E + 8, dqb.ptr, E + 16, dkb.ptr, E + 24, dvb.ptr, E + 32, B, Lq, Lk, heads,
                                         mb.ptr if mb else None, T + 1 if mb else 0, wsb.ptr, nws, stream()), "fx_mha_masked_bwd_bf16")
    torch.cuda.synchronize()
    for b in (dqb, dkb, dvb, wsb):
        b.assert_guards()
    return dqb.get().reshape(B, Lq, E), dkb.get().reshape(B, Lk, E), dvb.get().reshape(B, Lk, E)


def mha_gate(c, got, what):
    pre = "mha_bwd_masked" if c["mask"] is not None else "mha_bwd"
    for name, g in zip(("dq", "dk", "dv"), got):
        helpers.gate(f"{pre}.{name}", what, g, c[name], c[name + "_mag"], BF, MEASURED, MARGIN)


def same_bits(a, b):
    return all(torch.equal(_bits(x.contiguous()), _bits(y.contiguous())) for x, y in zip(a, b))


# | Lq, Lk | reaches                                                                                     |
# | 1      | one row of one tile                                                                         |
# | 31, 33 | a partial tile; a full tile and one row                                                     |
# | 128    | exactly the AB_QT = 4 query tiles of one LDS chunk of the dK / dV kernel; one grid block    |
# | 129    | the next query chunk holds one row; a second grid block, three of its waves inactive        |
# | 256    | exactly the AB_CT = 8 key tiles of one LDS chunk of the dQ kernel                           |
# | 257    | the next key chunk holds one key                                                            |
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", TC.MHA_BWD_CASES, ids=TC.mid)
def test_mha_bwd(lib, case, masked):
    """dQ, dK, dV of both entry points over the (B, heads, Lq, Lk) table of TC.MHA_BWD_CASES in both layouts.  Every masked case holds a
    fully masked query (attends everywhere), a fully open one and one whose only allowed key is the last key, at both ends of the query
    range where there is room.  Unmasked: fx_mha_bwd_bf16 with o = None gives the bits of the masked entry with a null mask.
    Measured c: see MEASURED (mha_bwd.*, mha_bwd_masked.*)."""
    c = TC.mha_bwd_case(case, masked)
    for layout in ("fused", "separate"):
        got = mha_bwd_run(lib, c, layout)
        mha_gate(c, got, f"{TC.mid(case)} {layout}")
        if not masked:
            assert same_bits(got, mha_bwd_run(lib, c, layout, "plain"))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_mha_bwd_large_scores(lib, masked):
    """Scores of magnitude ~60 over nine key tiles in two LDS chunks: the statistics sweep rescales its running sums by
    exp2(m_old - m_new) from tile to tile, and the probabilities of the second sweep are exp2(s - lse) of large arguments."""
    c = TC.mha_bwd_case(TC.MHA_BWD_BIG, masked, big=True)
    assert c["smax"] > 40
    mha_gate(c, mha_bwd_run(lib, c, "fused"), f"{TC.mid(TC.MHA_BWD_BIG)} big")


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_mha_bwd_uniform_attention(lib, masked):
    """K = 0: P = 1 / (allowed keys), so dQ = dS K is exactly 0 and every key and query tile carries the same share of dV and dK - a dropped
    tile shifts them by a whole tile's share, far above the gate."""
    c = TC.mha_bwd_case(TC.MHA_BWD_UNIFORM, masked, uniform=True)
    got = mha_bwd_run(lib, c, "separate")
    assert not bool(got[0].float().any()), "dQ must be exactly 0 when K = 0"
    mha_gate(c, got, f"{TC.mid(TC.MHA_BWD_UNIFORM)} uniform")


def test_rejected_arguments(lib):
    """Leading dimensions below heads * 32 (inputs AND outputs), a short workspace, mask rows shorter than the keys need and a leading
    dimension that is no multiple of 8 are refused before anything is launched: the outputs keep their sentinel."""
    B, heads, Lq, Lk = 1, 2, 33, 33
    E, LD = heads * 32, heads * 32 + 8
    c = TC.mha_bwd_case(TC.MCase(B, heads, Lq, Lk), True)
    ib = [Buf(Lq, E, LD, BF, data=c[n]) for n in ("q", "k", "v", "do")]
    ob = [Buf(Lq, E, LD, BF) for _ in range(3)]
    mb = Buf(Lq, 2, 3, I32, data=TC.mask_words(c["mask"]))
    nws = lib.fx_mha_bwd_workspace_bytes(B, Lq, Lk, heads)
    wsb = Buf(1, nws // 4, nws // 4 + 8, F32)
    s = stream()

    def call(lds=(LD,) * 7, ws=nws, ldm=3, mask=True, plain=False):
        p = [b.ptr for b in ib + ob]
        if plain:
            return lib.fx_mha_bwd_bf16(p[0], lds[0], p[1], lds[1], p[2], lds[2], None, 0, p[3], lds[3], p[4], lds[4], p[5], lds[5], p[6], lds[6], B, Lq,
                                       Lk, heads, wsb.ptr, ws, s)
        return lib.fx_mha_masked_bwd_bf16(p[0], lds[0], p[1], lds[1], p[2], lds[2], p[3], lds[3], p[4], lds[4], p[5], lds[5], p[6], lds[6], B, Lq, Lk,
                                          heads, mb.ptr if mask else None, ldm if mask else 0, wsb.ptr, ws, s)

    def with_ld(i, v):
        return tuple(v if j == i else LD for j in range(7))

    bad = {}
    for i, n in enumerate(("ldq", "ldk", "ldv", "lddo", "lddq", "lddk", "lddv")):
        bad[f"{n} < heads * 32"] = lambda i=i: call(with_ld(i, 32))
        bad[f"{n} < heads * 32 (unmasked entry)"] = lambda i=i: call(with_ld(i, 32), plain=True)
        bad[f"{n} % 8"] = lambda i=i: call(with_ld(i, E + 4))
    bad["short workspace"] = lambda: call(ws=nws - 1)
    bad["short workspace (unmasked entry)"] = lambda: call(ws=nws - 1, plain=True)
    bad["ld_mask_words too small"] = lambda: call(ldm=1)
    for what, fn in bad.items():
        with pytest.raises(FocoosAmdError):
            check(fn(), what)
            pytest.fail(f"{what}: accepted")
    torch.cuda.synchronize()
    for b in ob + [wsb]:
        b.assert_guards(written=torch.zeros(b.rows, dtype=torch.bool))
    check(call(), "valid call")                                   # the same buffers with valid arguments are accepted
    torch.cuda.synchronize()
    for b in ob + [wsb]:
        b.assert_guards()
    mha_gate(c, [b.get().reshape(B, Lq, E) for b in ob], "after the rejected calls")
