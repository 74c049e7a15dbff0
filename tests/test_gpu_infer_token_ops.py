"""The small inference-side kernels, called directly on a real MI355X: csrc/token_ops.hip (row add, LayerNorm over 128 / 256 channels,
head-dim-32 attention, deformable-attention sampling), csrc/pixel_ops.hip (the two bilinear resizes, the two pools) and
csrc/select_ops.hip (row max, gather, fill, the K = 4 and N = 4 heads, the output head, the DETR post-process, top-k order).  Cases,
float64 references and magnitudes come from tests/infer_token_cases.py; tests/test_infer_token_cases_cpu.py checks those references
against independent formulations without a GPU.

Rules every case follows (those of tests/test_gpu_train_token_ops.py; the helpers are tests/helpers.Buf / gate)
* Guards: every device buffer sits inside guard rows and has a leading dimension above its column count (the engine calls these kernels
  on views: a slice of value_all, q / k / v packed in one buffer, outputs inside wider rows); flat arrays without a leading dimension
  are one-row buffers between guard rows.  Outputs are prefilled with a sentinel bit pattern and everything outside the written region
  must keep it bit for bit; the padding of floating-point inputs is NaN, so a read outside the logical region poisons the result.
* Exact where the arithmetic allows (one fp32 addition, maxima, copies, integer results): bit equality.
* Otherwise, element by element, no element excluded:  |got - ref| <= RND(ref) + c * mag.  RND(ref) is ONE rounding to the output type
  (2^-8 |ref| for bf16, 2^-24 |ref| for fp32, + 2^-126); mag is the float64 value of the same expression with every term in absolute
  value; c is the kernel's fp32-arithmetic slack: MEASURED[kernel] is the largest c any case of that kernel needed on an MI355X against
  the float64 reference, the gate is MARGIN = 4 times that (the fast-math intrinsics' error varies with the argument).  Every test
  prints the c it needs (EXCESS <kernel> <c> <case>) before it asserts.
  Expectations the figures were checked against: fp32 chains with one rounding need c near fp32 roundoff (6e-8) or below; attention
  rounds the un-normalised probabilities to bf16 before the second matrix product, c near 2^-9 = 2e-3."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FocoosAmdError, check  # noqa: E402
from tests import helpers  # noqa: E402
from tests import infer_token_cases as IC  # noqa: E402
from tests.helpers import Buf, _bits  # noqa: E402

BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
MARGIN = 4.0
# largest c = (|got - ref| - RND(ref)) / mag over all cases of the kernel, measured on an MI355X against the float64 reference
MEASURED = {
    "layernorm128": 2.203e-08,
    "layernorm256": 3.145e-08,
    "mha": 2.510e-03,
    "mha.split": 9.647e-04,
    "msda.mode0": 5.205e-09,
    "msda.mode1": 1.202e-09,
    "resize_u8": 1.642e-08,
    "resize_nhwc": 0.0,
    "avgpool": 0.0,
    "linear_k4_relu": 0.0,
    "bbox_head.unact": 7.882e-08,
    "bbox_head.new_ref": 8.992e-08,
    "detr_head_out.probs": 3.975e-08,
    "detr_head_out.boxes": 0.0,
}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load("bf16")            # the inference engines are bf16 whatever type a training step of the same process pinned


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gate(kernel, what, got, ref, mag, dtype=BF):
    helpers.gate(kernel, what, got, ref, mag, dtype, MEASURED, MARGIN)


def flat(t, dtype, out=False):
    """A flat array (no leading dimension in the API) as a one-row buffer between guard rows; t: the data, or for outputs the length."""
    if out:
        return Buf(1, t, t + 8, dtype)
    return Buf(1, t.numel(), t.numel() + 8, dtype, data=t)


def same_bits(got, ref):
    return torch.equal(_bits(got.contiguous()), _bits(ref.to(got.dtype).contiguous()))


def untouched(*bufs):
    for b in bufs:
        b.assert_guards(written=torch.zeros(b.rows, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ add_rows
@pytest.mark.parametrize("case", IC.ADD_ROWS_CASES, ids=lambda c: f"{c[0]}x{c[1]}y{c[2]}")
def test_add_rows(lib, case):
    """out[r] = x[r] + y[r % y_rows] with three different leading dimensions: bit-equal to bf16_rne of the float64 sum.  37 rows over 5 or 7
    rows of y: the wrap does not divide; 5 rows over 7: no wrap, y longer than x."""
    rows, cols, y_rows = case
    c = IC.add_rows_case(*case)
    xb, yb, ob = Buf(rows, cols, cols + 8, BF, data=c["x"]), Buf(y_rows, cols, cols + 16, BF, data=c["y"]), Buf(rows, cols, cols + 24, BF)
    check(lib.fx_add_rows_bf16(xb.ptr, cols + 8, yb.ptr, cols + 16, y_rows, ob.ptr, cols + 24, rows, cols, stream()), "fx_add_rows_bf16")
    torch.cuda.synchronize()
    ob.assert_guards()
    assert same_bits(ob.get(), c["ref"])


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_run(lib, c, cols, rows, ldx=None, ldr=None, ldo=None, cols_arg=None):
    xb = Buf(rows, cols, cols + 8, BF, data=c["x"])
    rb = Buf(rows, cols, cols + 4, BF, data=c["res"]) if c["res"] is not None else None
    gb, bb, ob = flat(c["gamma"], F32), flat(c["beta"], F32), Buf(rows, cols, cols + 12, BF)
    rc = lib.fx_layernorm_bf16(xb.ptr, ldx or cols + 8, rb.ptr if rb else None, (ldr or cols + 4) if rb else 0, gb.ptr, bb.ptr, ob.ptr, ldo or cols + 12,
                               rows, cols_arg or cols, stream())
    torch.cuda.synchronize()
    return rc, ob


@pytest.mark.parametrize("case", IC.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}{'+res' if c[2] else ''}-{c[3]}")
def test_layernorm(lib, case):
    """fx_layernorm_bf16 over 128 (layernorm128_kernel) and 256 channels, rows 1 / 4 / 9 (a workgroup is four rows: a partial one, a full
    one, two and a partial third), with and without residual, and at row mean 40 / spread 0.5 (two-pass variance).
    Measured c: see MEASURED (layernorm128, layernorm256)."""
    cols, rows, res, variant = case
    c = IC.layernorm_case(*case)
    rc, ob = ln_run(lib, c, cols, rows)
    check(rc, "fx_layernorm_bf16")
    ob.assert_guards()
    gate(f"layernorm{cols}", f"rows{rows} res{int(res)} {variant}", ob.get(), c["ref"], c["mag"])


# ------------------------------------------------------------------------------------------------ attention
# | Lq  | Lk   | reaches                                                              |
# | 1   | 1    | one query, one key                                                   |
# | 37  | 31   | one partial tile                                                     |
# | 130 | 32   | second query block, two of its waves inactive                        |
# | 77  | 448  | exactly the 14 tiles held in LDS                                     |
# | 77  | 449  | the next chunk holds one key                                         |
# | 7   | 1056 | T = 33: split path with a workspace, whole-key path without one      |
def mha_run(lib, c, heads, Lq, Lk, layout, use_ws):
    """layout "packed": q | k | v are column slices of ONE buffer with leading dimension 3 * heads * 32 (768 at 8 heads); "separate": three
    buffers with three leading dimensions.  Returns (out [B, Lq, E], whether the key-split path ran)."""
    B, E = c["B"], heads * 32
    masked = c["mask"] is not None
    if layout == "packed":
        rows = B * max(Lq, Lk)
        data = torch.full((rows, 3 * E), float("nan"))
        data[:B * Lq, :E], data[:B * Lk, E:2 * E], data[:B * Lk, 2 * E:] = c["q"].reshape(-1, E), c["k"].reshape(-1, E), c["v"].reshape(-1, E)
        pk = Buf(rows, 3 * E, 3 * E, BF, data=data)
        (qp, ldq), (kp, ldk), (vp, ldv) = (pk.ptr, 3 * E), (pk.ptr + 2 * E, 3 * E), (pk.ptr + 4 * E, 3 * E)
    else:
        qb, kb, vb = Buf(B * Lq, E, E + 8, BF, data=c["q"]), Buf(B * Lk, E, E + 16, BF, data=c["k"]), Buf(B * Lk, E, E + 24, BF, data=c["v"])
        (qp, ldq), (kp, ldk), (vp, ldv) = (qb.ptr, E + 8), (kb.ptr, E + 16), (vb.ptr, E + 24)
    ob = Buf(B * Lq, E, E + 12, BF)
    T = (Lk + 31) // 32
    mb = Buf(B * Lq, T, T + 1, I32, data=IC.mask_words(c["mask"])) if masked else None
    nws = lib.fx_mha_workspace_bytes(B, Lq, Lk, heads, int(masked)) if use_ws else 0
    wsb = flat(nws // 4, F32, out=True) if nws else None
    if masked or wsb:
        check(lib.fx_mha_masked_bf16(qp, ldq, kp, ldk, vp, ldv, ob.ptr, E + 12, B, Lq, Lk, heads, mb.ptr if mb else None, T + 1 if mb else 0,
                                     wsb.ptr if wsb else None, nws, stream()), "fx_mha_masked_bf16")
    else:
        check(lib.fx_mha_bf16(qp, ldq, kp, ldk, vp, ldv, ob.ptr, E + 12, B, Lq, Lk, heads, stream()), "fx_mha_bf16")
    torch.cuda.synchronize()
    ob.assert_guards()
    if wsb:
        wsb.assert_guards()
    return ob.get().reshape(B, Lq, E), bool(nws)


@pytest.mark.parametrize("layout", ["packed", "separate"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("pair", IC.MHA_PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_mha(lib, pair, masked, layout):
    """fx_mha_bf16 / fx_mha_masked_bf16 at 8 heads over the (Lq, Lk) table above.  Every masked case holds a fully masked query (attends
    everywhere), a fully open one and one whose only allowed key is the last key, at both ends of the query range.  (7, 1056) runs twice:
    with the workspace (key-split kernel + merge kernel) and without (one workgroup walks all 33 tiles in three LDS chunks).
    Measured c: see MEASURED (mha, mha.split)."""
    Lq, Lk = pair
    c = IC.mha_case(Lq, Lk, 8, masked)
    for use_ws in ((True, False) if Lk == 1056 else (False,)):
        out, split = mha_run(lib, c, 8, Lq, Lk, layout, use_ws)
        assert split == use_ws
        gate("mha.split" if split else "mha", f"{Lq}x{Lk} {'masked' if masked else 'plain'} {layout}", out, c["ref"], c["mag"])


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_mha_two_heads(lib, masked):
    """heads = 2 (E = 64) with ldq = 72 > 64 and, packed, ld 192: the head index / leading dimension arithmetic away from 8 x 32 = 256."""
    c = IC.mha_case(37, 31, 2, masked)
    for layout in ("separate", "packed"):
        out, _ = mha_run(lib, c, 2, 37, 31, layout, False)
        gate("mha", f"37x31 heads2 {'masked' if masked else 'plain'} {layout}", out, c["ref"], c["mag"])


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_mha_large_scores(lib, masked):
    """Scores of magnitude ~60 over 15 key tiles in two LDS chunks: the running maximum rises from tile to tile and the accumulated output
    and sum are rescaled by exp2(m_old - m_new) each time; a missed rescale is off by factors of e^10."""
    c = IC.mha_case(77, 449, 8, masked, big=True)
    assert c["smax"] > 40
    out, _ = mha_run(lib, c, 8, 77, 449, "packed", False)
    gate("mha", f"77x449 big {'masked' if masked else 'plain'}", out, c["ref"], c["mag"])


# ------------------------------------------------------------------------------------------------ deformable sampling
def msda_run(lib, c, mode, shift, M=8):
    """value: the 256-column slice at column 256 of a [B * S][1536] buffer (value_all of the engine), ldo = 272.  shift = 1: the offsets
    (mode 1: offsets | logits) start one float into their buffer, so their rows are not 16-byte aligned."""
    B, Q, S, L, P = c["B"], c["Q"], c["S"], c["L"], c["P"]
    data = torch.full((B * S, 1536), float("nan"))
    data[:, 256:512] = c["value"].reshape(B * S, 256)
    vb = Buf(B * S, 1536, 1536, BF, data=data)
    sb = flat(torch.tensor(c["shapes"], dtype=torch.int32), I32)
    stb = flat(torch.tensor(c["starts"], dtype=torch.int32), I32)
    n_loc, n_att = 8 * L * P * 2, 8 * L * P
    ob = Buf(B * Q, 256, 272, BF)

    def shifted(t, cols, ld):
        d = torch.full((B * Q, cols + shift), float("nan"))
        d[:, shift:] = t.reshape(B * Q, cols)
        return Buf(B * Q, cols + shift, ld, F32, data=d)

    if mode == 0:
        lb, ab, rb = shifted(c["loc"], n_loc, n_loc + 8), Buf(B * Q, n_att, n_att + 4, F32, data=c["attn"]), None
        lp, ld_loc, ap, ld_att = lb.ptr + 4 * shift, n_loc + 8, ab.ptr, n_att + 4
    else:
        lb = shifted(torch.cat([c["off"].reshape(B * Q, n_loc), c["logits"].reshape(B * Q, n_att)], 1), n_loc + n_att, n_loc + n_att + 8)
        rb = flat(c["ref4"], F32)
        lp, ld_loc = lb.ptr + 4 * shift, n_loc + n_att + 8
        ap, ld_att = lp + 4 * n_loc, ld_loc
    fast = L == 3 and P == 4 and lp % 16 == 0 and ap % 16 == 0 and ld_loc % 4 == 0 and ld_att % 4 == 0 and (rb is None or rb.ptr % 16 == 0)
    rc = lib.fx_msda_bf16(vb.ptr + 2 * 256, 1536, sb.ptr, stb.ptr, L, P, lp, ld_loc, ap, ld_att, rb.ptr if rb else None, mode, ob.ptr, 272, B, S, Q, M,
                          stream())
    torch.cuda.synchronize()
    return rc, ob, fast


@pytest.mark.parametrize("mode", [0, 1], ids=["core", "fused"])
def test_msda_l3p4_and_generic(lib, mode):
    """Levels 5x7, 3x4, 2x2 with 4 points: 16-byte aligned rows of offsets / logits reach msda_l3p4_kernel, the same inputs one float into
    their buffer reach the generic msda_kernel; both are gated against the float64 reference with the same constant.  Samples at exactly
    0 and 1, half a pixel outside each border and at +-1e6, on every level (tests/test_infer_token_cases_cpu.py asserts where the taps fall).
    Measured c: see MEASURED (msda.mode0, msda.mode1)."""
    c = IC.msda_case(IC.MSDA_L3, 4, mode)
    for shift in (0, 1):
        rc, ob, fast = msda_run(lib, c, mode, shift)
        check(rc, "fx_msda_bf16")
        assert fast == (shift == 0), "the aligned call must meet the l3p4 kernel's conditions, the shifted one must not"
        ob.assert_guards()
        gate(f"msda.mode{mode}", f"L3P4 {'l3p4' if fast else 'generic'}", ob.get().reshape(c["ref"].shape), c["ref"], c["mag"])


@pytest.mark.parametrize("mode", [0, 1], ids=["core", "fused"])
def test_msda_generic_l2p3(lib, mode):
    """L = 2, P = 3: msda_kernel<mode> only (6 points per head: its loops are not the unrolled 12)."""
    c = IC.msda_case(IC.MSDA_L2, 3, mode)
    rc, ob, fast = msda_run(lib, c, mode, 0)
    check(rc, "fx_msda_bf16")
    assert not fast
    ob.assert_guards()
    gate(f"msda.mode{mode}", "L2P3 generic", ob.get().reshape(c["ref"].shape), c["ref"], c["mag"])


# ------------------------------------------------------------------------------------------------ resizes and pools
@pytest.mark.parametrize("sizes", IC.RESIZE_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_u8(lib, sizes):
    """fx_resize_bilinear_u8 (uint8 HWC -> fp32): up x2 (exact fp32 coordinates), down by 2.25 / 1.8, and the identity (bit-exact).
    Measured c: see MEASURED (resize_u8)."""
    (H, W), (Ho, Wo) = sizes
    c = IC.resize_u8_case(*sizes)
    xb, yb = flat(c["x"], U8), flat(Ho * Wo * 3, F32, out=True)
    check(lib.fx_resize_bilinear_u8(xb.ptr, H, W, yb.ptr, Ho, Wo, stream()), "fx_resize_bilinear_u8")
    torch.cuda.synchronize()
    yb.assert_guards()
    got = yb.get().reshape(Ho, Wo, 3)
    if (H, W) == (Ho, Wo):
        assert torch.equal(got, c["x"].float())
    gate("resize_u8", f"{H}x{W}->{Ho}x{Wo}", got, c["ref"], c["mag"], F32)


@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("sizes", IC.RESIZE_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_nhwc(lib, sizes, Cc):
    """fx_resize_bilinear_nhwc_bf16 at C = 8 (one vector per pixel: the shift path) and C = 24 (three: the division path), input and output
    as views (ld = C + 8 / C + 16), two images.  The identity is bit-exact.  Measured c: see MEASURED (resize_nhwc)."""
    (H, W), (Ho, Wo) = sizes
    c = IC.resize_nhwc_case(*sizes, Cc)
    B = c["x"].shape[0]
    xb, yb = Buf(B * H * W, Cc, Cc + 8, BF, data=c["x"]), Buf(B * Ho * Wo, Cc, Cc + 16, BF)
    check(lib.fx_resize_bilinear_nhwc_bf16(xb.ptr, Cc + 8, yb.ptr, Cc + 16, B, H, W, Cc, Ho, Wo, stream()), "fx_resize_bilinear_nhwc_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    got = yb.get().reshape(B, Ho, Wo, Cc)
    if (H, W) == (Ho, Wo):
        assert same_bits(got, c["x"])
    gate("resize_nhwc", f"{H}x{W}->{Ho}x{Wo} C{Cc}", got, c["ref"], c["mag"])


@pytest.mark.parametrize("case", IC.MAXPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}{'neg' if c[2] else ''}")
def test_maxpool(lib, case):
    """fx_maxpool3x3s2_nhwc_bf16, bit for bit: 1x1 (every tap but one is padding), a single row, odd and even sizes, and an input of
    negative values only (the padding is -inf, not 0)."""
    H, W, _ = case
    c = IC.maxpool_case(*case)
    B, Cc = c["x"].shape[0], c["x"].shape[3]
    Ho, Wo = c["ref"].shape[1:3]
    xb, yb = Buf(B * H * W, Cc, Cc + 8, BF, data=c["x"]), Buf(B * Ho * Wo, Cc, Cc + 16, BF)
    check(lib.fx_maxpool3x3s2_nhwc_bf16(xb.ptr, Cc + 8, yb.ptr, Cc + 16, B, H, W, Cc, stream()), "fx_maxpool3x3s2_nhwc_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    assert same_bits(yb.get().reshape(c["ref"].shape), c["ref"])


@pytest.mark.parametrize("case", IC.AVGPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_avgpool(lib, case):
    """fx_avgpool2x2_nhwc_bf16 (ceil mode: border windows of 1 or 2 taps divide by 1 or 2).  Measured c: see MEASURED (avgpool)."""
    H, W = case
    c = IC.avgpool_case(*case)
    B, Cc = c["x"].shape[0], c["x"].shape[3]
    Ho, Wo = c["ref"].shape[1:3]
    xb, yb = Buf(B * H * W, Cc, Cc + 8, BF, data=c["x"]), Buf(B * Ho * Wo, Cc, Cc + 16, BF)
    check(lib.fx_avgpool2x2_nhwc_bf16(xb.ptr, Cc + 8, yb.ptr, Cc + 16, B, H, W, Cc, stream()), "fx_avgpool2x2_nhwc_bf16")
    torch.cuda.synchronize()
    yb.assert_guards()
    gate("avgpool", f"{H}x{W}", yb.get().reshape(c["ref"].shape), c["ref"], c["mag"])


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("cols", IC.ROWMAX_COLS)
def test_rowmax(lib, cols):
    """fx_rowmax_f32 over the first `cols` of 368 columns (NaN behind them), 5 rows (a partial second workgroup), one row of -inf: exact."""
    c = IC.rowmax_case(cols)
    xb, ob = Buf(5, cols, 368, F32, data=c["x"]), flat(5, F32, out=True)
    check(lib.fx_rowmax_f32(xb.ptr, 368, ob.ptr, 5, cols, stream()), "fx_rowmax_f32")
    torch.cuda.synchronize()
    ob.assert_guards()
    assert same_bits(ob.get()[0], c["ref"])


@pytest.mark.parametrize("cols", [8, 256])
def test_gather_fill(lib, cols):
    """fx_gather_rows_bf16 / fx_fill_rows_bf16 with rows_per_batch = 11 != k = 4, three images, repeated indices, views: bit for bit; the
    rows fill does not name keep their content, everything around the matrix keeps the sentinel; n_idx = 0 leaves it all untouched."""
    B, rpb, k = 3, 11, 4
    c = IC.gather_fill_case(cols, B, rpb, k)
    sb, ib, ob = Buf(B * rpb, cols, cols + 8, BF, data=c["src"]), flat(c["idx"], I32), Buf(B * k, cols, cols + 16, BF)
    check(lib.fx_gather_rows_bf16(sb.ptr, cols + 8, rpb, ib.ptr, k, ob.ptr, cols + 16, B, cols, stream()), "fx_gather_rows_bf16")
    xb, rib, rvb = Buf(B * rpb, cols, cols + 8, BF, prefill=c["src"]), flat(c["rows_idx"], I32), flat(c["rowv"], BF)
    check(lib.fx_fill_rows_bf16(xb.ptr, cols + 8, rpb, None, 0, rvb.ptr, B, cols, stream()), "fx_fill_rows_bf16 n_idx = 0")
    torch.cuda.synchronize()
    xb.assert_guards()
    assert same_bits(xb.get().reshape(B, rpb, cols), c["src"])
    check(lib.fx_fill_rows_bf16(xb.ptr, cols + 8, rpb, rib.ptr, len(c["rows_idx"]), rvb.ptr, B, cols, stream()), "fx_fill_rows_bf16")
    torch.cuda.synchronize()
    ob.assert_guards()
    xb.assert_guards()
    assert same_bits(ob.get().reshape(B, k, cols), c["gathered"])
    assert same_bits(xb.get().reshape(B, rpb, cols), c["filled"])


@pytest.mark.parametrize("N", [8, 512])
def test_linear_k4_relu(lib, N):
    """fx_linear_k4_relu, 3 rows, N = 8 (one vector per row) and 512, output as a view.  Measured c: see MEASURED (linear_k4_relu)."""
    c = IC.linear_k4_case(N)
    xb, wb, bb, ob = flat(c["x"], F32), flat(c["w"], F32), flat(c["b"], F32), Buf(3, N, N + 8, BF)
    check(lib.fx_linear_k4_relu(xb.ptr, wb.ptr, bb.ptr, ob.ptr, N + 8, 3, N, stream()), "fx_linear_k4_relu")
    torch.cuda.synchronize()
    ob.assert_guards()
    gate("linear_k4_relu", f"N{N}", ob.get(), c["ref"], c["mag"])


@pytest.mark.parametrize("mode", [0, 1], ids=["decoder", "encoder"])
@pytest.mark.parametrize("K", [128, 256])
def test_bbox_head(lib, K, mode):
    """fx_bbox_head at K = 128 (half of the lanes idle) and 256, 5 rows (a partial second workgroup), ldh = K + 4.  mode 0: reference boxes
    0, 1, 1e-7, 1 - 1e-7, -0.01 and 1.01 (inverse_sigmoid's clamps); mode 1: anchors gathered through idx.  Both outputs (pre-sigmoid and
    new reference) are fp32.  Measured c: see MEASURED (bbox_head.unact, bbox_head.new_ref)."""
    rows = 5
    c = IC.bbox_head_case(K, mode, rows)
    hb, wb, bb = Buf(rows, K, K + 4, BF, data=c["h"]), flat(c["w"], F32), flat(c["b"], F32)
    nb, ub = flat(rows * 4, F32, out=True), flat(rows * 4, F32, out=True)
    if mode == 0:
        rb = flat(c["ref4"], F32)
        rc = lib.fx_bbox_head(hb.ptr, K + 4, wb.ptr, bb.ptr, rb.ptr, None, None, rows, 0, nb.ptr, ub.ptr, rows, K, stream())
    else:
        ab, ib = flat(c["anchors"], F32), flat(c["idx"], I32)
        rc = lib.fx_bbox_head(hb.ptr, K + 4, wb.ptr, bb.ptr, None, ab.ptr, ib.ptr, rows, 1, nb.ptr, ub.ptr, rows, K, stream())
    check(rc, "fx_bbox_head")
    torch.cuda.synchronize()
    nb.assert_guards()
    ub.assert_guards()
    gate("bbox_head.unact", f"K{K} mode{mode}", ub.get().reshape(rows, 4), c["u"], c["mag_u"], F32)
    gate("bbox_head.new_ref", f"K{K} mode{mode}", nb.get().reshape(rows, 4), c["new"], c["mag_new"], F32)


@pytest.mark.parametrize("K", [4, 365])
def test_detr_head_out(lib, K):
    """fx_detr_head_out with K = 4 (every column also writes a box coordinate) and 365 of 368 columns (NaN behind them), logits 0, +-30
    and -100.  Measured c: see MEASURED (detr_head_out.probs, detr_head_out.boxes)."""
    rows = 5
    c = IC.head_out_case(K, rows)
    lb, rb = Buf(rows, K, 368, F32, data=c["logits"]), flat(c["ref4"], F32)
    pb, xb = flat(rows * K, F32, out=True), flat(rows * 4, F32, out=True)
    check(lib.fx_detr_head_out(lb.ptr, 368, rb.ptr, pb.ptr, xb.ptr, rows, K, stream()), "fx_detr_head_out")
    torch.cuda.synchronize()
    pb.assert_guards()
    xb.assert_guards()
    gate("detr_head_out.probs", f"K{K}", pb.get().reshape(rows, K), c["probs"], c["mag_p"], F32)
    gate("detr_head_out.boxes", f"K{K}", xb.get().reshape(rows, 4), c["boxes"], c["mag_b"], F32)


@pytest.mark.parametrize("entry", ["rows", "rows_ws"])
@pytest.mark.parametrize("case", IC.TOPK_CASES, ids=lambda c: f"n{c[0]}")
def test_topk_order(lib, case, entry):
    """fx_topk_rows_f32 / fx_topk_rows_ws_f32 on rows of n values inside a leading dimension ld > n with NaN behind them: indices and values
    bit for bit in the documented order (value descending, index ascending among equals = one stable sort).  Row 2 puts zeros of both
    signs across the cut: -0.0 and +0.0 are equal, the two of lowest index are taken (the first a -0.0) and come back as +0.0.  n = 8200
    makes the workspace entry point run its two-level form (chunks of 8192)."""
    n, ld, k = case
    c = IC.topk_case(*case)
    sb, vb, ib = Buf(3, n, ld, F32, data=c["s"]), flat(3 * k, F32, out=True), flat(3 * k, I32, out=True)
    if entry == "rows":
        check(lib.fx_topk_rows_f32(sb.ptr, ld, 3, n, k, vb.ptr, ib.ptr, stream()), "fx_topk_rows_f32")
    else:
        nws = lib.fx_topk_rows_workspace_bytes(3, n, k)
        assert (nws > 0) == (n > 8192)
        wsb = flat(nws // 4, I32, out=True) if nws else None
        check(lib.fx_topk_rows_ws_f32(sb.ptr, ld, 3, n, k, vb.ptr, ib.ptr, wsb.ptr if wsb else None, nws, stream()), "fx_topk_rows_ws_f32")
        torch.cuda.synchronize()
        if wsb:
            wsb.assert_guards()
    torch.cuda.synchronize()
    vb.assert_guards()
    ib.assert_guards()
    assert torch.equal(ib.get().reshape(3, k).long(), c["order"]), "indices must be bit-exact"
    assert same_bits(vb.get().reshape(3, k), c["vals"])


def test_detr_postprocess_ties_and_threshold(lib):
    """fx_detr_postprocess on box coordinates whose product with the image size (512, 1024) is exactly j + 0.5 - even j, odd j, negative:
    torch.round's half-to-even, bit for bit over ALL top_k slots - and on scores of which one equals the threshold (strict >: not
    counted).  Labels, queries, integer boxes and count are exact."""
    c = IC.postprocess_case()
    B, Q, K, top_k = c["B"], c["Q"], c["K"], c["top_k"]
    vb, ib, bb = flat(c["val"], F32), flat(c["idx"], I32), flat(c["boxes"], F32)
    sb = flat(torch.tensor(c["sizes"], dtype=torch.int32), I32)
    lab, qq, ob, cnt = flat(B * top_k, I32, out=True), flat(B * top_k, I32, out=True), flat(B * top_k * 4, I32, out=True), flat(B, I32, out=True)
    check(lib.fx_detr_postprocess(vb.ptr, ib.ptr, bb.ptr, sb.ptr, B, Q, K, top_k, c["thr"], lab.ptr, qq.ptr, ob.ptr, cnt.ptr, stream()), "fx_detr_postprocess")
    torch.cuda.synchronize()
    for b in (lab, qq, ob, cnt):
        b.assert_guards()
    assert torch.equal(lab.get().reshape(B, top_k), c["labels"]) and torch.equal(qq.get().reshape(B, top_k), c["queries"])
    assert torch.equal(ob.get().reshape(B, top_k, 4), c["obox"])
    assert torch.equal(cnt.get()[0], c["count"])


# ------------------------------------------------------------------------------------------------ rejections
def test_rejected_arguments(lib):
    """Every argument check the cases above lean on, called once with the offending argument on otherwise valid buffers: FocoosAmdError
    and no launch - the outputs keep the sentinel.  The buffers are allocated with the LARGE leading dimensions, so the shorter / odd
    ones handed to the library would stay inside them even if a check were missing."""
    s = stream()
    rows, cols = 4, 256
    x, out = Buf(rows, cols, cols + 8, BF, data=torch.zeros(rows, cols)), Buf(rows, cols, cols + 8, BF)
    f32v, f32o = flat(torch.zeros(1024), F32), flat(1024, F32, out=True)
    i32v, i32o = flat(torch.zeros(64, dtype=torch.int32), I32), flat(64, I32, out=True)
    X, O, LD = x.ptr, out.ptr, cols + 8
    calls = {
        "add_rows ldx < cols": lambda: lib.fx_add_rows_bf16(X, cols - 8, X, LD, 1, O, LD, rows, cols, s),
        "add_rows ldy % 8": lambda: lib.fx_add_rows_bf16(X, LD, X, LD - 4, 1, O, LD, rows, cols, s),
        "add_rows cols % 8": lambda: lib.fx_add_rows_bf16(X, LD, X, LD, 1, O, LD, rows, 60, s),
        "add_rows y_rows 0": lambda: lib.fx_add_rows_bf16(X, LD, X, LD, 0, O, LD, rows, cols, s),
        "layernorm cols 64": lambda: lib.fx_layernorm_bf16(X, LD, None, 0, f32v.ptr, f32v.ptr, O, LD, rows, 64, s),
        "layernorm ldx % 4": lambda: lib.fx_layernorm_bf16(X, cols + 2, None, 0, f32v.ptr, f32v.ptr, O, LD, rows, cols, s),
        "layernorm ldo % 4": lambda: lib.fx_layernorm_bf16(X, LD, None, 0, f32v.ptr, f32v.ptr, O, cols + 2, rows, cols, s),
        "layernorm ldr % 4": lambda: lib.fx_layernorm_bf16(X, LD, X, cols + 2, f32v.ptr, f32v.ptr, O, LD, rows, cols, s),
        "layernorm ldx < cols": lambda: lib.fx_layernorm_bf16(X, cols - 4, None, 0, f32v.ptr, f32v.ptr, O, LD, rows, cols, s),
        "mha ldq < heads * 32": lambda: lib.fx_mha_bf16(X, 128, X, LD, X, LD, O, LD, 1, rows, rows, 8, s),
        "mha ldk < heads * 32": lambda: lib.fx_mha_bf16(X, LD, X, 128, X, LD, O, LD, 1, rows, rows, 8, s),
        "mha ldv < heads * 32": lambda: lib.fx_mha_bf16(X, LD, X, LD, X, 128, O, LD, 1, rows, rows, 8, s),
        "mha ldo < heads * 32": lambda: lib.fx_mha_bf16(X, LD, X, LD, X, LD, O, 128, 1, rows, rows, 8, s),
        "mha ldk % 8": lambda: lib.fx_mha_bf16(X, LD, X, cols + 4, X, LD, O, LD, 1, rows, rows, 8, s),
        "mha mask words short": lambda: lib.fx_mha_masked_bf16(X, LD, X, LD, X, LD, O, LD, 1, 1, 64, 8, i32v.ptr, 1, None, 0, s),
        "msda M 4": lambda: lib.fx_msda_bf16(X, LD, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 16, f32v.ptr, 8, None, 0, O, LD, 1, 1, 1, 4, s),
        "msda ldv < 256": lambda: lib.fx_msda_bf16(X, 248, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 16, f32v.ptr, 8, None, 0, O, LD, 1, 1, 1, 8, s),
        "msda ldo % 4": lambda: lib.fx_msda_bf16(X, LD, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 16, f32v.ptr, 8, None, 0, O, cols + 2, 1, 1, 1, 8, s),
        "msda ld_loc short": lambda: lib.fx_msda_bf16(X, LD, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 15, f32v.ptr, 8, None, 0, O, LD, 1, 1, 1, 8, s),
        "msda ld_attn short": lambda: lib.fx_msda_bf16(X, LD, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 16, f32v.ptr, 7, None, 0, O, LD, 1, 1, 1, 8, s),
        "msda mode 1 without ref": lambda: lib.fx_msda_bf16(X, LD, i32v.ptr, i32v.ptr, 1, 1, f32v.ptr, 16, f32v.ptr, 8, None, 1, O, LD, 1, 1, 1, 8, s),
        "resize_nhwc ldx < C": lambda: lib.fx_resize_bilinear_nhwc_bf16(X, 8, O, LD, 1, 1, 1, 16, 1, 1, s),
        "resize_nhwc C % 8": lambda: lib.fx_resize_bilinear_nhwc_bf16(X, LD, O, LD, 1, 1, 1, 12, 1, 1, s),
        "resize_u8 Ho 0": lambda: lib.fx_resize_bilinear_u8(X, 1, 1, f32o.ptr, 0, 1, s),
        "maxpool ldy % 8": lambda: lib.fx_maxpool3x3s2_nhwc_bf16(X, LD, O, cols + 4, 1, 1, 1, 8, s),
        "avgpool ldx < C": lambda: lib.fx_avgpool2x2_nhwc_bf16(X, 8, O, LD, 1, 1, 1, 16, s),
        "rowmax ldx < cols": lambda: lib.fx_rowmax_f32(f32v.ptr, 7, f32o.ptr, 2, 8, s),
        "gather lds < cols": lambda: lib.fx_gather_rows_bf16(X, 8, 1, i32v.ptr, 1, O, LD, 1, 16, s),
        "gather ldo % 8": lambda: lib.fx_gather_rows_bf16(X, LD, 1, i32v.ptr, 1, O, cols + 4, 1, 16, s),
        "fill without indices": lambda: lib.fx_fill_rows_bf16(O, LD, rows, None, 1, X, 1, cols, s),
        "fill ldx < cols": lambda: lib.fx_fill_rows_bf16(O, 8, rows, i32v.ptr, 1, X, 1, 16, s),
        "linear_k4 N % 8": lambda: lib.fx_linear_k4_relu(f32v.ptr, f32v.ptr, f32v.ptr, O, LD, 1, 12, s),
        "linear_k4 ldo < N": lambda: lib.fx_linear_k4_relu(f32v.ptr, f32v.ptr, f32v.ptr, O, 8, 1, 16, s),
        "bbox_head K % 4": lambda: lib.fx_bbox_head(X, LD, f32v.ptr, f32v.ptr, f32v.ptr, None, None, 1, 0, f32o.ptr, None, 1, 130, s),
        "bbox_head ldh < K": lambda: lib.fx_bbox_head(X, 128, f32v.ptr, f32v.ptr, f32v.ptr, None, None, 1, 0, f32o.ptr, None, 1, 256, s),
        "bbox_head mode 0 without ref": lambda: lib.fx_bbox_head(X, LD, f32v.ptr, f32v.ptr, None, None, None, 1, 0, f32o.ptr, None, 1, 256, s),
        "bbox_head mode 1 without idx": lambda: lib.fx_bbox_head(X, LD, f32v.ptr, f32v.ptr, None, f32v.ptr, None, 1, 1, f32o.ptr, None, 1, 256, s),
        "head_out K < 4": lambda: lib.fx_detr_head_out(f32v.ptr, 8, f32v.ptr, f32o.ptr, f32o.ptr, 1, 3, s),
        "head_out ldl < K": lambda: lib.fx_detr_head_out(f32v.ptr, 7, f32v.ptr, f32o.ptr, f32o.ptr, 1, 8, s),
        "topk k > n": lambda: lib.fx_topk_rows_f32(f32v.ptr, 8, 1, 8, 9, f32o.ptr, i32o.ptr, s),
        "topk ld < n": lambda: lib.fx_topk_rows_f32(f32v.ptr, 7, 1, 8, 2, f32o.ptr, i32o.ptr, s),
        "topk k > 1024": lambda: lib.fx_topk_rows_f32(f32v.ptr, 1024, 1, 1024, 1025, f32o.ptr, i32o.ptr, s),
        "postprocess top_k 0": lambda: lib.fx_detr_postprocess(f32v.ptr, i32v.ptr, f32v.ptr, i32v.ptr, 1, 1, 1, 0, 0.5, i32o.ptr, i32o.ptr, i32o.ptr, i32o.ptr, s),
    }
    for what, call in calls.items():
        with pytest.raises(FocoosAmdError):
            check(call(), what)
    torch.cuda.synchronize()
    untouched(out, f32o, i32o)


def test_layernorm_rejections_leave_the_output(lib):
    """cols = 64: FX_ERR_UNSUPPORTED ("unsupported"); a leading dimension that is not a multiple of 4: invalid argument."""
    c = IC.layernorm_case(128, 4, True, "plain")
    rc, ob = ln_run(lib, c, 128, 4, cols_arg=64)
    with pytest.raises(FocoosAmdError, match="unsupported"):
        check(rc, "fx_layernorm_bf16")
    untouched(ob)
    for kw in ({"ldx": 130}, {"ldr": 130}, {"ldo": 134}):
        rc, ob = ln_run(lib, c, 128, 4, **kw)
        with pytest.raises(FocoosAmdError):
            check(rc, "fx_layernorm_bf16")
        untouched(ob)


def test_msda_other_head_count_is_unsupported(lib):
    c = IC.msda_case(IC.MSDA_L2, 3, 0)
    rc, ob, _ = msda_run(lib, c, 0, 0, M=4)
    with pytest.raises(FocoosAmdError, match="unsupported"):
        check(rc, "fx_msda_bf16")
    untouched(ob)
