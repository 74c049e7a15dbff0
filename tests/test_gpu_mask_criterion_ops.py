"""The mask criterion kernels (csrc/mask_criterion_ops.hip) called directly on a real MI355X, every output gated per element against the
float64 references of tests/mask_criterion_cases.py (checked on the CPU by tests/test_mask_criterion_cases_cpu.py):
  point_sample_kernel<float / uint8_t>                      fx_point_sample_f32
  mask_match_cost_kernel                                    fx_mask_match_cost_f32 (and fx_mask_match_cost_ws_f32 above 64 targets)
  mask_match_partial_kernel + mask_match_finish_kernel      fx_mask_match_cost_ws_f32
  mask_label_ce_kernel, mask_point_loss_kernel<float / uint8_t>, mask_loss_final_kernel     fx_mask_set_loss_f32
  mask_label_ce_bwd_kernel, mask_point_loss_bwd_lds_kernel, mask_point_loss_bwd_kernel      fx_mask_set_loss_bwd_f32
  mask_label_cls_kernel, mask_label_cls_bwd_kernel          dispatch of fx_mask_set_loss_cls_f32 / _cls_bwd_f32 (the kernels themselves:
                                                            tests/test_gpu_mask_class_loss.py)

Rules every case follows
* Views and guards: inputs lie between guard rows with NaN padding (leading dimensions above the logical width for the logits), outputs
  are prefilled with a sentinel bit pattern and everything outside the written region must keep it; workspaces are exactly the size the
  library asks for, followed by guard bytes.  Planes of unmatched queries hold NaN in pred_masks (never read) and 1.0 in dmasks (must
  keep it bit for bit: the sentinel cannot guard an accumulated output).
* Gate: |got - ref| <= one fp32 rounding of ref + c * mag per element, c = MARGIN * MEASURED[kernel] (MEASURED: the largest c any case
  needed on an MI355X against float64; the margin absorbs the run-to-run order of the atomic sums).  Every dmasks gate is asserted to lie
  below the smallest contribution of one point of the case at that point's main tap: a dropped or extra point cannot pass.
* Bit equality, no gate: exact point samples, selected sets, zero columns and rows, untouched planes and padding, determinism.
* The backward contract the tests pin (include/focoos_amd.h): the selection is read from the forward's workspace; dmasks must be zero in
  matched planes on entry and holds the gradient on return; unmatched planes are untouched; CE writes K + 1 columns of dlogits.
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
from focoos_amd._lib import check  # noqa: E402
from tests import helpers  # noqa: E402
from tests import mask_criterion_cases as MC  # noqa: E402
from tests.helpers import U32, Buf, _bits  # noqa: E402

DEV = "cuda:0"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MARGIN = 4.0
INV = -1            # FX_ERR_INVALID_ARGUMENT
# largest c over all cases of the kernel, measured on an MI355X against the float64 reference
MEASURED = {
    "point_sample.f32": 1.133e-07,
    "point_sample.u8": 1.069e-07,
    "point_sample.free": 5.872e-08,
    "match_cost": 8.976e-08,
    "match_cost_ws": 1.597e-07,
    "set_loss.out3": 2.042e-08,
    "set_loss_bwd.dlogits": 6.281e-07,
    "set_loss_bwd.dmasks.lds": 9.872e-08,
    "set_loss_bwd.dmasks.atomic": 8.893e-08,
    "set_loss_bwd.dmasks.lds.free": 1.431e-08,
    "set_loss_bwd.dmasks.atomic.free": 1.431e-08,
}
# fx_tune reads FX_MPL_BWD_LDS once per process: with 0 (the child of test_set_loss_bwd_on_the_atomic_kernel) every backward runs the atomic form
ATOMIC = os.environ.get("FX_MPL_BWD_LDS") == "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load("bf16")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def inp(data, dtype, ld=None):
    """A 2-D input between guard rows (NaN padding; sentinel for integers)."""
    rows, cols = data.shape
    return Buf(rows, cols, ld or cols, dtype, data=data)


class Raw:
    """`nbytes` bytes at a 256-byte aligned address (+ `shift`), sentinel bytes before and after."""
    PAD = 256

    def __init__(self, nbytes, shift=0):
        self.n, self.shift = nbytes, shift
        self.full = torch.full((nbytes + 2 * self.PAD,), 0x5A, dtype=U8, device=DEV)
        assert self.full.data_ptr() % 256 == 0
        self.ptr = self.full.data_ptr() + self.PAD + shift

    def body(self):
        return self.full[self.PAD + self.shift:self.PAD + self.shift + self.n].cpu()

    def assert_guards(self):
        f = self.full.cpu()
        assert bool((f[:self.PAD + self.shift] == 0x5A).all()) and bool((f[self.PAD + self.shift + self.n:] == 0x5A).all()), "bytes outside the workspace changed"

    def untouched(self):
        return bool((self.full == 0x5A).all())


def bits_equal(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ------------------------------------------------------------------------------------------------ 1. point sample
def run_point_sample(lib, c, R, src_index, coord_index):
    H, W, P = c["H"], c["W"], c["P"]
    sb = inp(c["src"].reshape(-1, H * W), U8 if c["u8"] else F32)
    cb = inp(c["coords"].reshape(-1, P * 2), F32)
    si = inp(torch.tensor([src_index], dtype=I32), I32) if src_index is not None else None
    ci = inp(torch.tensor([coord_index], dtype=I32), I32) if coord_index is not None else None
    ob = Buf(R, P, P, F32)
    check(lib.fx_point_sample_f32(sb.ptr, int(c["u8"]), H, W, si.ptr if si else None, cb.ptr, ci.ptr if ci else None, ob.ptr, R, P, stream()), "fx_point_sample_f32")
    torch.cuda.synchronize()
    ob.assert_guards()
    return ob.get()


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("P", MC.PS_POINTS)
@pytest.mark.parametrize("hw", MC.PS_PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_point_sample(lib, hw, P, u8):
    """Dyadic coordinates (the fp32 source index is exact) with c = 0, c = 1, the mixed corners and c = 0.5 first; R = 1 and 5 rows, with
    and without src_index / coord_index (the indices repeat and skip planes).  Measured c: MEASURED point_sample.*"""
    c = MC.point_sample_case(hw[0], hw[1], P, u8)
    key = "point_sample.u8" if u8 else "point_sample.f32"
    for R, si, ci in ((1, None, None), (5, None, None), (5, [5, 0, 2, 2, 1], None), (5, None, [4, 1, 1, 0, 3]), (1, [3], [2]), (5, [5, 0, 2, 2, 1], [4, 1, 1, 0, 3])):
        got = run_point_sample(lib, c, R, si, ci)
        ref, mag = MC.point_sample_ref(c, si if si is not None else list(range(R)), ci if ci is not None else list(range(R)))
        helpers.gate(key, f"{hw} P={P} R={R} idx={si is not None}/{ci is not None}", got, ref, mag, F32, MEASURED, MARGIN)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_point_sample_free_coordinates(lib, u8):
    """torch.rand coordinates on a 40 x 48 plane: the magnitude carries the coordinate term."""
    c = MC.point_sample_case(40, 48, 257, u8, free=True)
    got = run_point_sample(lib, c, 5, [5, 0, 2, 2, 1], [4, 1, 1, 0, 3])
    ref, mag = MC.point_sample_ref(c, [5, 0, 2, 2, 1], [4, 1, 1, 0, 3])
    helpers.gate("point_sample.free", f"40x48 u8={u8}", got, ref, mag, F32, MEASURED, MARGIN)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_point_sample_pixel_centres_are_exact(lib, u8):
    """At the pixel centres of a 64 x 32 plane the weights are (1, 0, 0, 0): the output equals the plane bit for bit."""
    H, W = 64, 32
    g = MC.gen(5)
    src = torch.randint(0, 256, (2, H, W), generator=g, dtype=U8) if u8 else torch.randn(2, H, W, generator=g) * 3
    c = {"src": src, "coords": MC.pixel_centres(H, W)[None], "H": H, "W": W, "P": H * W, "u8": u8}
    got = run_point_sample(lib, c, 2, None, [0, 0])
    assert bits_equal(got, src.reshape(2, -1).float())


# ------------------------------------------------------------------------------------------------ 2. match cost
def run_match_cost(lib, c, cls_sigmoid, entry):
    """entry "plain": fx_mask_match_cost_f32; "ws": fx_mask_match_cost_ws_f32 with exactly fx_mask_match_cost_workspace_bytes bytes.
    Returns (cost [B, Q, Tmax], workspace bytes asked for, the workspace)."""
    B, Q, P, K, Tmax = c["B"], c["Q"], c["P"], c["K"], c["Tmax"]
    lb = inp(c["logits"].reshape(B * Q, K + 1), F32, ld=K + 4)
    # the point rows are followed by at least 64 NaN floats: a tile load past P or past the last row reads NaN, not another allocation
    gp = (64 + P - 1) // P
    pb = inp(torch.cat([c["pred"], torch.full((gp, P), float("nan"))]), F32)
    tb = inp(torch.cat([c["tgt"], torch.full((gp, P), float("nan"))]), F32)
    lab, off = inp(c["labels"].view(1, -1), I32), inp(c["offsets"].view(1, -1), I32)
    cb = Buf(B * Q, Tmax, Tmax, F32)
    w = MC.MATCH_W
    args = (lb.ptr, K + 4, pb.ptr, tb.ptr, lab.ptr, off.ptr, B, Q, K, P, Tmax, w[0], w[1], w[2], int(cls_sigmoid), cb.ptr)
    nws, ws = 0, None
    if entry == "plain":
        check(lib.fx_mask_match_cost_f32(*args, stream()), "fx_mask_match_cost_f32")
    else:
        nws = int(lib.fx_mask_match_cost_workspace_bytes(B, Q, Tmax))
        ws = Raw(max(nws, 16))
        assert ws.ptr % 16 == 0
        check(lib.fx_mask_match_cost_ws_f32(*args, ws.ptr, nws, stream()), "fx_mask_match_cost_ws_f32")
    torch.cuda.synchronize()
    cb.assert_guards()
    if ws is not None:
        ws.assert_guards()
    return cb.get().reshape(B, Q, Tmax), nws, ws


@pytest.mark.parametrize("cls_sigmoid", [0, 1], ids=["softmax", "sigmoid"])
@pytest.mark.parametrize("case", MC.MATCH_CASES, ids=MC.match_id)
def test_match_cost(lib, case, cls_sigmoid):
    """Both entry points against float64, element by element (the table of MC.MATCH_CASES says what each size reaches).  Columns t >= T
    of an image and every row of an image without targets are exactly 0.  With more than 64 targets the ws entry reports a zero
    workspace, leaves the one it is given alone and returns the bits of the untiled kernel; otherwise it writes its partial sums.
    Measured c: MEASURED match_cost, match_cost_ws."""
    c = MC.match_case(case)
    ref, mag = MC.match_cost_ref(c, bool(cls_sigmoid))
    off = c["offsets"].tolist()
    plain, _, _ = run_match_cost(lib, c, cls_sigmoid, "plain")
    tiled, nws, ws = run_match_cost(lib, c, cls_sigmoid, "ws")
    tiled_ran = c["Tmax"] <= 64
    assert nws == (c["B"] * MC.mmc_splits(c["B"], c["Q"]) * c["Q"] * (3 * c["Tmax"] + 2) * 4 if tiled_ran else 0)
    assert ws.untouched() == (not tiled_ran)
    if not tiled_ran:
        assert bits_equal(tiled, plain)
    for name, got in (("match_cost", plain), ("match_cost_ws" if tiled_ran else "match_cost", tiled)):
        for b in range(c["B"]):
            T = off[b + 1] - off[b]
            assert not bool(got[b, :, T:].view(I32).any()), f"{name}: columns t >= T of image {b} must be +0.0"
        helpers.gate(name, f"{MC.match_id(case)} sigmoid={cls_sigmoid}", got, ref, mag, F32, MEASURED, MARGIN)


# ------------------------------------------------------------------------------------------------ 3. / 4. set loss and its gradients
class SetRun:
    """One case of fx_mask_set_loss_f32 and its backward on the device.  ldl = K + 1 + 3 with NaN padding."""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c
        B, Q, K = c["B"], c["Q"], c["K"]
        self.rows, self.ldl = B * Q, K + 4
        self.matched = MC.matched_rows(c)
        pm = c["pred_masks"].clone()
        pm[~self.matched] = float("nan")
        self.lb = inp(c["logits"].reshape(self.rows, K + 1), F32, ld=self.ldl)
        self.pb = inp(pm, F32)
        self.tb = inp(c["tgt_masks"], U8 if c["u8"] else F32)
        self.lab, self.off = inp(c["labels"].view(1, -1), I32), inp(c["offsets"].view(1, -1), I32)
        self.pi, self.ti = inp(c["pred_idx"].view(1, -1), I32), inp(c["tgt_idx"].view(1, -1), I32)
        self.ro = inp(c["rand_over"].reshape(c["sum_T"], -1), F32)
        self.re = inp(c["rand_extra"].reshape(c["sum_T"], -1), F32) if c["n_extra"] else None
        self.nws = int(lib.fx_mask_set_loss_workspace_bytes(B, Q, c["sum_T"], c["n_over"]))
        assert self.nws == (B * Q * 2 + c["sum_T"] * 4 + 1) * 8 + c["sum_T"] * c["n_over"] * 5 + 16
        self.ws = Raw(self.nws)

    def head(self, **kw):
        c = self.c
        a = dict(logits=self.lb.ptr, ldl=self.ldl, rand_over=self.ro.ptr, n_over=c["n_over"], n_extra=c["n_extra"], num_points=c["num_points"], K=c["K"])
        a.update(kw)
        return (a["logits"], a["ldl"], self.pb.ptr, c["h"], c["w"], self.tb.ptr, int(c["u8"]), c["H"], c["W"], self.lab.ptr, self.off.ptr, c["sum_T"],
                self.pi.ptr, self.ti.ptr, a["rand_over"], a["n_over"], self.re.ptr if self.re else None, a["n_extra"], a["num_points"], c["B"], c["Q"], a["K"])

    def tail(self, mode, num_masks=None, alpha=0.25, gamma=2.0):
        c = self.c
        nm = c["num_masks"] if num_masks is None else num_masks
        return (c["eos"],) + (() if mode is None else (mode, alpha, gamma)) + (nm, *c["weights"])

    def forward_rc(self, out, mode=None, ws_ptr=None, nws=None, num_masks=None, **kw):
        fn = self.lib.fx_mask_set_loss_f32 if mode is None else self.lib.fx_mask_set_loss_cls_f32
        return fn(*self.head(**kw), *self.tail(mode, num_masks), self.ws.ptr if ws_ptr is None else ws_ptr, self.nws if nws is None else nws, out.ptr, stream())

    def forward(self, mode=None):
        out = Buf(1, 3, 8, F32)
        check(self.forward_rc(out, mode), "fx_mask_set_loss")
        torch.cuda.synchronize()
        out.assert_guards()
        self.ws.assert_guards()
        return out.get().reshape(3)

    def backward_rc(self, g, dl, lddl, dm, mode=None, ws_ptr=None, nws=None, num_masks=None, **kw):
        fn = self.lib.fx_mask_set_loss_bwd_f32 if mode is None else self.lib.fx_mask_set_loss_cls_bwd_f32
        return fn(*self.head(**kw), *self.tail(mode, num_masks), self.ws.ptr if ws_ptr is None else ws_ptr, self.nws if nws is None else nws, g.ptr, dl.ptr, lddl,
                  dm.ptr, stream())

    def dmasks_buf(self, matched_fill=0.0):
        """dmasks between guard rows: matched planes hold `matched_fill` (0: the contract), planes of unmatched queries 1.0."""
        c = self.c
        pre = torch.ones(self.rows, c["h"] * c["w"])
        pre[self.matched] = matched_fill
        return Buf(self.rows, c["h"] * c["w"], c["h"] * c["w"], F32, prefill=pre)

    def backward(self, grads, mode=None, cols=None, matched_fill=0.0):
        """Returns (dmasks [rows, h*w] with the verified 1.0 of the unmatched planes replaced by 0, dlogits [rows, lddl]).  CE: lddl = K + 1 + 5 and the columns >= K + 1 keep the sentinel; the other
        modes write all lddl columns."""
        c = self.c
        cols = c["K"] + 1 if cols is None else cols
        lddl = c["K"] + 6
        g = inp(torch.tensor([grads]), F32)
        dl = Buf(self.rows, cols if mode is None else lddl, lddl, F32)
        dm = self.dmasks_buf(matched_fill)
        check(self.backward_rc(g, dl, lddl, dm, mode), "fx_mask_set_loss_bwd")
        torch.cuda.synchronize()
        dl.assert_guards()
        return self.dmasks_result(dm), dl.get()

    def dmasks_result(self, dm):
        """The contents of a dmasks_buf after a backward: guards intact, the planes of unmatched queries still 1.0 bit for bit (returned
        as the 0 the reference holds there)."""
        dm.assert_guards()
        got = dm.get()
        assert bool((got[~self.matched].view(I32) == torch.tensor(1.0).view(I32)).all()), "the plane of an unmatched query changed"
        got[~self.matched] = 0.0
        return got


def form_of(c):
    return "atomic" if ATOMIC or MC.bands(c["h"], c["w"]) is None else "lds"


def dmasks_key(c):
    """The free-coordinate case has a gate of its own: its magnitude carries the coordinate terms, so the c it needs is far smaller."""
    return "set_loss_bwd.dmasks." + form_of(c) + (".free" if c["free"] else "")


def gate_dmasks(c, ref, got, what):
    """The per-element gate, and: at the main tap of every point the gate lies below that point's own contribution."""
    key = dmasks_key(c)
    worst = MC.point_gate_ratio(ref, MARGIN * MEASURED[key])
    print(f"POINTGATE {c['name']} {what}: largest gate / smallest-point contribution = {worst:.3e}")
    assert worst < 1.0, f"{c['name']}: a point contributes less than the gate at its main tap ({worst:.3e})"
    helpers.gate(key, f"{c['name']} {what}", got, ref["dmasks"], ref["dmasks_mag"], F32, MEASURED, MARGIN)


@pytest.mark.parametrize("k", MC.SEL_K_IMP, ids=lambda k: f"k{k}")
@pytest.mark.parametrize("n_over", MC.SEL_N_OVER, ids=lambda n: f"n{n}")
def test_set_loss_selection(lib, n_over, k):
    """The radix select and the tie ranks of mask_point_loss_kernel (MC.selection_case): n_over below, at and above the 1024 threads
    (chunks of one and of two candidates, the last chunk partial), k_imp = 1, 100, n_over and 0 (n_extra = num_points), 40 candidates
    tied at |x| = 1.5 of which exactly `need` must be taken in index order.  The selected set is read off the backward: dmasks is nonzero
    exactly at the pixels of the reference's selected candidates and of the extra points.  out3 is gated too: the ties sit on different
    targets.  Measured c: MEASURED set_loss.out3, set_loss_bwd.*"""
    c = MC.selection_case(n_over, k)
    ref = MC.selection_ref(n_over, k)
    run = SetRun(lib, c)
    out3 = run.forward()
    helpers.gate("set_loss.out3", c["name"], out3, ref["out3"], ref["out3_mag"], F32, MEASURED, MARGIN)
    dm, dl = run.backward(MC.SEL_GRADS)
    want = MC.expected_pixels(c, ref)
    extra, missing = (dm != 0) & ~want, (dm == 0) & want
    assert not bool(extra.any()) and not bool(missing.any()), (f"{c['name']}: {int(extra.sum())} pixels of unselected candidates hold a gradient, "
                                                               f"{int(missing.sum())} selected ones hold none; first {extra.nonzero()[:1].tolist()} {missing.nonzero()[:1].tolist()}")
    gate_dmasks(c, ref, dm, "selection")
    helpers.gate("set_loss_bwd.dlogits", c["name"], dl, ref["dlogits"], ref["dlogits_mag"], F32, MEASURED, MARGIN)


@pytest.mark.parametrize("name", list(MC.SET_CASES))
def test_set_loss_forward(lib, name):
    """out3 of the value cases (MC.SET_CASES: one pair; nine pairs over three images with the middle one empty and permuted indices; f32
    and u8 targets at 4 x the prediction size; distinct weights, num_masks != sum_T), gated per value, and two runs bit-identical - out3
    and the whole workspace (pair sums, candidate logits, selection flags).  Measured c: MEASURED set_loss.out3"""
    c = MC.set_case(name)
    ref = MC.set_ref(name)
    run = SetRun(lib, c)
    a = run.forward()
    wa = run.ws.body()
    run.ws = Raw(run.nws)
    b = run.forward()
    assert bits_equal(a, b) and torch.equal(wa, run.ws.body()), "two runs differ"
    helpers.gate("set_loss.out3", name, a, ref["out3"], ref["out3_mag"], F32, MEASURED, MARGIN)
    # the selection flags the forward left behind are the reference's selected set
    nsel = c["sum_T"] * c["n_over"]
    flags = wa[run.nws - 16 - nsel:run.nws - 16].reshape(c["sum_T"], c["n_over"])
    for n, sel in enumerate(ref["sel"]):
        want = torch.zeros(c["n_over"], dtype=U8)
        want[sel] = 1
        assert torch.equal(flags[n], want), f"{name}: pair {n} selected another set"


BWD_PARAMS = [(n, "all") for n in MC.SET_CASES] + [("one-pair", "no-dice"), ("one-pair", "no-bce"), ("three-bands", "no-dice"), ("two-bands", "no-bce")]


@pytest.mark.parametrize("name,gk", BWD_PARAMS, ids=[f"{n}-{g}" for n, g in BWD_PARAMS])
def test_set_loss_bwd(lib, name, gk):
    """dmasks per pixel and dlogits per element under distinct upstream gradients on the device (g2 = 0 and g1 = 0 isolate the BCE and
    the dice term).  Plane shapes: 40 x 48 one band; 130 x 127 a second band of one row; 200 x 200 bands of 81, 81, 38 rows; 3 x 16384
    one row per band, so the two tap rows of every point fall into different workgroups; 2 x 16385 too wide for LDS - the atomic kernel.
    In a process started with FX_MPL_BWD_LDS=0 all of them run on the atomic kernel.  Rows: 5, 7, 21 (not multiples of 4) and 140 with 65
    targets in one image; K + 1 = 65; one row of logits near 60.  Measured c: MEASURED set_loss_bwd.*"""
    c = MC.set_case(name)
    ref = MC.set_ref(name, gk)
    run = SetRun(lib, c)
    run.forward()
    dm, dl = run.backward(MC.GRADS[gk])
    gate_dmasks(c, ref, dm, gk)
    helpers.gate("set_loss_bwd.dlogits", f"{name} {gk}", dl, ref["dlogits"], ref["dlogits_mag"], F32, MEASURED, MARGIN)


FORM_PARAMS = ["one-pair", "too-wide"]


@pytest.mark.parametrize("name", FORM_PARAMS)
def test_set_loss_bwd_form_and_prior_content(lib, name):
    """Which form ran, told by what lies outside the contract: over a matched plane that holds 1.0 instead of the required 0 the LDS form
    STORES its bands (the result passes the gate of the run over zeros: a prior 1.0 showing through would miss it by orders of magnitude;
    no bit equality, the add order inside LDS is not fixed), the atomic form ADDS (1 + gradient).  The contract is a zero plane;
    this only pins that `one-pair` runs the LDS form in the default process and the atomic one with FX_MPL_BWD_LDS=0, and `too-wide`
    (w = 16385 > MPB_LDS_FLOATS) the atomic one always."""
    c = MC.set_case(name)
    ref = MC.set_ref(name, "all")
    run = SetRun(lib, c)
    run.forward()
    zero, _ = run.backward(MC.GRADS["all"])
    ones, _ = run.backward(MC.GRADS["all"], matched_fill=1.0)
    m = run.matched
    if form_of(c) == "lds":
        gate_dmasks(c, ref, ones, "over a prior 1.0: the LDS form stores")
    else:
        key = dmasks_key(c)
        err = (ones[m].double() - (1.0 + ref["dmasks"][m])).abs()
        assert bool((err <= 8 * U32 + helpers.rnd(ref["dmasks"][m], F32) + MARGIN * MEASURED[key] * ref["dmasks_mag"][m]).all()), "the atomic form adds to prior content"
        assert float((ones[m].double() - zero[m].double()).abs().min()) > 0.5


def test_set_loss_bwd_on_the_atomic_kernel():
    """test_set_loss_bwd and the form test again in ONE fresh process with FX_MPL_BWD_LDS=0: mask_point_loss_bwd_kernel on every shape."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_mask_criterion_ops.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_set_loss_bwd and not on_the_atomic_kernel"],
                       cwd=ROOT, env=dict(os.environ, FX_MPL_BWD_LDS="0"), capture_output=True, text=True, timeout=300)
    tail = r.stdout[-2000:] + r.stderr[-500:]
    assert r.returncode == 0, tail
    summary = r.stdout.strip().splitlines()[-1]
    assert re.search(rf"\b{len(BWD_PARAMS) + len(FORM_PARAMS)} passed\b", summary) and "skipped" not in summary and "failed" not in summary, tail


@pytest.mark.parametrize("mode", [MC.FOCAL, MC.BCE, MC.BCE_FOCAL], ids=["focal", "bce", "bce_focal"])
def test_set_loss_cls_dispatch(lib, mode):
    """fx_mask_set_loss_cls_f32 / _cls_bwd_f32 in the three other class modes: out3[0] and dlogits have the bits of fx_mask_class_loss_f32 /
    _bwd_f32 called directly (whose kernels tests/test_gpu_mask_class_loss.py gates), all lddl columns are written with 0 in the padding,
    and the mask part is unchanged: out3[1:] has the bits of the CE entry, dmasks passes the same gate (two points on one pixel are
    added in LDS in either order, so its bits may differ from run to run)."""
    c = MC.set_case("three-images")
    ref = MC.set_ref("three-images", "all")
    K, B, Q = c["K"], c["B"], c["Q"]
    cols = K + 1 if mode == MC.FOCAL else K
    run = SetRun(lib, c)
    ce3 = run.forward()
    out3 = run.forward(mode)
    dm, dl = run.backward(MC.GRADS["all"], mode)
    assert bits_equal(out3[1:], ce3[1:])
    gate_dmasks(c, ref, dm, f"cls_mode {mode}")
    assert not bool(dl[:, cols:].view(I32).any()), "padding columns of dlogits must be +0.0"
    nws = int(lib.fx_mask_class_loss_workspace_bytes(B, Q))
    ws, o1 = Raw(nws), Buf(1, 1, 8, F32)
    lddl = K + 6
    d1 = Buf(run.rows, lddl, lddl, F32)
    g = inp(torch.tensor([MC.GRADS["all"][:1]]), F32)
    common = (run.lb.ptr, run.ldl, run.lab.ptr, run.off.ptr, run.pi.ptr, run.ti.ptr, B, Q, K, mode, 0.25, 2.0, c["num_masks"], c["weights"][0])
    check(lib.fx_mask_class_loss_f32(*common, ws.ptr, nws, o1.ptr, stream()), "fx_mask_class_loss_f32")
    check(lib.fx_mask_class_loss_bwd_f32(*common, g.ptr, d1.ptr, lddl, stream()), "fx_mask_class_loss_bwd_f32")
    torch.cuda.synchronize()
    assert bits_equal(out3[:1], o1.get().reshape(1)) and bits_equal(dl, d1.get())
    assert bool(torch.isfinite(dl).all()) and bool(dl[:, :cols].any())


# ------------------------------------------------------------------------------------------------ 5. rejected arguments
def test_rejected_arguments(lib):
    """Each of these returns FX_ERR_INVALID_ARGUMENT without a launch - out3, dlogits, dmasks and the workspace keep their sentinel - and
    the same arguments made valid are then accepted: out3, dlogits and dmasks (a fresh buffer with zeroed matched planes) pass their gates."""
    c = MC.selection_case(300, 100)
    ref = MC.selection_ref(300, 100)
    K = c["K"]
    run = SetRun(lib, c)
    out = Buf(1, 3, 8, F32)
    lddl = K + 6
    g = inp(torch.tensor([MC.SEL_GRADS]), F32)
    dl = Buf(run.rows, K + 1, lddl, F32)
    dm = Buf(run.rows, c["h"] * c["w"], c["h"] * c["w"], F32)
    big = Raw(run.nws + 8)

    def both(mode=None, lddl_=lddl, **kw):
        return (run.forward_rc(out, mode, **kw), run.backward_rc(g, dl, lddl_, dm, mode, **kw))

    assert both(ldl=K) == (INV, INV)                                          # ldl < K + 1
    assert both(mode=MC.BCE, ldl=K - 1) == (INV, INV)                         # ... below the K columns of the sigmoid modes
    assert run.backward_rc(g, dl, K, dm) == INV                               # lddl < K + 1 (only the backward has one)
    assert run.backward_rc(g, dl, K - 1, dm, MC.BCE_FOCAL) == INV             # ... below the K columns of the sigmoid modes
    assert both(n_over=c["k_imp"] - 1) == (INV, INV)                          # n_over < num_points - n_extra
    assert both(n_extra=c["num_points"] + 1) == (INV, INV)                    # n_extra > num_points
    assert both(nws=run.nws - 1) == (INV, INV)                                # the workspace one byte short
    assert both(ws_ptr=big.ptr + 4, nws=run.nws) == (INV, INV)                # ... misaligned by 4
    assert both(num_masks=0.0) == (INV, INV)
    assert both(mode=4) == (INV, INV) and both(mode=-1) == (INV, INV)         # an unknown cls_mode
    assert both(rand_over=None) == (INV, INV)                                 # sum_T > 0 and candidates needed, but no rand_over
    assert both(K=0) == (INV, INV)
    torch.cuda.synchronize()
    none = torch.zeros(run.rows, dtype=torch.bool)
    out.assert_guards(written=torch.zeros(1, dtype=torch.bool))
    dl.assert_guards(written=none)
    dm.assert_guards(written=none)
    assert run.ws.untouched() and big.untouched()
    # accepted: the forward, then the backward into zeroed matched planes
    dm = run.dmasks_buf()
    assert both() == (0, 0)
    torch.cuda.synchronize()
    helpers.gate("set_loss.out3", "after the rejected calls", out.get().reshape(3), ref["out3"], ref["out3_mag"], F32, MEASURED, MARGIN)
    out.assert_guards()
    dl.assert_guards()
    helpers.gate("set_loss_bwd.dlogits", "after the rejected calls", dl.get(), ref["dlogits"], ref["dlogits_mag"], F32, MEASURED, MARGIN)
    gate_dmasks(c, ref, run.dmasks_result(dm), "after the rejected calls")
