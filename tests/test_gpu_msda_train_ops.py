"""The deformable-attention training kernels, their prelude and the fused AdamW step of csrc/train_ops.hip, called directly through the
C ABI on a real MI355X under BOTH element types (libfocoos_amd.so = bfloat16, libfocoos_amd_fp16.so = IEEE half): fx_msda_f32_fwd / _bwd,
fx_msda_train_fwd / _bwd (value as element and as fp32, column slices of wider buffers), fx_msda_train_bwd_slab (all four value /
grad_out type combinations), fx_msda_bwd_slab_supported, fx_msda_prep_bf16 / fx_msda_prep_bwd_bf16, fx_adamw_step_f32 /
fx_adamw_step_scaled_f32.  Inputs, float64 references, magnitudes and tap counts come from tests/msda_train_cases.py, which
tests/test_msda_train_cases_cpu.py pins against independent formulations.  No test here compares one kernel with another.

* Every kernel is a case on its own: loc and attn of the core kernels come from the case, not from the prelude kernel; the prelude's
  backward reads the case's own aw.
* Outputs lie between guard rows (helpers.Buf) or in a column slice of a wider buffer (Slice) prefilled with a sentinel that everything
  outside the written region must keep bit for bit; inputs are padded with NaN.
* Exact runs (MC.EXACT_CASES): every output of every form equals the float64 reference as a number, element by element.
* Other runs, per element: |got - ref| <= c * mag (+ half a step of the 16-bit element for outputs stored in it; + 2^-126, below which
  fp32 may flush).  MEASURED[key] is the largest c any case of that key needed on an MI355X AGAINST THE FLOAT64 REFERENCE over both
  element types (printed as EXCESS ...), the gate is MARGIN = 4 times that and never above (n + 8) * 2^-24, n the
  number of terms of that element's sum: 4 L P for the forward and the point gradients, the pixel's tap count (+ 1 for a prefill) for
  the value gradient, 1 for the element-wise optimiser step.
* FX_MSDA_BWD_LEVEL_SPLIT=0 and FX_MSDA_BWD_POINT_SPLIT=2 are read once per process: each runs in ONE fresh child process over the exact
  runs and two random cases (P = 4, and P = 3 where the point split falls back to 1)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import FocoosAmdError, check  # noqa: E402
from tests import msda_train_cases as MC  # noqa: E402
from tests.helpers import GR, ROOT, U32, Buf, _bits  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
MARGIN = 4.0
FLOOR = 2.0 ** -126
# largest c over all cases of the key and both element types, measured on an MI355X against the float64 reference
MEASURED = {
    "fwd": 8.094e-09,
    "grad_attn": 4.734e-09,
    "grad_loc": 1.350e-08,
    "grad_value.atomic": 1.049e-07,
    "grad_value.slab": 7.888e-09,
    "prep.loc": 1.040e-07,
    "prep.aw": 1.541e-07,
    "prep.grad_off": 1.647e-08,
    "prep.grad_logit": 2.067e-08,
    "adamw.p": 1.847e-07,
    "adamw.m": 1.325e-07,
    "adamw.v": 2.237e-07,
    "adamw.total_norm": 2.545e-08,
}
CH = MC.CH
LDV, COL_V = 520, 260          # value as a column slice: row stride and first column (16-byte aligned for fp32, 8-byte for the element)
LDG, COL_G = 776, 516          # value gradient as a column slice
PREFILL = 0.5                  # what the accumulating atomic form finds in its slice


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


def gate(key, what, got, ref, mag, n, elem_dtype=None):
    """Print the c this output needs, then hold every element to min(MARGIN * MEASURED[key], (n + 8) * 2^-24) * mag; n an int or a tensor
    of the output's shape."""
    got, ref, mag = got.double().reshape(ref.shape), ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    ceil = (torch.as_tensor(n, dtype=torch.float64) + 8) * U32
    lim = torch.clamp(ceil, max=MARGIN * MEASURED[key]).expand(ref.shape)
    extra = torch.full_like(ref, FLOOR)
    if elem_dtype is not None:
        extra = extra + MC.half_step(ref.abs() + lim * mag, elem_dtype)
    err = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
    over = (err - extra).clamp_min(0)
    c = float((over / mag.clamp_min(1e-300)).max()) if over.numel() else 0.0
    share = float((over / (ceil.expand(ref.shape) * mag).clamp_min(1e-300)).max()) if over.numel() else 0.0
    print(f"EXCESS {key} {tag()} {c:.3e} ({share:.2f} of its (n + 8) * 2^-24) {what}")
    bad = over > lim * mag
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{key} {what}: {int(bad.sum())} of {bad.numel()} elements outside the gate (needs c = {c:.3e}, {share:.2f} of the ceiling; gate "
                             f"{MARGIN * MEASURED[key]:.3e}); first at {i}: got {got[i].item()!r} ref {ref[i].item()!r} mag {mag[i].item()!r}")
    return c


def exact(what, got, ref):
    got = got.double().reshape(ref.shape)
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.numel()} elements differ from the float64 reference"


class Slice:
    """CH columns starting at `col0` of a [rows][ld] device buffer between GR guard rows.  With `data` an input (NaN everywhere else),
    without an output (sentinel everywhere; `prefill` sets the slice)."""

    def __init__(self, rows, ld, col0, dtype, data=None, prefill=None):
        assert col0 + CH <= ld
        self.rows, self.ld, self.col0 = rows, ld, col0
        self.full = torch.empty(rows + 2 * GR, ld, dtype=dtype, device=DEV)
        self.sent = {2: 0x5A5A, 4: 0x5A5A5A5A}[self.full.element_size()]
        if data is not None:
            self.full.fill_(float("nan"))
            self.full[GR:GR + rows, col0:col0 + CH] = data.reshape(rows, CH).to(device=DEV, dtype=dtype)
        else:
            _bits(self.full).fill_(self.sent)
            if prefill is not None:
                self.full[GR:GR + rows, col0:col0 + CH] = prefill

    @property
    def ptr(self):
        return self.full.data_ptr() + (GR * self.ld + self.col0) * self.full.element_size()

    def get(self):
        return self.full[GR:GR + self.rows, self.col0:self.col0 + CH].cpu()

    def assert_guards(self, untouched=False):
        b = _bits(self.full).cpu().clone()
        if not untouched:
            b[GR:GR + self.rows, self.col0:self.col0 + CH] = self.sent
        assert bool((b == self.sent).all()), "a guard row or a column outside the slice changed"


class Dev:
    """The device operands every core entry point shares for one case."""

    def __init__(self, c):
        self.c = c
        B, Q, L, P, S = c["B"], c["Q"], c["L"], c["P"], c["S"]
        self.shapes = torch.tensor(c["shapes"], dtype=torch.int32, device=DEV)
        self.starts = torch.tensor(c["starts"], dtype=torch.int32, device=DEV)
        self.shapes_host = np.ascontiguousarray(np.array(c["shapes"], dtype=np.int32).reshape(-1))
        self.loc = Buf(B * Q * MC.M, L * P * 2, L * P * 2, F32, data=c["loc"])
        self.attn = Buf(B * Q * MC.M, L * P, L * P, F32, data=c["attn"])
        self.dims = (B, S, Q, MC.M)

    def value(self, kind):
        """kind: 'f32' contiguous fp32, 'f32s' / 'elem' a column slice of fp32 / the element type -> (buffer, value_bf16, ldv)."""
        rows = self.c["B"] * self.c["S"]
        if kind == "f32":
            return Buf(rows, CH, CH, F32, data=self.c["value"]), 0, CH
        return Slice(rows, LDV, COL_V, F32 if kind == "f32s" else adt(), data=self.c["value"]), int(kind == "elem"), LDV

    def grad_out(self, as_elem):
        return Buf(self.c["B"] * self.c["Q"], CH, CH, adt() if as_elem else F32, data=self.c["go"])

    def point_outs(self):
        c = self.c
        n = c["B"] * c["Q"] * MC.M
        return Buf(n, c["L"] * c["P"] * 2, c["L"] * c["P"] * 2, F32), Buf(n, c["L"] * c["P"], c["L"] * c["P"], F32)


def check_point_grads(c, r, gl, ga, what):
    torch.cuda.synchronize()
    gl.assert_guards()
    ga.assert_guards()
    n = 4 * c["L"] * c["P"]
    if c["exact"]:
        exact(f"{what} grad_loc", gl.get(), r["grad_loc"])
        exact(f"{what} grad_attn", ga.get(), r["grad_attn"])
    else:
        gate("grad_loc", what, gl.get(), r["grad_loc"], r["grad_loc_mag"], n)
        gate("grad_attn", what, ga.get(), r["grad_attn"], r["grad_attn_mag"], n)


# ------------------------------------------------------------------------------------------------ 1. forward
FWD_FORMS = ("f32", "f32s", "elem")


@pytest.mark.parametrize("name", MC.GATED_CASES + MC.EXACT_CASES)
def test_msda_fwd(lib, name):
    """fx_msda_f32_fwd, and fx_msda_train_fwd with the value as an fp32 and as an element-typed column slice (ldv = 520, first column 260,
    NaN in every other column) vs the float64 grid_sample reference: exact runs equal, the others within the gate of `fwd`."""
    c, r = MC.core_case(name), MC.core_ref(name)
    d = Dev(c)
    B, S, Q, Mh = d.dims
    for form in FWD_FORMS:
        vb, v16, ldv = d.value(form)
        out = Buf(B * Q, CH, CH, F32)
        if form == "f32":
            rc = lib.fx_msda_f32_fwd(vb.ptr, d.shapes.data_ptr(), d.starts.data_ptr(), c["L"], c["P"], d.loc.ptr, d.attn.ptr, out.ptr, B, S, Q, Mh, stream())
        else:
            rc = lib.fx_msda_train_fwd(vb.ptr, v16, ldv, d.shapes.data_ptr(), d.starts.data_ptr(), c["L"], c["P"], d.loc.ptr, d.attn.ptr, out.ptr, B, S, Q, Mh,
                                       stream())
        check(rc, "fx_msda fwd")
        torch.cuda.synchronize()
        out.assert_guards()
        if c["exact"]:
            exact(f"{name} {form} out", out.get(), r["out"])
        else:
            gate("fwd", f"{name} {form}", out.get(), r["out"], r["out_mag"], 4 * c["L"] * c["P"])


# ------------------------------------------------------------------------------------------------ 2. backward with fp32 atomics
ATOMIC_FORMS = ("f32", "f32s_acc", "elem_acc", "elem_zero")


def atomic_run(lib, d, form):
    """-> (grad_value buffer, grad_loc, grad_attn, accumulated onto PREFILL?)"""
    c = d.c
    B, S, Q, Mh = d.dims
    go = d.grad_out(False)
    gl, ga = d.point_outs()
    if form == "f32":
        vb, _, _ = d.value("f32")
        gv = Buf(B * S, CH, CH, F32)                                       # garbage (the sentinel): the call zeroes it
        rc = lib.fx_msda_f32_bwd(vb.ptr, d.shapes.data_ptr(), d.starts.data_ptr(), c["L"], c["P"], d.loc.ptr, d.attn.ptr, go.ptr, gv.ptr, gl.ptr, ga.ptr, B, S, Q,
                                 Mh, stream())
        acc = False
    else:
        vb, v16, ldv = d.value("elem" if form.startswith("elem") else "f32s")
        acc = form.endswith("_acc")
        gv = Slice(B * S, LDG, COL_G, F32, prefill=PREFILL) if acc else Buf(B * S, CH, CH, F32)
        rc = lib.fx_msda_train_bwd(vb.ptr, v16, ldv, d.shapes.data_ptr(), d.starts.data_ptr(), c["L"], c["P"], d.loc.ptr, d.attn.ptr, go.ptr, gv.ptr,
                                   LDG if acc else CH, 0 if acc else 1, gl.ptr, ga.ptr, B, S, Q, Mh, stream())
    check(rc, f"fx_msda bwd {form}")
    torch.cuda.synchronize()
    gv.assert_guards()
    return gv, gl, ga, acc


@pytest.mark.parametrize("name", MC.GATED_CASES + MC.EXACT_CASES)
def test_msda_bwd_atomic(lib, name):
    """fx_msda_f32_bwd (zeroes a sentinel-filled grad_value itself), fx_msda_train_bwd with zero_grad_value = 0 onto a slice (ldg = 776,
    first column 516) prefilled with 0.5 - expected 0.5 + gradient, every other column untouched - for the value as fp32 and as element,
    and with zero_grad_value = 1 (ldg = 256) onto garbage.  Untapped pixels: exactly 0 (exactly the prefill)."""
    c, r = MC.core_case(name), MC.core_ref(name)
    d = Dev(c)
    terms = MC.pixel_terms(c, r).reshape(-1, CH)
    for form in ATOMIC_FORMS:
        gv, gl, ga, acc = atomic_run(lib, d, form)
        what = f"{name} {form}"
        check_point_grads(c, r, gl, ga, what)
        ref = r["grad_value"].reshape(-1, CH) + (PREFILL if acc else 0.0)
        if c["exact"]:
            exact(f"{what} grad_value", gv.get(), ref)
        else:
            gate("grad_value.atomic", what, gv.get(), ref, r["grad_value_mag"].reshape(-1, CH) + (PREFILL if acc else 0.0), terms + int(acc))


def _child(env, k, n):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_msda_train_ops.py"), "-q", "-x", "-p", "no:cacheprovider", "-k", k],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-500:]
    assert r.returncode == 0, tail
    summary = r.stdout.strip().splitlines()[-1]
    assert re.search(rf"\b{n} passed\b", summary) and "skipped" not in summary and "failed" not in summary, tail


CHILD_K = "test_msda_bwd_atomic and (exact or crowd or l3p3 or l8p4)"     # exact, exact3 (P = 3), crowd, l3p3 (P = 3), l8p4 (P = 4) x two element types


def test_msda_bwd_atomic_unsplit():
    """test_msda_bwd_atomic over the exact runs and two random cases in ONE fresh process with FX_MSDA_BWD_LEVEL_SPLIT=0: a wave per
    (batch, query) walks all levels."""
    _child({"FX_MSDA_BWD_LEVEL_SPLIT": "0"}, CHILD_K, 10)


def test_msda_bwd_atomic_point_split():
    """The same in ONE fresh process with FX_MSDA_BWD_POINT_SPLIT=2: two waves per (batch, query, level) at P = 4; at P = 3 (exact3, l3p3)
    the split must fall back to 1 - a split of 3 points by 2 would drop the third."""
    _child({"FX_MSDA_BWD_POINT_SPLIT": "2"}, CHILD_K, 10)


# ------------------------------------------------------------------------------------------------ 3. backward by binning (slab form)
def slab_run(lib, d, v_elem, go_elem):
    c = d.c
    B, S, Q, Mh = d.dims
    vb, v16, ldv = d.value("elem" if v_elem else "f32s")
    go = d.grad_out(go_elem)
    gl, ga = d.point_outs()
    gv = Slice(B * S, LDG, COL_G, adt())                                   # sentinel-filled: every pixel of the slice must be overwritten
    assert lib.fx_msda_bwd_slab_supported(d.shapes_host.ctypes.data, c["L"], c["P"], Q, Mh, int(go_elem)) == 1
    check(lib.fx_msda_train_bwd_slab(vb.ptr, v16, ldv, d.shapes.data_ptr(), d.starts.data_ptr(), d.shapes_host.ctypes.data, c["L"], c["P"], d.loc.ptr, d.attn.ptr,
                                     go.ptr, int(go_elem), gv.ptr, LDG, gl.ptr, ga.ptr, B, S, Q, Mh, stream()), "fx_msda_train_bwd_slab")
    torch.cuda.synchronize()
    gv.assert_guards()
    return gv, gl, ga


def slab_check(lib, name, combos):
    c, r = MC.core_case(name), MC.core_ref(name)
    d = Dev(c)
    terms = MC.pixel_terms(c, r).reshape(-1, CH)
    for v_elem, go_elem in combos:
        gv, gl, ga = slab_run(lib, d, v_elem, go_elem)
        what = f"{name} slab value={'elem' if v_elem else 'f32'} go={'elem' if go_elem else 'f32'}"
        check_point_grads(c, r, gl, ga, what)
        got = gv.get()
        assert bool(torch.isfinite(got.float()).all()), f"{what}: a pixel kept the sentinel or is not finite"
        if c["exact"]:
            exact(f"{what} grad_value", got, r["grad_value"].reshape(-1, CH))
        else:
            gate("grad_value.slab", what, got, r["grad_value"].reshape(-1, CH), r["grad_value_mag"].reshape(-1, CH), terms, adt())
        assert bool((got.double()[terms == 0] == 0).all()), f"{what}: an untapped pixel is not 0"


@pytest.mark.parametrize("name", MC.GATED_CASES + MC.EXACT_CASES)
def test_msda_bwd_slab(lib, name):
    """fx_msda_train_bwd_slab for the four (value, grad_out) type combinations of the point-gradient kernel = both types of the value
    kernel, onto a sentinel-filled slice (ldg = 776, first column 516) of the element type: every pixel overwritten, untapped ones with 0,
    the other columns untouched.  The value gradient is gated with half an element step on top; exact runs (crowd: pixels of 95 .. 129
    entries, seven set-aside pixels per slab) equal the float64 reference."""
    slab_check(lib, name, [(True, True), (True, False), (False, True), (False, False)])


@pytest.mark.parametrize("name", MC.QMAX_CASES)
def test_msda_bwd_slab_at_q_max(lib, name):
    """The largest Q the slab form admits at P = 4 for each grad_out type, found by bisecting fx_msda_bwd_slab_supported and equal to the
    restated LDS formula (the dynamic LDS grows to its 160 KiB limit through hipFuncSetAttribute); Q_max + 1 and L = 9 are unsupported."""
    go_elem = name.endswith("16")
    sh = np.ascontiguousarray(np.array([4, 4, 2, 2] + [1, 1] * 7, dtype=np.int32))
    lo, hi = 1, 4096
    assert lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 2, 4, lo, 8, int(go_elem)) == 1 and lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 2, 4, hi, 8, int(go_elem)) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 2, 4, mid, 8, int(go_elem)) == 1:
            lo = mid
        else:
            hi = mid
    assert lo == MC.q_max(4, go_elem) == MC.core_case(name)["Q"]
    assert lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 2, 4, lo + 1, 8, int(go_elem)) == 0 and lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 9, 4, 8, 8, int(go_elem)) == 0
    assert lib.fx_msda_bwd_slab_supported(sh.ctypes.data, 8, 4, 8, 8, int(go_elem)) == 1
    slab_check(lib, name, [(True, go_elem), (False, go_elem)])


def test_group_backward_takes_the_atomic_form_when_the_slab_form_is_unsupported(lib):
    """focoos_amd.train._msda_group_backward with Q = Q_max + 1: the sink gets an fp32 buffer and the fp32-atomic entry point runs."""
    from focoos_amd.train import ValueGradSink, _msda_group_backward, _shape_host, _shape_tensors

    shapes = [[4, 4], [2, 2]]
    B, S, Q, L, P = 1, 20, MC.q_max(4, True) + 1, 2, 4
    g = MC.gen(77)
    value = torch.randn(B, S, CH, generator=g).to(adt()).to(DEV)
    lc = torch.rand(B, Q, MC.M, L, P, 2, generator=g).to(DEV)
    aw = torch.softmax(torch.randn(B, Q, MC.M, L * P, generator=g), -1).view(B, Q, MC.M, L, P).to(DEV)
    go = torch.randn(B, Q, CH, generator=g).to(adt()).to(DEV)
    st, ss = _shape_tensors(shapes, value.device)
    seen = []

    class Spy(ValueGradSink):
        def __setattr__(self, k, v):
            if k == "buf" and v is not None:
                seen.append(v.dtype)
            object.__setattr__(self, k, v)

    sink = Spy(1)
    gv, gl, ga = _msda_group_backward(value, st, ss, lc, aw, go, sink, 0, (B, S, Q, MC.M, MC.D, L, P, CH), _shape_host(shapes))
    torch.cuda.synchronize()
    assert sink.slab is False and seen == [torch.float32] and gv.dtype == adt() and bool(torch.isfinite(gv.float()).all())


# ------------------------------------------------------------------------------------------------ 4. prelude
def sid(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", MC.PREP_SHAPES, ids=sid)
def test_msda_prep(lib, shape):
    """fx_msda_prep_bf16 vs the float64 softmax and location arithmetic: padded ld_off / ld_logit (NaN in the padding), equal logits,
    logits over +-80 (exp underflows: the weight must come out 0 or a subnormal, never NaN), ref_wh = 0."""
    c = MC.prep_case(shape)
    BQ, Mh, L, P = shape
    LP = L * P
    off = Buf(BQ, Mh * LP * 2, Mh * LP * 2 + 8, adt(), data=c["off"])
    lg = Buf(BQ, Mh * LP, Mh * LP + 24, adt(), data=c["logit"])
    ref = Buf(BQ, 4, 4, F32, data=c["ref"])
    loc, aw = Buf(BQ * Mh, LP * 2, LP * 2, F32), Buf(BQ * Mh, LP, LP, F32)
    check(lib.fx_msda_prep_bf16(off.ptr, off.ld, lg.ptr, lg.ld, ref.ptr, loc.ptr, aw.ptr, BQ, Mh, L, P, stream()), "fx_msda_prep_bf16")
    torch.cuda.synchronize()
    loc.assert_guards()
    aw.assert_guards()
    (l_ref, l_mag), (a_ref, a_mag) = MC.prep_fwd_ref(c)
    gate("prep.loc", sid(shape), loc.get(), l_ref.reshape(BQ * Mh, -1), l_mag.expand_as(l_ref).reshape(BQ * Mh, -1), 1)
    gate("prep.aw", sid(shape), aw.get(), a_ref.reshape(BQ * Mh, -1), a_mag.reshape(BQ * Mh, -1), LP)


@pytest.mark.parametrize("shape", MC.PREP_SHAPES, ids=sid)
def test_msda_prep_bwd(lib, shape):
    """fx_msda_prep_bwd_bf16 from the case's own aw, grad_loc, grad_attn vs aw * (ga - sum aw ga) and gl * ref_wh * 0.5 / P, stored in
    the element type (half a step on top of the gate) into padded rows whose padding keeps the sentinel."""
    c = MC.prep_case(shape)
    BQ, Mh, L, P = shape
    LP = L * P
    gl, ga, aw = (Buf(BQ * Mh, n, n, F32, data=c[k]) for k, n in (("grad_loc", LP * 2), ("grad_attn", LP), ("aw", LP)))
    ref = Buf(BQ, 4, 4, F32, data=c["ref"])
    g_off, g_lg = Buf(BQ, Mh * LP * 2, Mh * LP * 2 + 8, adt()), Buf(BQ, Mh * LP, Mh * LP + 24, adt())
    check(lib.fx_msda_prep_bwd_bf16(gl.ptr, ga.ptr, aw.ptr, ref.ptr, g_off.ptr, g_off.ld, g_lg.ptr, g_lg.ld, BQ, Mh, L, P, stream()), "fx_msda_prep_bwd_bf16")
    torch.cuda.synchronize()
    g_off.assert_guards()
    g_lg.assert_guards()
    (o_ref, o_mag), (g_ref, g_mag) = MC.prep_bwd_ref(c)
    gate("prep.grad_off", sid(shape), g_off.get(), o_ref, o_mag, 1, adt())
    gate("prep.grad_logit", sid(shape), g_lg.get(), g_ref, g_mag, LP, adt())


# ------------------------------------------------------------------------------------------------ 5. AdamW
class AdamWBufs:
    def __init__(self, c, grad_scale=1.0):
        n = c["numel"]
        self.n = n
        self.p, self.m, self.v = (Buf(1, n, n, F32, prefill=c[k].reshape(1, n)) for k in ("p", "m", "v"))
        self.g = Buf(1, n, n, F32, data=c["g"] * grad_scale)
        cs, cl, clr, cwd = MC.adamw_chunks()
        self.nchunks = len(cs)
        self.cs = torch.tensor(cs, dtype=torch.int64, device=DEV)
        self.cl = torch.tensor(cl, dtype=torch.int32, device=DEV)
        self.clr = torch.tensor(clr, dtype=torch.float32, device=DEV)
        self.cwd = torch.tensor(cwd, dtype=torch.float32, device=DEV)
        self.norm = Buf(1, 1, 4, F32)

    def verify(self, c, what):
        torch.cuda.synchronize()
        lr, wd = MC.adamw_per_element()
        p1, m1, v1, norm, mags = MC.adamw_ref(c["p"], c["g"], c["m"], c["v"], c["step"], lr, wd, c["max_norm"])
        for b in (self.p, self.m, self.v, self.norm):
            b.assert_guards()
        gate("adamw.p", what, self.p.get()[0], p1, mags[0], 1)
        gate("adamw.m", what, self.m.get()[0], m1, mags[1], 1)
        gate("adamw.v", what, self.v.get()[0], v1, mags[2], 1)
        gate("adamw.total_norm", what, self.norm.get()[0], torch.tensor([norm], dtype=torch.float64), torch.tensor([norm], dtype=torch.float64), 1)
        lr0 = slice(256, 512)
        assert torch.equal(self.p.get()[0][lr0], c["p"][lr0]), f"{what}: lr = 0 changed a parameter"
        assert not torch.equal(self.m.get()[0][lr0], c["m"][lr0])


def test_adamw_chunk_table_is_flat_adamws(lib):
    from focoos_amd.train import FlatAdamW

    assert FlatAdamW.CHUNK == MC.ADAMW_CHUNK
    opt = FlatAdamW([(f"t{i}", (n,), lr, wd) for i, (n, lr, wd) in enumerate(MC.ADAMW_TENSORS)], DEV)
    cs, cl, clr, cwd = MC.adamw_chunks()
    assert opt.chunk_start.cpu().tolist() == cs and opt.chunk_len.cpu().tolist() == cl and opt.nchunks == len(cs)
    assert torch.equal(opt.chunk_lr.cpu(), torch.tensor(clr, dtype=F32)) and torch.equal(opt.chunk_wd.cpu(), torch.tensor(cwd, dtype=F32))
    assert max(cl) == FlatAdamW.CHUNK and cl.count(FlatAdamW.CHUNK) == 2 and 1 in cl


@pytest.mark.parametrize("run", range(len(MC.ADAMW_RUNS)))
def test_adamw_step(lib, run):
    """fx_adamw_step_f32 on ONE flat buffer of tensors of 1, 255, 256, 257, 65535, 65536 and 65537 elements (a chunk of exactly CHUNK, a
    chunk of one element), one with lr = 0, one without weight decay; max_grad_norm 0 (no clipping) and 0.1 with the norm below and above
    it; steps 1, 2 and 10000 - vs clip_grad_norm_ + AdamW in float64, element by element."""
    c = MC.adamw_case(run)
    b = AdamWBufs(c)
    ws = torch.empty(lib.fx_adamw_workspace_bytes() // 8, dtype=torch.float64, device=DEV)
    check(lib.fx_adamw_step_f32(b.p.ptr, b.g.ptr, b.m.ptr, b.v.ptr, b.n, b.cs.data_ptr(), b.cl.data_ptr(), b.clr.data_ptr(), b.cwd.data_ptr(), b.nchunks, c["step"],
                                MC.ADAMW_BETAS[0], MC.ADAMW_BETAS[1], MC.ADAMW_EPS, c["max_norm"], ws.data_ptr(), b.norm.ptr, stream()), "fx_adamw_step_f32")
    b.verify(c, f"run {run} {MC.ADAMW_RUNS[run]}")


@pytest.mark.parametrize("run", range(len(MC.ADAMW_RUNS)))
def test_adamw_step_scaled(lib, run):
    """fx_adamw_step_scaled_f32 on the same cases with grads = 1024 * g (the unscale is exact) and good_steps preset to step - 1: the same
    reference; the record afterwards holds the same scale, good_steps = step, growth_tracker + 1 and no skipped step."""
    c = MC.adamw_case(run)
    b = AdamWBufs(c, grad_scale=1024.0)
    ws = torch.empty(lib.fx_adamw_workspace_bytes() // 8, dtype=torch.float64, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    state.view(F32)[0] = 1024.0
    state[1], state[2] = 5, c["step"] - 1
    check(lib.fx_adamw_step_scaled_f32(b.p.ptr, b.g.ptr, b.m.ptr, b.v.ptr, b.n, b.cs.data_ptr(), b.cl.data_ptr(), b.clr.data_ptr(), b.cwd.data_ptr(), b.nchunks,
                                       MC.ADAMW_BETAS[0], MC.ADAMW_BETAS[1], MC.ADAMW_EPS, c["max_norm"], ws.data_ptr(), b.norm.ptr, state.data_ptr(), 2.0, 0.5, 2000,
                                       stream()), "fx_adamw_step_scaled_f32")
    b.verify(c, f"scaled run {run} {MC.ADAMW_RUNS[run]}")
    st = state.cpu()
    assert float(st.view(F32)[0]) == 1024.0 and st[1:].tolist() == [6, c["step"], 0]


# ------------------------------------------------------------------------------------------------ 6. refusals
INVALID, UNSUPPORTED = -1, -3


def test_msda_refusals(lib):
    """Every core entry point: M != 8 is FX_ERR_UNSUPPORTED; ldv < 256, ldv % 4 != 0, a misaligned value pointer, ldg < 256,
    zero_grad_value with ldg != 256, level sizes that do not sum to S (slab), a NULL pointer in each position are
    FX_ERR_INVALID_ARGUMENT; Q_max + 1 on the slab entry point is FX_ERR_UNSUPPORTED.  No output changes."""
    c = MC.core_case("l3p3")
    d = Dev(c)
    B, S, Q, Mh = d.dims
    L, P = c["L"], c["P"]
    vb, _, _ = d.value("elem")
    go, go16 = d.grad_out(False), d.grad_out(True)
    out = Buf(B * Q, CH, CH, F32)
    gl, ga = d.point_outs()
    gv32, gv16 = Slice(B * S, LDG, COL_G, F32), Slice(B * S, LDG, COL_G, adt())
    sh, st, host = d.shapes.data_ptr(), d.starts.data_ptr(), d.shapes_host.ctypes.data
    esz = vb.full.element_size()

    def fwd(value=vb.ptr, ldv=LDV, shapes=sh, starts=st, loc=d.loc.ptr, attn=d.attn.ptr, o=out.ptr, Mh=8):
        return lib.fx_msda_train_fwd(value, 1, ldv, shapes, starts, L, P, loc, attn, o, B, S, Q, Mh, stream())

    def bwd(value=vb.ptr, ldv=LDV, shapes=sh, starts=st, loc=d.loc.ptr, attn=d.attn.ptr, g=go.ptr, gv=gv32.ptr, ldg=LDG, zero=0, l=gl.ptr, a=ga.ptr, Mh=8):
        return lib.fx_msda_train_bwd(value, 1, ldv, shapes, starts, L, P, loc, attn, g, gv, ldg, zero, l, a, B, S, Q, Mh, stream())

    def slab(value=vb.ptr, ldv=LDV, shapes=sh, starts=st, hs=host, loc=d.loc.ptr, attn=d.attn.ptr, g=go16.ptr, gv=gv16.ptr, ldg=LDG, l=gl.ptr, a=ga.ptr, Mh=8, S_=S,
             Q_=Q):
        return lib.fx_msda_train_bwd_slab(value, 1, ldv, shapes, starts, hs, L, P, loc, attn, g, 1, gv, ldg, l, a, B, S_, Q_, Mh, stream())

    common = {"ldv < 256": {"ldv": 252}, "ldv % 4": {"ldv": LDV + 2}, "value misaligned": {"value": vb.ptr + esz}, "value NULL": {"value": None},
              "shapes NULL": {"shapes": None}, "starts NULL": {"starts": None}, "loc NULL": {"loc": None}, "attn NULL": {"attn": None}}
    bad_fwd = dict(common, **{"out NULL": {"o": None}})
    bad_bwd = dict(common, **{"grad_out NULL": {"g": None}, "grad_value NULL": {"gv": None}, "grad_loc NULL": {"l": None}, "grad_attn NULL": {"a": None},
                              "ldg < 256": {"ldg": 252}, "zero_grad_value with ldg != 256": {"zero": 1}})
    bad_slab = dict(common, **{"grad_out NULL": {"g": None}, "grad_value NULL": {"gv": None}, "grad_loc NULL": {"l": None}, "grad_attn NULL": {"a": None},
                               "ldg < 256": {"ldg": 252}, "shapes_host NULL": {"hs": None}, "levels do not sum to S": {"S_": S + 1},
                               "grad_out misaligned": {"g": go16.ptr + esz}})
    for name, call, bad in (("fx_msda_train_fwd", fwd, bad_fwd), ("fx_msda_train_bwd", bwd, bad_bwd), ("fx_msda_train_bwd_slab", slab, bad_slab)):
        for what, kw in bad.items():
            assert call(**kw) == INVALID, f"{name}: {what}"
        assert call(Mh=4) == UNSUPPORTED, f"{name}: M = 4"
    assert slab(Q_=MC.q_max(P, True) + 1) == UNSUPPORTED
    f32v = d.value("f32")[0]
    assert lib.fx_msda_f32_fwd(f32v.ptr, sh, st, L, P, d.loc.ptr, d.attn.ptr, out.ptr, B, S, Q, 4, stream()) == UNSUPPORTED
    assert lib.fx_msda_f32_fwd(None, sh, st, L, P, d.loc.ptr, d.attn.ptr, out.ptr, B, S, Q, 8, stream()) == INVALID
    assert lib.fx_msda_f32_bwd(f32v.ptr, sh, st, L, P, d.loc.ptr, d.attn.ptr, go.ptr, None, gl.ptr, ga.ptr, B, S, Q, 8, stream()) == INVALID
    assert lib.fx_msda_f32_bwd(f32v.ptr, sh, st, L, P, d.loc.ptr, d.attn.ptr, go.ptr, gv32.ptr, gl.ptr, ga.ptr, B, S, Q, 4, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    for b in (out, gl, ga):
        b.assert_guards(written=torch.zeros(b.rows, dtype=torch.bool))
    gv32.assert_guards(untouched=True)
    gv16.assert_guards(untouched=True)
    with pytest.raises(FocoosAmdError, match="invalid argument"):
        check(fwd(ldv=252), "fx_msda_train_fwd")
    with pytest.raises(FocoosAmdError, match="unsupported"):
        check(fwd(Mh=4), "fx_msda_train_fwd")
    assert fwd() == 0 and bwd() == 0 and slab() == 0
    torch.cuda.synchronize()


def test_prep_and_adamw_refusals(lib):
    """The prelude: a NULL pointer in each position, a leading dimension below the row, a misaligned ref, a size of 0.  fx_adamw_step_f32:
    step < 1, a NULL pointer in each position, no chunks.  fx_adamw_step_scaled_f32: growth_factor < 1, backoff_factor outside (0, 1],
    growth_interval < 1, a NULL state.  Nothing is written."""
    shape = MC.PREP_SHAPES[3]
    c = MC.prep_case(shape)
    BQ, Mh, L, P = shape
    LP = L * P
    off, lg = Buf(BQ, Mh * LP * 2, Mh * LP * 2 + 8, adt(), data=c["off"]), Buf(BQ, Mh * LP, Mh * LP + 24, adt(), data=c["logit"])
    ref = Buf(BQ, 4, 4, F32, data=c["ref"])
    loc, aw = Buf(BQ * Mh, LP * 2, LP * 2, F32), Buf(BQ * Mh, LP, LP, F32)

    def prep(o=off.ptr, ldo=off.ld, g=lg.ptr, ldl=lg.ld, r=ref.ptr, lo=loc.ptr, a=aw.ptr, BQ=BQ, L=L):
        return lib.fx_msda_prep_bf16(o, ldo, g, ldl, r, lo, a, BQ, Mh, L, P, stream())

    bad = {"off NULL": {"o": None}, "logit NULL": {"g": None}, "ref NULL": {"r": None}, "loc NULL": {"lo": None}, "aw NULL": {"a": None}, "ld_off short": {"ldo": Mh * LP * 2 - 2},
           "ld_logit short": {"ldl": Mh * LP - 1}, "ref misaligned": {"r": ref.ptr + 4}, "BQ 0": {"BQ": 0}, "L 0": {"L": 0}}
    for what, kw in bad.items():
        assert prep(**kw) == INVALID, f"fx_msda_prep_bf16: {what}"
    gl, ga, awi = (Buf(BQ * Mh, n, n, F32, data=c[k]) for k, n in (("grad_loc", LP * 2), ("grad_attn", LP), ("aw", LP)))
    g_off, g_lg = Buf(BQ, Mh * LP * 2, Mh * LP * 2 + 8, adt()), Buf(BQ, Mh * LP, Mh * LP + 24, adt())

    def prep_bwd(l=gl.ptr, a=ga.ptr, w=awi.ptr, r=ref.ptr, o=g_off.ptr, ldo=g_off.ld, g=g_lg.ptr, ldl=g_lg.ld, BQ=BQ):
        return lib.fx_msda_prep_bwd_bf16(l, a, w, r, o, ldo, g, ldl, BQ, Mh, L, P, stream())

    bad = {"grad_loc NULL": {"l": None}, "grad_attn NULL": {"a": None}, "aw NULL": {"w": None}, "ref NULL": {"r": None}, "grad_off NULL": {"o": None},
           "grad_logit NULL": {"g": None}, "ld_off short": {"ldo": Mh * LP * 2 - 2}, "ld_logit short": {"ldl": Mh * LP - 1}, "ref misaligned": {"r": ref.ptr + 4}, "BQ 0": {"BQ": 0}}
    for what, kw in bad.items():
        assert prep_bwd(**kw) == INVALID, f"fx_msda_prep_bwd_bf16: {what}"
    torch.cuda.synchronize()
    for b in (loc, aw, g_off, g_lg):
        b.assert_guards(written=torch.zeros(b.rows, dtype=torch.bool))
    assert prep() == 0 and prep_bwd() == 0

    ca = MC.adamw_case(1)
    b = AdamWBufs(ca)
    ws = torch.empty(lib.fx_adamw_workspace_bytes() // 8, dtype=torch.float64, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    state.view(F32)[0] = 1024.0

    def step(p=b.p.ptr, g=b.g.ptr, m=b.m.ptr, v=b.v.ptr, cs=b.cs.data_ptr(), cl=b.cl.data_ptr(), clr=b.clr.data_ptr(), cwd=b.cwd.data_ptr(), nch=b.nchunks, st=1,
             w=ws.data_ptr()):
        return lib.fx_adamw_step_f32(p, g, m, v, b.n, cs, cl, clr, cwd, nch, st, 0.9, 0.999, 1e-8, 0.1, w, b.norm.ptr, stream())

    bad = {"step 0": {"st": 0}, "step -1": {"st": -1}, "params NULL": {"p": None}, "grads NULL": {"g": None}, "exp_avg NULL": {"m": None}, "exp_avg_sq NULL": {"v": None},
           "chunk_start NULL": {"cs": None}, "chunk_len NULL": {"cl": None}, "chunk_lr NULL": {"clr": None}, "chunk_wd NULL": {"cwd": None}, "no chunks": {"nch": 0},
           "workspace NULL": {"w": None}, "workspace misaligned": {"w": ws.data_ptr() + 4}}
    for what, kw in bad.items():
        assert step(**kw) == INVALID, f"fx_adamw_step_f32: {what}"

    def scaled(s=state.data_ptr(), growth=2.0, backoff=0.5, interval=2000, p=b.p.ptr):
        return lib.fx_adamw_step_scaled_f32(p, b.g.ptr, b.m.ptr, b.v.ptr, b.n, b.cs.data_ptr(), b.cl.data_ptr(), b.clr.data_ptr(), b.cwd.data_ptr(), b.nchunks, 0.9, 0.999,
                                            1e-8, 0.1, ws.data_ptr(), b.norm.ptr, s, growth, backoff, interval, stream())

    bad = {"state NULL": {"s": None}, "growth_factor < 1": {"growth": 0.5}, "backoff_factor 0": {"backoff": 0.0}, "backoff_factor > 1": {"backoff": 1.5},
           "growth_interval 0": {"interval": 0}, "params NULL": {"p": None}}
    for what, kw in bad.items():
        assert scaled(**kw) == INVALID, f"fx_adamw_step_scaled_f32: {what}"
    torch.cuda.synchronize()
    for buf, k in ((b.p, "p"), (b.m, "m"), (b.v, "v")):
        buf.assert_guards()
        assert torch.equal(buf.get()[0], ca[k]), f"a refused optimiser step changed {k}"
    b.norm.assert_guards(written=torch.zeros(1, dtype=torch.bool))
    assert state.cpu()[1:].tolist() == [0, 0, 0]
