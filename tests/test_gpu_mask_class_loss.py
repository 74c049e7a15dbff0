"""fx_mask_class_loss_f32 / fx_mask_class_loss_bwd_f32 (csrc/mask_criterion_ops.hip: mask_label_cls_kernel, mask_label_cls_bwd_kernel - the
focal_loss / bce_loss / bce_focal_loss branches of the mask families' SetCriterion.loss_labels) on a real MI355X against the float64 run
of the REAL reference recorded in tests/golden/mask_class_loss.npz.  For bce_focal_loss the fixture mirrors the reference's call site
(loss.py:446-457) with sigmoid_focal_loss written from the published formula - torchvision's own code is not what is compared.

Cases (B, Q, K): (1,1,1) one row of a four-row block; (2,7,80) a tail block and K+1 = 81 = a wave of 64 lanes plus a remainder;
(3,5,149) three passes of a wave with a ragged last one and an image without targets; (2,100,19) K+1 < 64 under a padded leading
dimension.  Logits ~ N(0, 3^2) with +-30 planted, also on matched classes.  Every case runs with a tight and a padded leading dimension;
the padding, and the last column that bce_loss drops under cls_sigmoid, hold NaN in the input: a read of either poisons the outputs.

The bounds are derived in tests/mask_class_loss_cases.py from the kernels' operation sequence (no figure of a kernel's output enters)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from tests import mask_class_loss_cases as MC  # noqa: E402

DEV = "cuda:0"
W_CE, GRAD = 2.0, 0.5      # powers of two: the scaling of the reference values is exact


@pytest.fixture(params=["bf16", "fp16"])
def lib(request):
    """Both builds export the kernels (they read fp32 logits: the element type changes nothing in them)."""
    assert torch.cuda.is_available()
    prev = _lib.set_compute_dtype(request.param)
    yield _lib.load()
    _lib.set_compute_dtype(prev)


def _case(ci, name):
    c = MC.load_cases()[ci]
    return c, c["variants"][name]


@pytest.mark.parametrize("ld_pad", [0, 5])
@pytest.mark.parametrize("ci,name", MC.case_ids(), ids=[f"c{ci}-{n}" for ci, n in MC.case_ids()])
def test_loss_and_gradient_match_float64_reference(lib, ci, name, ld_pad):
    case, var = _case(ci, name)
    K, cols = case["K"], var["cols"]
    loss, dl, guards_ok = MC.run_kernels(lib, case, var, ld_pad=ld_pad, w_ce=W_CE, grad=GRAD)
    assert guards_ok, "rows outside the [B*Q] slab were written"
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dl).all()), "NaN / inf in an output (a NaN input column was read, or an unstable form)"
    assert bool((dl[..., cols:] == 0).all()), "columns outside the loss (dropped last column, leading-dimension padding) must get exactly 0"
    tol_loss, _ = MC.bounds(case, var, W_CE)
    _, tol_d = MC.bounds(case, var, W_CE * GRAD)
    ref_loss = var["loss64"] * W_CE
    ref_d = var["dlogits64"][..., :cols].double() * (W_CE * GRAD)
    err_loss = abs(float(loss) - ref_loss)
    err_d = (dl[..., :cols].double() - ref_d).abs()
    ratio = float((err_d / tol_d).max())
    ref32 = abs(var["loss32"] - var["loss64"]) * W_CE
    print(f"CLASSLOSS c{ci} {name} ld+{ld_pad} K{K}: loss err {err_loss:.3e} bound {tol_loss:.3e} (reference fp32 vs fp64 {ref32:.3e}); "
          f"dlogits max err {float(err_d.max()):.3e} max err/bound {ratio:.3e}")
    assert err_loss <= tol_loss, f"loss {float(loss)!r} vs {ref_loss!r}: error {err_loss:.3e} > bound {tol_loss:.3e}"
    assert ratio <= 1.0, f"dlogits: error / bound = {ratio:.3e}"
    if name == "bce_drop":   # the last column really is ignored: same bits as the variant that never had it
        loss2, dl2, _ = MC.run_kernels(lib, case, case["variants"]["bce"], ld_pad=ld_pad + 1, w_ce=W_CE, grad=GRAD)
        assert torch.equal(loss, loss2) and torch.equal(dl[..., :K], dl2[..., :K])


@pytest.mark.parametrize("ci,name", MC.case_ids(), ids=[f"c{ci}-{n}" for ci, n in MC.case_ids()])
def test_two_runs_are_bit_identical(lib, ci, name):
    case, var = _case(ci, name)
    a = MC.run_kernels(lib, case, var, ld_pad=3)
    b = MC.run_kernels(lib, case, var, ld_pad=3)
    assert a[0].view(torch.int32).item() == b[0].view(torch.int32).item()
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_upstream_gradient_and_weight_scale_dlogits(lib):
    """dlogits is linear in w_ce * grad (powers of two: exactly), the loss in w_ce."""
    case, var = _case(1, "bce_drop")
    l1, d1, _ = MC.run_kernels(lib, case, var, w_ce=1.0, grad=1.0)
    l2, d2, _ = MC.run_kernels(lib, case, var, w_ce=4.0, grad=0.125)
    assert float(l2) == 4.0 * float(l1)
    assert torch.equal(d2, d1 * 0.5)


def test_invalid_arguments_return_the_error_code_without_a_launch(lib):
    """K < 1, a leading dimension below the columns read, an unknown mode (and ce_loss, which these entry points do not compute), a NULL
    pointer, a short workspace: FX_ERR_INVALID_ARGUMENT, and the refused call touches no output."""
    B, Q, K = 2, 3, 4
    logits = torch.zeros(B * Q, K + 1, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    off = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(B * Q * 2, dtype=torch.float64, device=DEV)
    out = torch.full((1,), 7.0, device=DEV)
    dl = torch.full((B * Q, K + 1), 7.0, device=DEV)
    g = torch.ones(1, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K=K, ldl=K + 1, mode=MC.BCE, logits_ptr=logits.data_ptr(), nws=ws.numel() * 8, lddl=K + 1, num_masks=1.0):
        common = (logits_ptr, ldl, i32.data_ptr(), off.data_ptr(), i32.data_ptr(), i32.data_ptr(), B, Q, K, mode, 0.75, 2.0, num_masks, 1.0)
        return (lib.fx_mask_class_loss_f32(*common, ws.data_ptr(), nws, out.data_ptr(), st),
                lib.fx_mask_class_loss_bwd_f32(*common, g.data_ptr(), dl.data_ptr(), lddl, st))

    INV = -1   # FX_ERR_INVALID_ARGUMENT
    assert call(K=0) == (INV, INV)
    assert call(K=-3) == (INV, INV)
    assert call(mode=MC.BCE, ldl=K - 1, lddl=K - 1) == (INV, INV)
    assert call(mode=MC.BCE_FOCAL, ldl=K - 1, lddl=K - 1) == (INV, INV)
    assert call(mode=MC.FOCAL, ldl=K, lddl=K) == (INV, INV)             # the softmax reads K + 1 columns
    assert call(mode=0) == (INV, INV)
    assert call(mode=4) == (INV, INV)
    assert call(mode=-1) == (INV, INV)
    assert call(logits_ptr=None) == (INV, INV)
    assert call(num_masks=0.0) == (INV, INV)
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()) and float(out) == 7.0, "a refused call wrote an output"
    assert call(mode=MC.FOCAL, lddl=K) == (0, INV)                      # lddl alone too small: only the backward refuses
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all()) and bool(torch.isfinite(out).all())
    out.fill_(7.0)
    assert call(nws=ws.numel() * 8 - 8)[0] == INV                       # a short workspace: only the forward needs one
    torch.cuda.synchronize()
    assert float(out) == 7.0
    assert call(mode=MC.BCE, ldl=K, lddl=K) == (0, 0)                    # K columns suffice for the sigmoid losses
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
