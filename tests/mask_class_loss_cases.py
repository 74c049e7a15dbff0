"""Shared by tests/test_mask_class_loss_cpu.py, tests/test_gpu_mask_class_loss.py and tests/test_gpu_train_cls_sigmoid.py: the cases of
tests/golden/mask_class_loss.npz (scripts/make_golden_mask_class_loss.py: the REAL reference's SetCriterion.loss_labels for focal_loss,
bce_loss with / without the dropped last column, bce_focal_loss, in fp32 and in float64 with autograd), the error bounds of the fp32
kernels against the float64 values, and the direct kernel call.

Error bounds.  U = 2^-24.  Everything is derived from the kernels' operation sequence and the inputs; nothing comes from a kernel's output.
An accurate libm call (expf, logf, log1pf, expm1f, powf: <= 2 ulp) costs 4 U relative, an fp32 add / mul / div 1 U.  Row partials and
everything after them are float64 (error ~2^-53, ignored); the final (float) cast and the multiplication by w_ce cost 2 U.

* sigmoid losses (BCE, BCE_FOCAL), z = x for target 1, -x for target 0.  Every quantity is a product / sum of POSITIVE terms, each
  computed directly (softplus(-z) = max(-z, 0) + log1p(exp(-|z|)), sigmoid(-z) = 1 / (1 + exp(z)), sigmoid(z) likewise - never as a
  difference), so errors are relative to the element itself:
    BCE        element and gradient: c_rel = 32 U      (exp, log1p, add / exp, add, div; three factors of the gradient's coefficient)
    BCE_FOCAL  a_t * s^gamma * bce: s to 8 U, s^gamma to (8 gamma + 4) U, bce 8 U, p_t 8 U, products: c_rel = (8 gamma + 48) U
  loss: a lane adds ceil(K / 64) elements in fp32, so  |loss - ref| <= (c_rel + ceil(K / 64) + 8) U * sum|elements| * scale / num_masks.
  dlogits: |d - ref| <= c_rel U |ref| (+ the fp32 flush floor 2^-126).
* softmax focal loss.  With R = (K + 1) + 2 max|x| + 16 the relative error of every exp(x - max) / of their sum (the rounding of
  x - max moves the exponent by up to 2 max|x| U, expf 4 U, at most K + 1 additions), ce = (max - x_y) + log(sum) - two non-negative
  terms - has the ABSOLUTE error E = U (R + 4 ce).  L = a ce u^gamma, u = 1 - p_t = -expm1(-ce); D = dL/dce = a (u^gamma + gamma ce
  u^(gamma-1) p_t) <= a (1 + gamma) because ce p_t / u <= 1; |dD/dce| <= a gamma (gamma + 2) for gamma >= 1 (same inequality, ce p_t <= 1/e).
    loss: sum over rows [a (1 + gamma) E + (4 gamma + 16) U L] / (B Q) + 4 U |loss|, times scale
    dlogits[c] = coef D (p_c - [c == y]), the kernel takes p_y - 1 = -u:
      a gamma (gamma + 2) E m_c + D (c == y ? E p_y + 4 U u : p_c (R + 2) U) + (4 gamma + 28) U D m_c,  m_c = |p_c - [c == y]|, times scale / (B Q)
  (the E terms dominate: an absolute 1e-5-ish error of ce is what fp32 logits of magnitude 30 allow).
* the float64 reference's own error.  The reference forms 1 - p_t and sigmoid(x) - t as differences; in float64 that leaves an absolute error
  of a few 2^-53 times the gradient's other factors where p_t -> 1 (x = 30 on the matched class: sigmoid(30) - 1 = -9.4e-14 carries a
  relative error of 1e-3).  The kernels do not cancel there, so the gradient bounds get REF64 = 8 (1 + gamma) (1 + |x| or ce) 2^-53 times
  the element's scale: ~1e-14, far below anything a wrong kernel produces."""
import ctypes as C
import functools
import math

import numpy as np
import torch

from tests.helpers import load_golden

U32 = 2.0 ** -24
FLOOR = 2.0 ** -126
U64 = 2.0 ** -53
MODE_NAMES = {1: "focal_loss", 2: "bce_loss", 3: "bce_focal_loss"}
FOCAL, BCE, BCE_FOCAL = 1, 2, 3


@functools.lru_cache(maxsize=None)
def load_cases():
    g = load_golden("mask_class_loss.npz")
    cases = []
    for ci, (B, Q, K) in enumerate(g["cases"].tolist()):
        sizes = g[f"c{ci}_sizes"].tolist()
        offsets = np.zeros(B + 1, np.int64)
        offsets[1:] = np.cumsum(sizes)
        c = {"ci": ci, "B": B, "Q": Q, "K": K, "sizes": sizes, "offsets": offsets, "logits": torch.from_numpy(g[f"c{ci}_logits"]),
             "labels": torch.from_numpy(g[f"c{ci}_labels"]), "pred_idx": torch.from_numpy(g[f"c{ci}_pred_idx"]),
             "tgt_idx": torch.from_numpy(g[f"c{ci}_tgt_idx"]), "num_masks": float(g[f"c{ci}_num_masks"]), "variants": {}}
        tc = torch.full((B, Q), K, dtype=torch.int64)                   # target class per row, K = no object
        for b in range(B):
            o0, o1 = offsets[b], offsets[b + 1]
            tc[b, c["pred_idx"][o0:o1]] = c["labels"][o0:o1][c["tgt_idx"][o0:o1]]
        c["target_classes"] = tc
        for name in g[f"c{ci}_variants"].tolist():
            mode, sig, width, alpha, gamma = g[f"c{ci}_{name}_params"].tolist()
            c["variants"][name] = {"name": name, "mode": int(mode), "cls_sigmoid": bool(sig), "width": int(width), "alpha": alpha, "gamma": gamma,
                                   "cols": K + 1 if int(mode) == FOCAL else K, "loss32": float(g[f"c{ci}_{name}_loss32"]),
                                   "loss64": float(g[f"c{ci}_{name}_loss64"]), "dlogits64": torch.from_numpy(g[f"c{ci}_{name}_dlogits64"])}
        cases.append(c)
    return cases


def case_ids():
    return [(c["ci"], name) for c in load_cases() for name in c["variants"]]


def bounds(case, var, scale):
    """(bound on |scale * loss - kernel loss|, bound [B,Q,cols] on |scale * dlogits64 - kernel dlogits|): see the module docstring."""
    B, Q, K = case["B"], case["Q"], case["K"]
    a, gm = var["alpha"], var["gamma"]
    y = case["target_classes"]
    if var["mode"] == FOCAL:
        assert gm >= 1.0
        x = case["logits"][..., : K + 1].double()
        R = (K + 1) + 2.0 * float(x.abs().max()) + 16.0
        lse = torch.logsumexp(x, -1)
        p = torch.softmax(x, -1)
        hot = torch.nn.functional.one_hot(y, K + 1).double()
        ce = lse - x.gather(-1, y.unsqueeze(-1)).squeeze(-1)
        E = U32 * (R + 4.0 * ce)
        pt = torch.exp(-ce)
        u = -torch.expm1(-ce)
        af = a if a >= 0 else 1.0
        L = af * ce * u ** gm
        D = af * (u ** gm + gm * ce * u ** (gm - 1.0) * pt)
        tol_loss = scale * float((af * (1.0 + gm) * E + (4.0 * gm + 16.0) * U32 * L).sum()) / (B * Q) + 4.0 * U32 * abs(var["loss64"] * scale)
        m = (p - hot).abs()
        per = torch.where(hot.bool(), (E * pt + 4.0 * U32 * u).unsqueeze(-1).expand_as(p), p * (R + 2.0) * U32)
        tol_d = scale / (B * Q) * (af * gm * (gm + 2.0) * E.unsqueeze(-1) * m + D.unsqueeze(-1) * per + (4.0 * gm + 28.0) * U32 * D.unsqueeze(-1) * m
                                   + 8.0 * (1.0 + gm) * (1.0 + ce.unsqueeze(-1)) * U64) + FLOOR
        return tol_loss, tol_d
    x = case["logits"][..., :K].double()
    hot = torch.nn.functional.one_hot(y, K + 1)[..., :K].double()
    z = x * (2.0 * hot - 1.0)
    el = torch.nn.functional.softplus(-z)
    c_rel = 32.0
    if var["mode"] == BCE_FOCAL:
        a_t = (a * hot + (1.0 - a) * (1.0 - hot)) if a >= 0 else torch.ones_like(hot)
        el = a_t * torch.sigmoid(-z) ** gm * el
        c_rel = 8.0 * gm + 48.0
    tol_loss = (c_rel + math.ceil(K / 64) + 8.0) * U32 * float(el.sum()) * scale / case["num_masks"]
    gm_ref = gm if var["mode"] == BCE_FOCAL else 0.0
    tol_d = c_rel * U32 * (var["dlogits64"][..., :K].double() * scale).abs() + 8.0 * (1.0 + gm_ref) * (1.0 + x.abs()) * U64 * scale / case["num_masks"] + FLOOR
    return tol_loss, tol_d


GUARD_ROWS = 2


def run_kernels(lib, case, var, ld_pad=0, w_ce=2.0, grad=0.5, nan_unread=True, dev="cuda:0"):
    """fx_mask_class_loss_f32 + fx_mask_class_loss_bwd_f32 on the case: logits [B*Q][width + ld_pad] between guard rows, padding (and with
    ``nan_unread`` the dropped last column of the bce_loss-with-cls_sigmoid variant) NaN; dlogits prefilled with NaN.  Returns (loss f32
    scalar tensor, dlogits [B,Q,ld] on the CPU, True if the guard rows of dlogits kept their fill)."""
    from focoos_amd._lib import check

    B, Q, K = case["B"], case["Q"], case["K"]
    width, ld, rows = var["width"], var["width"] + ld_pad, B * Q
    buf = torch.full((rows + 2 * GUARD_ROWS, ld), float("nan"), dtype=torch.float32)
    buf[GUARD_ROWS:GUARD_ROWS + rows, :width] = case["logits"][..., :width].reshape(rows, width)
    if nan_unread:
        buf[GUARD_ROWS:GUARD_ROWS + rows, var["cols"]:] = float("nan")
    buf = buf.to(dev)
    dl = torch.full((rows + 2 * GUARD_ROWS, ld), float("nan"), dtype=torch.float32, device=dev)
    i32 = lambda t: (t if len(t) else torch.zeros(1, dtype=torch.int64)).to(device=dev, dtype=torch.int32)   # noqa: E731
    labels, pi, ti = i32(case["labels"]), i32(case["pred_idx"]), i32(case["tgt_idx"])
    off = torch.from_numpy(case["offsets"]).to(device=dev, dtype=torch.int32)
    nws = int(lib.fx_mask_class_loss_workspace_bytes(B, Q))
    assert nws == B * Q * 16
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    g = torch.tensor([grad], dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (buf[GUARD_ROWS].data_ptr(), ld, labels.data_ptr(), off.data_ptr(), pi.data_ptr(), ti.data_ptr(), B, Q, K, var["mode"], var["alpha"],
              var["gamma"], case["num_masks"], w_ce)
    check(lib.fx_mask_class_loss_f32(*common, ws.data_ptr(), nws, out.data_ptr(), st), "fx_mask_class_loss_f32")
    check(lib.fx_mask_class_loss_bwd_f32(*common, g.data_ptr(), dl[GUARD_ROWS].data_ptr(), ld, st), "fx_mask_class_loss_bwd_f32")
    torch.cuda.synchronize()
    dl = dl.cpu()
    guards_ok = bool(torch.isnan(dl[:GUARD_ROWS]).all() and torch.isnan(dl[GUARD_ROWS + rows:]).all())
    return out.cpu()[0], dl[GUARD_ROWS:GUARD_ROWS + rows].reshape(B, Q, ld), guards_ok


def class_loss_direct(lib, logits, labels, offsets, pred_idx, tgt_idx, K, mode, alpha, gamma, num_masks, w_ce, grad=1.0):
    """The two entry points on device tensors: logits f32 [B,Q,C] contiguous; labels / offsets / pred_idx / tgt_idx int32 as the criterion
    holds them.  Returns (w_ce * loss as a 0-d device tensor, dlogits [B,Q,C] under the upstream gradient ``grad``)."""
    from focoos_amd._lib import check

    assert logits.dtype == torch.float32 and logits.is_contiguous()
    B, Q, Cc = logits.shape
    dev = logits.device
    ws = torch.empty(int(lib.fx_mask_class_loss_workspace_bytes(B, Q)) // 8, dtype=torch.float64, device=dev)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    dl = torch.full_like(logits, float("nan"))
    g = torch.tensor([grad], dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    common = (logits.data_ptr(), Cc, labels.data_ptr(), offsets.data_ptr(), pred_idx.data_ptr(), tgt_idx.data_ptr(), B, Q, K, mode, alpha, gamma,
              float(num_masks), float(w_ce))
    check(lib.fx_mask_class_loss_f32(*common, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), st), "fx_mask_class_loss_f32")
    check(lib.fx_mask_class_loss_bwd_f32(*common, g.data_ptr(), dl.data_ptr(), Cc, st), "fx_mask_class_loss_bwd_f32")
    return out[0], dl
