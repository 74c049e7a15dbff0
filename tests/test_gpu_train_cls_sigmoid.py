"""Training the two mask families with ``cls_sigmoid: true`` (the reference then builds its criterion with loss_class_type="bce_loss" and a
sigmoid matcher, fai_mf/modelling.py:660-697, bisenetformer/modelling.py:557-593) on a real MI355X, at the smallest configurations the
training tests of the families use (fai-mf-m-ade / bisenetformer-m-ade, 128 x 160, two images, 1024 sample points).

The class-loss arithmetic itself is pinned to the float64 reference fixture in tests/test_gpu_mask_class_loss.py; here the criterion inside
the training graph must give what those entry points give on the same logits, matches and num_masks, for every decoder layer."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from focoos_amd import _lib  # noqa: E402
from focoos_amd._lib import check  # noqa: E402
from focoos_amd.mask_criterion import _MaskTargets  # noqa: E402
from focoos_amd.ports import MaskFormerTargets  # noqa: E402
from focoos_amd.registry import ModelRegistry  # noqa: E402
from focoos_amd.synth import synth_image_structured, synth_state_dict  # noqa: E402
from oracle import train_oracle as T  # noqa: E402
from tests import mask_class_loss_cases as MC  # noqa: E402

DEV = "cuda:0"
FAMILIES = {"fai_mf": "fai-mf-m-ade", "bisenetformer": "bisenetformer-m-ade"}
SIZE = (128, 160)


class _SameDrawsEveryStep:
    """``rand`` of the matcher / criterion: uniform draws on the device from a generator that ``reset()`` rewinds, so that repeated
    evaluations on one batch see the same sample points; ``rec`` keeps what was handed out since the last reset."""

    def __init__(self, seed):
        self.seed, self.g, self.rec = seed, None, []

    def reset(self):
        self.g = torch.Generator(device=DEV).manual_seed(self.seed)
        self.rec = []

    def __call__(self, *shape, device):
        if self.g is None:
            self.reset()
        t = torch.rand(*shape, generator=self.g, device=device)
        self.rec.append(t)
        return t


def _trainable_class(family):
    if family == "fai_mf":
        from focoos_amd.train_mf import FAIMaskFormerTrainable as cls
    else:
        from focoos_amd.train_bf import BisenetFormerTrainable as cls
    return cls


def _build(family, cls_sigmoid, rand=None):
    cfg = dict(ModelRegistry.get_model_info(FAMILIES[family])["config"], criterion_num_points=1024, cls_sigmoid=cls_sigmoid)
    model = _trainable_class(family)(cfg, norm="FrozenBN", rand=rand).to(DEV)
    model.load_state_dict(synth_state_dict(cfg, 51, family=family), strict=True)
    model.train()
    return cfg, model


def _batch(cfg):
    imgs = [synth_image_structured(210 + i, *SIZE) for i in range(2)]
    labels, masks = T.synth_mask_targets(11, 2, int(cfg["num_classes"]), SIZE, counts=(3, 4))
    targets = [MaskFormerTargets(labels=l.to(DEV), masks=m.to(DEV)) for l, m in zip(labels, masks)]
    return torch.from_numpy(np.stack(imgs)).to(DEV), targets


def _loss_keys(cfg):
    n = int(cfg["transformer_predictor_dec_layers"])
    return sorted(f"loss_{k}{s}" for k in ("ce", "mask", "dice") for s in [""] + [f"_{i}" for i in range(n)])


def _leaf_sets(out):
    """The prediction sets as fp32 leaves (main set first, then the auxiliary ones): the criterion's gradient at the class head's logits
    arrives in ``.grad`` unrounded."""
    sets = [out] + list(out["aux_outputs"])
    leaves = [{"pred_logits": s["pred_logits"].detach().float().contiguous().requires_grad_(True),
               "pred_masks": s["pred_masks"].detach().float().contiguous().requires_grad_(True)} for s in sets]
    return leaves, dict(leaves[0], aux_outputs=leaves[1:])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_trainable_constructs_with_cls_sigmoid(family):
    """Raised NotImplementedError before the class-loss kernels existed."""
    cfg, model = _build(family, True)
    crit = model.head.criterion.fn
    assert crit.loss_class_type == "bce_loss" and crit.cls_sigmoid is True and crit.matcher.cls_sigmoid is True
    assert model.head.predictor.forward_prediction_heads.classifier.weight.shape[0] == int(cfg["num_classes"]) + 1    # modelling.py:53: the head keeps K + 1 outputs
    _, model = _build(family, False)
    crit = model.head.criterion.fn
    assert crit.loss_class_type == "ce_loss" and crit.cls_sigmoid is False and crit.matcher.cls_sigmoid is False


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_step_losses_and_class_head_gradient_equal_the_kernels(family):
    rand = _SameDrawsEveryStep(3)
    cfg, model = _build(family, True, rand)
    K = int(cfg["num_classes"])
    x, targets = _batch(cfg)
    losses = model(x, targets)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert sorted(losses) == _loss_keys(cfg)                              # the reference's keys, one triple per decoder layer
    assert all(np.isfinite(float(v.detach())) for v in losses.values()), {k: float(v.detach()) for k, v in losses.items()}
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)
    wc = model.head.predictor.forward_prediction_heads.classifier
    assert float(wc.weight.grad.abs().max()) > 0 and float(wc.weight.grad[K].abs().max()) == 0.0    # the no-object output is outside the BCE loss

    # the criterion again on fp32 leaves of the same prediction sets, against the stand-alone entry points
    lib = _lib.load()
    crit = model.head.criterion.fn
    leaves, outputs = _leaf_sets(model.last_outputs)
    rand.reset()
    l2 = crit(outputs, targets)
    sum(v for k, v in l2.items() if k.startswith("loss_ce")).backward()
    tg = _MaskTargets(targets, torch.device(DEV))
    num_masks = max(float(tg.n), 1.0)
    for j, leaf in enumerate(leaves):
        key = "loss_ce" + ("" if j == 0 else f"_{j - 1}")
        assert float(l2[key]) == float(losses[key])                       # same logits (the 16-bit ones, widened), same draws
        pi, ti = crit.all_matches[j]
        ref_loss, ref_d = MC.class_loss_direct(lib, leaf["pred_logits"].detach(), tg.labels, tg.offsets, pi, ti, K, MC.BCE, crit.focal_alpha, crit.focal_gamma,
                                               num_masks, crit.weight_dict["loss_ce"], 1.0)
        torch.cuda.synchronize()
        d = leaf["pred_logits"].grad
        assert d.shape[-1] == K + 1 and bool((d[..., K] == 0).all())
        # both paths launch the same kernels on the same arguments and add the same float64 row partials in the same order
        assert torch.equal(d, ref_d), (key, float((d - ref_d).abs().max()))
        assert abs(float(l2[key]) - float(ref_loss)) <= 4 * MC.U32 * abs(float(ref_loss)), (key, float(l2[key]), float(ref_loss))
        # and what they compute is the BCE of the reference on these logits: float64 torch, the bounds of tests/mask_class_loss_cases.py
        case = {"B": d.shape[0], "Q": d.shape[1], "K": K, "logits": leaf["pred_logits"].detach().cpu(), "num_masks": num_masks}
        tc = torch.full(d.shape[:2], K, dtype=torch.int64)
        off = tg.off_host
        for b in range(d.shape[0]):
            tc[b, pi[off[b]:off[b + 1]].cpu().long()] = tg.labels[off[b]:off[b + 1]].cpu().long()[ti[off[b]:off[b + 1]].cpu().long()]
        case["target_classes"] = tc
        x64 = case["logits"][..., :K].double().requires_grad_(True)
        hot = torch.nn.functional.one_hot(tc, K + 1)[..., :K].double()
        l64 = torch.nn.functional.binary_cross_entropy_with_logits(x64, hot, reduction="none").mean(1).sum() * d.shape[1] / num_masks
        l64.backward()
        var = {"mode": MC.BCE, "alpha": crit.focal_alpha, "gamma": crit.focal_gamma, "loss64": float(l64), "dlogits64": x64.grad}
        w = float(crit.weight_dict["loss_ce"])
        tol_loss, tol_d = MC.bounds(case, var, w)
        assert abs(float(ref_loss) - w * float(l64)) <= tol_loss, (key, float(ref_loss), w * float(l64), tol_loss)
        assert float(((ref_d[..., :K].cpu().double() - w * x64.grad).abs() / tol_d).max()) <= 1.0, key


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_three_optimizer_steps_lower_the_loss(family):
    from focoos_amd.train_detr import TrainStep

    rand = _SameDrawsEveryStep(4)
    cfg, model = _build(family, True, rand)
    x, targets = _batch(cfg)
    ts = TrainStep(model, lr=1e-4, max_grad_norm=0.1)
    totals = []
    for _ in range(4):                                                   # the fourth call reports the loss after three updates
        rand.reset()
        out = ts.step(x, targets)
        totals.append(sum(float(v) for v in out.values()))
    torch.cuda.synchronize()
    print(f"{family} cls_sigmoid total loss per step: {[round(t, 4) for t in totals]}")
    assert all(np.isfinite(t) for t in totals)
    assert totals[3] < totals[0], totals


def test_bisenetformer_fp16_step_with_cls_sigmoid():
    """The loss-scaled fp16 step (what the benchmark's BiSeNetFormer training run uses): the class loss reads fp32 logits, so the scale only
    reaches it through the upstream gradient of dlogits."""
    from focoos_amd.train_detr import TrainStep

    with _lib.using_compute_dtype("fp16"):
        rand = _SameDrawsEveryStep(5)
        cfg, model = _build("bisenetformer", True, rand)
        x, targets = _batch(cfg)
        ts = TrainStep(model)
        assert ts.dtype_name == "fp16" and ts.opt.scaler is not None
        before = ts.opt.flat_p.clone()
        for _ in range(3):
            rand.reset()
            out = ts.step(x, targets)
        torch.cuda.synchronize()
        st = ts.opt.scaler_state()
        assert sorted(out) == _loss_keys(cfg) and all(np.isfinite(float(v)) for v in out.values())
        assert st["good_steps"] >= 1, st
        assert bool(torch.isfinite(ts.opt.flat_p).all()) and not torch.equal(before, ts.opt.flat_p)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ce_path_is_untouched_without_cls_sigmoid(family):
    """cls_sigmoid: false through the same harness: every set's three losses and the class-logit gradient equal, bit for bit, a direct call
    of fx_mask_set_loss_f32 / fx_mask_set_loss_bwd_f32 with the argument list the criterion has always built for the CE loss."""
    rand = _SameDrawsEveryStep(6)
    cfg, model = _build(family, False, rand)
    K = int(cfg["num_classes"])
    x, targets = _batch(cfg)
    with torch.no_grad():
        out = model.forward_outputs(x)
    crit = model.head.criterion.fn
    assert crit.loss_class_type == "ce_loss"
    leaves, outputs = _leaf_sets(out)
    rand.reset()
    losses = crit(outputs, targets)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert sorted(losses) == _loss_keys(cfg)
    lib = _lib.load()
    tg = _MaskTargets(targets, torch.device(DEV))
    P, B = crit.num_points, len(targets)
    n_over, n_extra = int(P * crit.oversample_ratio), P - int(crit.importance_sample_ratio * P)
    wd = crit.weight_dict
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    draws = iter(rand.rec)
    for j, leaf in enumerate(leaves):
        for _ in range(B):
            next(draws)                                                   # the matcher's points
        r_over, r_extra = next(draws).float().contiguous(), next(draws).float().contiguous()
        assert r_over.shape == (tg.n, n_over, 2) and r_extra.shape == (tg.n, n_extra, 2)
        logits, pm = leaf["pred_logits"].detach(), leaf["pred_masks"].detach()
        Q, K1 = logits.shape[1:]
        assert K1 == K + 1
        h, w = pm.shape[-2:]
        pi, ti = crit.all_matches[j]
        ws = torch.empty(lib.fx_mask_set_loss_workspace_bytes(B, Q, tg.n, n_over) // 8 + 1, dtype=torch.float64, device=DEV)
        out3 = torch.empty(3, dtype=torch.float32, device=DEV)
        args = (logits.data_ptr(), K1, pm.data_ptr(), h, w, tg.masks.data_ptr(), tg.is_u8, tg.H, tg.W, tg.labels.data_ptr(), tg.offsets.data_ptr(), tg.n,
                pi.data_ptr(), ti.data_ptr(), r_over.data_ptr(), n_over, r_extra.data_ptr(), n_extra, P, B, Q, K1 - 1, float(crit.eos_coef),
                max(float(tg.n), 1.0), float(wd["loss_ce"]), float(wd["loss_mask"]), float(wd["loss_dice"]), ws.data_ptr(), ws.numel() * 8)
        check(lib.fx_mask_set_loss_f32(*args, out3.data_ptr(), st), "fx_mask_set_loss_f32")
        g3 = torch.ones(3, dtype=torch.float32, device=DEV)
        dlogits, dmasks = torch.empty_like(logits), torch.zeros_like(pm)
        check(lib.fx_mask_set_loss_bwd_f32(*args, g3.data_ptr(), dlogits.data_ptr(), K1, dmasks.data_ptr(), st), "fx_mask_set_loss_bwd_f32")
        torch.cuda.synchronize()
        s = "" if j == 0 else f"_{j - 1}"
        got = torch.stack([losses[f"loss_ce{s}"], losses[f"loss_mask{s}"], losses[f"loss_dice{s}"]])
        assert torch.equal(got.view(torch.int32), out3.view(torch.int32)), (s, got.tolist(), out3.tolist())
        assert torch.equal(leaf["pred_logits"].grad, dlogits), s
        # the mask gradient is summed per plane band with LDS float atomics: the order of the additions, and so the last bits, vary between runs
        assert torch.allclose(leaf["pred_masks"].grad, dmasks, rtol=1e-4, atol=1e-6 * float(dmasks.abs().max())), s


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_focoos_model_train_with_cls_sigmoid_validates_and_reloads(tmp_path, family):
    """``FocoosModel.train`` end to end on a cls_sigmoid configuration: two iterations, a validation (the inference engine applies the sigmoid,
    engine_mf.py / engine_bf.py), the best weights reloaded - no refusal anywhere - and the public eval entry point reproduces the record."""
    from focoos_amd.model import ModelManager
    from tests.test_gpu_train_validation import _args, _artifacts, _sem_entries

    fm = ModelManager.get(FAMILIES[family], seed=4, criterion_num_points=1024, cls_sigmoid=True)
    assert fm.model_info.config.get("cls_sigmoid") is True and fm.model_info.config.get("postprocessing_type") == "semantic"
    data = _sem_entries(4, fm.model.num_classes)
    name = f"cls_sigmoid_{family}"
    args = _args(tmp_path, name, max_iters=2, batch_size=2, eval_period=2)
    fm.train(args, data, data)
    folder, records, info, ck = _artifacts(tmp_path, name)
    assert [r["iteration"] for r in records] == [2] and np.isfinite(records[0]["sem_seg/mIoU"])
    assert info["val_metrics"] == records[0] and ck["iteration"] == 2
    res = fm.eval(args, data, save_json=False)["sem_seg"]
    assert {f"sem_seg/{k}": v for k, v in res.items()} == {k: v for k, v in records[0].items() if k != "iteration"}
