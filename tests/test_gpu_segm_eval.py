"""COCO segm AP on the MI355X: fx_mf_eval_masks (csrc/coco_segm_eval.hip) against the torch path (eval_postprocess + instance_inference on
the device) bit for bit and against an fp64 restatement of the sampling, fx_coco_mask_inter against numpy, fx_coco_match_segm against the
naive restatement tests/cocoeval_segm_ref.py with zero exceptions (LDS and workspace paths), the refusals, and
FocoosModel.eval_instance_segmentation end to end.  Gates: DESIGN.md section 13; measured values are printed (``MEASURED``)."""
import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

from focoos_amd import _lib
from focoos_amd import detection_eval as D
from focoos_amd import segm_eval as G
from focoos_amd.ports import DetectionDatasetEntry, MaskFormerModelOutput, TrainerArgs
from focoos_amd.processor import MaskFormerProcessor
from focoos_amd.synth import synth_image_structured
from tests import cocoeval_segm_ref as R
from tests import segm_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = time.perf_counter()


def _torch_path(lo, probs, Hin, Win, sizes, T, K):
    """eval_postprocess + instance_inference on the device from fx_mf_upsample_probs_f32's output; per image (Instances, top-k flat indices)"""
    lib = _lib.load("bf16")
    B, Q, h, w = lo.shape
    up = torch.empty(B, Q, Hin, Win, device=DEV)
    _lib.check(lib.fx_mf_upsample_probs_f32(lo.data_ptr(), h, w, up.data_ptr(), Hin, Win, B * Q, torch.cuda.current_stream().cuda_stream))
    proc = MaskFormerProcessor({"num_classes": K, "top_k": T, "mask_threshold": S.MASK_THRESHOLD, "postprocessing_type": "instance"})
    ents = [DetectionDatasetEntry(image=torch.zeros(3, Hin, Win, dtype=torch.uint8), height=H, width=W) for H, W in sizes]
    res = proc.eval_postprocess(MaskFormerModelOutput(logits=probs, masks=up, loss=None), ents)
    idx = [probs[i].flatten(0, 1).topk(T, sorted=False)[1].cpu().numpy() for i in range(B)]      # instance_inference's own call, repeated
    return [r["instances"] for r in res], idx


score_bound = S.score_bound      # the derivation is in tests/segm_scenes.py (scripts/bench_eval_instseg.py uses the same bound)


@pytest.mark.parametrize("name", ["b1", "b5"])
def test_eval_masks_vs_torch_path_and_fp64(name):
    h, w, Hin, Win, sizes = S.SAMPLING_CASES[name]
    Q, K, T = 100, 7, 100
    lo, probs = S.sampling_inputs(name, Q, K)
    lo_d, probs_d = lo.to(DEV), probs.to(DEV)
    B = len(sizes)
    dm = G.eval_masks(lo_d, probs_d, Hin, Win, sizes, T, S.MASK_THRESHOLD)
    dm2 = G.eval_masks(lo_d[:1].contiguous(), probs_d[:1].contiguous(), Hin, Win, sizes[:1], T, S.MASK_THRESHOLD)   # image 0 alone
    torch.cuda.synchronize()
    insts, tidx = _torch_path(lo_d, probs_d, Hin, Win, sizes, T, K)
    idx, label, query = dm.idx.cpu().numpy(), dm.label.cpu().numpy(), dm.query.cpu().numpy()
    score, count, box, psum = dm.score.cpu().numpy(), dm.count.cpu().numpy(), dm.box.cpu().numpy(), dm.psum.cpu().numpy()
    assert torch.equal(dm.score[0], dm2.score[0]) and torch.equal(dm.psum[0], dm2.psum[0]), "scores depend on the batch composition"
    delta = S.sampling_delta(h, w, Hin, Win)
    bits_diff = near = total = wrong = 0
    max_err = max_rel_bound = max_torch = 0.0
    multi = empty = full = 0
    for b, (H, W) in enumerate(sizes):
        inst = insts[b]
        tm, tb = inst.masks.tensor.cpu().numpy(), inst.boxes.tensor.cpu().numpy()
        ts, tc = inst.scores.cpu().numpy(), inst.classes.cpu().numpy()
        pos = {int(v): j for j, v in enumerate(tidx[b])}
        assert sorted(pos) == sorted(int(v) for v in idx[b]), "the two top-k selections differ"
        assert np.array_equal(label[b], idx[b] % K) and np.array_equal(query[b], idx[b] // K)
        refq = sorted(set(query[b].tolist()))
        assert dm.qlist[b, : int(dm.nref[b])].cpu().tolist() == refq
        multi += int(len(refq) < T)
        m64 = S.sample_fp64(lo[b], Hin, Win, H, W).numpy()
        planes = {}
        for q in refq:
            words = dm.plane_words(b, q)
            planes[q] = MaskFormerProcessor.unpack_masks(words[None], H, W)[0]
            raw = np.unpackbits(words.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")
            assert not raw[:, W:].any(), "tail bits are not zero"
            clear = np.abs(m64[q] - S.MASK_THRESHOLD) > delta
            near += int((~clear).sum())
            total += H * W
            wrong += int(((planes[q] != (m64[q] > S.MASK_THRESHOLD)) & clear).sum())
        for j in range(T):
            q, k = int(query[b, j]), pos[int(idx[b, j])]
            bits_diff += int((planes[q] != tm[k]).sum())
            n = int(tm[k].sum())
            assert int(count[b, q]) == n and np.array_equal(box[b, q].astype(np.float32), tb[k]), (b, j)
            assert int(label[b, j]) == int(tc[k])
            empty += int(n == 0)
            full += int(n == H * W)
            exact = float(probs[b].flatten()[idx[b, j]].double()) * float(m64[q][planes[q]].sum()) / (n + 1e-3)
            bound = score_bound(float(probs[b].flatten()[idx[b, j]]), H, W, h, w, Hin, Win)
            err = abs(float(score[b, j]) - exact)
            max_err, max_rel_bound = max(max_err, err), max(max_rel_bound, err / bound)
            assert err <= bound, (b, j, err, bound)
            max_torch = max(max_torch, abs(float(score[b, j]) - float(ts[k])))
    share = near / total
    print(f"MEASURED eval_masks {name}: {bits_diff} mask bits differ from the torch path over {B * T} slots; fp64 gate: {wrong} wrong of "
          f"{total - near} clear pixels, {near} within delta = {delta:.3e} ({100 * share:.4f} %); score |dev - fp64| max {max_err:.3e} "
          f"({max_rel_bound:.3f} of its bound), |dev - torch fp32| max {max_torch:.3e}; {empty} empty and {full} full masks among the slots")
    assert bits_diff == 0 and wrong == 0
    assert share <= 1e-3
    assert multi >= 1 and empty >= 1 and full >= 1
    assert max_torch <= 2 * max(score_bound(1.0, H, W, h, w, Hin, Win) for H, W in sizes)   # both are within the bound of the fp64 value


# ---------------------------------------------------------------------------------------------------------------- inter + match
def _device_scene(scene):
    """a scene as the kernels' inputs: every detection its own query, masks packed on the host; padding slots carry label -1"""
    ims = scene["images"]
    B, T = len(ims), max(len(im["cls"]) for im in ims)
    Q = T
    assert Q <= 128
    sizes_host = np.array([[im["height"], im["width"]] for im in ims], np.int32)
    word_off = G._word_offsets(sizes_host, [Q] * B)
    words = np.zeros(int(word_off[-1]) * 8, np.uint8)
    label, score = np.full((B, T), -1, np.int32), np.zeros((B, T), np.float32)
    query = np.tile(np.arange(T, dtype=np.int32), (B, 1))
    count, box = np.zeros((B, Q), np.int32), np.zeros((B, Q, 4), np.int32)
    qlist, nref = np.tile(np.arange(Q, dtype=np.int32), (B, 1)), np.zeros(B, np.int32)
    for b, im in enumerate(ims):
        n = len(im["cls"])
        p = D.pack_rows(im["masks"])
        words[int(word_off[b]) * 8: int(word_off[b]) * 8 + p.size] = p.reshape(-1)
        label[b, :n], score[b, :n], nref[b] = im["cls"], im["score"], n
        count[b, :n], box[b, :n] = D.popcount(p), G._tight_boxes(im["masks"])
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    dm = G.DeviceMasks(B=B, Q=Q, T=T, sizes_host=sizes_host, word_off_host=word_off, n_words=int(word_off[-1]), sizes=t(sizes_host),
                       word_off=t(word_off), words=t(words.view(np.int64)), qlist=t(qlist), nref=t(nref), count=t(count), box=t(box),
                       label=t(label), score=t(score), query=t(query))
    gts = [D.ground_truth_masks(DetectionDatasetEntry(height=im["height"], width=im["width"], annotations=S.annotations(im))) for im in ims]
    return dm, gts


def _check_scene(scene, tag, expect_ws=None):
    K = len(scene["class_names"])
    dm, gts = _device_scene(scene)
    B, T, Q = dm.B, dm.T, dm.Q
    npig = torch.zeros(K, 4, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    inter, gcount, offs, off_d, n_gt = G.device_mask_inter(dm, gts)
    rank, matched, ignored = G.device_match_segm(dm.label, dm.score, dm.query, dm.count, inter, gcount, offs, off_d, gts, K, npig, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    pairs = 0
    if n_gt:                                     # every pair against numpy
        it, gc = inter.cpu().numpy(), gcount.cpu().numpy()
        for b, im in enumerate(scene["images"]):
            gm = gts[b][0]
            Gb, n = len(gm), len(im["cls"])
            if Gb == 0:
                continue
            assert np.array_equal(gc[offs[b]: offs[b + 1]], gm.reshape(Gb, -1).sum(1)), tag
            want = (im["masks"][:, None] & gm[None]).reshape(n, Gb, -1).sum(2)
            got = it[Q * offs[b]: Q * offs[b] + Q * Gb].reshape(Q, Gb)[:n]
            assert np.array_equal(got, want), f"{tag}: intersections of image {b} differ"
            pairs += n * Gb
    rank, matched, ignored = rank.cpu().numpy(), matched.cpu().numpy().view(np.uint64), ignored.cpu().numpy().view(np.uint64)
    ref = R.evaluate_images(R.with_pixels(S.ref_images(scene)), K)
    want_rank = np.full(rank.shape, -1, np.int32)
    want_m, want_i = np.zeros(rank.shape, np.uint64), np.zeros(rank.shape, np.uint64)
    want_npig = np.zeros((K, 4), np.int64)
    for (img, c), e in ref.items():
        b = [im["image_id"] for im in scene["images"]].index(img)
        slots = np.flatnonzero(scene["images"][b]["cls"] == c)
        for a in range(4):
            want_npig[c, a] += e["npig"][a]
        for r, j in enumerate(e["order"]):
            s = slots[j]
            want_rank[b, s] = r
            for a in range(4):
                for t in range(10):
                    want_m[b, s] |= np.uint64(int(e["matched"][a][t][r]) << (10 * a + t))
                    want_i[b, s] |= np.uint64(int(e["ignored"][a][t][r]) << (10 * a + t))
    bad = int((rank != want_rank).sum()) + int((matched != want_m).sum()) + int((ignored != want_i).sum())
    assert bad == 0, f"{tag}: {bad} rank / matched / ignored words differ"
    assert np.array_equal(npig.cpu().numpy(), want_npig), tag
    max_gt = max([0] + [int(np.unique(g[1], return_counts=True)[1].max()) for g in gts if len(g[1])])
    used_ws = int(_lib.load("bf16").fx_coco_match_workspace_bytes(max_gt)) > 0
    assert expect_ws is None or used_ws == expect_ws, (tag, max_gt)
    G.device_match_segm(dm.label, dm.score, dm.query, dm.count, inter, gcount, offs, off_d, gts, K, npig, status)      # a second call accumulates
    torch.cuda.synchronize()
    assert np.array_equal(npig.cpu().numpy(), 2 * want_npig) and int(status.item()) == 0
    return int((want_rank >= 0).sum()), int(want_npig.sum()), pairs, used_ws


def test_inter_and_match_kernels_equal_restatement_on_random_scenes():
    scored = gt = pairs = 0
    for seed in range(200):
        s, g, p, _ = _check_scene(S.make_scene(seed), f"scene {seed}")
        scored, gt, pairs = scored + s, gt + g, pairs + p
    print(f"MEASURED segm kernels, 200 random scenes: {pairs} intersections equal numpy, {scored} scored detections x 40 decisions, {gt} "
          "non-ignored gt counts, 0 differences")


def test_inter_and_match_kernels_on_hand_derived_cases():
    with open(os.path.join(os.path.dirname(__file__), "golden", "coco_segm_cases.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        _check_scene(S.golden_scene(c), c["name"], expect_ws=False)
    print(f"MEASURED segm kernels, {len(cases)} hand-derived cases: 0 differences")


def test_workspace_path_one_pixel_gt_and_last_column():
    big = S.make_scene(1000, n_images=1, n_classes=1, max_gt=10, max_det=40, canvas=(50, 130))
    rs = np.random.RandomState(5)
    im = big["images"][0]
    im["masks"] = np.stack([S._shape(rs, 50, 130) for _ in range(110)])          # 110 detections of one class: the cut to 100 is live
    im["cls"], im["score"] = np.zeros(110, np.int64), (rs.randint(1, 64, size=110) / 64.0).astype(np.float32)
    im["gts"] = [{"mask": im["masks"][int(rs.randint(110))] if i % 3 == 0 else S._shape(rs, 50, 130), "category_id": 0,
                  "iscrowd": int(rs.rand() < 0.1)} for i in range(60)]
    s, g, p, _ = _check_scene(big, "G = 60, D = 110", expect_ws=True)
    print(f"MEASURED segm kernels, workspace path: G = 60, {s} scored detections, {g} non-ignored gt counts, {p} intersections, 0 differences")
    edge = S.make_scene(1001, n_images=2, n_classes=2, max_gt=4, max_det=12)
    for im in edge["images"]:
        H, W = im["height"], im["width"]
        one, col = np.zeros((H, W), bool), np.zeros((H, W), bool)
        one[H - 1, W - 1] = True                 # a gt of one pixel, in the last column of the last row
        col[:, W - 1] = True                     # a mask that is the last column
        im["gts"] += [{"mask": one, "category_id": 0, "iscrowd": 0}, {"mask": col, "category_id": 1, "iscrowd": 0}]
        im["masks"] = np.concatenate([im["masks"], col[None], one[None]])
        im["cls"], im["score"] = np.concatenate([im["cls"], [1, 0]]), np.concatenate([im["score"], np.float32([0.5, 0.25])])
    _, _, p, _ = _check_scene(edge, "one-pixel gt / last column", expect_ws=False)
    assert p > 0


def test_invalid_arguments_leave_outputs_untouched():
    lib = _lib.load("bf16")
    B, Q, K, T, h, w, Hin, Win = 2, 4, 3, 8, 4, 4, 16, 16
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda *sh: torch.full(sh, -7, dtype=torch.int32, device=DEV)   # noqa: E731
    f32 = lambda *sh: torch.full(sh, -7.0, dtype=torch.float32, device=DEV)   # noqa: E731
    lo, val, idx = torch.rand(B, Q, h, w, device=DEV), torch.rand(B, T, device=DEV), torch.zeros(B, T, dtype=torch.int32, device=DEV)
    sizes_h = np.array([[20, 70], [9, 33]], np.int32)
    woff_h = G._word_offsets(sizes_h, [Q] * B)
    nw = int(woff_h[-1])
    sizes, woff = torch.from_numpy(sizes_h).to(DEV), torch.from_numpy(woff_h).to(DEV)
    words = torch.full((nw,), -7, dtype=torch.int64, device=DEV)
    qlist, nref, count, box, psum = i32(B, Q), i32(B), i32(B, Q), i32(B, Q, 4), f32(B, Q)
    label, query, score = i32(B, T), i32(B, T), f32(B, T)
    need = int(lib.fx_mf_eval_masks_workspace_bytes(B, Q, 20))
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=DEV)

    def masks(lo_p=lo.data_ptr(), Qx=Q, Kx=K, Tx=T, sizes_host=sizes_h, woff_host=woff_h, nwx=nw, words_p=words.data_ptr(), ws_n=need,
              count_p=count.data_ptr(), ws_p=ws.data_ptr()):
        return lib.fx_mf_eval_masks(lo_p, val.data_ptr(), idx.data_ptr(), B, Qx, Kx, Tx, h, w, Hin, Win, sizes.data_ptr(), sizes_host.ctypes.data,
                                    woff.data_ptr(), woff_host.ctypes.data, nwx, 0.5, words_p, qlist.data_ptr(), nref.data_ptr(), count_p,
                                    box.data_ptr(), psum.data_ptr(), label.data_ptr(), query.data_ptr(), score.data_ptr(), ws_p, ws_n, s)

    bad_off = woff_h.copy()
    bad_off[1] -= 1                              # image 0's span is one word short
    rcs = [masks(lo_p=None), masks(lo_p=lo.data_ptr() + 2), masks(Qx=129), masks(Qx=0), masks(Kx=0), masks(Kx=-1), masks(Tx=0),
           masks(sizes_host=np.array([[20, 70], [0, 33]], np.int32)), masks(woff_host=bad_off), masks(woff_host=-woff_h - 1), masks(nwx=nw - 1),
           masks(words_p=None), masks(words_p=words.data_ptr() + 4), masks(ws_n=need - 1), masks(ws_p=None), masks(count_p=count.data_ptr() + 2)]
    # intersections and matching
    gt_h = np.array([0, 2, 3], np.int64)
    gwoff_h = G._word_offsets(sizes_h, [2, 1])
    gwords = torch.zeros(int(gwoff_h[-1]), dtype=torch.int64, device=DEV)
    gbox, gt_d, gwoff = torch.zeros(3, 4, dtype=torch.int32, device=DEV), torch.from_numpy(gt_h).to(DEV), torch.from_numpy(gwoff_h).to(DEV)
    inter, gcount = i32(Q * 3), i32(3)
    dwords = torch.zeros(nw, dtype=torch.int64, device=DEV)
    ok_q, ok_n, ok_box = torch.zeros(B, Q, dtype=torch.int32, device=DEV), torch.ones(B, dtype=torch.int32, device=DEV), torch.zeros(B, Q, 4, dtype=torch.int32, device=DEV)

    def inter_call(Qx=Q, gt_host=gt_h, gwoff_host=gwoff_h, ngw=int(gwoff_h[-1]), n_gt=3, inter_p=inter.data_ptr(), gw_p=gwords.data_ptr(),
                   woff_host=woff_h):
        return lib.fx_coco_mask_inter(dwords.data_ptr(), woff.data_ptr(), woff_host.ctypes.data, nw, ok_q.data_ptr(), ok_n.data_ptr(),
                                      ok_box.data_ptr(), B, Qx, T, sizes.data_ptr(), sizes_h.ctypes.data, gw_p, gwoff.data_ptr(),
                                      gwoff_host.ctypes.data, ngw, gbox.data_ptr(), gt_d.data_ptr(), gt_host.ctypes.data, n_gt, inter_p,
                                      gcount.data_ptr(), s)

    bad_g = gwoff_h.copy()
    bad_g[2] -= 1
    rcs += [inter_call(Qx=129), inter_call(gt_host=np.array([0, 3, 2], np.int64)), inter_call(gt_host=np.array([0, 2, 4], np.int64)),
            inter_call(gwoff_host=bad_g), inter_call(ngw=int(gwoff_h[-1]) - 1), inter_call(n_gt=-1), inter_call(inter_p=None),
            inter_call(gw_p=gwords.data_ptr() + 4), inter_call(woff_host=bad_off)]
    gcat, gflag, garea = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV), torch.ones(3, dtype=torch.float64, device=DEV)
    rank, m, ig = i32(B, T), torch.full((B, T), -7, dtype=torch.int64, device=DEV), torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    npig, status = torch.full((K, 4), -7, dtype=torch.int64, device=DEV), i32(1)
    ok_l, ok_s, ok_c, ok_i = torch.zeros(B, T, dtype=torch.int32, device=DEV), torch.rand(B, T, device=DEV), torch.zeros(B, Q, dtype=torch.int32, device=DEV), torch.zeros(Q * 3, dtype=torch.int32, device=DEV)
    big_ws = torch.zeros(max(16, int(lib.fx_coco_match_workspace_bytes(700))), dtype=torch.uint8, device=DEV)

    def match(label_p=ok_l.data_ptr(), Qx=Q, Kx=K, Tx=T, gt_host=gt_h, n_gt=3, max_gt=2, query_p=ok_l.data_ptr(), inter_p=ok_i.data_ptr(),
              rank_p=rank.data_ptr(), ws_p=None, ws_n=0):
        return lib.fx_coco_match_segm(label_p, ok_s.data_ptr(), query_p, ok_c.data_ptr(), B, Tx, Kx, Qx, inter_p, gcount.data_ptr(), gcat.data_ptr(),
                                      gflag.data_ptr(), garea.data_ptr(), gt_d.data_ptr(), gt_host.ctypes.data, n_gt, max_gt, rank_p, m.data_ptr(),
                                      ig.data_ptr(), npig.data_ptr(), status.data_ptr(), ws_p, ws_n, s)

    rcs += [match(label_p=None), match(Qx=129), match(Qx=0), match(Kx=0), match(Tx=0), match(gt_host=np.array([0, 3, 2], np.int64)), match(n_gt=-1),
            match(max_gt=-1), match(query_p=None), match(inter_p=None), match(rank_p=rank.data_ptr() + 2), match(max_gt=700),
            match(max_gt=700, ws_p=big_ws.data_ptr(), ws_n=big_ws.numel() - 1)]
    assert all(rc == -1 for rc in rcs), rcs
    torch.cuda.synchronize()
    for t in (words, qlist, nref, count, box, label, query, inter, gcount, rank, m, ig, npig, status):
        assert bool((t == -7).all())
    assert bool((psum == -7.0).all()) and bool((score == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- end to end
def _instseg_data(fm, n=12, size=512, seed=0):
    """n images at two original sizes; ground truth = the model's own 6 best non-empty masks per image (the torch path's), shifted by a
    seeded 1-3 px, one a crowd.  Returns (entries, per image the torch path's Instances and top-k flat indices)."""
    rs = np.random.RandomState(seed)
    data, torch_out = [], []
    for i in range(n):
        img = torch.from_numpy(synth_image_structured(700 + i, size, size)).permute(2, 0, 1).contiguous()
        H, W = ((384, 512), (333, 500))[i % 2]
        e = DetectionDatasetEntry(image=img, height=H, width=W, image_id=i)
        out = fm.model.forward(img.permute(1, 2, 0)[None].contiguous().to(DEV))
        inst = fm.processor.eval_postprocess(out, [e])[0]["instances"]
        tidx = out.logits[0].flatten(0, 1).topk(fm.processor.top_k, sorted=False)[1].cpu().numpy()
        masks, scores = inst.masks.tensor.cpu().numpy(), inst.scores.cpu().numpy()
        anns, used = [], set()
        for j in np.argsort(-scores, kind="mergesort"):
            q = int(tidx[j]) // fm.model.num_classes
            if q in used or not masks[j].any():
                continue
            used.add(q)
            m = np.roll(masks[j], int(rs.randint(1, 4)), axis=int(rs.randint(2)))
            anns.append({"segmentation": m.astype(np.uint8), "category_id": int(inst.classes[j]), "iscrowd": 0})
            if len(anns) == 6:
                break
        e.annotations = anns
        data.append(e)
        torch_out.append((masks, scores, inst.classes.cpu().numpy(), tidx))
    next(a for e in data for a in e.annotations)["iscrowd"] = 1
    return data, torch_out


def test_eval_instance_segmentation_end_to_end(tmp_path, flat_small_shapes):
    """Kernel routing is pinned (flat_small_shapes) as in test_gpu_detection_eval.py: with one routing an image is computed independently of
    its batch, and the evaluator's dicts must then be equal exactly."""
    from focoos_amd.model import ModelManager

    fm = ModelManager.get("fai-mf-m-coco-ins", device=DEV, seed=1)
    names = list(fm.model_info.classes)
    K, T = fm.model.num_classes, fm.processor.top_k
    data, torch_out = _instseg_data(fm)
    n_plans = len(fm.model.engine.plans)
    t = time.perf_counter()
    res4 = fm.eval_instance_segmentation(TrainerArgs(run_name="seg4", output_dir=str(tmp_path), batch_size=4), data)
    dt4 = time.perf_counter() - t
    res1 = fm.eval_instance_segmentation(TrainerArgs(run_name="seg1", output_dir=str(tmp_path), batch_size=1), data, save_json=False)
    assert len(fm.model.engine.plans) == n_plans
    mixed, alltorch = D.InstanceSegmentationEvaluator(names), D.InstanceSegmentationEvaluator(names)
    plans_before = set(fm.model.engine.plans.keys())
    cat_all, dev_all, torch_all, bound = [], [], [], 0.0
    for e, (masks, tscore, tcls, tidx) in zip(data, torch_out):
        x = e.image.permute(1, 2, 0)[None].contiguous().to(DEV)
        pl = fm.model.engine.forward(x, full_masks=False)
        dm = G.eval_masks(pl.mask_probs, pl.probs, x.shape[1], x.shape[2], [(e.height, e.width)], T, fm.processor.mask_threshold)
        idx, dscore, dlabel = dm.idx[0].cpu().numpy(), dm.score[0].cpu().numpy(), dm.label[0].cpu().numpy()
        pos = {int(v): j for j, v in enumerate(tidx)}
        order = np.array([pos[int(v)] for v in idx])             # the torch path's slots in the device path's slot order
        assert np.array_equal(tcls[order], dlabel)
        mixed.process([e], [{"masks": masks[order], "scores": dscore, "classes": dlabel}])
        alltorch.process([e], [{"masks": masks[order], "scores": tscore[order], "classes": dlabel}])
        cat_all.append(dlabel), dev_all.append(dscore), torch_all.append(tscore[order])
        # each score is within score_bound of the fp64 value, so the two differ by <= 2 bounds and a pair that changes order is <= 4 apart
        bound = max(bound, 4 * score_bound(1.0, e.height, e.width, pl.mask_probs.shape[-2], pl.mask_probs.shape[-1], x.shape[1], x.shape[2]))
    # The dicts depend on the scores only through each category's stable descending order over all the images (images ascending, slots in
    # order: accumulate()'s sort, and the per-image ranking is its restriction), so G.score_order_inversions sees every pair that can change
    # a decision, across images too: no inverted pair -> equal dicts; an inverted pair must be closer than the bound.
    swaps, worst = G.score_order_inversions(np.concatenate(cat_all), np.concatenate(dev_all), np.concatenate(torch_all))
    for k in [k for k in fm.model.engine.plans.keys() if k not in plans_before]:
        del fm.model.engine.plans[k]
    host, host_torch = mixed.evaluate(), alltorch.evaluate()
    ap = res4["segm"]["AP"]
    print(f"MEASURED eval_instance_segmentation end to end: {len(data)} images, {sum(len(e.annotations) for e in data)} gt masks, AP {ap}, "
          f"AP50 {res4['segm']['AP50']}, all-torch AP {host_torch['segm']['AP']}, {swaps} score-order swaps between the device and the torch "
          f"scores, batch 4 run {dt4:.2f} s")
    assert list(res4["segm"])[:6] == D.METRICS and len(res4["segm"]) == 6 + len(names)
    assert res4 == res1, "batch 4 and batch 1 disagree"
    assert res4 == host, "the device path and InstanceSegmentationEvaluator fed with the torch path's masks and the device scores disagree"
    assert worst <= bound, "two scores farther apart than the score bounds allow change order between the device and the torch path"
    if swaps == 0:              # only the scores differ between the two, and they order every category alike
        assert host_torch == res4, "the all-torch dict differs although no score pair changes order"
    assert ap is not None and 0.0 < ap < 100.0
    out = tmp_path / "seg4_eval"
    metrics = json.loads((out / "metrics.json").read_text())[0]
    info = json.loads((out / "model_info.json").read_text())
    assert list(metrics)[:6] == ["segm/" + m for m in D.METRICS] and metrics["segm/AP"] == ap and info["val_metrics"] == metrics
    assert not (tmp_path / "seg1_eval").exists()


def test_runtime_report():
    print(f"MEASURED test_gpu_segm_eval.py runtime so far {time.perf_counter() - T0:.1f} s")
