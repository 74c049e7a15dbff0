"""Seeded random instance-segmentation scenes shared by tests/test_segm_eval_cpu.py and tests/test_gpu_segm_eval.py, the converters between
the forms a scene is fed in (tests/cocoeval_segm_ref.py's dicts, InstanceSegmentationEvaluator.process's raw arrays, the kernels' packed
words) and the seeded inputs of the sampling tests.

A scene: 1-4 images on small canvases whose widths are not multiples of 64 (some below 64, some spanning three words), 1-4 classes, 0-10
ground-truth masks and 1-40 detections per image.  A mask is a union of rectangles and ellipses.  Most detections are derived from a
ground-truth mask - the mask itself, a shifted copy, or the left t-th of a plain rectangle whose width is a multiple of 20, which puts the
IoU exactly on a threshold - so ties and on-threshold IoUs are common; some are empty.  10 % of the ground truth is crowd, a fifth carries
an explicit ``area``; scores come from a 1/64 grid, so duplicates are common."""
import numpy as np

from focoos_amd.ports import DetectionDatasetEntry

CANVASES = [(24, 65), (40, 70), (33, 100), (50, 130), (31, 47), (20, 191)]


def _shape(rs, H, W):
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(int(rs.randint(1, 4))):
        cy, cx = rs.randint(0, H), rs.randint(0, W)
        ry, rx = rs.randint(2, max(3, H // 2)), rs.randint(2, max(3, W // 3))
        if rs.rand() < 0.5:
            m |= (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
        else:
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def _plain_rect(rs, H, W):
    w = 20 * int(rs.randint(1, max(2, W // 20)))
    h = int(rs.randint(2, H))
    x0, y0 = int(rs.randint(0, W - w + 1)), int(rs.randint(0, H - h + 1))
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m, (x0, y0, w, h)


def make_scene(seed, n_images=None, n_classes=None, max_gt=10, max_det=40, canvas=None):
    rs = np.random.RandomState(seed)
    K = int(rs.randint(1, 5)) if n_classes is None else n_classes
    images = []
    for i in range(int(rs.randint(1, 5)) if n_images is None else n_images):
        H, W = CANVASES[int(rs.randint(len(CANVASES)))] if canvas is None else canvas
        G, D = int(rs.randint(0, max_gt + 1)), int(rs.randint(1, max_det + 1))
        gts, rects = [], []
        for _ in range(G):
            if rs.rand() < 0.4:
                m, r = _plain_rect(rs, H, W)
            else:
                m, r = _shape(rs, H, W), None
            g = {"mask": m, "category_id": int(rs.randint(K)), "iscrowd": int(rs.rand() < 0.10)}
            if rs.rand() < 0.2:
                g["area"] = float(rs.choice([10.0, 500.0, 1024.0, 2000.0, 9216.0, 20000.0]))
            gts.append(g)
            rects.append(r)
        masks, cls = [], []
        for _ in range(D):
            u = rs.rand()
            if G and u < 0.7:
                s = int(rs.randint(G))
                m = gts[s]["mask"].copy()
                if rects[s] is not None and rs.rand() < 0.6:        # the left t-th of the rectangle: IoU = t exactly
                    x0, y0, w, h = rects[s]
                    t = rs.choice([0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 1.0])
                    m[:, x0 + int(round(w * t)):] = False
                elif rs.rand() < 0.5:
                    m = np.roll(m, int(rs.randint(-3, 4)), axis=int(rs.randint(2)))
                c = gts[s]["category_id"] if rs.rand() < 0.8 else int(rs.randint(K))
            elif u < 0.78:
                m, c = np.zeros((H, W), bool), int(rs.randint(K))   # an empty predicted mask
            else:
                m, c = _shape(rs, H, W), int(rs.randint(K))
            masks.append(m)
            cls.append(c)
        images.append({"image_id": i, "height": H, "width": W, "masks": np.stack(masks), "cls": np.array(cls, np.int64),
                       "score": (rs.randint(1, 64, size=D) / 64.0).astype(np.float32), "gts": gts})
    return {"class_names": [f"c{k}" for k in range(K)], "images": images}


def ref_images(scene):
    """tests/cocoeval_segm_ref.py's input"""
    out = []
    for im in scene["images"]:
        dets = [{"mask": im["masks"][j].astype(int).tolist(), "score": float(im["score"][j]), "category_id": int(im["cls"][j])}
                for j in range(len(im["cls"]))]
        gts = [dict(g, mask=np.asarray(g["mask"]).astype(int).tolist()) for g in im["gts"]]
        out.append({"image_id": im["image_id"], "dets": dets, "gts": gts})
    return out


def annotations(im, form="dense"):
    """the ground truth of a scene image as annotation dicts: ``segmentation`` dense (2-D array) or uncompressed RLE"""
    anns = []
    for g in im["gts"]:
        a = {k: v for k, v in g.items() if k != "mask"}
        m = np.asarray(g["mask"], bool)
        if form == "dense":
            a["segmentation"] = m.astype(np.uint8)
        else:
            flat = m.T.reshape(-1)                                  # column-major
            change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
            runs = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
            a["segmentation"] = {"size": [m.shape[0], m.shape[1]], "counts": ([0] if flat.size and flat[0] else []) + runs}
        anns.append(a)
    return anns


def entries_and_outputs(scene, form="dense"):
    """(inputs, outputs) of InstanceSegmentationEvaluator.process in the raw-array form"""
    inputs = []
    for im in scene["images"]:
        inputs.append(DetectionDatasetEntry(image_id=im["image_id"], height=im["height"], width=im["width"], annotations=annotations(im, form)))
    outputs = [{"masks": im["masks"].copy(), "scores": im["score"].copy(), "classes": im["cls"].copy()} for im in scene["images"]]
    return inputs, outputs


def _raster(rects, H, W):
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in rects:
        m[y0:y1, x0:x1] = True
    return m


def golden_scene(case):
    """a case of tests/golden/coco_segm_cases.json (masks as unions of [x0, y0, x1, y1) rectangles) in make_scene's form"""
    images = []
    for im in case["images"]:
        H, W = im["height"], im["width"]
        d = im["dets"]
        gts = [dict({k: v for k, v in g.items() if k != "rects"}, mask=_raster(g["rects"], H, W)) for g in im["gts"]]
        images.append({"image_id": im["image_id"], "height": H, "width": W,
                       "masks": np.stack([_raster(x["rects"], H, W) for x in d]) if d else np.zeros((0, H, W), bool),
                       "score": np.array([x["score"] for x in d], np.float32), "cls": np.array([x["category_id"] for x in d], np.int64),
                       "gts": gts})
    return {"class_names": list(case["class_names"]), "images": images}


# ---------------------------------------------------------------------------------------------------------------- sampling inputs
SAMPLING_CASES = {          # name -> (h, w, Hin, Win, original sizes)
    "b1": (16, 20, 64, 80, [(131, 173)]),
    "b5": (24, 32, 96, 128, [(131, 173), (41, 57), (77, 300), (64, 64), (97, 31)]),
}
MASK_THRESHOLD = 0.5


def sampling_inputs(name, Q=100, K=7):
    """(lo [B, Q, h, w] f32, probs [B, Q, K] f32) of a sampling case.  The mask probabilities are sigmoids of smooth, steep fields, as a
    trained mask head gives them: few pixels interpolate to a value near the threshold.  Planted in image 0: query 3 is selected for
    several classes, query 4 is all zeros (an empty mask that is selected), query 5 all ones."""
    import torch

    h, w, Hin, Win, sizes = SAMPLING_CASES[name]
    g = torch.Generator().manual_seed(len(sizes) * 101 + h)
    B = len(sizes)
    coarse = torch.randn(B, Q, max(2, h // 4), max(2, w // 4), generator=g)
    lo = torch.sigmoid(12.0 * torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)).float()
    probs = torch.softmax(torch.randn(B, Q, K, generator=g) * 3, -1).float()
    probs[0, 3, :3] = torch.tensor([0.99, 0.98, 0.97])
    lo[0, 4], probs[0, 4, 0] = 0.0, 0.96
    lo[0, 5], probs[0, 5, 1] = 1.0, 0.95
    return lo.contiguous(), probs.contiguous()


def sampling_delta(h, w, Hin, Win):
    """Bound on |fp32 two-stage sample - exact| for values in [0, 1].  u = 2^-24.  Per axis of a stage the source coordinate
    (dst + 0.5) * fl(in / out) - 0.5 carries three roundings of quantities <= in, so it is off by <= 3 u in; the interpolant is piecewise
    linear with slope <= 1 per source pixel (values in [0, 1]) and continuous across a changed floor, so the value moves by <= 3 u in.  A
    1-D lerp w0 a + w1 b rounds w0 = 1 - w1 and three operations on values <= 1: 4 u; two axes, two stages: 16 u.  Stage 2 is a convex
    combination of stage-1 values, so stage-1 errors are not amplified.  Total 3 u (h + w + Hin + Win) + 16 u; 4 u (...) + 16 u is used to
    cover the second-order terms."""
    u = 2.0 ** -24
    return 4 * u * (h + w + Hin + Win) + 16 * u


def score_bound(val, H, W, h, w, Hin, Win):
    """|device score - fp64 restatement| for one slot, the restatement being val64 * sum64(m64 over the device mask) / (n + 1e-3).
    S (fp32): every term passes through at most D additions - 6 levels of the lane tree, ceil(SG_ROWS ceil(W / 64) / 4) items of its
    wavefront, 3 for the four wavefronts, ceil(H / SG_ROWS) tile partials - so |S - sum m| <= D u sum m (first order; terms >= 0).  Each
    fp32 m differs from its fp64 value by <= delta (sampling_delta).  With sum m <= n: |S / (n + 1e-3) - exact| <= D u + delta, plus u for
    float(n) + 1e-3f and u for the division, both relative to a quotient <= 1.  The product with val adds u.  Everything x 1.01 for the
    second-order terms."""
    u = 2.0 ** -24
    ww = (W + 63) // 64
    depth = 6 + -(-8 * ww // 4) + 3 + -(-H // 8)
    return 1.01 * val * (depth * u + sampling_delta(h, w, Hin, Win) + 3 * u)


def sample_fp64(lo, Hin, Win, H, W):
    """the two bilinear resizes (align_corners=False) of lo [Q, h, w] in float64 on the CPU: [Q, H, W]"""
    import torch
    import torch.nn.functional as F

    up = F.interpolate(lo.double()[None], size=(Hin, Win), mode="bilinear", align_corners=False)
    return F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False)[0]
