"""A deliberately naive restatement of COCO segm AP (computeIoU / evaluateImg / accumulate / summarize for iouType "segm", useCats,
maxDets 100): a mask is the Python set of its pixels, built by a loop over every pixel; an intersection is a set intersection; every
float is a Python float, one IEEE operation at a time.  Written from the description of the protocol; it shares no code with focoos_amd/
and is the checker of InstanceSegmentationEvaluator, fx_coco_mask_inter and fx_coco_match_segm.

Input: ``images`` = list of {"image_id": int, "dets": [{"mask": 2-D 0/1 rows, "score": s, "category_id": c}, ...], "gts": [{"mask": 2-D 0/1
rows, "category_id": c, optional "iscrowd" / "area" / "ignore"}, ...]}; images whose ``dets`` is empty are dropped with their ground truth.
A detection with an empty mask is a detection of area 0.  The tail of the protocol (thresholds, area ranges, summarize) is the bbox
restatement's, imported from tests/cocoeval_ref.py."""
import numpy as np

from tests.cocoeval_ref import MAX_DETS, _stable_desc, area_ranges, iou_thresholds, recall_thresholds, summarize


def pixels(mask):
    s = set()
    for y, row in enumerate(mask):
        for x, v in enumerate(row):
            if v:
                s.add((y, x))
    return s


def mask_iou(d, g, crowd):
    """maskApi rleIou: d, g pixel sets"""
    inter = len(d & g)
    if inter == 0:
        return 0.0
    u = len(d) if crowd else len(d) + len(g) - inter
    return float(inter) / float(u)


def match_image_category(dets, gts):
    """dets / gts of ONE category in ONE image (dataset order), each with "px" (pixel set).  Returns {"order", "matched" [a][t][d],
    "ignored" [a][t][d], "npig" [a], "inter" [d][g] (in ``order``)}."""
    order = _stable_desc([float(d["score"]) for d in dets])[:MAX_DETS]
    dpx = [dets[i]["px"] for i in order]
    G = []
    for g in gts:
        crowd = bool(g.get("iscrowd", 0))
        area = float(g["area"]) if "area" in g else float(len(g["px"]))
        G.append((g["px"], crowd, area, crowd or bool(g.get("ignore", 0))))
    ious = [[mask_iou(d, g[0], g[1]) for g in G] for d in dpx]
    res = {"order": order, "matched": [], "ignored": [], "npig": []}
    for lo, hi in area_ranges():
        gig = [g[3] or g[2] < lo or g[2] > hi for g in G]
        gorder = [i for i in range(len(G)) if not gig[i]] + [i for i in range(len(G)) if gig[i]]
        res["npig"].append(sum(1 for v in gig if not v))
        m_a, i_a = [], []
        for t in iou_thresholds():
            taken = [False] * len(G)
            m_t, i_t = [], []
            for di in range(len(dpx)):
                best = min(t, 1 - 1e-10)
                m = -1
                for gi in gorder:
                    if taken[gi] and not G[gi][1]:
                        continue
                    if m > -1 and not gig[m] and gig[gi]:
                        break
                    if ious[di][gi] < best:
                        continue
                    best = ious[di][gi]
                    m = gi
                if m == -1:
                    da = float(len(dpx[di]))
                    m_t.append(False)
                    i_t.append(da < lo or da > hi)
                else:
                    taken[m] = True
                    m_t.append(True)
                    i_t.append(bool(gig[m]))
            m_a.append(m_t)
            i_a.append(i_t)
        res["matched"].append(m_a)
        res["ignored"].append(i_a)
    return res


def with_pixels(images):
    out = []
    for im in images:
        out.append({"image_id": im["image_id"], "dets": [dict(d, px=pixels(d["mask"])) for d in im["dets"]],
                    "gts": [dict(g, px=pixels(g["mask"])) for g in im["gts"]]})
    return out


def evaluate_images(images, K):
    """{(image_id, category): match_image_category result} over the images that have at least one detection (``images`` of with_pixels)"""
    out = {}
    for im in images:
        if len(im["dets"]) == 0:
            continue
        for c in range(K):
            d = [x for x in im["dets"] if x["category_id"] == c]
            g = [x for x in im["gts"] if x["category_id"] == c]
            if d or g:
                out[(im["image_id"], c)] = match_image_category(d, g)
    return out


def accumulate(images, K):
    """precision[t][r][k][a], -1 where nothing can be computed"""
    ev = evaluate_images(images, K)
    ids = sorted(im["image_id"] for im in images if len(im["dets"]))
    dets_of = {im["image_id"]: im["dets"] for im in images}
    thr, rec, areas = iou_thresholds(), recall_thresholds(), area_ranges()
    P = [[[[-1.0 for _ in areas] for _ in range(K)] for _ in rec] for _ in thr]
    for k in range(K):
        for a in range(len(areas)):
            E = [(i, ev[(i, k)]) for i in ids if (i, k) in ev]
            if not E:
                continue
            npig = sum(e["npig"][a] for _, e in E)
            if npig == 0:
                continue
            scores = []
            for i, e in E:
                dk = [x for x in dets_of[i] if x["category_id"] == k]
                scores += [float(dk[j]["score"]) for j in e["order"]]
            order = _stable_desc(scores)
            for t in range(len(thr)):
                m, ig = [], []
                for _, e in E:
                    m += e["matched"][a][t]
                    ig += e["ignored"][a][t]
                tp = fp = 0
                rc, pr = [], []
                for j in order:
                    if not ig[j]:
                        if m[j]:
                            tp += 1
                        else:
                            fp += 1
                    rc.append(float(tp) / npig)
                    pr.append(float(tp) / (float(fp) + float(tp) + float(np.spacing(1))))
                for j in range(len(pr) - 1, 0, -1):
                    if pr[j] > pr[j - 1]:
                        pr[j - 1] = pr[j]
                j = 0
                for r, rt in enumerate(rec):
                    while j < len(rc) and rc[j] < rt:
                        j += 1
                    P[t][r][k][a] = pr[j] if j < len(pr) else 0.0
    return P


def evaluate(images, class_names):
    if not any(len(im["dets"]) for im in images):
        return {}
    return {"segm": summarize(accumulate(with_pixels(images), len(class_names)), class_names)}
