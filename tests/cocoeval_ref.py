"""A deliberately naive restatement of COCO bbox AP (computeIoU / evaluateImg / accumulate / summarize of the COCO evaluation protocol,
useCats, maxDets 100) in nested Python loops on Python floats (IEEE double, one operation at a time).  Written from the description of the
algorithm; it shares no code with focoos_amd/ and is the checker of focoos_amd/detection_eval.py and csrc/coco_eval.hip.

Input: ``images`` = list of {"image_id": int, "dets": [{"bbox": [x, y, w, h], "score": s, "category_id": c}, ...],
"gts": [{"bbox": [x, y, w, h], "category_id": c, optional "iscrowd" / "area" / "ignore"}, ...]}; images whose ``dets`` is empty are
dropped with their ground truth (the reference evaluator's behaviour)."""
import numpy as np

MAX_DETS = 100


def iou_thresholds():
    return [float(v) for v in np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)]


def recall_thresholds():
    return [float(v) for v in np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)]


def area_ranges():
    return [[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10]]


def bb_iou(d, g, crowd):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    da = d[2] * d[3]
    ga = g[2] * g[3]
    u = da if crowd else da + ga - i
    return i / u


def _stable_desc(scores):
    """indices by descending score, ties in input order (insertion into a list: no library sort)"""
    out = []
    for i, s in enumerate(scores):
        p = len(out)
        while p > 0 and scores[out[p - 1]] < s:
            p -= 1
        out.insert(p, i)
    return out


def _gt_fields(g):
    bb = [float(v) for v in g["bbox"]]
    crowd = bool(g.get("iscrowd", 0))
    area = float(g["area"]) if "area" in g else bb[2] * bb[3]
    ign = crowd or bool(g.get("ignore", 0))
    return bb, crowd, area, ign


def match_image_category(dets, gts):
    """dets / gts of ONE category in ONE image (dataset order).  Returns {"order": indices into dets by descending score (cut to 100),
    "matched": [a][t][d] bool, "ignored": [a][t][d] bool, "npig": [a] int}."""
    order = _stable_desc([float(d["score"]) for d in dets])[:MAX_DETS]
    dbox = [[float(v) for v in dets[i]["bbox"]] for i in order]
    G = [_gt_fields(g) for g in gts]
    ious = [[bb_iou(db, g[0], g[1]) for g in G] for db in dbox]
    res = {"order": order, "matched": [], "ignored": [], "npig": []}
    for lo, hi in area_ranges():
        gig = [g[3] or g[2] < lo or g[2] > hi for g in G]
        gorder = [i for i in range(len(G)) if not gig[i]] + [i for i in range(len(G)) if gig[i]]
        res["npig"].append(sum(1 for v in gig if not v))
        m_a, i_a = [], []
        for t in iou_thresholds():
            taken = [False] * len(G)
            m_t, i_t = [], []
            for di in range(len(dbox)):
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
                    da = dbox[di][2] * dbox[di][3]
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


def evaluate_images(images, K):
    """{(image_id, category): match_image_category result} for every pair that has a detection or a ground-truth box, over the images
    that have at least one detection."""
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
                    while j < len(rc) and rc[j] < rt:     # first index with rc >= rt (rc and rec both ascend: j never goes back)
                        j += 1
                    P[t][r][k][a] = pr[j] if j < len(pr) else 0.0
    return P


def _mean(vals):
    """mean of the values > -1 in the given order; numpy's own (pairwise) summation so that the last bit agrees with np.mean"""
    v = [x for x in vals if x > -1]
    return float(np.mean(np.array(v, dtype=np.float64))) if v else -1.0


def summarize(P, class_names):
    K = len(class_names)
    T, R = len(P), len(P[0])

    def ap(ts, a):
        return _mean([P[t][r][k][a] for t in ts for r in range(R) for k in range(K)])

    allt = list(range(T))
    stats = [ap(allt, 0), ap([0], 0), ap([5], 0), ap(allt, 1), ap(allt, 2), ap(allt, 3)]
    res = {}
    for name, s in zip(["AP", "AP50", "AP75", "APs", "APm", "APl"], stats):
        res[name] = s * 100 if s >= 0 else None
    if K > 1:
        for k, name in enumerate(class_names):
            s = _mean([P[t][r][k][0] for t in allt for r in range(R)])
            res["AP-" + name] = s * 100 if s >= 0 else None
    return res


def evaluate(images, class_names):
    if not any(len(im["dets"]) for im in images):
        return {}
    return {"bbox": summarize(accumulate(images, len(class_names)), class_names)}
