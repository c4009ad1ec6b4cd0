"""TEST INFRASTRUCTURE ONLY: a plain numpy / float64 statement of what cddpm_eval_volume and cddpm_eval_set promise
(include/cddpm.h, "evaluation metrics"; the kernels are csrc/eval_metrics.hip). It exists so that the device metrics can
be checked at any shape: tests/golden/eval_metrics.json was recorded from the reference at one geometry, and this file is
tied to that record by tests/test_metrics_oracle_host.py. numpy, scipy and the standard library only.

What is stated, with the line of the reference's src/utils/utils_eval.py it stands for:

    reconstruction errors  :36-41    fp32 per-voxel terms |e| and e * e, float64 means over all voxels, seg > 0, seg == 0
    curve                  sklearn's _binary_clf_curve: one point per distinct score, scores descending, -0 equal to +0
    AUROC                  :549-552  auc(roc_curve(...)): the trapezoids summed exactly in Python integers over 2 P N
    AUPRC                  :555-558  average_precision_score as scikit-learn 1.0.1 computes it: NaN without a positive
    find_best_val          :508-539  10 steps, float64 probe points (numpy 1.22), compared as float32
    healthy thresholds     :290-296  roc_curve(drop_intermediate = True), first retained point with fpr > p
    prediction             :96       diff > float32(threshold)
    component filter       :489-503  scipy.ndimage.label with the full 3 x 3 x 3 structure, components of <= 7 voxels go
    counts, row outputs    :102-178  on the filtered mask per volume, on the unfiltered one per row

Volumes are [R, D1, D2] float32 arrays; R is the axis the reference's "per-slice" loop walks.
Only tests/ may import this file.
"""
import math

import numpy as np
import scipy.ndimage

NAN = float("nan")
SMALL_COMPONENT = 7          # components of at most this many voxels are cleared


# ---- curve -----------------------------------------------------------------------------------------------------------
def distinct_curve(scores, labels):
    """(thresholds, tps, fps): one point per distinct score in descending order, tps / fps the numbers of positives /
    negatives with a score >= that threshold. thresholds float32, tps / fps int64."""
    x = np.asarray(scores, np.float32).reshape(-1) + np.float32(0.0)        # -0 + 0 = +0: the two zeros are one score
    y = (np.asarray(labels).reshape(-1) != 0).astype(np.int64)
    order = np.argsort(-x.astype(np.float64), kind="stable")                 # stable, descending
    xs, ys = x[order], y[order]
    ends = np.r_[np.nonzero(xs[1:] != xs[:-1])[0], xs.size - 1]              # where a run of equal scores ends
    tps = np.cumsum(ys)[ends]
    fps = ends + 1 - tps
    return xs[ends], tps, fps


def auroc(tps, fps):
    P, N = int(tps[-1]), int(fps[-1])
    if P <= 0 or N <= 0:
        return NAN
    t0, f0 = np.r_[0, tps[:-1]], np.r_[0, fps[:-1]]
    twice_area = sum(((fps - f0) * (tps + t0)).tolist())                     # each product < 2^63; the sum in Python ints
    return twice_area / (2 * P * N)                                          # int / int: correctly rounded


def auprc(tps, fps):
    P = int(tps[-1])
    if P <= 0:
        return NAN                                                           # scikit-learn 1.0.1: 0 / 0 recall
    t = tps.astype(np.float64)
    t0 = np.r_[0.0, t[:-1]]
    return math.fsum(((t - t0) * (t / (t + fps.astype(np.float64)))).tolist()) / P


def retained(tps, fps):
    """roc_curve's drop_intermediate: a point stays where the second difference of fps or of tps is non-zero; the first
    and the last always stay"""
    keep = np.ones(tps.size, bool)
    if tps.size > 2:
        keep[1:-1] = (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0)
    return keep


def fpr_thresholds(thresholds, tps, fps, bounds=(0.01, 0.05, 0.10)):
    """per bound p the threshold of the first retained point with fpr > p (fpr = fps / N in float64); needs N > 0"""
    N = int(fps[-1])
    if N <= 0:
        raise ValueError("fpr thresholds need a negative")
    keep = retained(tps, fps)
    thr, fpr = thresholds[keep], fps[keep].astype(np.float64) / float(N)
    return [float(thr[int(np.argmax(fpr > p))]) for p in bounds]


# ---- find_best_val ---------------------------------------------------------------------------------------------------
def dice_above(x, y, q):
    """dice of (x > float32(q)) against y: 2 |P n G| / (|P| + |G|), NaN for 0 / 0"""
    p = x > np.float32(q)
    den = int(np.count_nonzero(p)) + int(np.count_nonzero(y))
    return 2 * int(np.count_nonzero(p & y)) / den if den else NAN


def find_best_val(scores, labels, steps=10):
    """the greedy search over (0, max(x)): returns (best dice, its threshold). NaN compares false, as in numpy."""
    x = np.asarray(scores, np.float32).reshape(-1)
    y = np.asarray(labels).reshape(-1) != 0
    bottom, top = 0.0, float(x.max())
    best, point = 0.0, 0.0
    for _ in range(steps):
        if bottom == top:
            top = 1.0
        center = bottom + (top - bottom) * 0.5
        qb, qt = bottom + (top - bottom) * 0.25, bottom + (top - bottom) * 0.75
        vb, vt = dice_above(x, y, qb), dice_above(x, y, qt)
        if vb >= vt:
            if vb >= best:
                best, point = vb, qb
            top = center
        else:
            if vt >= best:
                best, point = vt, qt
            bottom = center
    return best, point


# ---- components ------------------------------------------------------------------------------------------------------
def component_sizes(pred):
    """(label volume, sizes with sizes[0] = background count) under 26-connectivity"""
    lab, _ = scipy.ndimage.label(pred, structure=np.ones((3, 3, 3)))
    return lab, np.bincount(lab.reshape(-1))


def filter_small_components(pred):
    lab, sizes = component_sizes(pred)
    small = sizes <= SMALL_COMPONENT
    small[0] = False
    return pred & ~small[lab]


# ---- the two entry points --------------------------------------------------------------------------------------------
def _mean(v):
    return float(np.sum(v, dtype=np.float64) / v.size) if v.size else NAN


def eval_volume(recon, orig, seg, mask, diff, *, voxel_metrics=True, component_filter=True, row_curve=True, threshold=None):
    """dict with the slots of the volume record by name (lower case, without the CDDPM_EVAL_ prefix) and the arrays
    row_score [R] float32, row_label [R] int32, row_counts [R, 3] int64 (#pred, #pred & seg, #seg; unfiltered), pred
    [R, D1, D2] bool (filtered). Slots that the flags leave out are NaN / absent."""
    recon, orig, seg, mask, diff = (np.ascontiguousarray(a, np.float32) for a in (recon, orig, seg, mask, diff))
    R = diff.shape[0]
    e = recon - orig                                                         # fp32, as torch computes the terms
    e1, e2 = np.abs(e), e * e
    les, hea, msk = seg > 0, seg == 0, mask > 0
    out = dict(l1_all=_mean(e1), l1_lesion=_mean(e1[les]), l1_healthy=_mean(e1[hea]),
               l2_all=_mean(e2), l2_lesion=_mean(e2[les]), l2_healthy=_mean(e2[hea]),
               score_vol=_mean(diff[msk]), lesion=int(np.count_nonzero(les)), voxels=int(diff.size))
    for k in ("auroc", "auprc", "best_dice", "best_threshold", "threshold", "max", "pred1_seg0", "pred1_seg1", "row_auroc", "row_auprc"):
        out[k] = NAN
    score = np.zeros(R, np.float32)
    for r in range(R):
        if msk[r].any():
            score[r] = np.float32(_mean(diff[r][msk[r]]))                    # 0 for a row without mask
    out["row_score"] = score
    out["row_label"] = les.reshape(R, -1).any(axis=1).astype(np.int32)
    if voxel_metrics:
        thr, tps, fps = distinct_curve(diff, les)
        out["auroc"], out["auprc"] = auroc(tps, fps), auprc(tps, fps)
        out["best_dice"], out["best_threshold"] = find_best_val(diff, les)
        out["threshold"] = float(threshold) if threshold is not None else out["best_threshold"]
        out["max"] = float(diff.max() + np.float32(0.0))
        pred = diff > np.float32(out["threshold"])
        flat, lf = pred.reshape(R, -1), les.reshape(R, -1)
        out["row_counts"] = np.stack([flat.sum(1), (flat & lf).sum(1), lf.sum(1)], axis=1).astype(np.int64)
        if component_filter:
            pred = filter_small_components(pred)
        out["pred"] = pred
        out["pred1_seg0"] = int(np.count_nonzero(pred & ~les))
        out["pred1_seg1"] = int(np.count_nonzero(pred & les))
    if row_curve:
        _, tps, fps = distinct_curve(out["row_score"], out["row_label"])
        out["row_auroc"], out["row_auprc"] = auroc(tps, fps), auprc(tps, fps)
    return out


def eval_set(x, y, healthy):
    """dict auroc, auprc, t_1p, t_5p, t_10p (NaN without a negative), best_dice, best_threshold, max. healthy: the
    labels are read as all zero."""
    x = np.asarray(x, np.float32).reshape(-1)
    y = np.zeros(x.size, bool) if healthy else np.asarray(y).reshape(-1) != 0
    thr, tps, fps = distinct_curve(x, y)
    t = fpr_thresholds(thr, tps, fps) if int(fps[-1]) > 0 else [NAN, NAN, NAN]
    best, point = find_best_val(x, y)
    return dict(auroc=auroc(tps, fps), auprc=auprc(tps, fps), t_1p=t[0], t_5p=t[1], t_10p=t[2], best_dice=best,
                best_threshold=point, max=float(x.max() + np.float32(0.0)))
