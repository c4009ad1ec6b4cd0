"""CPU: what oracle/metrics_oracle.py (the live reference of tests/test_gpu_eval_metrics_shapes.py) rests on, and the
conditions that the inputs of tests/metric_shape_cases.py are chosen for.

  * the restatement reproduces what the reference recorded in tests/golden/eval_metrics.json, for every case of
    tests/eval_cases.py, with the tolerances of the device test (0 for its EXACT keys, 1e-12 otherwise);
  * its curve agrees with scikit-learn where that is installed (AUPRC only with a positive: without one scikit-learn >= 1.3
    returns 0.0 where 1.0.1, the version the fixture's version_handling records, returns NaN);
  * its labelling agrees with a breadth-first search;
  * every case reaches the path it is named for, so that a device case cannot go soft silently."""
import json
import math
import os

import numpy as np
import pytest
import scipy.ndimage

import eval_cases as EC
import eval_oracle as EO
import metric_shape_cases as MC
import metrics_oracle as MO
from conftest import GOLD
from test_gpu_eval_metrics import close


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "eval_metrics.json")) as f:
        return json.load(f)


def postprocessed(kind, seed, cfg):
    """the [H, W, S] arrays of one eval_cases volume and its residual after eval_oracle's post-processing"""
    recon, orig, seg, mask = (t[0, 0].numpy() for t in EC.volume(kind, seed))
    diff = EO.residual(orig, recon)
    if cfg["erodeBrainmask"]:
        diff = EO.apply_brainmask_volume(diff, mask)
    if cfg["medianFiltering"]:
        diff = EO.apply_3d_median_filter(diff, cfg.get("kernelsize_median", 5))
    return recon, orig, seg, mask, np.ascontiguousarray(diff, np.float32)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_restatement_reproduces_the_golden_fixture(fixture, name):
    case, ref = EC.CASES[name], fixture["cases"][name]
    healthy = case["dataset"] == "IXI"
    node = "node" in case["dataset"].lower()
    masks = [np.unpackbits(np.frombuffer(bytes.fromhex(m), np.uint8))[:EC.H * EC.W * EC.S].reshape(EC.H, EC.W, EC.S).astype(bool)
             for m in ref["filtered_masks"]]
    threshold, checked, nmask = {}, 0, 0
    for (stage, vols), want in zip(case["phases"], ref["phases"]):
        assert want["stage"] == stage
        ed = want["eval_dict"]
        xs, ys = [], []
        for i, (kind, seed) in enumerate(vols):
            recon, orig, seg, mask, diff = postprocessed(kind, seed, case["cfg"])
            xs.append(diff.reshape(-1))
            ys.append(seg.reshape(-1) > 0)
            if healthy:
                continue
            got = MO.eval_volume(recon, orig, seg, mask, diff, voxel_metrics=True, component_filter=not node, row_curve=True,
                                 threshold=threshold["total"] if stage == "test" else None)
            p1s0, p1s1 = got["pred1_seg0"], got["pred1_seg1"]
            p0s1 = got["lesion"] - p1s1
            mine = {"AUCPerVol": got["auroc"], "AUPRCPerVol": got["auprc"], "BestDicePerVol": got["best_dice"],
                    "BestThresholdPerVol": got["threshold"],
                    # confusion_matrix(pred, seg).ravel() under the reference's names: TP = #(0, 0), FP = #(0, 1), TN = #(1, 0), FN = #(1, 1)
                    "TPPerVol": got["voxels"] - p1s0 - p1s1 - p0s1, "FPPerVol": p0s1, "TNPerVol": p1s0, "FNPerVol": p1s1}
            for key, g in mine.items():
                assert close(key, g, ed[key][i]), (name, stage, i, key, g, ed[key][i])
                checked += 1
            if not node:
                assert np.array_equal(got["pred"], masks[nmask]), (name, stage, i)
                nmask += 1
        if stage != "val":
            continue
        x, y = np.concatenate(xs), np.concatenate(ys)
        got = MO.eval_set(x, y, healthy)
        if healthy:
            for key in ("t_1p", "t_5p", "t_10p"):
                assert close(key, got[key], ed[key]), (name, key, got[key], ed[key])
                checked += 1
        else:
            threshold["total"] = got["best_threshold"]
            assert got["best_threshold"] == want["threshold"]["total"], (name, got["best_threshold"], want["threshold"])
            checked += 1
    assert nmask == len(masks) and checked >= (3 if healthy else 9)


# ---- against scikit-learn --------------------------------------------------------------------------------------------
def _scores(kind, n, rng):
    y = rng.random(n) < 0.1
    x = (rng.standard_normal(n) * 0.05 + 0.2 * y * rng.random(n)).astype(np.float32)
    if kind == "quantised":
        x = (np.round(64 * x) / 64).astype(np.float32)
    if kind == "constant":
        x = np.full(n, 0.5, np.float32)
    return x, y


@pytest.mark.filterwarnings("ignore:No positive samples")
@pytest.mark.parametrize("kind", ["continuous", "quantised", "constant"])
def test_curve_against_scikit_learn(kind):
    pytest.importorskip("sklearn")
    from sklearn.metrics import auc, average_precision_score, roc_curve
    rng = np.random.Generator(np.random.PCG64(17))
    for n in (300, 70001):
        x, y = _scores(kind, n, rng)
        thr, tps, fps = MO.distinct_curve(x, y)
        fpr, tpr, sk_thr = roc_curve(y.astype(int), x, pos_label=1)
        assert abs(MO.auroc(tps, fps) - auc(fpr, tpr)) <= 1e-12
        assert int(tps[-1]) > 0 and abs(MO.auprc(tps, fps) - average_precision_score(y.astype(int), x)) <= 1e-12
        # roc_curve retains the same points (it puts one more in front: fpr = tpr = 0, threshold inf)
        keep = MO.retained(tps, fps)
        assert np.array_equal(thr[keep], sk_thr[1:].astype(np.float32))
        # the healthy thresholds as _test_end reads them off roc_curve with all-zero labels
        hf, _, ht = roc_curve(np.zeros(n, int), x, pos_label=1)
        want = [float(ht[np.argmax(hf > p)]) for p in (0.01, 0.05, 0.10)]
        got = MO.eval_set(x, y, healthy=True)
        assert [got["t_1p"], got["t_5p"], got["t_10p"]] == want
        assert math.isnan(got["auroc"]) and math.isnan(got["auprc"])


def test_labelling_against_breadth_first_search():
    rng = np.random.Generator(np.random.PCG64(23))
    for shape, p in (((9, 8, 4), 0.2), ((1, 12, 11), 0.35), ((14, 5, 1), 0.3)):
        v = rng.random(shape) < p
        comps = MC.brute_force_components(v)
        lab, sizes = MO.component_sizes(v)
        assert sorted(sizes[1:].tolist()) == sorted(len(c) for c in comps)
        for c in comps:
            assert len({int(lab[q]) for q in c}) == 1
        want = np.zeros(shape, bool)
        for c in comps:
            if len(c) > 7:
                for q in c:
                    want[q] = True
        assert np.array_equal(MO.filter_small_components(v), want)


def test_restatement_edge_rules():
    # -0 and +0 are one score; a run of equal scores is one point
    thr, tps, fps = MO.distinct_curve(np.array([0.0, -0.0, 1.0, 1.0, -1.0], np.float32), [1, 0, 1, 0, 0])
    assert thr.tolist() == [1.0, 0.0, -1.0] and tps.tolist() == [1, 2, 2] and fps.tolist() == [1, 2, 3]
    assert MO.auroc(tps, fps) == (1 * 1 + 1 * 3 + 1 * 4) / (2 * 2 * 3)
    # bottom == top: the search runs over (0, 1); without a positive every dice is 0 / 0 or 0
    assert MO.find_best_val(np.zeros(5, np.float32), np.zeros(5)) == (0.0, 0.0)
    best, point = MO.find_best_val(np.zeros(5, np.float32), np.ones(5))
    assert best == 0.0 and 0.0 < point < 1.0
    one = MO.eval_set(np.full(4, 0.5, np.float32), np.ones(4, np.int8), healthy=False)
    assert math.isnan(one["auroc"]) and one["auprc"] == 1.0 and math.isnan(one["t_1p"])


# ---- the conditions the cases of metric_shape_cases.py are chosen for ------------------------------------------------
def test_shapes_reach_the_loop_edges():
    C = [s[1] * s[2] for s in MC.SMALL]
    assert min(C) < MC.EB and MC.EB in C and MC.EB + 1 in C
    assert any(s[0] == 1 for s in MC.SMALL) and any(s[2] == 1 for s in MC.SMALL) and any(s[0] > MC.EB for s in MC.SMALL)
    assert any(all(d % 2 == 1 for d in s[:2]) and s[0] * s[1] * s[2] % MC.EB for s in MC.SMALL)
    assert MC.CURVE_STRIDE < np.prod(MC.MID) < MC.GRID_STRIDE < np.prod(MC.BIG)
    assert MC.SET_SIZES[0] == MC.EB + 1 and MC.CURVE_STRIDE < MC.SET_SIZES[1] < MC.GRID_STRIDE < MC.SET_SIZES[2]
    # n goes up, down and up again through the one workspace
    n = [int(np.prod(s)) for s, _, _ in MC.SCORE_CASES]
    top = n.index(np.prod(MC.MID))
    assert n[0] < n[top] > n[top + 2] < n[-1] and n[-1] == max(n)
    for shape in MC.SMALL + [MC.MID]:
        for regime in MC.REGIMES if shape != MC.MID else ("continuous", "quantised"):
            assert sum(1 for c in MC.SCORE_CASES if c[:2] == (shape, regime)) == 1
    assert [c[:2] for c in MC.SCORE_CASES if c[0] == MC.BIG] == [(MC.BIG, "continuous")]


@pytest.mark.parametrize("shape", MC.SMALL + [MC.MID], ids=str)
def test_score_regimes_are_what_they_claim(shape):
    seeds = {(s, g): seed for s, g, seed in MC.SCORE_CASES}
    R = shape[0]
    for regime in MC.REGIMES:
        if (shape, regime) not in seeds:
            continue
        v = MC.volume(shape, regime, seeds[shape, regime])
        thr, tps, fps = MO.distinct_curve(v["diff"], v["seg"] > 0)
        P, N, M = int(tps[-1]), int(fps[-1]), thr.size
        rows_les = (v["seg"] > 0).reshape(R, -1).any(1)
        rows_mask = (v["mask"] > 0).reshape(R, -1).any(1)
        o = MO.eval_volume(**v)
        if regime == "continuous":
            assert P > 0 and N > 0 and M > 0.98 * v["diff"].size, (shape, M)
            assert 0.5 < o["auroc"] < 1.0 and 0.0 < o["best_dice"] < 1.0
            if shape == MC.MID:
                assert M > MC.CURVE_STRIDE, f"{M} distinct scores of {v['diff'].size}"
        if regime == "quantised":
            assert 10 <= M <= 100 and P > 0 and N > 0, (shape, M)
        if regime == "constant":
            assert M == 1 and thr[0] == 0.5 and o["auroc"] == 0.5
        if regime == "zero":
            assert M == 1 and o["max"] == 0.0 and not o["pred"].any()     # bottom == top: the search runs over (0, 1)
        if regime == "nolesion":
            assert P == 0 and all(math.isnan(o[k]) for k in ("auroc", "auprc", "l1_lesion"))
        if regime == "alllesion":
            assert N == 0 and math.isnan(o["auroc"]) and o["auprc"] == 1.0 and math.isnan(o["l1_healthy"])
        if regime == "rowmask" and R > 1:
            assert rows_mask.any() and (~rows_mask).any() and (rows_les & ~rows_mask).any()
        if regime == "nomask":
            assert not rows_mask.any() and math.isnan(o["score_vol"]) and not o["row_score"].any()
        if R == 1:
            assert math.isnan(o["row_auroc"])                             # a row curve over one item
        if R > 2 and regime in ("continuous", "quantised", "rowmask"):
            assert rows_les.any() and (~rows_les).any() and not math.isnan(o["row_auroc"])
        if R > MC.EB and regime == "rowmask":                             # the 300-point row curve: all three kinds of row beyond 256
            tail = slice(MC.EB, R)
            assert rows_les[tail].any() and (~rows_les[tail]).any() and (~rows_mask[tail]).any()
        if regime in ("continuous", "quantised"):                         # the filter has work to do on a natural threshold
            assert o["row_counts"][:, 0].sum() > 0


def test_the_large_volume_has_more_distinct_scores_than_one_grid_round():
    (seed,) = [seed for s, g, seed in MC.SCORE_CASES if s == MC.BIG]
    v = MC.volume(MC.BIG, "continuous", seed)
    thr, tps, fps = MO.distinct_curve(v["diff"], v["seg"] > 0)
    assert thr.size > MC.GRID_STRIDE, f"{thr.size} distinct scores of {v['diff'].size}"
    assert int(tps[-1]) > 0 and int(fps[-1]) > 0


def test_set_cases_are_what_they_claim():
    assert {g for n, g, _ in MC.SET_CASES if n == MC.SET_SIZES[0]} == set(MC.SET_REGIMES)
    assert [g for n, g, _ in MC.SET_CASES if n == MC.SET_SIZES[1]] == ["continuous", "quantised"]
    assert [g for n, g, _ in MC.SET_CASES if n == MC.SET_SIZES[2]] == ["continuous"]
    for n, regime, seed in MC.SET_CASES:
        x, y = MC.score_set(n, regime, seed)
        assert x.dtype == np.float32 and y.dtype == np.int8 and x.size == y.size == n
        thr, tps, fps = MO.distinct_curve(x, y)
        P, N, M = int(tps[-1]), int(fps[-1]), thr.size
        if regime == "continuous":
            assert P > 0 and N > 0
            if n == MC.SET_SIZES[1]:
                assert M > MC.CURVE_STRIDE, f"{M} distinct scores of {n}"
            if n == MC.SET_SIZES[2]:
                assert M > MC.GRID_STRIDE, f"{M} distinct scores of {n}"
        if regime in ("quantised", "signedzero"):
            assert 10 <= M <= 100 and P > 0 and N > 0
        if regime == "signedzero":
            z = x[x == 0]
            assert np.signbit(z).any() and (~np.signbit(z)).any() and thr.tolist().count(0.0) == 1
        if regime == "negative":
            assert (x < 0).any() and (x > 0).any() and P > 0 and N > 0
        if regime in ("constant", "zero"):
            assert M == 1
        assert (P == 0) == (regime == "nolesion") and (N == 0) == (regime == "alllesion")
        # healthy = 1 reads the labels as zero: N = n > 0 whatever they are
        h = MO.eval_set(x, y, healthy=True)
        assert not any(math.isnan(h[k]) for k in ("t_1p", "t_5p", "t_10p")) and h["t_1p"] >= h["t_5p"] >= h["t_10p"]


@pytest.mark.parametrize("name", [c for c in MC.COMPONENT_CASES if c != "dense_big"])
def test_component_cases_are_what_they_claim(name):
    v, thr = MC.component_case(name)
    pred = v["diff"] > np.float32(thr)
    lab, sizes = MO.component_sizes(pred)
    sizes = sizes[1:]
    kept = MO.filter_small_components(pred)
    if name in MC.SPARSE:
        n7, n8 = int((sizes == 7).sum()), int((sizes == 8).sum())
        assert n7 >= 1 and n8 >= 1, f"{name}: {n7} components of 7 voxels, {n8} of 8"
        assert 0 < kept.sum() < pred.sum(), f"{name}: {int(kept.sum())} of {int(pred.sum())} foreground voxels kept"
        assert 0.5 < 1 - kept.sum() / pred.sum() < 0.99
    if name == "dense_odd":
        assert sizes.max() > 0.95 * pred.sum() and (sizes <= 7).any() and 0.25 < pred.mean() < 0.35
    if name == "serpentine":
        fg, length = MC.serpentine()
        assert np.array_equal(fg, pred) and MC.EB < length <= 4096 and sizes.max() == length, length
        assert sorted(sizes.tolist()) == [1, 1, 1, 7, length] and kept.sum() == length
        # one voxel wide: no 2 x 2 x 2 block is full, and it runs both ways along a line's memory order
        full = fg[:-1, :-1, :-1] & fg[1:, :-1, :-1] & fg[:-1, 1:, :-1] & fg[:-1, :-1, 1:]
        assert not full.any()
    if name == "line_ends":
        fg, pairs, control = MC.line_end_pairs()
        D0, D1, D2 = fg.shape
        flat = lambda q: (q[0] * D1 + q[1]) * D2 + q[2]
        assert np.array_equal(fg, pred)
        assert flat(pairs[0][1]) - flat(pairs[0][0]) == 1 and flat(pairs[1][1]) - flat(pairs[1][0]) == D2
        assert pairs[0][0][2] == D2 - 1 and pairs[0][1][2] == 0 and pairs[1][0][1] == D1 - 1 and pairs[1][1][1] == 0
        for a, b in pairs:
            assert lab[a] != lab[b] and sizes[lab[a] - 1] == 4 and sizes[lab[b] - 1] == 4
        assert sorted(sizes.tolist()) == [4] * 8 + [8]
        assert kept.sum() == 8 and all(kept[q] for q in control)
    if name == "full":
        assert pred.all() and kept.all()
    if name == "empty":
        assert not pred.any()
    # the seg box makes both confusion counts informative wherever something is kept
    o = MO.eval_volume(**v, threshold=thr)
    assert np.array_equal(o["pred"], kept)
    assert o["pred1_seg0"] + o["pred1_seg1"] == kept.sum()
    if name in ("sparse_mid", "dense_odd", "serpentine", "full"):
        assert o["pred1_seg0"] > 0 and o["pred1_seg1"] > 0


def test_the_large_dense_case_has_one_component_across_the_grid_rounds():
    v, thr = MC.component_case("dense_big")
    pred = v["diff"] > np.float32(thr)
    lab, sizes = MO.component_sizes(pred)
    big = int(np.argmax(sizes[1:])) + 1
    idx = np.nonzero(lab.reshape(-1) == big)[0]
    assert sizes[big] > 0.95 * pred.sum() and (sizes[1:] <= 7).sum() > 50
    assert idx[0] < MC.EB * 64 and idx[-1] >= MC.GRID_STRIDE          # its voxels lie in the first and in the second round
    assert np.count_nonzero(pred.reshape(-1)[MC.GRID_STRIDE:]) > 1000
    # and components of 7, 8 and more voxels lie wholly in the second round, where only that round can count them
    first = scipy.ndimage.minimum(np.arange(lab.size).reshape(lab.shape), lab, index=np.arange(1, sizes.size))
    tail = sizes[1:][(first >= MC.GRID_STRIDE) & (np.arange(1, sizes.size) != big)]
    n7, n8, more = int((tail == 7).sum()), int((tail == 8).sum()), int((tail > 8).sum())
    assert n7 >= 1 and n8 >= 1 and more >= 1, f"second round: {n7} components of 7 voxels, {n8} of 8, {more} larger"
    assert MC.BIG[1] * MC.BIG[2] == np.prod(MC.BIG) - MC.GRID_STRIDE      # the last plane is exactly that round
