"""GPU: the evaluation metric kernels (csrc/eval_metrics.hip through CddpmEngine.eval_volume / eval_set) against the live
reference oracle/metrics_oracle.py at the shapes, score regimes and foreground layouts of tests/metric_shape_cases.py: rows
shorter than, equal to and one longer than a block, more rows than a block, more distinct scores than one round of the
curve kernels, more voxels than one round of the grid-stride kernels, components that many blocks join at once.
tests/test_metrics_oracle_host.py ties the reference to the recorded results of tests/golden/eval_metrics.json and asserts
that each case reaches the path it is named for.

All cases go through one engine in file order, so that its workspace is grown and then reused at smaller sizes.
Tolerances are those of tests/test_gpu_eval_metrics.py: none for counts, masks, thresholds and the search's results, 1e-12
for the curve areas, 1e-9 + 1e-6 relative for the fp32 means."""
import functools

import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_oracle as EO
import metric_shape_cases as MC
import metrics_oracle as MO
from conftest import load_pkg
from test_gpu_eval_metrics import Recorder, close

pytestmark = pytest.mark.gpu

# slot of the volume record (include/cddpm.h) -> the reference's name; grouped by the tolerance() key that governs them
EXACT_SLOTS = {7: "lesion", 8: "voxels", 11: "best_dice", 12: "best_threshold", 13: "threshold", 14: "max", 15: "pred1_seg0",
               16: "pred1_seg1"}
AREA_SLOTS = {9: "auroc", 10: "auprc", 17: "row_auroc", 18: "row_auprc"}
MEAN_SLOTS = {0: "l1_all", 1: "l1_lesion", 2: "l1_healthy", 3: "l2_all", 4: "l2_lesion", 5: "l2_healthy", 6: "score_vol"}
SET_EXACT = {2: "t_1p", 3: "t_5p", 4: "t_10p", 5: "best_dice", 6: "best_threshold", 7: "max"}
SET_AREA = {0: "auroc", 1: "auprc"}
EXACT_KEY, AREA_KEY, MEAN_KEY = "TPPerVol", "AUCPerVol", "l1recoErrorAll"      # keys of tolerance() with those three rules


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


@functools.lru_cache(maxsize=None)
def score_reference(shape, regime, seed):
    return MO.eval_volume(**MC.volume(shape, regime, seed))


@functools.lru_cache(maxsize=None)
def component_reference(name):
    v, thr = MC.component_case(name)
    return MO.eval_volume(**v, threshold=thr)


@functools.lru_cache(maxsize=None)
def set_reference(n, regime, seed, healthy):
    return MO.eval_set(*MC.score_set(n, regime, seed), healthy)


def run_volume(eng, v, threshold=None):
    t = {k: torch.from_numpy(a).cuda() for k, a in v.items()}
    out = eng.eval_volume(t["recon"], t["orig"], t["seg"], t["mask"], t["diff"], voxel_metrics=True, component_filter=True,
                          row_curve=True, threshold=threshold)
    torch.cuda.synchronize()
    return out


def check_volume(tag, out, want):
    rec = out["record"].cpu().numpy()
    print(tag, {n: (float(rec[i]), want[n]) for i, n in {**EXACT_SLOTS, **AREA_SLOTS, **MEAN_SLOTS}.items()})
    assert np.array_equal(out["pred"].cpu().numpy().astype(bool), want["pred"]), (tag, "pred")
    assert np.array_equal(out["row_counts"].cpu().numpy(), want["row_counts"]), (tag, "row_counts")
    assert np.array_equal(out["row_label"].cpu().numpy(), want["row_label"]), (tag, "row_label")
    for key, slots in ((EXACT_KEY, EXACT_SLOTS), (AREA_KEY, AREA_SLOTS), (MEAN_KEY, MEAN_SLOTS)):
        for i, name in slots.items():
            assert close(key, rec[i], want[name]), (tag, name, float(rec[i]), want[name])
    score = out["row_score"].cpu().numpy()
    assert all(close("AnomalyScoreRecoPerSlice", g, w) for g, w in zip(score.tolist(), want["row_score"].tolist())), (tag, "row_score")


def bitwise_equal(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in ("record", "row_score", "row_label", "row_counts", "pred"))


@pytest.mark.parametrize("shape,regime,seed", MC.SCORE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_volume_scores(eng, shape, regime, seed):
    """every score regime at every small shape, 81 920 voxels (continuous and quantised) between them, 1 064 960 last"""
    check_volume((shape, regime), run_volume(eng, MC.volume(shape, regime, seed)), score_reference(shape, regime, seed))


@pytest.mark.parametrize("healthy", [False, True], ids=["labelled", "healthy"])
@pytest.mark.parametrize("n,regime,seed", MC.SET_CASES, ids=str)
def test_set_scores(eng, n, regime, seed, healthy):
    """cddpm_eval_set: AUROC / AUPRC and the search over the labelled set, the thresholds at fpr > 1 / 5 / 10 % wherever the set
    has a negative (always, read as healthy)"""
    x, y = MC.score_set(n, regime, seed)
    out = eng.eval_set(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), healthy=healthy).cpu().numpy()
    want = set_reference(n, regime, seed, healthy)
    print((n, regime, healthy), out.tolist(), want)
    negatives = healthy or regime != "alllesion"
    for i, name in SET_EXACT.items():
        if name.startswith("t_") and not negatives:
            continue                                     # without a negative the reference never computes them
        assert close(EXACT_KEY, out[i], want[name]), (n, regime, healthy, name, float(out[i]), want[name])
    for i, name in SET_AREA.items():
        assert close(AREA_KEY, out[i], want[name]), (n, regime, healthy, name, float(out[i]), want[name])


_first_dense_big = {}


@pytest.mark.parametrize("name", MC.COMPONENT_CASES)
def test_component_filter(eng, name):
    """foreground chosen by the threshold override: sparse and dense random voxels, a long thin path, voxels adjacent in memory
    that are no neighbours, everything, nothing"""
    v, thr = MC.component_case(name)
    out = run_volume(eng, v, threshold=thr)
    if name == "dense_big":
        _first_dense_big["out"] = out
    check_volume(name, out, component_reference(name))


def test_dense_big_second_run_is_bitwise_identical(eng):
    """320 000 voxels of one component hooked together by every block at once: whichever order the unions land in, the
    record, the filtered mask and the row counts come out the same"""
    v, thr = MC.component_case("dense_big")
    first = _first_dense_big.get("out") or run_volume(eng, v, threshold=thr)
    again = run_volume(eng, v, threshold=thr)
    assert bitwise_equal(first, again)


def test_small_case_is_unchanged_by_a_larger_workspace(eng):
    shape, regime, seed = next(c for c in MC.SCORE_CASES if c[:2] == ((33, 19, 4), "quantised"))
    small = MC.volume(shape, regime, seed)
    before = run_volume(eng, small)
    big = run_volume(eng, MC.volume(*MC.SCORE_CASES[-1]))
    after = run_volume(eng, small)
    assert bitwise_equal(before, after)
    check_volume("after", after, score_reference(shape, regime, seed))
    check_volume("big", big, score_reference(*MC.SCORE_CASES[-1]))


def div(a, b):
    return (float("nan") if a == 0 else float("inf")) if b == 0 else a / b


@pytest.mark.parametrize("H,W,D", MC.STEP_SHAPES, ids=str)
def test_native_test_step_takes_rows_along_h(eng, H, W, D):
    """_test_step on a volume with H != W: per-volume entries equal to the reference applied with R = H to eval_oracle's
    post-processed residual; the per-slice lists have one entry per row of H (per row with lesion)"""
    UE = load_pkg("utils_eval")
    recon, orig, seg, mask = MC.step_volume(H, W, D, 801)
    diff = EO.apply_3d_median_filter(EO.apply_brainmask_volume(EO.residual(orig, recon), mask), 5)
    want = MO.eval_volume(recon, orig, seg, mask, np.ascontiguousarray(diff, np.float32))
    host = EC.Host("Brats21", EC.CFG, diffusion=Recorder(eng))
    host.stage, host.eval_dict = "val", UE.get_eval_dictionary()
    UE._test_step(host, *(torch.from_numpy(a)[None, None].cuda() for a in (recon, orig, seg, mask)), 0, ["v0"], torch.tensor(1))
    ed = {k: EC.plain(v) for k, v in host.eval_dict.items()}
    p1s0, p1s1, L, n = want["pred1_seg0"], want["pred1_seg1"], want["lesion"], want["voxels"]
    rows = np.nonzero(want["row_label"])[0]
    assert 0 < rows.size < H and want["row_label"].size == H != W
    expect = {"AUCPerVol": [want["auroc"]], "AUPRCPerVol": [want["auprc"]], "BestDicePerVol": [want["best_dice"]],
              "BestThresholdPerVol": [want["best_threshold"]], "TPPerVol": [n - p1s0 - L], "FPPerVol": [L - p1s1],
              "TNPerVol": [p1s0], "FNPerVol": [p1s1], "DiceScorePerVol": [div(2 * p1s1, p1s0 + p1s1 + L)], "lesionSizePerVol": [L],
              "lesionSizePerSlice": [int(want["row_counts"][r, 2]) for r in rows],
              "DiceScorePerSlice": [div(2 * int(want["row_counts"][r, 1]), int(want["row_counts"][r, 0] + want["row_counts"][r, 2]))
                                    for r in rows],
              "labelPerSlice": want["row_label"].tolist(), "AnomalyScoreRecoPerSlice": want["row_score"].tolist(),
              "AUCAnomalyRecoPerSlice": [want["row_auroc"]], "AUPRCAnomalyRecoPerSlice": [want["row_auprc"]],
              "AnomalyScoreRecoPerVol": [want["score_vol"]], "l1recoErrorAll": [want["l1_all"]],
              "l2recoErrorUnhealthy": [want["l2_lesion"]]}
    for key, w in expect.items():
        print(key, ed[key] if len(w) < 4 else ed[key][:4], w if len(w) < 4 else w[:4])
        assert close(key, ed[key], w), (key, ed[key], w)
    assert 0 < p1s1 < L and p1s0 > 0 and 0.5 < want["auroc"] < 1.0          # the case is informative
