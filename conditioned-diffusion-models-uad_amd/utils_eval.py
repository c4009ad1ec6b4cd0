"""Device-side mirrors of the residual-map helpers of the reference's evaluation step (src/utils/utils_eval.py):
same names, argument meaning and array layout ([H, W, S] volumes, squeezable singleton axes), on HIP tensors.

    residual_volume          utils_eval.py:29-33   |orig - recon| (the reference's `residualmode` test is always true: L1)
    apply_brainmask_volume   utils_eval.py:454-460 per slice: volume * binary_erosion(mask, cross, iterations = W // 25)
    apply_3d_median_filter   utils_eval.py:462-464 scipy.ndimage.median_filter(volume, (k, k, k))

The metric pass itself (csrc/eval_metrics.hip through CddpmEngine.eval_volume / eval_set) is behind the evaluation hooks the
DDPM_2D mirror uses standalone, with the reference's names and arguments:

    get_eval_dictionary      utils_eval.py:321-441  the reference's key set
    _test_step               utils_eval.py:18-194   per volume: reconstruction errors, AUROC / AUPRC, find_best_val, the
                                                    26-connected component filter, confusion counts, per-row metrics and
                                                    anomaly scores; the validation set accumulates in a device buffer
    _test_end                utils_eval.py:196-297  aggregates (numpy on the lists, as the reference), threshold['total'] or
                                                    the healthy thresholds t_1p / t_5p / t_10p from the accumulated set

They follow the reference as its environment ran it (numpy 1.22, scikit-learn 1.0.1, scikit-image 0.18.3), quirks included:
the swapped confusion-matrix names, fpr = fp / (fp + tp), NaN AUROC / AUPRC for a volume without lesion, "per-slice" metrics
over axis 0 of the [H, W, D] volume. The Hausdorff distance (utils_eval.py:131-135, monai's compute_hausdorff_distance in the
reference) is computed on the device (csrc/eval_hausdorff.hip through CddpmEngine.hausdorff) when cfg.evalHausdorff is true: pinned to
scipy bit for bit, unpinned to monai (its rules are restated in include/cddpm.h; monai reads a non-boolean ground truth as == 1, this
pass as != 0). Without the key HausPerVol gets NaN, which _test_end drops, as before.
Not built: image grids (log_images), calc_thresh, the KLDBackprop branches, resizedEvaluation = False (NotImplementedError).
No CPU fallback: the functions need an engine (a loaded libcddpm_hip.so) and HIP tensors.
"""
import math
import warnings
from typing import Optional

import numpy as np
import torch


def _to_shw(vol: torch.Tensor) -> torch.Tensor:
    v = vol.squeeze()
    if v.dim() != 3:
        raise RuntimeError(f"expected a volume that squeezes to [H, W, S], got shape {tuple(vol.shape)}")
    return v.permute(2, 0, 1).contiguous().float()


def _from_shw(v: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return v.permute(1, 2, 0).contiguous().reshape(like.shape)


def residual_volume(engine, data_orig: torch.Tensor, final_volume: torch.Tensor, *, squared: bool = False) -> torch.Tensor:
    """diff_volume of _test_step: torch.abs(data_orig - final_volume) (or the square), same shape as data_orig."""
    out = engine.residual_postprocess(_to_shw(data_orig), _to_shw(final_volume), None, squared=squared)
    return _from_shw(out, data_orig)


def apply_brainmask_volume(engine, vol: torch.Tensor, mask_vol: torch.Tensor, erode: bool = True, iterations: int = 10) -> torch.Tensor:
    """The reference ignores `erode` and `iterations`: it always erodes, vol.squeeze().shape[1] // 25 times (:458).
    With fewer than 25 columns that count is 0, which scipy reads as "erode until nothing changes": an empty mask."""
    v = _to_shw(vol)
    n = v.shape[2] // 25
    if n == 0:
        return torch.zeros_like(vol) * vol
    return _from_shw(engine.residual_postprocess(v, None, _to_shw(mask_vol), erode_iterations=n), vol)


def apply_3d_median_filter(engine, volume: torch.Tensor, kernelsize: int = 5) -> torch.Tensor:
    return _from_shw(engine.residual_postprocess(_to_shw(volume), None, None, median_k=kernelsize), volume)


def postprocess_residual(engine, data_orig: torch.Tensor, final_volume: torch.Tensor, data_mask: Optional[torch.Tensor], *,
                         erodeBrainmask: bool = True, medianFiltering: bool = True, kernelsize_median: int = 5) -> torch.Tensor:
    """The three steps of _test_step (:29-33, :64-71) in one call: one pass over the volume + one median pass."""
    o = _to_shw(data_orig)
    n = o.shape[2] // 25
    use_mask = erodeBrainmask and data_mask is not None
    if use_mask and n == 0:
        return torch.zeros_like(data_orig)
    out = engine.residual_postprocess(o, _to_shw(final_volume), _to_shw(data_mask) if use_mask else None,
                                      erode_iterations=n if use_mask else 0, median_k=kernelsize_median if medianFiltering else 0)
    return _from_shw(out, data_orig)


# ---------------------------------------------------------------------------------------------------------------------------------
# the evaluation hooks (utils_eval.py:18-297)

HEALTHY_SETS = ["IXI"]
_SCALARS = ("l1reconstructionErrorMean", "l1reconstructionErrorStd", "l2reconstructionErrorMean", "l2reconstructionErrorStd")
_LISTS = """IDs x reconstructions diffs diffs_volume Segmentation reconstructionTimes latentSpace Age AgeGroup
l1reconstructionErrors l2reconstructionErrors l1recoErrorAll l1recoErrorUnhealthy l1recoErrorHealthy l2recoErrorAll
l2recoErrorUnhealthy l2recoErrorHealthy HausPerVol TPPerVol FPPerVol FNPerVol TNPerVol TPRPerVol FPRPerVol TPTotal FPTotal
FNTotal TNTotal TPRTotal FPRTotal PrecisionPerVol RecallPerVol PrecisionPerSlice RecallPerSlice lesionSizePerSlice
lesionSizePerVol Dice DiceScorePerSlice DiceScorePerVol BestDicePerVol BestThresholdPerVol AUCPerVol AUPRCPerVol
SpecificityPerVol AccuracyPerVol KLD_to_learned_prior labelPerSlice labelPerVol""".split()
_GRAD_ELBO = "TP FP FN TN TPR FPR Dice DiceScorePerVol BestDicePerVol BestThresholdPerVol AUCPerVol AUPRCPerVol".split()
_PER_SLICE = [f"{m}Anomaly{s}PerSlice" for s in ("Comb", "KLD", "Reco", "Age") for m in ("AUC", "AUPRC")] + \
    [f"AnomalyScore{s}PerSlice" for s in ("Comb", "KLD", "Reco", "RecoBin", "Age")]
_PER_VOL = [f"AnomalyScore{s}PerVol" for s in ("Comb", "Combi", "CombMean", "Reg", "RegMean", "Reco", "CombPrior", "CombiPrior",
                                               "Age", "RecoMean")]
_KL = [f"{m}{k}PerVol" for k in ("KLComb", "KL") for m in ("TP", "FP", "TN", "FN", "TPR", "FPR", "AUC", "AUPRC", "BestDice")] + \
    ["DiceScoreKLPerVol", "DiceScoreKLCombPerVol"]


def get_eval_dictionary():
    """the reference's eval_dict (utils_eval.py:321-441): every key it creates, the four scalar entries at 0.0, lists elsewhere"""
    d = {k: [] for k in _LISTS + [f"{k}gradELBO" for k in _GRAD_ELBO] + _PER_SLICE + _PER_VOL + _KL}
    d.update({k: 0.0 for k in _SCALARS})
    return d


def _div(a, b) -> float:
    """numpy's float64 true division of two counts: 0 / 0 = NaN, x / 0 = inf"""
    if b == 0:
        return math.nan if a == 0 else math.copysign(math.inf, a)
    return a / b


def _eval_engine(self, device):
    """the UNet mirror's engine, as _gen_noise takes it (any geometry serves: the metric entry points use no model state)"""
    return self.diffusion._engine(1, 4, 4, device)


class _DeviceSet:
    """the validation set of _test_step (:142-148: np.append per volume) as a device buffer that doubles when it fills"""

    def __init__(self, device):
        self.x = torch.empty(0, dtype=torch.float32, device=device)
        self.y = torch.empty(0, dtype=torch.int8, device=device)
        self.n = 0

    def append(self, x: torch.Tensor, y: torch.Tensor):
        need = self.n + x.numel()
        if need > self.x.numel():
            cap = max(need, 2 * self.x.numel())
            nx = torch.empty(cap, dtype=torch.float32, device=self.x.device)
            ny = torch.empty(cap, dtype=torch.int8, device=self.x.device)
            nx[:self.n] = self.x[:self.n]
            ny[:self.n] = self.y[:self.n]
            self.x, self.y = nx, ny
        self.x[self.n:need] = x.reshape(-1)
        self.y[self.n:need] = y.reshape(-1)
        self.n = need

    def view(self):
        return self.x[:self.n], self.y[:self.n]


def _test_step(self, final_volume, data_orig, data_seg, data_mask, batch_idx, ID, label_vol):
    """utils_eval.py:18-194 on the device. The volumes stay there; the scalars and the per-row lists come back in one copy."""
    self.healthy_sets = list(HEALTHY_SETS)
    if not self.cfg.resizedEvaluation:
        raise NotImplementedError("resizedEvaluation = False interpolates to new_size, which the 4-slice data_orig cannot match")
    final_volume = final_volume.squeeze()
    dev = final_volume.device
    eng = _eval_engine(self, dev)
    orig = data_orig.squeeze().float().contiguous()
    seg = data_seg.squeeze().float().contiguous()
    mask = data_mask.squeeze().float().contiguous()
    recon = final_volume.float().contiguous()
    diff = postprocess_residual(eng, orig, recon, mask, erodeBrainmask=bool(self.cfg["erodeBrainmask"]),
                                medianFiltering=bool(self.cfg["medianFiltering"]),
                                kernelsize_median=self.cfg.get("kernelsize_median", 5)).contiguous()
    dataset = self.dataset[0]
    healthy = dataset in self.healthy_sets
    voxel = bool(self.cfg.evalSeg) and not healthy
    override = None
    if voxel:
        if self.cfg["threshold"] != "auto":
            raise NotImplementedError("a fixed cfg threshold (the reference: 'never used')")
        if "test" in self.stage:
            override = self.threshold["total"]          # KeyError without a validation pass, as in the reference (:92-93)
    res = eng.eval_volume(recon, orig, seg, mask, diff, voxel_metrics=voxel, component_filter="node" not in dataset.lower(),
                          row_curve=not healthy, threshold=override)
    if "val" in self.stage:
        if batch_idx == 0 or not isinstance(getattr(self, "diffs_list", None), _DeviceSet):
            self.diffs_list = _DeviceSet(dev)
        self.diffs_list.append(diff, (seg > 0).to(torch.int8))
    rec = res["record"].cpu().numpy()
    row_score = res["row_score"].cpu().numpy()
    row_label = res["row_label"].cpu().numpy()
    ed = self.eval_dict
    for k, i in (("l1recoErrorAll", 0), ("l1recoErrorUnhealthy", 1), ("l1recoErrorHealthy", 2), ("l2recoErrorAll", 3),
                 ("l2recoErrorUnhealthy", 4), ("l2recoErrorHealthy", 5)):
        ed[k].append(float(rec[i]))
    if voxel:
        n, L = int(rec[8]), int(rec[7])
        p1s0, p1s1 = int(rec[15]), int(rec[16])
        pred1 = p1s0 + p1s1
        p0s1 = L - p1s1
        p0s0 = n - pred1 - p0s1
        best_thr = float(rec[13]) if override is None else override
        ed["lesionSizePerVol"].append(L)
        ed["DiceScorePerVol"].append(_div(2 * p1s1, pred1 + L))
        ed["BestDicePerVol"].append(float(rec[11]))
        ed["BestThresholdPerVol"].append(best_thr)
        ed["AUCPerVol"].append(float(rec[9]))
        ed["AUPRCPerVol"].append(float(rec[10]))
        # confusion_matrix(pred, seg).ravel() names (:102): TP = #(0, 0), FP = #(0, 1), TN = #(1, 0), FN = #(1, 1)
        ed["TPPerVol"].append(p0s0)
        ed["FPPerVol"].append(p0s1)
        ed["TNPerVol"].append(p1s0)
        ed["FNPerVol"].append(p1s1)
        ed["TPRPerVol"].append(_div(p1s1, L))
        ed["FPRPerVol"].append(_div(p1s0, pred1))            # fpr() of the reference: fp / (fp + tp)
        ed["IDs"].append(ID[0])
        ed["AccuracyPerVol"].append((p1s1 + p0s0) / n)
        ed["PrecisionPerVol"].append(p1s1 / pred1 if pred1 else 0.0)
        ed["RecallPerVol"].append(p1s1 / L if L else 0.0)
        ed["SpecificityPerVol"].append(p1s0 / (p1s0 + p0s1 + 0.0000001))
        if self.cfg.get("evalHausdorff"):                   # :131-135: filtered prediction (unfiltered for 'node' sets) against data_seg
            ed["HausPerVol"].append(float(eng.hausdorff(res["pred"], seg)["record"][0]))
        else:
            ed["HausPerVol"].append(math.nan)               # the default: _test_end drops it
        counts = res["row_counts"].cpu().numpy()
        for r in np.nonzero(row_label)[0]:                  # rows with lesion, unfiltered prediction (:137-144)
            p, pg, g = (int(v) for v in counts[r])
            ed["DiceScorePerSlice"].append(_div(2 * pg, p + g))
            ed["PrecisionPerSlice"].append(pg / p if p else 0.0)
            ed["RecallPerSlice"].append(pg / g if g else 0.0)
            ed["lesionSizePerSlice"].append(g)
    if not healthy:
        ed["AUCAnomalyRecoPerSlice"].append(float(rec[17]))
        ed["AUPRCAnomalyRecoPerSlice"].append(float(rec[18]))
        ed["labelPerSlice"].extend(int(v) for v in row_label)
        ed["AnomalyScoreRecoPerSlice"].extend(float(v) for v in row_score)
    if self.cfg.get("use_postprocessed_score", True):
        score = float(rec[6])
        for k in ("AnomalyScoreRecoPerVol", "AnomalyScoreCombPerVol", "AnomalyScoreCombiPerVol", "AnomalyScoreCombPriorPerVol",
                  "AnomalyScoreCombiPriorPerVol"):
            ed[k].append(score)
    ed["labelPerVol"].append(label_vol.item() if hasattr(label_vol, "item") else label_vol)


_AGGREGATES = [  # (output name, list, nan-aware) of _test_end (:199-244)
    ("l1recoErrorAll", "l1recoErrorAll", True), ("l2recoErrorAll", "l2recoErrorAll", True),
    ("l1recoErrorHealthy", "l1recoErrorHealthy", True), ("l1recoErrorUnhealthy", "l1recoErrorUnhealthy", True),
    ("l2recoErrorHealthy", "l2recoErrorHealthy", True), ("l2recoErrorUnhealthy", "l2recoErrorUnhealthy", True),
    ("AUPRCPerVol", "AUPRCPerVol", True), ("AUCPerVol", "AUCPerVol", True), ("DicePerVol", "DiceScorePerVol", True),
    ("BestDicePerVol", "BestDicePerVol", False), ("BestThresholdPerVol", "BestThresholdPerVol", False),
    ("TPPerVol", "TPPerVol", True), ("FPPerVol", "FPPerVol", True), ("TNPerVol", "TNPerVol", True), ("FNPerVol", "FNPerVol", True),
    ("TPRPerVol", "TPRPerVol", True), ("FPRPerVol", "FPRPerVol", True),
    ("PrecisionPerVol", "PrecisionPerVol", False), ("RecallPerVol", "RecallPerVol", False),
    ("PrecisionPerSlice", "PrecisionPerSlice", False), ("RecallPerSlice", "RecallPerSlice", False),
    ("AccuracyPerVol", "AccuracyPerVol", False), ("SpecificityPerVol", "SpecificityPerVol", False)]


def _aggregate(ed):
    """the host part of _test_end: mean / std of the lists with numpy, as the reference computes them"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for out, src, nan in _AGGREGATES:
            mean, std = (np.nanmean, np.nanstd) if nan else (np.mean, np.std)
            ed[out + "Mean"] = mean(ed[src])
            ed[out + "Std"] = std(ed[src])
        h = np.array(ed["HausPerVol"])
        h = h[np.isfinite(h)]
        ed["HausPerVolMean"] = np.nanmean(h)
        ed["HausPerVolStd"] = np.nanstd(h)


def _test_end(self):
    """utils_eval.py:196-297: the aggregates on the host; the validation set's threshold search / healthy thresholds on the device"""
    _aggregate(self.eval_dict)
    if "test" in self.stage:
        del self.threshold
    if "val" in self.stage:
        x, y = self.diffs_list.view()
        eng = _eval_engine(self, x.device)
        if self.dataset[0] not in self.healthy_sets:
            out = eng.eval_set(x, y, healthy=False).cpu().numpy()
            self.threshold["total"] = float(out[6])
        else:
            out = eng.eval_set(x, y, healthy=True).cpu().numpy()
            self.threshholds_healthy = {"thresh_1p": float(out[2]), "thresh_5p": float(out[3]), "thresh_10p": float(out[4])}
            self.eval_dict["t_1p"] = self.threshholds_healthy["thresh_1p"]
            self.eval_dict["t_5p"] = self.threshholds_healthy["thresh_5p"]
            self.eval_dict["t_10p"] = self.threshholds_healthy["thresh_10p"]
