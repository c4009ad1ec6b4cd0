"""Times the device evaluation metric pass against the CPU one it replaces.

  * one volume at 96 x 96 x 4 (the experiment's evaluation shape): residual post-processing + CddpmEngine.eval_volume, the whole
    per-volume device work of the native _test_step, ending in the copy of the record to the host;
  * the validation-set threshold search and the healthy thresholds over about 4e6 voxels (CddpmEngine.eval_set).
When scipy / scikit-learn are importable it also times what the reference does per volume on the CPU (scipy erosion +
median filter, roc_curve + auc, average_precision_score, the 20-probe find_best_val, scipy 26-connected labelling) and over the
set (find_best_val, roc_curve). Warm-up first, then the median of --repeats timed runs; one JSON line.

    python tools/eval_metrics_bench.py [--repeats 20] [--set-voxels 4000000]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import eval_cases as EC  # noqa: E402

PKG = "conditioned-diffusion-models-uad_amd"


def median_ms(fn, repeats, sync=True):
    fn()
    fn()
    ts = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def cpu_volume_pass(fv, orig, seg, mask):
    import scipy.ndimage as ndi
    from sklearn.metrics import auc, average_precision_score, roc_curve
    diff = np.abs(orig - fv)
    strel = ndi.generate_binary_structure(2, 1)
    for s in range(diff.shape[2]):
        diff[:, :, s] *= ndi.binary_erosion(mask[:, :, s] > 0, structure=strel, iterations=diff.shape[1] // 25)
    diff = ndi.median_filter(diff, (5, 5, 5))
    x, y = diff.ravel(), seg.ravel() > 0
    fpr, tpr, _ = roc_curve(y.astype(int), x)
    auc(fpr, tpr)
    average_precision_score(y.astype(int), x)
    lo, hi, best = 0.0, float(x.max()), 0.0
    for _ in range(10):
        w = hi - lo
        d = [2 * np.sum((x > q) & y) / (np.sum(x > q) + np.sum(y)) for q in (lo + w * 0.25, lo + w * 0.75)]
        lo, hi = (lo, lo + w * 0.5) if d[0] >= d[1] else (lo + w * 0.5, hi)
        best = max(best, max(d))
    lab, _ = ndi.label(diff > lo, structure=np.ones((3, 3, 3)))
    np.bincount(lab.ravel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--set-voxels", type=int, default=4_000_000)
    a = ap.parse_args()
    UE = importlib.import_module(PKG + ".utils_eval")
    eng_mod = importlib.import_module(PKG + ".engine")
    eng = eng_mod.CddpmEngine(timesteps=10, max_batch=1, max_h=32, max_w=32)
    fv, orig, seg, mask = (t[0, 0].cuda() for t in EC.volume("lesion", 11))

    def volume_pass():
        diff = UE.postprocess_residual(eng, orig, fv, mask).contiguous()
        r = eng.eval_volume(fv, orig, seg, mask, diff, voxel_metrics=True, component_filter=True, row_curve=True)
        r["record"].cpu()

    res = {"volume_shape": [EC.H, EC.W, EC.S], "device_volume_ms": median_ms(volume_pass, a.repeats)}
    n = a.set_voxels
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(n, device="cuda", generator=g)
    y = (torch.rand(n, device="cuda", generator=g) < 0.02).to(torch.int8)
    res["set_voxels"] = n
    res["device_set_search_ms"] = median_ms(lambda: eng.eval_set(x, y, healthy=False).cpu(), a.repeats)
    res["device_healthy_thresholds_ms"] = median_ms(lambda: eng.eval_set(x, y, healthy=True).cpu(), a.repeats)
    try:
        import scipy  # noqa: F401
        import sklearn  # noqa: F401
        have_cpu = True
    except ImportError:
        have_cpu = False
    if have_cpu:
        from sklearn.metrics import roc_curve
        h = [t.cpu().numpy() for t in (fv, orig, seg, mask)]
        res["cpu_volume_ms"] = median_ms(lambda: cpu_volume_pass(*h), max(3, a.repeats // 4), sync=False)
        xh, yh = x.cpu().numpy(), y.cpu().numpy().astype(bool)

        def cpu_set():
            lo, hi = 0.0, float(xh.max())
            for _ in range(10):
                w = hi - lo
                d = [2 * np.sum((xh > q) & yh) / (np.sum(xh > q) + np.sum(yh)) for q in (lo + w * 0.25, lo + w * 0.75)]
                lo, hi = (lo, lo + w * 0.5) if d[0] >= d[1] else (lo + w * 0.5, hi)
        res["cpu_set_search_ms"] = median_ms(cpu_set, 3, sync=False)
        res["cpu_healthy_thresholds_ms"] = median_ms(lambda: roc_curve(np.zeros(n, int), xh), 3, sync=False)
    else:
        res["cpu"] = "scipy / scikit-learn not importable: not measured"
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
