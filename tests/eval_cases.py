"""Evaluation-metric cases shared by tools/make_golden_metrics.py (which records the reference's results) and the tests that
replay them on the device: inputs regenerated from seeds (numpy PCG64), the call sequence of a Lightning test loop
(on_test_start -> _test_step per volume -> _test_end) and the stand-in for the LightningModule those functions read."""
import math

import numpy as np
import torch

H, W, S = 96, 96, 4          # the experiment's evaluation shape: 96 x 96 slices, 4 of them (W // 25 = 3 erosions)

CFG = dict(resizedEvaluation=True, evalSeg=True, erodeBrainmask=True, medianFiltering=True, threshold="auto",
           saveOutputImages=False, kernelsize_median=5)
RAW = dict(CFG, erodeBrainmask=False, medianFiltering=False)        # the residual as it is: components keep their shape

# name -> dataset, cfg, phases [(stage, [volume spec, ...])]; a spec is (kind, seed)
CASES = {
    "val_then_test": dict(dataset="Brats21", cfg=CFG, phases=[("val", [("lesion", 11), ("lesion", 12), ("lesion", 13)]),
                                                              ("test", [("lesion", 21), ("lesion", 22)])]),
    "healthy_val": dict(dataset="IXI", cfg=CFG, phases=[("val", [("healthy", 100 + i) for i in range(28)])]),   # 1.03e6 voxels
    "no_lesion": dict(dataset="Brats21", cfg=CFG, phases=[("val", [("nolesion", 31), ("lesion", 32)])]),
    "zero_residual": dict(dataset="Brats21", cfg=CFG, phases=[("val", [("zero", 41)])]),
    "ties": dict(dataset="Brats21", cfg=CFG, phases=[("val", [("ties", 51), ("ties", 52)])]),
    "components": dict(dataset="Brats21", cfg=RAW, phases=[("val", [("components", 61)])]),
    "node": dict(dataset="MSLUB_node", cfg=RAW, phases=[("val", [("components", 61)])]),
}


class Cfg(dict):
    __getattr__ = dict.get


class Host:
    """what _test_step / _test_end read from and write to the LightningModule (DDPM_2D.on_test_start sets the same)"""

    def __init__(self, dataset, cfg, diffusion=None):
        self.cfg, self.dataset, self.diffusion = Cfg(cfg), [dataset], diffusion
        self.threshold = {}
        self.diffs_list, self.seg_list = [], []


def _brain(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    ry, rx = 0.40 + 0.03 * rng.random(), 0.36 + 0.03 * rng.random()
    m = ((yy - H / 2) / (ry * H)) ** 2 + ((xx - W / 2) / (rx * W)) ** 2 < 1.0     # rows near the top and bottom have no brain
    return np.repeat(m[:, :, None], S, axis=2)


def _components():
    """7- and 8-voxel components joined only through corners or edges, some touching the volume's borders, single voxels"""
    v = np.zeros((H, W, S), np.float32)
    for i in range(7):                                      # corner chain of 7: removed
        v[10 + i, 10 + i, [0, 1, 2, 3, 2, 1, 0][i]] = 1
    for i in range(8):                                      # edge chain of 8 in one slice: kept
        v[30 + i, 30 + i, 0] = 1
    for i in range(8):                                      # corner chain of 8 across slices: kept
        v[50 + i, 20 + i, [0, 1, 2, 3, 3, 2, 1, 0][i]] = 1
    v[0, 95, 3] = v[0, 94, 2] = v[1, 95, 3] = v[1, 93, 3] = v[0, 92, 2] = v[2, 94, 3] = v[1, 91, 3] = 1   # corner of the volume: 7
    v[95, 0, :] = 1
    v[94, 1, :] = 1                                         # edge of the volume: 8
    v[70, 70, 1] = v[70, 80, 2] = v[20, 75, 3] = 1          # single voxels
    v[60:64, 60:64, 1:3] = 1                                # a 32-voxel block
    return v


def volume(kind, seed):
    """(final_volume, data_orig, data_seg, data_mask) as float32 [1, 1, H, W, S] CPU tensors"""
    rng = np.random.Generator(np.random.PCG64(seed))
    orig = rng.random((H, W, S), dtype=np.float32)
    mask = _brain(rng).astype(np.float32)
    seg = np.zeros((H, W, S), np.float32)
    if kind in ("lesion", "ties"):
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(2):
            cy, cx, r = rng.integers(30, 66), rng.integers(30, 66), rng.integers(5, 11)
            seg[((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)] = 1.0
        seg *= mask
    noise = rng.standard_normal((H, W, S)).astype(np.float32)
    recon = orig + np.float32(0.05) * noise - np.float32(0.35) * seg * rng.random((H, W, S), dtype=np.float32)
    if kind == "ties":
        recon = orig + np.round(noise * 4).astype(np.float32) / np.float32(32) - np.float32(0.25) * seg
    if kind == "zero":
        recon = orig.copy()
    if kind == "components":
        orig = np.zeros((H, W, S), np.float32)
        recon = _components()
        mask = np.ones((H, W, S), np.float32)
        seg = np.zeros((H, W, S), np.float32)
        seg[28:40, 28:40, 0] = 1
        seg[94:96, 0:2, :] = 1
        seg[10:14, 10:14, :] = 1
    recon = recon.astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None]
    return t(recon), t(orig), t(seg), t(mask)


def run_case(ue, case, host, to_device=lambda x: x, after_step=None):
    """the Lightning test loop over one case with the module `ue` (the reference's utils_eval or this package's): per phase a
    fresh eval_dict (on_test_start), _test_step per volume, _test_end. Returns per phase (eval_dict, threshold after)."""
    out = []
    for stage, vols in case["phases"]:
        host.stage = stage
        host.eval_dict = ue.get_eval_dictionary()
        if not hasattr(host, "threshold"):
            host.threshold = {}
        for b, (kind, seed) in enumerate(vols):
            fv, orig, seg, mask = (to_device(x) for x in volume(kind, seed))
            ue._test_step(host, fv, orig, seg, mask, b, [f"{kind}{seed}"], torch.tensor(1 if kind != "healthy" else 0))
            if after_step is not None:
                after_step(host, kind)
        ue._test_end(host)
        out.append((host.eval_dict, dict(getattr(host, "threshold", {}))))
    return out


def plain(v):
    """eval_dict values as JSON-able Python numbers (tensors and numpy scalars included)"""
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, torch.Tensor):
        v = v.item()
    if isinstance(v, (np.generic,)):
        v = v.item()
    if isinstance(v, float) and math.isnan(v):
        return float("nan")
    return v
