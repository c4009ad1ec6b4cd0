"""GPU: the native evaluation metric pass (csrc/eval_metrics.hip through CddpmEngine.eval_volume / eval_set and the
_test_step / _test_end of this package's utils_eval.py) against the reference's own results on the cases of
tests/eval_cases.py (tests/golden/eval_metrics.json, made by tools/make_golden_metrics.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_cases as EC
from conftest import GOLD, load_pkg

pytestmark = pytest.mark.gpu

EXACT = {"TPPerVol", "FPPerVol", "TNPerVol", "FNPerVol", "lesionSizePerVol", "lesionSizePerSlice", "labelPerSlice", "labelPerVol",
         "BestDicePerVol", "BestThresholdPerVol", "t_1p", "t_5p", "t_10p", "HausPerVol"}


def tolerance(key):
    if key in EXACT:
        return 0.0, 0.0
    if "recoError" in key or "AnomalyScore" in key:       # fp32 means (torch) against fixed-order float64 sums; the
        return 1e-9, 1e-6                                 # std of such values carries their fp32 rounding as absolute error
    return 1e-12, 1e-12


def close(key, got, want):
    atol, rtol = tolerance(key)
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(close(key, g, w) for g, w in zip(got, want))
    got, want = float(got), float(want)
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= atol + rtol * abs(want)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "eval_metrics.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


@pytest.fixture(scope="module")
def UE():
    return load_pkg("utils_eval")


class Recorder:
    """the engine as DDPM_2D.diffusion._engine hands it out, keeping what eval_volume returned"""

    def __init__(self, eng):
        self.eng, self.volumes = eng, []

    def _engine(self, B, H, W, device):
        return self

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def eval_volume(self, *a, **k):
        out = self.eng.eval_volume(*a, **k)
        self.volumes.append(out)
        return out


def unpack_mask(hexstr):
    return np.unpackbits(np.frombuffer(bytes.fromhex(hexstr), np.uint8))[:EC.H * EC.W * EC.S].reshape(EC.H, EC.W, EC.S).astype(bool)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_native_test_step_and_test_end_against_the_reference(eng, UE, fixture, name):
    case, ref = EC.CASES[name], fixture["cases"][name]
    rec = Recorder(eng)
    host = EC.Host(case["dataset"], case["cfg"], diffusion=rec)
    res = EC.run_case(UE, case, host, to_device=lambda t: t.cuda())
    checked = 0
    for (ed, thr), want in zip(res, ref["phases"]):
        for key, w in want["eval_dict"].items():
            assert close(key, EC.plain(ed[key]), w), (name, want["stage"], key, EC.plain(ed[key]), w)
            checked += 1
        for key in ed:               # nothing filled that the reference leaves empty
            if isinstance(ed[key], list) and ed[key] and key not in ("IDs",):
                assert key in want["eval_dict"], key
        assert {k: float(v) for k, v in thr.items()} == {k: float(v) for k, v in want["threshold"].items()}
    assert checked > 40
    # the filtered masks, bit for bit: one per volume with voxel metrics, unless the dataset's name contains 'node'
    masks = [unpack_mask(m) for m in ref["filtered_masks"]]
    if "node" not in case["dataset"].lower() and case["dataset"] != "IXI":
        assert len(masks) == len(rec.volumes)
        for v, m in zip(rec.volumes, masks):
            assert np.array_equal(v["pred"].cpu().numpy().astype(bool), m)
    else:
        assert masks == []


def test_component_filter_individually(eng):
    fv, orig, seg, mask = (t[0, 0].cuda() for t in EC.volume("components", 61))
    diff = (orig - fv).abs()
    out = {f: eng.eval_volume(fv, orig, seg, mask, diff, voxel_metrics=True, component_filter=f, row_curve=False, threshold=0.5)
           for f in (True, False)}
    raw = (diff > 0.5).cpu().numpy()
    kept = out[True]["pred"].cpu().numpy().astype(bool)
    assert np.array_equal(out[False]["pred"].cpu().numpy().astype(bool), raw)
    assert kept.sum() == 8 + 8 + 8 + 32 and not kept[10:17, 10:17, :].any() and kept[30:38, 30:38, 0].sum() == 8
    assert not kept[0:3, 90:96, :].any() and kept[94:96, 0:2, :].sum() == 8 and not kept[70, 70, 1]


def test_curve_and_threshold_search_individually(eng, fixture):
    """AUROC / AUPRC of one volume, find_best_val over a validation set and the healthy thresholds over 1.03e6 voxels,
    each through the engine directly"""
    UE = load_pkg("utils_eval")
    val = fixture["cases"]["val_then_test"]["phases"][0]
    xs, ys = [], []
    for i, (kind, seed) in enumerate(EC.CASES["val_then_test"]["phases"][0][1]):
        fv, orig, seg, mask = (t.cuda() for t in EC.volume(kind, seed))
        diff = UE.postprocess_residual(eng, orig.squeeze(), fv.squeeze(), mask.squeeze()).contiguous()
        s = seg.squeeze().contiguous()
        r = eng.eval_volume(fv.squeeze().contiguous(), orig.squeeze().contiguous(), s, mask.squeeze().contiguous(), diff,
                            voxel_metrics=True, component_filter=True, row_curve=True)["record"].cpu().numpy()
        assert abs(r[9] - val["eval_dict"]["AUCPerVol"][i]) <= 1e-12 and abs(r[10] - val["eval_dict"]["AUPRCPerVol"][i]) <= 1e-12
        xs.append(diff.reshape(-1))
        ys.append((s > 0).to(torch.int8).reshape(-1))
    out = eng.eval_set(torch.cat(xs), torch.cat(ys), healthy=False).cpu().numpy()
    assert out[6] == fixture["cases"]["val_then_test"]["phases"][0]["threshold"]["total"]
    xs = []
    for kind, seed in EC.CASES["healthy_val"]["phases"][0][1]:
        fv, orig, seg, mask = (t[0, 0].cuda() for t in EC.volume(kind, seed))
        xs.append(UE.postprocess_residual(eng, orig, fv, mask).reshape(-1))
    x = torch.cat(xs)
    assert x.numel() > 10 ** 6
    out = eng.eval_set(x, torch.zeros(x.numel(), dtype=torch.int8, device=x.device), healthy=True).cpu().numpy()
    want = fixture["cases"]["healthy_val"]["phases"][0]["eval_dict"]
    assert (out[2], out[3], out[4]) == (want["t_1p"], want["t_5p"], want["t_10p"])


def test_second_run_is_bitwise_identical(eng):
    UE = load_pkg("utils_eval")
    fv, orig, seg, mask = (t[0, 0].cuda() for t in EC.volume("lesion", 11))
    diff = UE.postprocess_residual(eng, orig, fv, mask).contiguous()
    runs = [eng.eval_volume(fv, orig, seg, mask, diff, voxel_metrics=True, component_filter=True, row_curve=True) for _ in range(2)]
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
    x = diff.reshape(-1).repeat(30)
    y = (seg > 0).to(torch.int8).reshape(-1).repeat(30)
    s1, s2 = eng.eval_set(x, y, healthy=False), eng.eval_set(x, y, healthy=False)
    assert torch.equal(s1.view(torch.uint8), s2.view(torch.uint8))


def test_engine_rejects_bad_inputs(eng):
    v = torch.zeros(4, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="shape"):
        eng.eval_volume(v, v, v, v, torch.zeros(4, 8, 4, device="cuda"), voxel_metrics=True, component_filter=True, row_curve=True)
    with pytest.raises(RuntimeError, match="float32"):
        eng.eval_volume(v.double(), v, v, v, v, voxel_metrics=True, component_filter=True, row_curve=True)
    with pytest.raises(RuntimeError, match="int8"):
        eng.eval_set(v.reshape(-1), torch.zeros(256, dtype=torch.int32, device="cuda"), healthy=False)


def test_standalone_ddpm2d_evaluation_end_to_end(sd_np, UE):
    """the mirror outside the reference tree: on_test_start / test_step / on_test_end fill eval_dict with the native metric
    pass, equal to the native functions applied to the returned final_volume"""
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500,
               timesteps=1000, noise_ensemble=False, **EC.CFG)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous() * 2 - 1

    mod = M.DDPM_2D(cfg, encoder=Enc())
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    mod = mod.cuda()
    H = W = 32
    rng = np.random.Generator(np.random.PCG64(7))
    vol = torch.from_numpy(rng.random((1, 1, H, W, 6), dtype=np.float32)).cuda()
    seg = torch.zeros_like(vol)
    seg[..., 10:18, 12:20, :] = 2.0
    mask = torch.zeros_like(vol)
    mask[..., 3:29, 4:28, :] = 1.0
    mod.on_test_start()
    outs = []
    for b in range(2):
        batch = {"vol": {"data": vol}, "vol_orig": {"data": vol}, "seg_orig": {"data": seg}, "mask_orig": {"data": mask},
                 "seg_available": True, "Dataset": ["Brats21"], "stage": "val", "ID": [f"v{b}"], "label": torch.tensor([1])}
        outs.append(mod.test_step(batch, b))
    mod.on_test_end()
    ed = mod.eval_dict
    assert len(ed["AUCPerVol"]) == 2 and len(ed["DiceScorePerVol"]) == 2 and "total" in mod.threshold
    # the same through the native functions on a stand-in host
    host = EC.Host("Brats21", EC.CFG, diffusion=mod.diffusion)
    host.stage, host.eval_dict = "val", UE.get_eval_dictionary()
    sl = slice(1, 5)                                             # the 4 centre slices test_step takes
    for b, o in enumerate(outs):
        UE._test_step(host, o["final_volume"], vol[..., sl], seg[..., sl], mask[..., sl], b, [f"v{b}"], torch.tensor([1]))
    UE._test_end(host)
    for k, v in host.eval_dict.items():              # identical computations: equal, NaN where NaN
        if isinstance(v, list) and v:
            a, b = EC.plain(ed[k]), EC.plain(v)
            assert len(a) == len(b) and all(same_or_nan(x, y) for x, y in zip(a, b)), k
        elif k.endswith("Mean") or k.endswith("Std"):
            assert same_or_nan(float(ed[k]), float(v)), k
    assert host.threshold["total"] == mod.threshold["total"]
    mod.diffusion.model._hip.close()


def same_or_nan(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))
