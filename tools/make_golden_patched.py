"""Fixtures for the patched DDPM (tests/golden/patched/): outputs of the REFERENCE's own BoxSampler (src/utils/patch_sampling.py)
and of its `DDPM_2D_patched.DDPM_2D.test_step` (src/models/DDPM_2D_patched.py), imported by path through oracle/ref_harness.py.

Build container only (the reference tree does not travel to the GPU machine). The reference class is imported UNMODIFIED; stand-ins
are registered only for modules missing here: pytorch_lightning (LightningModule = nn.Module with `device`, `log`,
`save_hyperparameters`), torchio (DATA = 'data'), wandb, numba (ref_harness), torchvision.transforms, skimage.measure and monai (names
only: nothing of them runs). `_test_step` of the imported module is replaced by a capture of `final_volume`; the per-box
reconstructions are recorded by wrapping `diffusion.forward`. `noisetype` is unset, so the reference draws torch.randn_like once per
box: the harness hands it the SAME seeded field every time, which is what one `gen_noise` field shared by all boxes is (:178-188).

    python tools/make_golden_patched.py          # writes tests/golden/patched/*.npz + MANIFEST.json, seconds
"""
import importlib
import json
import os
import sys
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")     # the MKL code path tests/conftest.py pins

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import cddpm_oracle as O  # noqa: E402
import ref_harness as R  # noqa: E402

synth = importlib.import_module("conditioned-diffusion-models-uad_amd.synth")
OUT = os.path.join(ROOT, "tests", "golden", "patched")
GRIDS = [(32, 32, 16, False), (32, 32, 12, False), (32, 32, 12, True), (16, 48, 16, False)]      # H, W, patch, overlap
SINGLE = [(0, 3, 32, 32, 16), (1, 3, 32, 32, 12), (7, 4, 16, 48, 16)]                           # seed, batch, H, W, patch
STITCH = {"p16_paste": dict(patch_size=16), "p12_ragged_paste": dict(patch_size=12),
          "p12_overlap_cut": dict(patch_size=12, overlap=True, agg_overlap="cut"),
          "p12_overlap_avg": dict(patch_size=12, overlap=True, agg_overlap="avg")}
OBJECTIVES = {"x0_l1_inpaint": dict(objective="pred_x0", loss="l1", inpaint=True),
              "noise_l2_box": dict(objective="pred_noise", loss="l2", inpaint=False)}
S, H, W, T_TEST = 3, 32, 32, 351          # test_step reconstructs at t = test_timesteps - 1 = 350
SEEDS = dict(weights=0, x01=2, noise=3)


class Cfg(dict):
    __getattr__ = dict.get


def stand_ins():
    R.import_reference()                  # torchvision / ema_pytorch / numba
    class LightningModule(torch.nn.Module):
        device = torch.device("cpu")
        def log(self, *a, **k): pass
        def save_hyperparameters(self, *a, **k): pass
    for name, attrs in {"pytorch_lightning": {}, "pytorch_lightning.core": {},
                        "pytorch_lightning.core.lightning": dict(LightningModule=LightningModule),
                        "torchio": dict(DATA="data"), "wandb": {}, "monai": {}, "skimage": {},
                        "skimage.measure": dict(regionprops=None, label=None)}.items():
        if name not in sys.modules:
            R._stub(name, **attrs)
    tvt = sys.modules["torchvision.transforms"]
    for n in ("ToTensor", "ToPILImage"):
        if not hasattr(tvt, n):
            setattr(tvt, n, None)


def boxes_fixture(BoxSampler):
    out, man = {}, {}
    x = lambda b, h, w: torch.zeros(b, 1, h, w)
    for h, w, p, ov in GRIDS:
        key = f"grid_{h}x{w}_p{p}{'_overlap' if ov else ''}"
        bs = BoxSampler(Cfg(patch_size=p, overlap=ov))
        out[key], out[key + "_cut"] = bs.sample_grid(x(2, h, w)).numpy(), bs.sample_grid_cut(x(2, h, w)).numpy()
        man[key] = dict(H=h, W=w, patch_size=p, overlap=ov, batch=2, K=int(out[key].shape[1]))
    for seed, b, h, w, p in SINGLE:
        key = f"single_seed{seed}_B{b}_{h}x{w}_p{p}"
        torch.manual_seed(seed)
        bs = BoxSampler(Cfg(patch_size=p))
        out[key] = np.stack([bs.sample_single_box(x(b, h, w)).numpy() for _ in range(2)])       # two draws in a row
        man[key] = dict(seed=seed, batch=b, H=h, W=w, patch_size=p, draws=2)
    np.savez_compressed(os.path.join(OUT, "boxes.npz"), **out)
    return man


def test_step_fixtures(mod):
    sd = O.to_torch_sd(synth.synth_state_dict(SEEDS["weights"], num_classes=None))
    x01 = torch.from_numpy(synth.synth_slices(SEEDS["x01"], 0, S, H, W))
    noise = torch.from_numpy(synth.noise_z(SEEDS["noise"], 0, 0, S, H, W))
    vol = x01[:, 0].permute(1, 2, 0)[None, None].contiguous()           # [1,1,H,W,D]
    man = {}
    for sname, scfg in STITCH.items():
        for oname, ocfg in OBJECTIVES.items():
            # imageDim 96 / rescaleFactor 3: a 32 x 32 model whose attention_resolutions formula gives (3, 6, 12) -- the middle block only
            cfg = Cfg(imageDim=[96, 96, S], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], test_timesteps=T_TEST, lr=1e-4,
                      **scfg, **ocfg)
            m = mod.DDPM_2D(cfg)
            m.diffusion.model.load_state_dict(sd, strict=True)
            m.diffusion.use_spatial_transformer = False
            m.eval()
            captured, recos = {}, []
            mod._test_step = lambda self, final_volume, *a, **k: captured.update(final_volume=final_volume.clone())
            inner = m.diffusion.forward

            def recording(*a, _inner=inner, **k):
                loss, reco = _inner(*a, **k)
                recos.append(reco.clone())
                return loss, reco
            m.diffusion.forward = recording
            m.on_test_start()
            batch = {"Dataset": "synthetic", "vol": {"data": vol}, "vol_orig": {"data": vol}, "seg_orig": {"data": vol},
                     "mask_orig": {"data": torch.ones_like(vol)}, "seg_available": False, "ID": ["0"], "age": 0, "stage": "test", "label": 0}
            K = int(m.boxes.sample_grid(x01).shape[1])
            with torch.no_grad(), R.injected_randn([noise] * K):
                m.test_step(batch, 0)
            key = f"{sname}__{oname}"
            arrays = dict(final_volume=captured["final_volume"].numpy(), loss_diff=np.float32(m.eval_dict["AnomalyScoreRegPerVol"][-1]))
            if oname == "x0_l1_inpaint":
                arrays["recos"] = torch.stack(recos).numpy()              # [K,S,1,H,W]: what each box's forward returned
            np.savez_compressed(os.path.join(OUT, key + ".npz"), **arrays)
            man[key] = dict(cfg={k: v for k, v in cfg.items()}, K=K, t=T_TEST - 1, loss_diff=float(arrays["loss_diff"]))
            print(key, "K", K, "loss_diff", float(arrays["loss_diff"]))
    return man


def main():
    os.makedirs(OUT, exist_ok=True)
    stand_ins()
    from src.utils.patch_sampling import BoxSampler  # type: ignore
    mod = importlib.import_module("src.models.DDPM_2D_patched")
    manifest = dict(
        generator="tools/make_golden_patched.py", torch=torch.__version__, mkl_cbwr=os.environ["MKL_CBWR"], threads=torch.get_num_threads(),
        seeds=SEEDS, slices=S, H=H, W=W,
        source="reference DDPM_2D_patched.DDPM_2D.test_step, imported unmodified with stand-ins for missing modules only; "
               "_test_step replaced by a capture of final_volume; one seeded noise field handed to every box's randn_like",
        boxes=boxes_fixture(BoxSampler), test_step=test_step_fixtures(mod))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
