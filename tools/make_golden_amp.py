"""Fixtures of the REFERENCE under fp16 autocast (tests/golden/amp/): what its users get at test time with the Trainer's
`precision: 16` (configs/trainer/default.yaml; Lightning wraps test_step / validation_step in autocast), and the yardstick of the
engine's precision-16 reconstruction (tests/test_gpu_precision16.py).

Build container only (the reference tree does not travel to the GPU machine). The reference is imported UNMODIFIED through
oracle/ref_harness.py and run under `torch.autocast("cpu", dtype=torch.float16)`: conv2d, conv1d, linear and einsum come back fp16,
GroupNorm32 and the softmax compute in float, as on a GPU. Same seeds, weights and inputs as the fp32 fixtures of tests/golden
(oracle/make_golden.py, oracle/make_golden_arch.py); output arrays only.

    unet_fwd_B2_32x32.npz            t500, tmixed    the experiment's descriptor (128 x (1, 2, 2), three ResBlocks) at 2 x 32 x 32
    arch_<case>.npz                  t500, tmixed    tests/arch_cases.py: attn_levels, deep4, cond4 at their own geometries
    loop_B2_32x32_T1000_start8.npz   out             p_sample_loop with injected noise
    patched_p16_paste__x0_l1_inpaint.npz  final_volume   the patched DDPM's test_step at the smallest geometry of tests/golden/patched
                                                     (3 slices of 32 x 32, four 16 x 16 boxes, t = 350), made as
                                                     tools/make_golden_patched.py makes its fp32 counterpart

Every recorded array must be finite (an overflow would make the fixture measure a range exit, not rounding): a case that is not is
dropped, named in MANIFEST.json under "dropped", and the run ends with a non-zero status.

    python tools/make_golden_amp.py          # seconds to a minute on 8 threads
"""
import importlib
import json
import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")     # the MKL code path tests/conftest.py pins

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import arch_cases as A  # noqa: E402
import cddpm_oracle as O  # noqa: E402
import ref_harness as R  # noqa: E402
from make_golden_arch import save_npz  # noqa: E402  (fixed zip timestamps: a second run reproduces the bytes)

synth = importlib.import_module("conditioned-diffusion-models-uad_amd.synth")
OUT = os.path.join(ROOT, "tests", "golden", "amp")
SEED_W, SEED_COND, SEED_XT, SEED_Z = 0, 1, 2, 3      # the seeds of every other fixture under tests/golden
ARCH = ("attn_levels", "deep4", "cond4")
LOOP = dict(H=32, W=32, B=2, timesteps=1000, start_t=8)


def autocast():
    return torch.autocast("cpu", dtype=torch.float16)


def forward_case(model, x, cond, B):
    """the reference UNet under autocast at the two recorded timestep vectors -> {key: float32 array}, {key: output dtype}"""
    outs, dtypes = {}, {}
    for key in A.GOLDEN_T:
        with torch.no_grad(), autocast():
            r = model(x, A.timesteps(key, B), cond=cond)
        dtypes[key] = str(r.dtype)
        outs[key] = r.float().numpy()
    return outs, dtypes


def experiment_case():
    B, H, W = 2, 32, 32
    sd = O.to_torch_sd(synth.synth_state_dict(SEED_W))
    model, _d = R.build_reference(sd, image_size=(H, W), timesteps=1000)
    x = torch.from_numpy(synth.noise_xT(SEED_XT, 0, B, H, W))
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, 0, B))
    outs, dtypes = forward_case(model, x, cond, B)
    return outs, dict(B=B, H=H, W=W, timesteps={k: A.timesteps(k, B).tolist() for k in A.GOLDEN_T}, output_dtype=dtypes)


def arch_case(name):
    case = A.CASES[name]
    B, H, W = case["geometry"]
    kw = A.synth_kw(case)
    sd = O.to_torch_sd(synth.synth_state_dict(A.SEED_W, **kw))
    model, _d = R.build_reference(sd, image_size=(H, W), timesteps=1000, model_channels=kw["model_channels"],
                                  channel_mult=kw["channel_mult"], num_classes=kw["num_classes"], num_res_blocks=kw["num_res_blocks"],
                                  attention_resolutions=kw["attention_resolutions"])
    model.eval()
    x, cond = A.inputs(synth, case)
    outs, dtypes = forward_case(model, x, cond, B)
    return outs, dict(B=B, H=H, W=W, timesteps={k: A.timesteps(k, B).tolist() for k in A.GOLDEN_T}, output_dtype=dtypes)


def loop_case(H, W, B, timesteps, start_t):
    """oracle/make_golden.py::loop_case with the whole p_sample_loop inside the autocast region, as Lightning's test_step is"""
    sd = O.to_torch_sd(synth.synth_state_dict(SEED_W))
    _model, diff = R.build_reference(sd, image_size=(H, W), timesteps=timesteps)
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, 0, B))
    xT = torch.from_numpy(synth.noise_xT(SEED_XT, 0, B, H, W))
    zs = {t: torch.from_numpy(synth.noise_z(SEED_Z, t, 0, B, H, W)) for t in range(1, start_t)}
    draws = [xT] + [zs[t] for t in range(start_t - 1, 0, -1)]
    with torch.no_grad(), autocast(), R.injected_randn(draws):
        ref = diff.p_sample_loop((B, 1, H, W), cond=cond, start_t=start_t)
    return {"out": ref.float().numpy()}, dict(LOOP, output_dtype=str(ref.dtype))


PATCHED = ("p16_paste", "x0_l1_inpaint")


def patched_case():
    """tools/make_golden_patched.py::test_step_fixtures for one (stitch, objective) pair, test_step called inside the autocast region"""
    import make_golden_patched as MP
    MP.stand_ins()
    mod = importlib.import_module("src.models.DDPM_2D_patched")
    sname, oname = PATCHED
    sd = O.to_torch_sd(synth.synth_state_dict(MP.SEEDS["weights"], num_classes=None))
    x01 = torch.from_numpy(synth.synth_slices(MP.SEEDS["x01"], 0, MP.S, MP.H, MP.W))
    noise = torch.from_numpy(synth.noise_z(MP.SEEDS["noise"], 0, 0, MP.S, MP.H, MP.W))
    vol = x01[:, 0].permute(1, 2, 0)[None, None].contiguous()           # [1,1,H,W,D]
    cfg = MP.Cfg(imageDim=[96, 96, MP.S], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], test_timesteps=MP.T_TEST, lr=1e-4,
                 **MP.STITCH[sname], **MP.OBJECTIVES[oname])
    m = mod.DDPM_2D(cfg)
    m.diffusion.model.load_state_dict(sd, strict=True)
    m.diffusion.use_spatial_transformer = False
    m.eval()
    captured = {}
    mod._test_step = lambda self, final_volume, *a, **k: captured.update(final_volume=final_volume.clone())
    m.on_test_start()
    batch = {"Dataset": "synthetic", "vol": {"data": vol}, "vol_orig": {"data": vol}, "seg_orig": {"data": vol},
             "mask_orig": {"data": torch.ones_like(vol)}, "seg_available": False, "ID": ["0"], "age": 0, "stage": "test", "label": 0}
    K = int(m.boxes.sample_grid(x01).shape[1])
    with torch.no_grad(), autocast(), R.injected_randn([noise] * K):
        m.test_step(batch, 0)
    fv = captured["final_volume"]
    return {"final_volume": fv.float().numpy()}, dict(K=K, t=MP.T_TEST - 1, slices=MP.S, H=MP.H, W=MP.W, seeds=MP.SEEDS,
                                                       cfg={k: v for k, v in cfg.items()}, output_dtype=str(fv.dtype))


def main():
    os.makedirs(OUT, exist_ok=True)
    jobs = [("unet_fwd_B2_32x32", experiment_case)] + [("arch_" + n, lambda n=n: arch_case(n)) for n in ARCH]
    jobs.append(("loop_B2_32x32_T1000_start8", lambda: loop_case(**LOOP)))
    jobs.append(("patched_" + "__".join(PATCHED), patched_case))
    cases, dropped = {}, []
    for name, fn in jobs:
        arrays, entry = fn()
        bad = [k for k, v in arrays.items() if not np.isfinite(v).all()]
        if bad:
            dropped.append(dict(case=name, non_finite=bad))
            print(name, "DROPPED: non-finite", bad, flush=True)
            continue
        save_npz(os.path.join(OUT, name + ".npz"), **arrays)
        entry["max_abs"] = {k: float(np.abs(v).max()) for k, v in arrays.items()}
        cases[name] = entry
        print(name, entry["max_abs"], flush=True)
    manifest = dict(generator="tools/make_golden_amp.py", torch=torch.__version__, mkl_cbwr=os.environ["MKL_CBWR"],
                    threads=torch.get_num_threads(), autocast="torch.autocast('cpu', dtype=torch.float16)",
                    seeds=dict(weights=SEED_W, cond=SEED_COND, xT=SEED_XT, z=SEED_Z),
                    source="reference UNetModel.forward / GaussianDiffusion.p_sample_loop, imported unmodified (oracle/ref_harness.py), "
                           "called inside the autocast region; outputs converted to float32 (exact)",
                    cases=cases, dropped=dropped)
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    assert not dropped, dropped


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
