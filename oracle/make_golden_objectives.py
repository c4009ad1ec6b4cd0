"""ORACLE tooling -- build-container only: the `pred_noise` objective (cond_DDPM.py:411-414, :379-383, :612-644) and the
linear beta schedule (cond_DDPM.py:271-275, :326) on the REFERENCE (imported from /root/reference by ref_harness.py).

    python oracle/make_golden_objectives.py        # ~1 min        (--only-noclip: just the two clip_denoised=False cases)

Cases (outputs only; inputs are regenerated from seeds by synth.py):
  pn_loop_B2_32x32_T1000_start8    p_sample_loop, objective pred_noise, 8 steps of a T = 1000 cosine chain
  pn_loop_B2_32x32_T50_start0      p_sample_loop, objective pred_noise, the full T = 50 chain from pure noise
  pn_p_losses_B2_32x32_t499        GaussianDiffusion.forward -> p_losses, pred_noise, loss l2 (BASELINE config 5's loss)
  pn_ddim_B2_32x32_T1000_S10_eta1  ddim_sample, pred_noise, 10 steps, eta 1
  lin_loop_B2_32x32_T1000_start8   p_sample_loop, pred_x0, beta_schedule 'linear', 8 steps
  lin_schedule_T1000               the 13 buffers of the linear schedule
  noclip_p_sample_B2_32x32_t5, noclip_ddim_B2_32x32_T1000_S10_eta1     clip_denoised=False (one step / a DDIM chain)
The manifest records max|oracle - reference| per case.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")     # the MKL code path tests/conftest.py pins: the same bits on any x86 host

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
synth = importlib.import_module("conditioned-diffusion-models-uad_amd.synth")
import cddpm_oracle as O  # noqa: E402
import ref_harness as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SEED_W, SEED_COND, SEED_XT, SEED_Z = 0, 1, 2, 3


def build(sd, H, W, timesteps, objective, beta_schedule="cosine", loss_type="l1"):
    UNetModel, GaussianDiffusion = R.import_reference()
    model, _d = R.build_reference(sd, image_size=(H, W), timesteps=timesteps, objective=objective)
    diff = GaussianDiffusion(model, image_size=(H, W), timesteps=timesteps, sampling_timesteps=timesteps,
                             objective=objective, beta_schedule=beta_schedule, channels=1, loss_type=loss_type,
                             p2_loss_weight_gamma=0, cfg=None)
    diff.use_spatial_transformer = False
    diff.eval()
    return model, diff


def loop(sd, name, H, W, B, timesteps, start_t, objective, beta_schedule="cosine"):
    _m, diff = build(sd, H, W, timesteps, objective, beta_schedule)
    T = timesteps if start_t == 0 else start_t
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, 0, B))
    xT = torch.from_numpy(synth.noise_xT(SEED_XT, 0, B, H, W))
    zs = {t: torch.from_numpy(synth.noise_z(SEED_Z, t, 0, B, H, W)) for t in range(1, T)}
    with R.injected_randn([xT] + [zs[t] for t in range(T - 1, 0, -1)]):
        ref = diff.p_sample_loop((B, 1, H, W), cond=cond, start_t=start_t)
    buf = O.schedule_buffers(timesteps, beta_schedule)
    ora = O.p_sample_loop(xT, cond, sd, buf, lambda t: zs[t], start_t=start_t, objective=objective)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), out=ref.numpy())
    return dict(H=H, W=W, B=B, timesteps=timesteps, start_t=start_t, objective=objective, beta_schedule=beta_schedule,
                oracle_vs_reference_maxabs=float((ref - ora).abs().max()))


def noclip_cases(sd, cases):
    """clip_denoised=False (cond_DDPM.py:433, :467, :416-419, :426-427, :493): one p_sample step at t = 5 and a 10-step
    DDIM chain, pred_x0; the synthetic UNet's raw prediction leaves [-1,1], so the flag matters (asserted)."""
    B, H, W, T = 2, 32, 32, 1000
    _m, diff = build(sd, H, W, T, "pred_x0")
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, 0, B))
    x = torch.from_numpy(synth.noise_xT(SEED_XT, 0, B, H, W))
    z = torch.from_numpy(synth.noise_z(SEED_Z, 5, 0, B, H, W))
    with R.injected_randn([z]):
        ref = diff.p_sample(x.clone(), 5, clip_denoised=False, cond=cond)
    with R.injected_randn([z]):
        ref_clip = diff.p_sample(x.clone(), 5, clip_denoised=True, cond=cond)
    assert float((ref - ref_clip).abs().max()) > 1e-3, float((ref - ref_clip).abs().max())
    ora = O.p_sample(x, 5, cond, sd, O.schedule_buffers(T), z, clip_denoised=False)
    np.savez_compressed(os.path.join(GOLD, "noclip_p_sample_B2_32x32_t5.npz"), out=ref.numpy())
    cases["noclip_p_sample_B2_32x32_t5"] = dict(H=H, W=W, B=B, timesteps=T, t=5, clip_denoised=False,
                                                  oracle_vs_reference_maxabs=float((ref - ora).abs().max()))
    S, eta = 10, 1.0
    diff.sampling_timesteps, diff.is_ddim_sampling, diff.ddim_sampling_eta = S, True, eta
    diff.cfg = types.SimpleNamespace(noisetype="gauss")
    pairs = O.ddim_time_pairs(T, S, 0)
    zs = {time: torch.from_numpy(synth.noise_z(SEED_Z, time, 0, B, H, W)) for time, nxt in pairs if nxt > 0}
    with R.injected_randn([torch.zeros(B, 1, H, W), x] + [zs[time] for time, nxt in pairs if nxt > 0]):
        ref = diff.ddim_sample((B, 1, H, W), clip_denoised=False, cond=cond, x_start=None, start_t=0)
    ora = O.ddim_sample(x, cond, sd, O.schedule_buffers(T), lambda t: zs[t], S, eta, 0, None, clip_denoised=False)
    np.savez_compressed(os.path.join(GOLD, "noclip_ddim_B2_32x32_T1000_S10_eta1.npz"), out=ref.numpy())
    cases["noclip_ddim_B2_32x32_T1000_S10_eta1"] = dict(H=H, W=W, B=B, timesteps=T, S=S, eta=eta, clip_denoised=False,
                                                        oracle_vs_reference_maxabs=float((ref - ora).abs().max()))
    for k in ("noclip_p_sample_B2_32x32_t5", "noclip_ddim_B2_32x32_T1000_S10_eta1"):
        print(k, cases[k]["oracle_vs_reference_maxabs"], flush=True)


def main():
    torch.manual_seed(0)
    sd = O.to_torch_sd(synth.synth_state_dict(SEED_W))
    mpath = os.path.join(GOLD, "MANIFEST.json")
    manifest = json.load(open(mpath))
    cases = manifest["cases"]
    if "--only-noclip" in sys.argv:
        noclip_cases(sd, cases)
        manifest = json.load(open(mpath))          # (another generator may have written meanwhile: merge, do not overwrite)
        for k in ("noclip_p_sample_B2_32x32_t5", "noclip_ddim_B2_32x32_T1000_S10_eta1"):
            manifest["cases"][k] = cases[k]
        json.dump(manifest, open(mpath, "w"), indent=1, sort_keys=True)
        return
    noclip_cases(sd, cases)

    cases["pn_loop_B2_32x32_T1000_start8"] = loop(sd, "pn_loop_B2_32x32_T1000_start8", 32, 32, 2, 1000, 8, "pred_noise")
    cases["pn_loop_B2_32x32_T50_start0"] = loop(sd, "pn_loop_B2_32x32_T50_start0", 32, 32, 2, 50, 0, "pred_noise")
    cases["lin_loop_B2_32x32_T1000_start8"] = loop(sd, "lin_loop_B2_32x32_T1000_start8", 32, 32, 2, 1000, 8, "pred_x0", "linear")

    # linear schedule buffers
    _m, diff = build(sd, 32, 32, 1000, "pred_x0", "linear")
    names = list(O.schedule_buffers(1000, "linear").keys())
    np.savez_compressed(os.path.join(GOLD, "lin_schedule_T1000.npz"), **{n: getattr(diff, n).numpy() for n in names})
    ob = O.schedule_buffers(1000, "linear")
    cases["lin_schedule_T1000"] = {"buffers": names, "oracle_vs_reference_maxabs":
                                   max(float((getattr(diff, n) - ob[n]).abs().max()) for n in names)}

    # single-step reconstruction under pred_noise, l2 loss
    B, H, W = 2, 32, 32
    _m, diff = build(sd, H, W, 1000, "pred_noise", loss_type="l2")
    x01 = torch.from_numpy(synth.synth_slices(SEED_XT, 0, B, H, W))
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, 0, B))
    noise = torch.from_numpy(synth.noise_z(SEED_Z, 0, 0, B, H, W))
    with torch.no_grad():
        loss, reco = diff(x01, t=499, cond=cond, noise=noise)
    ol, orc = O.p_losses_recon(x01, torch.full((B,), 499, dtype=torch.long), cond, noise, sd, O.schedule_buffers(1000),
                               objective="pred_noise", loss_type="l2")
    np.savez_compressed(os.path.join(GOLD, "pn_p_losses_B2_32x32_t499.npz"), loss=loss.numpy(), reco=reco.numpy())
    cases["pn_p_losses_B2_32x32_t499"] = {"objective": "pred_noise", "loss_type": "l2",
                                          "oracle_vs_reference_maxabs": float((reco - orc).abs().max()),
                                          "loss_absdiff": float((loss - ol).abs())}

    # DDIM under pred_noise
    T, S, eta = 1000, 10, 1.0
    _m, diff = build(sd, H, W, T, "pred_noise")
    diff.sampling_timesteps, diff.is_ddim_sampling, diff.ddim_sampling_eta = S, True, eta
    diff.cfg = types.SimpleNamespace(noisetype="gauss")          # read at cond_DDPM.py:502
    xT = torch.from_numpy(synth.noise_xT(SEED_XT, 0, B, H, W))
    pairs = O.ddim_time_pairs(T, S, 0)
    zs = {time: torch.from_numpy(synth.noise_z(SEED_Z, time, 0, B, H, W)) for time, nxt in pairs if nxt > 0}
    with R.injected_randn([torch.zeros(B, 1, H, W), xT] + [zs[time] for time, nxt in pairs if nxt > 0]):
        ref = diff.ddim_sample((B, 1, H, W), cond=cond, x_start=None, start_t=0)
    ora = O.ddim_sample(xT, cond, sd, O.schedule_buffers(T), lambda t: zs[t], S, eta, 0, None, objective="pred_noise")
    np.savez_compressed(os.path.join(GOLD, "pn_ddim_B2_32x32_T1000_S10_eta1.npz"), out=ref.numpy())
    cases["pn_ddim_B2_32x32_T1000_S10_eta1"] = dict(H=H, W=W, B=B, timesteps=T, S=S, eta=eta, start_t=0, objective="pred_noise",
                                                    oracle_vs_reference_maxabs=float((ref - ora).abs().max()),
                                                    time_pairs=[list(p) for p in pairs])
    for k in ("pn_loop_B2_32x32_T1000_start8", "pn_loop_B2_32x32_T50_start0", "lin_loop_B2_32x32_T1000_start8",
              "lin_schedule_T1000", "pn_p_losses_B2_32x32_t499", "pn_ddim_B2_32x32_T1000_S10_eta1"):
        print(k, cases[k].get("oracle_vs_reference_maxabs"), flush=True)
    json.dump(manifest, open(mpath, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
