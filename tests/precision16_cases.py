"""What the precision-16 tests share (tests/test_precision16_host.py, tests/test_gpu_precision16.py): the four UNet cases of the AMP
fixtures (tests/golden/amp/, tools/make_golden_amp.py), their inputs, and per case the three CPU references every acceptance is
stated in -- the float64 oracle (the truth), the fp32 oracle, and the recorded output of the reference under fp16 autocast. Each
reference is computed once per process and never modified.

Acceptance of a precision-16 result `got` (the rule of the issue): against the float64 oracle, rms error <= 1.0 x the AMP fixture's
rms distance from the same float64 output and max error <= 2 x its max distance -- the engine rounds a strict subset of what fp16
autocast rounds (its accumulators, GroupNorm inputs and outputs stay fp32), so it gets no margin on rms; a maximum over ~10^3..10^4
similar errors scatters by tens of percent, hence the 2 on max."""
import functools
import importlib
import os

import numpy as np
import torch

import arch_cases as A
from conftest import GOLD

AMP = os.path.join(GOLD, "amp")
# the experiment's descriptor at 2 x 32 x 32 (the geometry of tests/golden/unet_fwd_B2_32x32.npz) in the form of an arch_cases case
EXPERIMENT = dict(model_channels=128, channel_mult=(1, 2, 2), num_res_blocks=3, attention_resolutions=A.DEFAULT_ATT, cond_dim=128,
                  geometry=(2, 32, 32))
FIXTURES = {"experiment": "unet_fwd_B2_32x32", "attn_levels": "arch_attn_levels", "deep4": "arch_deep4", "cond4": "arch_cond4"}
CHAIN = dict(name="loop_B2_32x32_T1000_start8", B=2, H=32, W=32, timesteps=1000, start_t=8)
SEED_Z = 3


def case(name):
    return EXPERIMENT if name == "experiment" else A.CASES[name]


def rms(d):
    return float(torch.as_tensor(d).double().pow(2).mean().sqrt())


def amp_fixture(fixture):
    return np.load(os.path.join(AMP, fixture + ".npz"))


def _synth():
    return importlib.import_module("conditioned-diffusion-models-uad_amd.synth")


@functools.lru_cache(maxsize=None)
def forward_refs(name):
    """{t-key: dict(r64=, r32=, amp=)} of a case, [B,1,H,W] each (r64 float64). The two timestep vectors go through the oracle as
    one batch of 2 B samples (every operation of the UNet is per sample)."""
    import cddpm_oracle as O
    synth, c = _synth(), case(name)
    B = c["geometry"][0]
    sd = O.to_torch_sd(synth.synth_state_dict(A.SEED_W, **A.synth_kw(c)))
    x, cond = A.inputs(synth, c)
    x2, cond2 = torch.cat([x, x]), None if cond is None else torch.cat([cond, cond])
    t2 = torch.cat([A.timesteps(k, B) for k in A.GOLDEN_T])
    with torch.no_grad():
        r32 = O.unet_forward(x2, t2, cond2, sd, **A.unet_kw(c))
        r64 = O.unet_forward(x2.double(), t2, None if cond2 is None else cond2.double(), O.to_float64(sd), **A.unet_kw(c))
    amp = amp_fixture(FIXTURES[name])
    return {k: dict(r64=r64[i * B:(i + 1) * B], r32=r32[i * B:(i + 1) * B], amp=torch.from_numpy(amp[k])) for i, k in enumerate(A.GOLDEN_T)}


def chain_inputs():
    """(x_T, cond, noise [start_t, B, 1, H, W] with z_t at index t) of the recorded 8-step chain"""
    synth = _synth()
    B, H, W, T = CHAIN["B"], CHAIN["H"], CHAIN["W"], CHAIN["start_t"]
    x = torch.from_numpy(synth.noise_xT(A.SEED_X, 0, B, H, W))
    cond = torch.from_numpy(synth.synth_cond(A.SEED_COND, 0, B))
    noise = torch.zeros(T, B, 1, H, W)
    for t in range(1, T):
        noise[t] = torch.from_numpy(synth.noise_z(SEED_Z, t, 0, B, H, W))
    return x, cond, noise


@functools.lru_cache(maxsize=None)
def chain_refs():
    """dict(r64=, r32=, amp=) of the chain: the float64 oracle, the fp32 reference fixture, the AMP reference fixture"""
    import cddpm_oracle as O
    synth = _synth()
    sd = O.to_torch_sd(synth.synth_state_dict(A.SEED_W))
    x, cond, noise = chain_inputs()
    buf = O.schedule_buffers(CHAIN["timesteps"])
    with torch.no_grad():
        r64 = O.p_sample_loop(x.double(), cond.double(), O.to_float64(sd), O.to_float64(buf), lambda t: noise[t].double(),
                              start_t=CHAIN["start_t"])
    r32 = torch.from_numpy(np.load(os.path.join(GOLD, CHAIN["name"] + ".npz"))["out"])
    return dict(r64=r64, r32=r32, amp=torch.from_numpy(amp_fixture(CHAIN["name"])["out"]))


PATCHED = dict(name="patched_p16_paste__x0_l1_inpaint", fp32="p16_paste__x0_l1_inpaint", S=3, H=32, W=32, patch_size=16, t=350,
               seeds=dict(weights=0, x01=2, noise=3))        # tools/make_golden_patched.py


def patched_inputs():
    """(x01 [S,1,H,W] in [0,1], noise [S,1,H,W]) of the patched DDPM's recorded test_step"""
    synth, c = _synth(), PATCHED
    x01 = torch.from_numpy(synth.synth_slices(c["seeds"]["x01"], 0, c["S"], c["H"], c["W"])).reshape(c["S"], 1, c["H"], c["W"])
    noise = torch.from_numpy(synth.noise_z(c["seeds"]["noise"], 0, 0, c["S"], c["H"], c["W"])).reshape(c["S"], 1, c["H"], c["W"])
    return x01, noise


@functools.lru_cache(maxsize=None)
def patched_refs():
    """dict(r64=, r32=, amp=) [S,1,H,W] of that test_step (pred_x0, inpaint, 16 x 16 boxes pasted). r64 restates it in float64: per
    box the UNet sees x0 = 2 x01 - 1 with q_sample(x0, t, noise) pasted into the box, its output is pasted into x0 inside the box,
    mapped to [0,1], and the boxes (a partition of the image) are pasted into the volume; all K S forwards as one oracle batch."""
    import cddpm_oracle as O
    synth, c = _synth(), PATCHED
    S, H, W, t = c["S"], c["H"], c["W"], c["t"]
    x01, noise = patched_inputs()
    boxes = importlib.import_module("conditioned-diffusion-models-uad_amd.patch_sampling").BoxSampler(
        dict(patch_size=c["patch_size"])).sample_grid(x01)                                       # [S,K,4] rows (x0, y1, x2, y3)
    K = boxes.shape[1]
    buf = O.to_float64(O.schedule_buffers(1000))
    x0, nz = x01.double() * 2 - 1, noise.double()
    q = buf["sqrt_alphas_cumprod"][t] * x0 + buf["sqrt_one_minus_alphas_cumprod"][t] * nz
    ys, xs = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    masks = []
    for k in range(K):
        b = boxes[:, k].long().view(S, 4, 1, 1, 1)
        masks.append((xs >= b[:, 0]) & (xs < b[:, 2]) & (ys >= b[:, 1]) & (ys < b[:, 3]))
    sd64 = O.to_float64(O.to_torch_sd(synth.synth_state_dict(c["seeds"]["weights"], num_classes=None)))
    with torch.no_grad():
        out = O.unet_forward(torch.cat([torch.where(m, q, x0) for m in masks]), torch.full((K * S,), t, dtype=torch.long), None, sd64)
    r64 = torch.zeros_like(x0)
    for k, m in enumerate(masks):
        r64 = torch.where(m, (out[k * S:(k + 1) * S] + 1) * 0.5, r64)
    vol = lambda a: torch.from_numpy(a)[0, 0].permute(2, 0, 1).unsqueeze(1).contiguous()         # [1,1,H,W,D] -> [D,1,H,W]
    r32 = vol(np.load(os.path.join(GOLD, "patched", c["fp32"] + ".npz"))["final_volume"])
    return dict(r64=r64, r32=r32, amp=vol(amp_fixture(c["name"])["final_volume"]))


def acceptance(got, ref):
    """(rms error, max error, AMP rms, AMP max, passes) of `got` against ref = dict(r64=, amp=); NaN fails"""
    d = got.detach().cpu().double() - ref["r64"]
    y = ref["amp"].double() - ref["r64"]
    e_rms, e_max, y_rms, y_max = rms(d), float(d.abs().max()), rms(y), float(y.abs().max())
    return e_rms, e_max, y_rms, y_max, bool(np.isfinite(e_rms) and e_rms <= 1.0 * y_rms and e_max <= 2.0 * y_max)


def format_acceptance(label, row):
    e_rms, e_max, y_rms, y_max, ok = row
    return (f"{label}: rms {e_rms:.3e} / AMP reference {y_rms:.3e} = {e_rms / y_rms:.3f}   max {e_max:.3e} / {y_max:.3e} = "
            f"{e_max / y_max:.3f}   {'ok' if ok else 'FAIL'}")
