"""Worst / median relative error of the training step's gradients against float64 autograd through the oracle, as JSON (one process per
arithmetic: the families are chosen once per process from the environment, e.g. CDDPM_TRAIN_PRECISION=16).
usage: python tools/train_grad_check.py [--attention-precision 16|32] [--attention-family f32|h3] [--gradient NAME] [--encoder-precision 16|32 --joint-steps N]
                                        [B H W [DESCRIPTOR]]
--attention-precision: UNetTrainer's attention_precision (16: the fp16-MFMA attention forward and backward; default 32).
--attention-family: UNetTrainer's attention_family, read where the attention precision is 32 (h3: fp32-grade fp16 splits; default f32).
--joint-steps N: instead of the gradient check, N joint optimisation steps (training_step(..., encoder=enc)) on one fixed batch with the
context encoder built at --encoder-precision (EncoderTrainer's precision) and dynamic loss scaling on; reports each step's loss, which
steps the guard skipped, skipped_steps and the final loss_scale.
--gradient NAME: also report "gradient_sha256", the digest of that parameter's gradient bits (to tell two arithmetics apart).
DESCRIPTOR: a JSON object {"model_channels":, "channel_mult":, "num_res_blocks":, "cond_dim":, "attention_resolutions":} of another UNet
than the experiment's (cond_dim 0: unconditioned; attention_resolutions absent: the experiment's (3, 6, 12), attention in the middle
block only)"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
PKG = "conditioned-diffusion-models-uad_amd"
import cddpm_oracle as oracle  # noqa: E402  (test infrastructure: this tool is a checker, not product code)

_ap = argparse.ArgumentParser()
_ap.add_argument("--attention-precision", default="32")
_ap.add_argument("--attention-family", default="f32")
_ap.add_argument("--gradient", default=None)
_ap.add_argument("--encoder-precision", default="32")
_ap.add_argument("--joint-steps", type=int, default=0)
_ap.add_argument("rest", nargs="*")
_a = _ap.parse_args()
sys.argv[1:] = _a.rest
B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (2, 32, 32)
tr, synth, sched = (importlib.import_module(PKG + "." + m) for m in ("training", "synth", "schedule"))
T = 1000
desc = json.loads(sys.argv[4]) if len(sys.argv) >= 5 else {}
arch = {k: (tuple(desc[k]) if k in ("channel_mult", "attention_resolutions") else desc[k])
        for k in ("model_channels", "channel_mult", "num_res_blocks", "attention_resolutions") if k in desc}
cond_dim = desc.get("cond_dim", 128)
encoder_precision = importlib.import_module(PKG + ".engine").precision_bits(_a.encoder_precision)
if _a.joint_steps > 0:
    et = importlib.import_module(PKG + ".encoder_training")
    dev = torch.device("cuda", 0)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, **arch).items()}, device=dev,
                             attention_precision=_a.attention_precision, attention_family=_a.attention_family, **arch)
    trainer.enable_loss_scaling()
    enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, trainer, precision=encoder_precision)
    x01 = torch.from_numpy(synth.synth_slices(3, 0, B, H, W)).reshape(B, 1, H, W).to(dev)
    noise = torch.from_numpy(synth.noise_xT(3, 0, B, H, W)).reshape(B, 1, H, W).to(dev)
    t = torch.tensor([(137 * (i + 1) + 3) % T for i in range(B)], dtype=torch.long, device=dev)
    losses, skipped = [], []
    for _ in range(_a.joint_steps):
        before = trainer.skipped_steps
        losses.append(float(tr.training_step(trainer, x01, None, t=t, noise=noise, objective="pred_noise", loss_type="l2", encoder=enc)))
        skipped.append(trainer.skipped_steps > before)
    print(json.dumps({"losses": losses, "skipped": skipped, "skipped_steps": trainer.skipped_steps, "step_count": trainer.step_count,
                      "loss_scale": trainer.loss_scale, "precision": tr.get_precision(), "attention_precision": trainer.attention_precision,
                      "encoder_precision": enc.precision, "finite_parameters": bool(torch.isfinite(enc.flat).all() and torch.isfinite(trainer.flat).all())}))
    sys.exit(0)
sd_np = synth.synth_state_dict(0, num_classes=cond_dim or None, **arch)
x01 = torch.from_numpy(synth.synth_slices(3, 0, B, H, W)).reshape(B, 1, H, W)
cond = torch.from_numpy(synth.synth_cond(3, 0, B, cond_dim)) if cond_dim else None
noise = torch.from_numpy(synth.noise_xT(3, 0, B, H, W)).reshape(B, 1, H, W)
t = torch.tensor([(137 * (i + 1) + 3) % T for i in range(B)], dtype=torch.long)
sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
buf64 = oracle.to_float64(oracle.schedule_buffers(T))
x0 = x01 * 2 - 1
ref_out = oracle.unet_forward(oracle.q_sample(x0.double(), t, noise.double(), buf64), t, cond.double() if cond_dim else None, sd, **arch)
dev = torch.device("cuda", 0)
trainer = tr.UNetTrainer({k: torch.from_numpy(v) for k, v in sd_np.items()}, device=dev, cond_dim=cond_dim or None,
                         attention_precision=_a.attention_precision, attention_family=_a.attention_family, **arch)
buf = sched.schedule_buffers(T)
xt = buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise
out = trainer.forward(xt.to(dev), t.to(dev), cond.to(dev) if cond_dim else None)
loss, dout = trainer.loss_and_grad(out, noise.to(dev), buf["p2_loss_weight"][t].to(dev).contiguous(), "l2")
grads = trainer.backward(dout)
torch.cuda.synchronize()
S = trainer.grad_scale
ref_out.backward(dout.double().cpu() / S)
errs = []
for k, v in sd.items():
    g = grads[k].double().cpu().reshape(v.grad.shape) / S
    errs.append(float((g - v.grad).abs().max() / (v.grad.abs().max() + 1e-30)))
res = {"forward_max_abs_err": float((out.double().cpu() - ref_out.detach()).abs().max()), "worst": max(errs), "median": float(np.median(errs)),
       "finite": bool(np.isfinite(errs).all()), "n": len(errs), "attention_precision": trainer.attention_precision,
       "attention_family": trainer.attention_family,
       "encoder_precision": encoder_precision}
if _a.gradient:
    res["gradient_sha256"] = hashlib.sha256(grads[_a.gradient].detach().cpu().contiguous().numpy().tobytes()).hexdigest()
print(json.dumps(res))
