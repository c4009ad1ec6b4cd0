"""The two whole-step cases of SparK pre-training that tests/test_gpu_spark_training.py checks against float64 autograd and
tools/spark_fp32_yardstick.py measures torch's own fp32 arithmetic on, with the metrics both use (those of
tests/test_gpu_encoder_training.py: every error is the largest absolute difference over the reference's largest magnitude, per tensor)."""
import numpy as np
import torch

import spark_reference as R

MASK_RATIO = 0.65
CASES = {
    # name: (B, side, loss_on_mask, delta_mask, drop scales given)
    "b12_64": (12, 64, True, 0.0, False),
    "b4_96": (4, 96, False, 0.5, True),
}


def case_inputs(name):
    """-> x [B,1,S,S] fp32 in [0, 1], active bool [B,1,f,f] (the reference's draw under the case's seed), drop scales, forward keywords"""
    B, S, on_mask, delta, drop = CASES[name]
    torch.manual_seed(B + S)
    x = torch.rand(B, 1, S, S)
    active = R.draw_mask(B, S // 32, MASK_RATIO)
    scales = None
    if drop:        # two blocks with a dropped / rescaled residual branch for some samples
        scales = {"layer2.1": torch.tensor([1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9]), "layer4.2": torch.tensor([0.0, 1 / 0.95, 1 / 0.95, 0.0])}
    return x, active, scales, dict(loss_on_mask=on_mask, delta_mask=delta)


def rel(got, want):
    want = want.double()
    return float((got.double().reshape(want.shape) - want).abs().max() / (want.abs().max() + 1e-30))


def step_metrics(got, want):
    """got, want: dict(loss, reco, latent, stats {name: tensor}, grads {name: tensor}) -> the figures the bounds are stated in"""
    per = sorted(((rel(got["grads"][k], g), k) for k, g in want["grads"].items() if g is not None), reverse=True)
    return dict(loss=rel(got["loss"], want["loss"]), reco=rel(got["reco"], want["reco"]), latent=rel(got["latent"], want["latent"]),
                running=max(rel(got["stats"][k], v) for k, v in want["stats"].items()),
                grad_worst=per[0][0], grad_worst_name=per[0][1], grad_median=float(np.median([e for e, _ in per])), grad_tensors=len(per))
