"""How far torch's own fp32 run of the SparK pre-training step lies from its float64 run, in the metrics of
tests/test_gpu_spark_training.py: the scale the bounds of that test are derived from (4 x these figures).
CPU only. Both runs are tests/spark_reference.py's restatement at synth_spark_state_dict(0); the float64 run differentiates the branch the
fp32 run is on (its activation masks), exactly as the GPU test treats the HIP step.

    python tools/spark_fp32_yardstick.py            # prints one JSON line per case"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import spark_reference as R                                                      # noqa: E402
from spark_step_cases import CASES, case_inputs, step_metrics                   # noqa: E402


def main():
    synth = importlib.import_module("conditioned-diffusion-models-uad_amd.synth")
    torch.set_num_threads(8)
    sd_np = synth.synth_spark_state_dict(0)
    for name in CASES:
        x, active, scales, kw = case_inputs(name)
        runs = {}
        masks = None
        for dtype in (torch.float32, torch.float64):
            sd = R.to_torch(sd_np, dtype)
            leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype == dtype and "running" not in k and k.split(".")[1] not in ("imn_m", "imn_s", "norm_black")}
            stats, acts = {}, {}
            out = R.spark_forward(x.to(dtype), sd, active, drop_scales=scales, stats=stats, act_masks=masks, acts=acts, **kw)
            out["loss"].backward()
            runs[dtype] = dict(loss=out["loss"].detach(), reco=out["reco"].detach(), latent=out["latent"].detach(), stats=stats,
                               grads={k: v.grad for k, v in leaves.items()})
            masks = R.masks_of(acts)
        m = step_metrics(runs[torch.float32], runs[torch.float64])
        print(json.dumps(dict(case=name, **m)))


if __name__ == "__main__":
    main()
