"""Times one batch of 32 augmented training slices from a resident bank of 96 x 96 x 50 volumes (CddpmEngine.augment_slices: the host check
of the two tables, their one asynchronous copy and cddpm_aug_slices, csrc/augment.hip). Two batches: the recipe's own draw
(IntensityAugment.draw: gamma p=.5, bias p=.25, blur p=.25, ghosting p=.5) and the worst case, every stage on in every sample.
Method: `--warmup` calls, then `--reps` calls each between two device events on the engine's stream, the median and the minimum of
those; the workspace is sized by the warm-up. Needs an MI355X: no device, no number. No target is set: what is measured is recorded.
The wall time of the float32 numpy / scipy restatement of the same 32 samples (tests/augment_reference.py) on this host's CPU with
`--threads` threads is printed beside it for scale only: another algorithm on another processor, no comparison of kernels.

`--recipe pipeline` times the eleven-slot pipeline the same way (CddpmEngine.augment_pipeline, cddpm_aug_pipeline): SliceAugment's own draw
(bias p=.25, noise, ghosting, blur, gamma, affine p=.5, flip p=.25, then the policy group) and every slot on in every sample, beside
the restatement of tests/augment_pipeline_reference.py, and writes profiles/augment_pipeline_bench.json.

    python tools/augment_bench.py [--reps 50] [--recipe intensity|pipeline] [--out profiles/augment_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "conditioned-diffusion-models-uad_amd"
SHAPE, VOLUMES, BATCH = (96, 96, 50), 16, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--recipe", choices=("intensity", "pipeline"), default="intensity")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pipe = a.recipe == "pipeline"
    a.out = a.out or os.path.join(ROOT, "profiles", "augment_pipeline_bench.json" if pipe else "augment_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: the augmentation is timed on an MI355X or not at all")
    import augment_reference as AR
    import augment_pipeline_reference as PR
    A = importlib.import_module(f"{PKG}.augment")
    eng = importlib.import_module(f"{PKG}.engine").CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16)
    stream = torch.cuda.current_stream(eng.device)
    rng = np.random.Generator(np.random.PCG64(0))
    vols = [(rng.random(SHAPE) - 0.02).astype(np.float32) for _ in range(VOLUMES)]
    bank = A.VolumeBank(vols, eng.device)
    order = A.epoch_order(0, 0, VOLUMES)
    pos = np.arange(BATCH)
    recipe = A.SliceAugment() if pipe else A.IntensityAugment()
    call, restate = (eng.augment_pipeline, PR.pipeline_slice) if pipe else (eng.augment_slices, AR.augment_slice)
    names = ("bias", "noise", "ghost", "blur", "gamma", "affine", "flip", "policy_gamma", "policy_bias", "policy_blur", "policy_ghost") if pipe else (
        "gamma", "bias", "blur", "ghost")
    drawn = recipe.draw(0, 0, pos, SHAPE[2], bank.spacing, volumes=order[pos % VOLUMES])
    every = (drawn[0].copy(), drawn[1].copy())
    every[0][:, 2] = (1 << len(names)) - 1
    rows = []
    for name, (meta, par) in (("recipe draw", drawn), ("every stage on", every)):
        for _ in range(a.warmup):
            out = call(bank, meta, par)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(bank, meta, par)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            ref = list(ex.map(lambda b: restate(vols[meta[b, 0]], meta[b], par[b], np.float32), range(BATCH)))
        host_ms = (time.perf_counter() - t0) * 1e3
        err = max(float(np.abs(got[b] - ref[b]).max()) for b in range(BATCH))
        row = dict(batch=name, samples=BATCH, shape=list(SHAPE), bank_volumes=VOLUMES,
                   stage_counts={k: int(((meta[:, 2] & (1 << i)) != 0).sum()) for i, k in enumerate(names)},
                   device_ms_median=statistics.median(ts), device_ms_min=min(ts), max_abs_delta_vs_float32_restatement=err,
                   scipy_host_ms=host_ms, scipy_host_threads=a.threads,
                   scipy_host_note="another algorithm on another processor: for scale only")
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup,
                       method=f"device events around one CddpmEngine.{call.__name__} call (table check, one H2D copy, "
                              f"{'cddpm_aug_pipeline' if pipe else 'cddpm_aug_slices'}), median",
                       rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
