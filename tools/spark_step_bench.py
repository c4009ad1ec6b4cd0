"""ms per SparK pre-training step (spark_training.SparKTrainer: forward, backward, AdamW) at 32 x 96 x 96 (the experiment's geometry) and
16 x 128 x 128, with, for scale, the dense EncoderTrainer's forward + backward alone at the same geometry. Device events around each
step, warm-up first, then the median of --steps timed steps. Needs the GPU; writes profiles/spark_step_bench.json.

    python tools/spark_step_bench.py [--steps 20] [--warmup 5] [--out profiles/spark_step_bench.json]

A first measurement: there is no target, and nothing on the GPU machine can be compared with the reference's PyTorch step."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"
GEOMETRIES = [(32, 96), (16, 128)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), steps=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spark_step_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed steps")
    synth, st, et, tr = (importlib.import_module(f"{PKG}.{m}") for m in ("synth", "spark_training", "encoder_training", "training"))
    dev = torch.device("cuda", 0)
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, note="first measurement; no target", cases=[])
    for B, S in GEOMETRIES:
        sd = synth.synth_spark_state_dict(0, input_size=S)
        x = torch.rand(B, 1, S, S, device=dev)
        f = S // 32
        keep = round(f * f * 0.35)
        active = torch.zeros(B, f * f, dtype=torch.bool).scatter_(1, torch.rand(B, f * f).argsort(1)[:, :keep], True).view(B, 1, f, f).to(dev)
        spark = st.SparKTrainer({k[len("model."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, dev)

        def step():
            spark.forward(x, active)
            spark.backward()
            spark.adamw_step(lr=1e-4)
        r_step = timed(step, args.steps, args.warmup)
        spark.close()
        ops = tr.UNetTrainer({"w": torch.zeros(64)}, device=dev, overlap_wgrad=False)
        ops._fit(B, S, S)
        enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, ops, 0.05)
        dcond = torch.randn(B, 128, device=dev)

        def dense():
            enc.forward(x)
            enc.backward(dcond)
        r_enc = timed(dense, args.steps, args.warmup)
        ops.close()
        case = dict(batch=B, side=S, spark_step=r_step, dense_encoder_forward_backward=r_enc)
        print(json.dumps(case))
        result["cases"].append(case)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(dict(spark_step_bench=args.out)))


if __name__ == "__main__":
    main()
