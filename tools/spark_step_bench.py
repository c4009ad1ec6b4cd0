"""ms per SparK pre-training step (spark_training.SparKTrainer: forward, backward, AdamW) at 32 x 96 x 96 (the experiment's geometry) and
16 x 128 x 128, with, for scale, the dense EncoderTrainer's forward + backward alone at the same geometry. Device events around each
step, warm-up first, then the median of --steps timed steps. Needs the GPU; writes profiles/spark_step_bench.json.

    python tools/spark_step_bench.py [--steps 20] [--warmup 5] [--precision 32 | 16 | 32 16] [--out profiles/spark_step_bench.json]

--precision: the SparKTrainer's (and the dense EncoderTrainer's) precision; 16 runs the ResNet's convolutions on the fp16-MFMA operators
under the default dynamic loss scale. Two values are measured INTERLEAVED: both trainers are built and warmed up, then timed in
alternating groups of five steps, so clock and thermal drift of the session falls on both alike.

No target is set, and nothing on the GPU machine can be compared with the reference's PyTorch step."""
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


GROUP = 5            # timed steps of one function before the turn passes to the next


def timed(fns, steps, warmup):
    """fns {key: function} -> {key: figures}: every function warmed up, then timed in alternating groups of GROUP steps"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    while any(len(v) < steps for v in ms.values()):
        for k, fn in fns.items():
            for _ in range(min(GROUP, steps - len(ms[k]))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), steps=steps, warmup=warmup) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", type=int, nargs="+", choices=(32, 16), default=[32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spark_step_bench.json"))
    args = ap.parse_args()
    precisions = list(dict.fromkeys(args.precision))
    if args.steps < 20:
        ap.error("--steps: at least 20 timed steps")
    synth, st, et, tr = (importlib.import_module(f"{PKG}.{m}") for m in ("synth", "spark_training", "encoder_training", "training"))
    dev = torch.device("cuda", 0)
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, precisions=precisions,
                  note="no target; several precisions are timed interleaved in groups of %d steps" % GROUP, cases=[])
    for B, S in GEOMETRIES:
        sd = synth.synth_spark_state_dict(0, input_size=S)
        x = torch.rand(B, 1, S, S, device=dev)
        f = S // 32
        keep = round(f * f * 0.35)
        active = torch.zeros(B, f * f, dtype=torch.bool).scatter_(1, torch.rand(B, f * f).argsort(1)[:, :keep], True).view(B, 1, f, f).to(dev)
        sparks = {p: st.SparKTrainer({k[len("model."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, dev, precision=p) for p in precisions}

        def step(spark):
            def run():
                spark.forward(x, active)
                spark.backward()
                spark.adamw_step(lr=1e-4)
            return run
        r_step = timed({p: step(t) for p, t in sparks.items()}, args.steps, args.warmup)
        skipped = {p: t.skipped_steps for p, t in sparks.items()}
        for t in sparks.values():
            t.close()
        ops = tr.UNetTrainer({"w": torch.zeros(64)}, device=dev, overlap_wgrad=False)
        ops._fit(B, S, S)
        encs = {p: et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, ops, 0.05, precision=p)
                for p in precisions}
        dcond = torch.randn(B, 128, device=dev)

        def dense(enc):
            def run():
                enc.forward(x)
                enc.backward(dcond)
            return run
        r_enc = timed({p: dense(e) for p, e in encs.items()}, args.steps, args.warmup)
        ops.close()
        for p in precisions:
            case = dict(batch=B, side=S, precision=p, spark_step=r_step[p], skipped_steps=skipped[p], dense_encoder_forward_backward=r_enc[p])
            print(json.dumps(case))
            result["cases"].append(case)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(dict(spark_step_bench=args.out)))


if __name__ == "__main__":
    main()
