#!/usr/bin/env python3
"""Times the attention operators of the three arithmetics (csrc/attention.hip) against each other in ONE session on one device:
f32 (exact fp32 MFMA), h3 (fp32-grade three-term fp16 splits) and p16 (plain fp16 operands), forward and backward.
    python tools/attention_family_bench.py [--out profiles/attention_h3_bench.json] [--rounds 5] [--samples 2]
Per shape and direction the three operators run in alternation, round after round, so that clock and temperature drift reach them
alike; a sample is a window of launches between two HIP events on the launch stream (the window sized from the warm-up call so that it
lasts about 50 ms, at most 10 launches), after a warm-up. Reported per operator: median, min and max of rounds x samples (>= 10) samples,
and the h3 and p16 medians as multiples of the f32 median of the same session -- never of a recorded number.
The comparison says nothing about accuracy: tests/test_gpu_attention_h3.py holds h3 to the exact operators' bounds."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"

# (B, N, C): a 64-slice reverse step's middle attention (32 x 32 tokens, four heads); 24 x 24 tokens, a multiple of neither the workgroup
# nor the tile; level-0 attention at 128 x 128. Backward: the 16 x 128 x 128 training step's middle and level-0 attention
FORWARD_SHAPES = [(64, 1024, 256), (4, 576, 256), (4, 16384, 128)]
BACKWARD_SHAPES = [(16, 1024, 256), (16, 16384, 128)]
ARITHMETICS = {"f32": dict(precision=32, family="f32"), "h3": dict(precision=32, family="h3"), "p16": dict(precision=16)}
TARGET_MS, MAX_WINDOW = 50.0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_h3_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=2)
    a = ap.parse_args()
    assert a.rounds * a.samples >= 10, "at least 10 samples per operator"
    import torch
    e = importlib.import_module(PKG + ".engine").CddpmEngine(timesteps=10, max_batch=1, max_h=32, max_w=32)

    def timed(op, window):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(window):
            op()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / window

    result = {"timer": "HIP events on the launch stream", "rounds": a.rounds, "samples_per_round": a.samples, "interleaved": list(ARITHMETICS),
              "ms_per_call": {}}
    for direction, shapes in (("forward", FORWARD_SHAPES), ("backward", BACKWARD_SHAPES)):
        for shape in shapes:
            B, N, C = shape
            g = torch.Generator().manual_seed(N + C)
            qkv = torch.randn(B, N, 3 * C, generator=g).cuda()
            da = torch.randn(B, N, C, generator=g).cuda()
            ops = {n: ((lambda kw=kw: e.op_attention_backward(qkv, da, **kw)) if direction == "backward" else (lambda kw=kw: e.op_attention(qkv, **kw)))
                   for n, kw in ARITHMETICS.items()}
            window = {}
            for n, op in ops.items():          # warm-up, and the window from what one call takes
                op()
                window[n] = max(1, min(MAX_WINDOW, int(TARGET_MS / max(timed(op, 1), 1e-3))))
            ms = {n: [] for n in ops}
            for _ in range(a.rounds):
                for n, op in ops.items():
                    ms[n].extend(timed(op, window[n]) for _ in range(a.samples))
            row = {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), samples=len(v), window=window[n]) for n, v in ms.items()}
            for n in ("h3", "p16"):
                row[n]["median_over_f32"] = row[n]["median_ms"] / row["f32"]["median_ms"]
            key = "x".join(map(str, shape)) + " " + direction
            result["ms_per_call"][key] = row
            print(key, " ".join(f"{n} {r['median_ms']:.4f} [{r['min_ms']:.4f} .. {r['max_ms']:.4f}]" for n, r in row.items()),
                  f"h3 / f32 {row['h3']['median_over_f32']:.3f}", flush=True)
            del qkv, da
    e.close()
    doc = {}
    if os.path.exists(a.out):          # tools/train_step_bench.py --out writes its comparison into the same file
        with open(a.out) as f:
            doc = json.load(f)
    doc["operators"] = result
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
