#!/usr/bin/env python3
"""A/B of the attention operators (csrc/attention.hip) across library builds, on one device: output bits, then interleaved timing.
Build a side-by-side library first, e.g. build.build_lib(tag="base") from a checkout of the commit to compare against ->
csrc/libcddpm_hip_base.so, then on the GPU box:
    python tools/attention_ab.py --run base prod [--out profiles/attention_ab.json]
A variant is "prod" (csrc/libcddpm_hip.so) or a tag. Each variant runs in its own process (CDDPM_LIB selects the .so) through the
engine: op_attention and op_attention_backward at precision 32 and 16.
    bits   sha256 of each operator's output bytes on seeded inputs at BIT_SHAPES; every digest of every variant must equal the first
           variant's (exit 1 otherwise: two builds that claim the same arithmetic in the same order give the same bytes)
    time   per operator at TIME_SHAPES (those of tools/precision16_bench.py): HIP events on the launch stream around a window of 10
           launches, after a warm-up; AB_SAMPLES (4) samples per process, AB_ROUNDS (3) rounds with the variants interleaved.
           verdict per operator and shape: the last variant's median inside or below the first variant's [min, max] of this run"""
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")

# (B, N, C): one key (every other key of the tile masked); below one tile, N % 4 != 0, four heads; one key into the second tile (a fully
# masked 32-key sub-tile); the same with N % 4 != 0; a second workgroup with one live query (the clamped row); N a multiple of neither
# the 128-row workgroup nor the 64-row tile; four heads, twelve blocks
BIT_SHAPES = [(1, 1, 64), (2, 15, 256), (1, 65, 64), (2, 67, 128), (1, 129, 128), (2, 240, 128), (1, 1536, 256)]
TIME_SHAPES = [(64, 1024, 256), (4, 16384, 128)]
WINDOW = 10


def operators(e, torch, shape):
    B, N, C = shape
    g = torch.Generator().manual_seed(N + C)
    qkv = torch.randn(B, N, 3 * C, generator=g).cuda()
    da = torch.randn(B, N, C, generator=g).cuda()
    return {"forward_32": lambda: e.op_attention(qkv, precision=32), "forward_16": lambda: e.op_attention(qkv, precision=16),
            "backward_32": lambda: e.op_attention_backward(qkv, da, precision=32),
            "backward_16": lambda: e.op_attention_backward(qkv, da, precision=16)}


def child(mode, samples):
    import torch
    e = importlib.import_module(PKG + ".engine").CddpmEngine(timesteps=10, max_batch=1, max_h=32, max_w=32)
    out = {}
    for shape in (BIT_SHAPES if mode == "bits" else TIME_SHAPES):
        for name, op in operators(e, torch, shape).items():
            key = "x".join(map(str, shape)) + " " + name
            if mode == "bits":
                out[key] = hashlib.sha256(op().cpu().numpy().tobytes()).hexdigest()
                continue
            op()          # warm-up
            ms = []
            for _ in range(samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(WINDOW):
                    op()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / WINDOW)
            out[key] = ms
    e.close()
    print(json.dumps(out))


def run_child(tag, mode, samples):
    env = dict(os.environ, CDDPM_LIB=os.path.join(CSRC, "libcddpm_hip.so" if tag == "prod" else f"libcddpm_hip_{tag}.so"))
    o = subprocess.run([sys.executable, __file__, "--child", mode, str(samples)], env=env, capture_output=True, text=True, timeout=300)
    if o.returncode != 0:          # stop (as on a timeout): nothing more is started on a device a child may have left faulted
        sys.exit(f"{tag} {mode} FAILED (exit {o.returncode}):\n{o.stderr[-2000:]}")
    return json.loads(o.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        return
    assert sys.argv[1] == "--run" and len(sys.argv) > 3, __doc__
    args = sys.argv[2:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "attention_ab.json")
    tags = args[:args.index("--out")] if "--out" in args else args
    rounds, samples = int(os.environ.get("AB_ROUNDS", "3")), int(os.environ.get("AB_SAMPLES", "4"))
    assert rounds * samples >= 10, "at least 10 samples per variant"
    result = {"variants": tags, "window": WINDOW, "timer": "HIP events on the launch stream", "digests": {}, "ms_per_call": {}}

    for tag in tags:
        result["digests"][tag] = run_child(tag, "bits", 0)
    differ = [(tag, k) for tag in tags[1:] for k, v in result["digests"][tags[0]].items() if result["digests"][tag][k] != v]
    result["bit_identical"] = not differ
    print(f"bits: {len(result['digests'][tags[0]])} digests per variant,", "all equal" if not differ else f"DIFFERENT: {differ}", flush=True)

    ms = {}
    for _ in range(rounds):          # interleaved rounds
        for tag in tags:
            for k, v in run_child(tag, "time", samples).items():
                ms.setdefault(k, {}).setdefault(tag, []).extend(v)
    slower = []
    for k, per in ms.items():
        row = {tag: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), samples=len(v)) for tag, v in per.items()}
        row["inside_or_below"] = row[tags[-1]]["median_ms"] <= row[tags[0]]["max_ms"]
        if not row["inside_or_below"]:
            slower.append(k)
        result["ms_per_call"][k] = row
        print(k, " ".join(f"{t} {r['median_ms']:.4f} [{r['min_ms']:.4f} .. {r['max_ms']:.4f}]" for t, r in row.items() if t in tags),
              "ok" if row["inside_or_below"] else "SLOWER", flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)
    if differ or slower:
        sys.exit(f"different bits: {differ}; median above {tags[0]}'s range: {slower}")


if __name__ == "__main__":
    main()
