"""Times precision-16 reconstruction against precision 32 (cddpm_set_precision), both in ONE process on two handles of the same
geometry, alternating per repeat, HIP events around the work on the launch stream:

    reverse    20 reverse steps (t = 999 .. 980, device Philox noise) at 64 x 128 x 128, reported per step
    forward    one UNet forward at 4 x 96 x 96 (a window of --inner forwards per repeat, reported per forward)
    attention  cddpm_op_attention against cddpm_op_attention_p16 at (B, N, C) = (64, 1024, 256) and (4, 16384, 128)
               (a window of --inner launches per repeat, reported per launch)
    attention_backward  cddpm_op_attention_backward against cddpm_op_attention_backward_p16 at the same two shapes, same protocol

The experiment's descriptor (128 x (1, 2, 2), three ResBlocks, attention in the middle block), synthetic weights. Per item and
precision: median, minimum and maximum over --reps repeats (at least 10) after a warm-up, and whether the two ranges overlap. Also
the per-class kernel time of one profiled reverse step per precision (cddpm_set_profiling: eager launches, events per launch).

    python tools/precision16_bench.py [--reps 12] [--inner 10] [--out profiles/precision16_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"
pkg = lambda sub: importlib.import_module(f"{PKG}.{sub}")
STEPS = 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def compare(work, reps, warmup=2, scale=1.0):
    """work: {label: callable}; the labels alternate inside every repeat. -> {label: dict(median_ms, min_ms, max_ms)}"""
    for _ in range(warmup):
        for fn in work.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in work}
    for _ in range(reps):
        for k, fn in work.items():
            ts[k].append(event_ms(fn) * scale)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ts.items()}


def verdict(row, slow, fast):
    """`fast` beats `slow` when its whole range lies below the other's"""
    row["speedup_of_medians"] = row[slow]["median_ms"] / row[fast]["median_ms"]
    row["ranges_overlap"] = not (row[fast]["max_ms"] < row[slow]["min_ms"] or row[slow]["max_ms"] < row[fast]["min_ms"])
    row["faster"] = None if row["ranges_overlap"] else (fast if row[fast]["max_ms"] < row[slow]["min_ms"] else slow)
    return row


def engines(max_batch, h, w, sd):
    E, sched = pkg("engine"), pkg("schedule")
    out = {}
    for bits in (32, 16):
        e = E.CddpmEngine(timesteps=1000, max_batch=max_batch, max_h=h, max_w=w, conv_family="h3", precision=bits)
        e.load_weights(sd)
        e.set_schedule(sched.schedule_buffers(1000), "pred_x0")
        out[f"p{bits}"] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision16_bench.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("precision16_bench needs an MI355X: no HIP device is visible (nothing is measured on the CPU)")
    synth = pkg("synth")
    sd = synth.synth_state_dict(0)
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, timer="HIP events on the launch stream")

    # ---- 20 reverse steps at 64 x 128 x 128
    B, H, W = 64, 128, 128
    eng = engines(B, H, W, sd)
    x_T = torch.from_numpy(synth.noise_xT(2, 0, B, H, W)).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
    bufs = {}
    for k, e in eng.items():
        e.prepare_cond(cond, B)
        bufs[k] = x_T.clone()

    work = {k: (lambda k=k: (bufs[k].copy_(x_T), eng[k].reverse_range_(bufs[k], 999, 1000 - STEPS, seed=7))) for k in eng}
    row = verdict(dict(B=B, H=H, W=W, steps=STEPS, unit="ms per reverse step", **compare(work, a.reps, warmup=1, scale=1.0 / STEPS)), "p32", "p16")
    finite = {k: bool(torch.isfinite(bufs[k]).all()) for k in eng}
    row["finite"] = finite
    row["p16_vs_p32_rms_after_20_steps"] = float((bufs["p16"] - bufs["p32"]).double().pow(2).mean().sqrt())
    classes = {}
    for k, e in eng.items():                     # one profiled step each: where the time goes
        e.set_profiling(True)
        e.get_profile()
        bufs[k].copy_(x_T)
        e.reverse_range_(bufs[k], 999, 999, seed=7)
        torch.cuda.synchronize()
        classes[k] = {n: round(v["ms"], 4) for n, v in e.get_profile().items() if v["launches"]}
        e.set_profiling(False)
    row["profiled_step_ms_by_class"] = classes
    result["reverse"] = row
    print(json.dumps(row), flush=True)
    for e in eng.values():
        e.close()
    del bufs

    # ---- one forward at 4 x 96 x 96
    B, H, W = 4, 96, 96
    eng = engines(B, H, W, sd)
    x = torch.from_numpy(synth.noise_xT(2, 0, B, H, W)).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
    outs = {k: torch.empty_like(x) for k in eng}
    for k, e in eng.items():
        e.prepare_cond(cond, B)

    def fwd(k):
        for _ in range(a.inner):
            eng[k].unet_forward(x, 500, None, out=outs[k])       # a uniform t: no host read-back inside the window
    row = verdict(dict(B=B, H=H, W=W, unit="ms per forward", **compare({k: (lambda k=k: fwd(k)) for k in eng}, a.reps, scale=1.0 / a.inner)), "p32", "p16")
    row["p16_vs_p32_rms"] = float((outs["p16"] - outs["p32"]).double().pow(2).mean().sqrt())
    result["forward"] = row
    print(json.dumps(row), flush=True)

    # ---- the attention operators
    e = eng["p32"]
    rows = []
    for (B, N, C) in ((64, 1024, 256), (4, 16384, 128)):
        qkv = torch.randn(B, N, 3 * C, generator=torch.Generator().manual_seed(N + C)).cuda()

        def att(bits):
            for _ in range(a.inner):
                e.op_attention(qkv, precision=bits)
        row = verdict(dict(B=B, N=N, C=C, unit="ms per launch", flops=4.0 * B * N * N * C,
                           **compare({"fp32": lambda: att(32), "p16": lambda: att(16)}, a.reps, scale=1.0 / a.inner)), "fp32", "p16")
        for k in ("fp32", "p16"):
            row[k]["tflops"] = row["flops"] / (row[k]["median_ms"] * 1e-3) / 1e12
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["attention"] = rows

    # ---- their backward operators: 9 N x N x 64 products per head executed (the forward's 2 recomputed + 7)
    rows = []
    for (B, N, C) in ((64, 1024, 256), (4, 16384, 128)):
        g = torch.Generator().manual_seed(N + C)
        qkv = torch.randn(B, N, 3 * C, generator=g).cuda()
        da = torch.randn(B, N, C, generator=g).cuda()

        def att_bwd(bits):
            for _ in range(a.inner):
                e.op_attention_backward(qkv, da, precision=bits)
        row = verdict(dict(B=B, N=N, C=C, unit="ms per call (two kernels)", flops=18.0 * B * N * N * C,
                           **compare({"fp32": lambda: att_bwd(32), "p16": lambda: att_bwd(16)}, a.reps, scale=1.0 / a.inner)), "fp32", "p16")
        for k in ("fp32", "p16"):
            row[k]["tflops"] = row["flops"] / (row[k]["median_ms"] * 1e-3) / 1e12
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["attention_backward"] = rows
    for e in eng.values():
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
