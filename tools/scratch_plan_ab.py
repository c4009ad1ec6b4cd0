#!/usr/bin/env python3
"""A/B of the operator-scratch planning across two source trees, on one device: weight-gradient and training-step bits, the bytes each
tree gives cddpm_op_set_scratch, then the training step's time with the two interleaved. Sibling of tools/attention_ab.py (same process
structure and sampling); the difference: a variant is a whole checkout, not a library tag, because the trainer of this tree asks its
library for sizes (cddpm_op_*_scratch) that an older library does not export. Build the checkout to compare against first
(`python __graft_entry__.py` in it), then on the GPU box:
    python tools/scratch_plan_ab.py --run BASE_ROOT [--out profiles/scratch_plan_ab.json]
Variants: "base" = BASE_ROOT, "prod" = this tree. Each runs in its own process on its own Python package and library.
    bits   sha256 of dw and db of cddpm_op_conv_wgrad at WGRAD_SHAPES and of the flat gradient buffer after one training step of two small
           descriptors, each at training precision 32 and 16; then of the optimizer's state (parameters, Adam's m and v, the control
           block, the loss scaler) after a few steps of every step path -- the UNet at the fixed scale with exponent refreshes, by hand
           under a dynamic loss scale through a skip, a back-off and a growth, with the context encoder trained jointly, SparK
           pre-training at precision 16 and 32 -- and after a resume from optimizer_state(), whose format is digested too
           (optimizer_bits); every digest must equal the base's (exit 1 otherwise)
    arena  the `bytes` of every cddpm_op_set_scratch call while a trainer is fitted to ARENA_GEOMETRIES (recorded, not compared)
    time   one 16 x 128 x 128 training step with the context encoder trained jointly (what tools/train_step_bench.py --encoder times) and
           one 32 x 96 x 96 SparK pre-training step at precision 16 (what tools/spark_step_bench.py times: the step most exposed to host
           overhead): HIP events around a window of WINDOW steps after a warm-up; AB_SAMPLES (4) samples per process, AB_ROUNDS (3)
           rounds with the variants interleaved. Verdict: prod's median inside or below base's [min, max] of this run"""
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "conditioned-diffusion-models-uad_amd"

# (k, Cin, Cout) at B = 9 (two batch groups, one ragged), 5 x 9 pixels: the two-pass kernels over k-images with 32-channel chunks, the
# single-pass 1x1 kernel (Cin an odd multiple of 32), the two-pass 1x1 with 64-channel chunks
WGRAD_SHAPES = [(3, 32, 64), (1, 96, 64), (1, 128, 64)]
STEP_CASES = {"cond4": dict(model_channels=128, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(3, 6, 12), cond_dim=4, geometry=(3, 12, 20)),
              "attn_levels": dict(model_channels=128, channel_mult=(1, 2, 2), num_res_blocks=1, attention_resolutions=(1, 2, 4), cond_dim=128,
                                  geometry=(2, 16, 24))}
ARENA_GEOMETRIES = [(16, 128, 128), (32, 96, 96), (64, 128, 128)]
WINDOW = 2


def _trainer(tr, synth, torch, case=None, params=None, **more):
    kw = {} if case is None else dict(model_channels=case["model_channels"], channel_mult=case["channel_mult"], num_res_blocks=case["num_res_blocks"],
                                      attention_resolutions=case["attention_resolutions"])
    if params is None:
        params = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, num_classes=(case["cond_dim"] if case else 128), **kw).items()}
    return tr.UNetTrainer(params, device=torch.device("cuda", 0), cond_dim=(case["cond_dim"] if case else 128), **kw, **more)


def _batch(synth, torch, B, H, W, cond_dim=128):
    x01 = torch.from_numpy(synth.synth_slices(1, 0, B, H, W)).reshape(B, 1, H, W).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, B, cond_dim)).cuda()
    noise = torch.from_numpy(synth.noise_xT(1, 0, B, H, W)).reshape(B, 1, H, W).cuda()
    t = torch.tensor([(137 * (i + 1)) % 1000 for i in range(B)], dtype=torch.long, device="cuda")
    return x01, cond, noise, t


def _spark(torch, B, side, precision, params=None):
    """a SparKTrainer on synth's state dict (or `params`), one batch and its cell mask drawn under a fixed seed at ratio 0.65 -- the
    batch tests/test_gpu_spark_training_p16.py steps"""
    synth, st, mirror = (importlib.import_module(f"{PKG}.{m}") for m in ("synth", "spark_training", "Spark_2D"))
    if params is None:
        params = {k[len("model."):]: torch.from_numpy(v) for k, v in synth.synth_spark_state_dict(0, input_size=side).items()}
    torch.manual_seed(B + side)
    x = torch.rand(B, 1, side, side)
    f = side // 32
    active = mirror.draw_mask(B, f, round(f * f * (1 - 0.65)))
    return st.SparKTrainer(params, torch.device("cuda", 0), precision=precision), x.cuda(), active.cuda()


def optimizer_bits(out, sha):
    """digests of the optimizer's state after a few steps of every step path, and after a resume (module docstring)"""
    import torch
    tr, synth, et = (importlib.import_module(f"{PKG}.{m}") for m in ("training", "synth", "encoder_training"))

    def canon(x):
        if torch.is_tensor(x):
            return [str(x.dtype), list(x.shape), sha(x)]
        if isinstance(x, dict):
            return [[k, canon(x[k])] for k in sorted(x)]
        return [canon(v) for v in x] if isinstance(x, (list, tuple)) else repr(x)

    def digest(tag, opt, **owners):
        for name, o in owners.items():
            out[f"{tag} {name} flat"], out[f"{tag} {name} m"], out[f"{tag} {name} v"] = sha(o.flat), sha(o.state["m"]), sha(o.state["v"])
        out[f"{tag} ctrl"] = sha(opt.ctrl)
        if opt.scaler is not None:
            out[f"{tag} scaler"] = sha(opt.scaler)

    def resume(tag, old, fresh, step, **owners):
        state = old.optimizer_state()
        out[f"{tag} optimizer_state format"] = hashlib.sha256(json.dumps(canon(state)).encode()).hexdigest()
        fresh.load_optimizer_state(state)
        step(fresh)
        torch.cuda.synchronize()
        digest(tag + " resumed", fresh, **{k: getattr(fresh, a) if a else fresh for k, a in owners.items()})

    case = STEP_CASES["cond4"]
    x01, cond, noise, t = _batch(synth, torch, *case["geometry"], case["cond_dim"])
    for bits in (32, 16):                # the fixed scale; exp_refresh 2: the second update refreshes the exponents before it re-packs
        tr.set_precision(bits)
        trainer = _trainer(tr, synth, torch, case, exp_refresh=2)
        for _ in range(3):
            tr.training_step(trainer, x01, cond, t=t, noise=noise)
        torch.cuda.synchronize()
        digest(f"cond4 p{bits} 3 steps", trainer, unet=trainer)
        trainer.close()

    def by_hand(trainer, inf=False):     # as tests/test_gpu_loss_scaling.py drives it: the unguarded adam_step guards, updates, rescales
        out_ = trainer.forward(x01 * 2 - 1, t, cond)
        _loss, dout = trainer.loss_and_grad(out_, noise, None, "l2")
        if inf:
            dout[0, 0, 3, 3] = float("inf")
        trainer.backward(dout)
        trainer.adam_step(lr=1e-4)
    trainer = _trainer(tr, synth, torch, case, exp_refresh=2)
    trainer.enable_loss_scaling(growth_interval=2)
    for i in range(4):                   # clean, skipped (back-off), clean, clean (growth)
        by_hand(trainer, inf=(i == 1))
    torch.cuda.synchronize()
    digest("cond4 p16 scaler by hand", trainer, unet=trainer)
    out["cond4 p16 scaler by hand counters"] = repr((trainer.step_count, trainer.skipped_steps, trainer.loss_scale, trainer.growth_tracker))
    resume("cond4 p16 scaler", trainer, _trainer(tr, synth, torch, case, params={k: v.clone() for k, v in trainer.p.items()}, exp_refresh=2),
           by_hand, unet=None)
    trainer.close()

    case = STEP_CASES["attn_levels"]     # at 2 x 64 x 64, the geometry tests/test_gpu_loss_scaling.py trains the encoder jointly at
    x01, cond, noise, t = _batch(synth, torch, 2, 64, 64, case["cond_dim"])
    trainer = _trainer(tr, synth, torch, case)
    trainer.enable_loss_scaling()
    enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, trainer, drop_path_rate=0.0)
    for _ in range(2):
        tr.training_step(trainer, x01, None, t=t, noise=noise, encoder=enc)
    torch.cuda.synchronize()
    digest("attn_levels p16 scaler + encoder 2 steps", trainer, unet=trainer, encoder=enc)
    trainer.close()
    tr.set_precision(32)

    def spark_step(spark):
        spark.forward(x, active, drop_scales={})
        spark.backward()
        spark.adamw_step(lr=1e-3)
    for precision, steps in ((16, 5), (32, 2)):      # 16: the default scaler, which backs off from 65536 on this batch in its first steps
        spark, x, active = _spark(torch, 4, 64, precision)
        for _ in range(steps):
            spark_step(spark)
        torch.cuda.synchronize()
        digest(f"spark p{precision} {steps} steps", spark, own=spark, encoder=spark.enc)
        out[f"spark p{precision} counters"] = repr((spark.step_count, spark.skipped_steps, spark.loss_scale))
        if precision == 16:
            fresh = _spark(torch, 4, 64, 16, params={k: v.clone() for k, v in spark.state_dict().items()})[0]
            resume("spark p16", spark, fresh, spark_step, own=None, encoder="enc")
            fresh.close()
        spark.close()


def _windows(torch, step, samples):
    """ms per step of `samples` windows of WINDOW steps between two HIP events, after a warm-up"""
    for _ in range(2):
        step()          # warm-up
    ms = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(WINDOW):
            step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / WINDOW)
    return ms


def child(root, mode, samples):
    sys.path.insert(0, root)
    import torch
    tr, synth = importlib.import_module(PKG + ".training"), importlib.import_module(PKG + ".synth")
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    out = {}
    if mode == "bits":
        e = importlib.import_module(PKG + ".engine").CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16)
        for bits in (32, 16):
            tr.set_precision(bits)
            for k, cin, cout in WGRAD_SHAPES:
                g = torch.Generator().manual_seed(k + cin)
                x, dy = torch.randn(9, 5, 9, cin, generator=g).cuda(), torch.randn(9, 5, 9, cout, generator=g).cuda()
                dw, db = e.op_conv_wgrad(x, None, None, False, dy, ksize=k)
                out[f"wgrad k{k} {cin}->{cout} p{bits} dw"], out[f"wgrad k{k} {cin}->{cout} p{bits} db"] = sha(dw), sha(db)
            for name, case in STEP_CASES.items():
                trainer = _trainer(tr, synth, torch, case)
                x01, cond, noise, t = _batch(synth, torch, *case["geometry"], case["cond_dim"])
                tr.training_step(trainer, x01, cond, t=t, noise=noise)
                torch.cuda.synchronize()
                out[f"step {name} p{bits} gflat"] = sha(trainer.gflat)
                trainer.close()
        tr.set_precision(32)
        e.close()
        optimizer_bits(out, sha)
    elif mode == "arena":
        lib = importlib.import_module(PKG + "._lib").load_library()
        set_scratch, seen = lib.cddpm_op_set_scratch, []
        lib.cddpm_op_set_scratch = lambda h, n: (seen.append(int(n)) if n else None, set_scratch(h, n))[1]     # main handle, then the side handle
        trainer = _trainer(tr, synth, torch)
        for g in ARENA_GEOMETRIES:
            del seen[:]
            trainer._fit(*g)
            out["x".join(map(str, g))] = list(seen)
        trainer.close()
    else:
        et = importlib.import_module(PKG + ".encoder_training")
        trainer = _trainer(tr, synth, torch)
        enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, trainer, drop_path_rate=0.05)
        x01, cond, noise, t = _batch(synth, torch, 16, 128, 128)
        step = lambda: tr.training_step(trainer, x01, cond, t=t, noise=noise, objective="pred_noise", loss_type="l2", encoder=enc)
        out["training step 16x128x128 + encoder"] = _windows(torch, step, samples)
        trainer.close()
        spark, x, active = _spark(torch, 32, 96, 16)

        def step():
            spark.forward(x, active)
            spark.backward()
            spark.adamw_step(lr=1e-4)
        out["SparK step 32x96x96 p16"] = _windows(torch, step, samples)
        spark.close()
    print(json.dumps(out))


def run_child(root, tag, mode, samples):
    env = {k: v for k, v in os.environ.items() if k != "CDDPM_LIB"}           # every tree loads the library built in it
    o = subprocess.run([sys.executable, __file__, "--child", root, mode, str(samples)], env=env, capture_output=True, text=True, timeout=600)
    if o.returncode != 0:          # stop (as on a timeout): nothing more is started on a device a child may have left faulted
        sys.exit(f"{tag} {mode} FAILED (exit {o.returncode}):\n{o.stderr[-2000:]}")
    return json.loads(o.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
        return
    assert sys.argv[1] == "--run" and len(sys.argv) > 2, __doc__
    args = sys.argv[2:]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "scratch_plan_ab.json")
    roots = {"base": os.path.abspath(args[0]), "prod": ROOT}
    rounds, samples = int(os.environ.get("AB_ROUNDS", "3")), int(os.environ.get("AB_SAMPLES", "4"))
    assert rounds * samples >= 10, "at least 10 samples per variant"
    result = {"variants": list(roots), "window": WINDOW, "timer": "HIP events on the launch stream", "digests": {}, "set_scratch_bytes": {},
              "ms_per_step": {}}

    for tag, root in roots.items():
        result["digests"][tag] = run_child(root, tag, "bits", 0)
    differ = [k for k, v in result["digests"]["base"].items() if result["digests"]["prod"][k] != v]
    result["bit_identical"] = not differ
    print(f"bits: {len(result['digests']['base'])} digests per variant,", "all equal" if not differ else f"DIFFERENT: {differ}", flush=True)
    for tag, root in roots.items():
        result["set_scratch_bytes"][tag] = run_child(root, tag, "arena", 0)
    print("cddpm_op_set_scratch bytes (main handle, side handle):", result["set_scratch_bytes"], flush=True)

    ms = {}
    for _ in range(rounds):          # interleaved rounds
        for tag, root in roots.items():
            for k, v in run_child(root, tag, "time", samples).items():
                ms.setdefault(k, {}).setdefault(tag, []).extend(v)
    slower = []
    for k, per in ms.items():
        row = {tag: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), samples=len(v)) for tag, v in per.items()}
        row["inside_or_below"] = row["prod"]["median_ms"] <= row["base"]["max_ms"]
        if not row["inside_or_below"]:
            slower.append(k)
        result["ms_per_step"][k] = row
        print(k, " ".join(f"{t} {r['median_ms']:.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]" for t, r in row.items() if t in roots),
              "ok" if row["inside_or_below"] else "SLOWER", flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)
    if differ or slower:
        sys.exit(f"different bits: {differ}; median above base's range: {slower}")


if __name__ == "__main__":
    main()
