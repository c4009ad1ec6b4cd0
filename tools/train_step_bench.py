"""Times the training step (training.py: forward + loss + backward + Adam, all on the HIP operators) on one GPU.
    python tools/train_step_bench.py [--batch 16] [--size 128] [--steps 5] [--warmup 2]
    python tools/train_step_bench.py --gpus N            (starts the N ranks itself: the line below as a child process)
    python tools/train_step_bench.py --attention-resolutions 1,2,4 --attention-family f32 h3 [--out profiles/attention_h3_bench.json]
                                                         (one trainer per family in ONE process, their steps interleaved; one GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/train_step_bench.py   (data-parallel, RCCL)
BASELINE config 5 is 128x1x128x128 over 8 GPUs data-parallel = 16 slices per GPU and step (weak scaling: --batch is per rank)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--encoder", action="store_true", help="train the context encoder (ResNet-50) jointly, as the reference does")
    ap.add_argument("--dropout", type=float, default=0.0, help="the UNet's dropout probability (cfg.dropout_unet); 0: no dropout launches")
    ap.add_argument("--attention-resolutions", default=None, metavar="DS[,DS...]",
                    help="down-sampling factors whose levels get attention behind every ResBlock (cfg.att_res), e.g. 1,2,4; default: the "
                         "experiment's 3,6,12 = attention in the middle block only")
    ap.add_argument("--attention-precision", default="32",
                    help="UNetTrainer's attention_precision: 16 = the fp16-MFMA attention forward and backward, 32 (default) = exact fp32")
    ap.add_argument("--attention-family", nargs="+", default=["f32"], metavar="FAMILY",
                    help="UNetTrainer's attention_family where the attention precision is 32: f32 (default) = exact fp32, h3 = fp32-grade fp16 "
                         "splits. Several families: one trainer each, timed step by step in alternation (median, min, max per family)")
    ap.add_argument("--out", default=None, help="with several families: merge the result into this JSON file under the key 'train_step'")
    ap.add_argument("--encoder-precision", default="32",
                    help="EncoderTrainer's precision (with --encoder): 16 = its convolutions on fp16 operands (fp16-MFMA kernels), 32 (default) = "
                         "fp32 FMA kernels")
    ap.add_argument("--phases", action="store_true", help="time forward / backward / adam separately (synchronises between them)")
    ap.add_argument("--gpus", type=int, default=1, help="N > 1 without RANK in the environment: start the N ranks (torchrun child) and relay rank 0's line")
    a = ap.parse_args()
    from bench import launch_plan, self_launch           # decided before anything touches the GPU
    plan = launch_plan(a.gpus, sys.argv[1:], os.environ, script=os.path.abspath(__file__))
    if plan is not None:
        self_launch(plan, os.environ)
    import torch
    tr = importlib.import_module(PKG + ".training")
    synth = importlib.import_module(PKG + ".synth")
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    ddp = "RANK" in os.environ                   # under torchrun (also with one rank: the RCCL path runs)
    if ddp:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    arch = {} if a.attention_resolutions is None else {"attention_resolutions": tuple(int(v) for v in a.attention_resolutions.split(","))}
    sd = synth.synth_state_dict(0, **arch)
    if len(a.attention_family) > 1:
        assert not ddp and not a.encoder and not a.phases, "several attention families: one GPU, the UNet's step only"
        return compare_families(a, tr, synth, torch, dev, sd, arch)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v) for k, v in sd.items()}, device=dev, dropout=a.dropout, dropout_seed=1,
                             attention_precision=a.attention_precision, attention_family=a.attention_family[0], **arch)
    enc = None
    if a.encoder:
        et = importlib.import_module(PKG + ".encoder_training")
        enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, trainer, drop_path_rate=0.05,
                                precision=a.encoder_precision)
    B, S, T = a.batch, a.size, 1000
    x01 = torch.from_numpy(synth.synth_slices(1, rank * B, B, S, S)).reshape(B, 1, S, S).to(dev)      # each rank its own slices
    cond = torch.from_numpy(synth.synth_cond(1, rank * B, B)).to(dev)
    noise = torch.from_numpy(synth.noise_xT(1, rank * B, B, S, S)).reshape(B, 1, S, S).to(dev)
    t = torch.tensor([(137 * (i + 1)) % T for i in range(B)], dtype=torch.long, device=dev)
    losses = []
    for _ in range(a.warmup):
        losses.append(float(tr.training_step(trainer, x01, cond, t=t, noise=noise, objective="pred_noise", loss_type="l2", all_reduce=ddp, encoder=enc, slice0=rank * B)))
    torch.cuda.synchronize()
    if ddp:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = tr.training_step(trainer, x01, cond, t=t, noise=noise, objective="pred_noise", loss_type="l2", all_reduce=ddp, encoder=enc, slice0=rank * B)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    if ddp:
        tmax = torch.tensor([dt], device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    losses.append(float(loss))
    bits = tr.get_precision()
    arith = "fp32-emulated convolutions" if bits == 32 else "fp16-operand convolutions (precision 16)"
    res = {"workload": f"training step {B}x1x{S}x{S} (noise-pred MSE, {arith}, Adam" + (", context encoder trained jointly)" if enc else ")"), "ms_per_step": dt * 1e3,
           "precision": bits, "dropout": a.dropout, "attention_resolutions": list(trainer.att_res), "attention_precision": trainer.attention_precision,
           "attention_family": trainer.attention_family, "encoder_precision": enc.precision if enc else None,
           "slices_per_s": world * B / dt, "n_gpus": world, "losses": losses, "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30}
    if a.phases:
        buf = importlib.import_module(PKG + ".schedule").schedule_buffers(T)
        x0 = x01 * 2 - 1
        xt = (buf["sqrt_alphas_cumprod"].to(dev)[t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"].to(dev)[t].reshape(-1, 1, 1, 1) * noise)
        ph = {}
        for _ in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = trainer.forward(xt, t, cond)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            _l, dout = trainer.loss_and_grad(out, noise, None, "l2")
            trainer.backward(dout)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            trainer.adam_step()
            torch.cuda.synchronize(); t3 = time.perf_counter()
            ph = {"forward_ms": (t1 - t0) * 1e3, "loss_backward_ms": (t2 - t1) * 1e3, "adam_repack_ms": (t3 - t2) * 1e3}
        res["phases"] = ph
    if rank == 0:
        print(json.dumps(res))
    if ddp:
        dist.barrier()
        dist.destroy_process_group()


def compare_families(a, tr, synth, torch, dev, sd, arch):
    """one trainer per attention family on the same weights and batch; after the warm-up, a.steps rounds of one step per family in
    alternation, each step timed on its own between two device synchronisations"""
    B, S, T = a.batch, a.size, 1000
    x01 = torch.from_numpy(synth.synth_slices(1, 0, B, S, S)).reshape(B, 1, S, S).to(dev)
    cond = torch.from_numpy(synth.synth_cond(1, 0, B)).to(dev)
    noise = torch.from_numpy(synth.noise_xT(1, 0, B, S, S)).reshape(B, 1, S, S).to(dev)
    t = torch.tensor([(137 * (i + 1)) % T for i in range(B)], dtype=torch.long, device=dev)
    trainers = {f: tr.UNetTrainer({k: torch.from_numpy(v) for k, v in sd.items()}, device=dev, dropout=a.dropout, dropout_seed=1,
                                  attention_precision=a.attention_precision, attention_family=f, **arch) for f in a.attention_family}
    step = lambda trainer: float(tr.training_step(trainer, x01, cond, t=t, noise=noise, objective="pred_noise", loss_type="l2"))
    ms, losses = {f: [] for f in trainers}, {f: [] for f in trainers}
    for i in range(a.warmup + a.steps):
        for f, trainer in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step(trainer)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[f].append((time.perf_counter() - t0) * 1e3)
            losses[f].append(loss)
    res = {"workload": f"training step {B}x1x{S}x{S} (noise-pred MSE, Adam), one trainer per attention family, steps interleaved",
           "precision": tr.get_precision(), "attention_resolutions": list(next(iter(trainers.values())).att_res),
           "attention_precision": next(iter(trainers.values())).attention_precision, "timer": "host clock between device synchronisations",
           "ms_per_step": {f: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), samples=len(v)) for f, v in ms.items()},
           "losses": losses, "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30}
    print(json.dumps(res))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["train_step"] = res
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    for trainer in trainers.values():
        trainer.close()


if __name__ == "__main__":
    main()
