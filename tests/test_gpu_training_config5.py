"""GPU: the training step bench.py times (config.training_step / config.training_step_precision16: BASELINE config 5's per-GPU share)
against float64 autograd at its own shape -- training.training_step on 16 x 1 x 128 x 128 slices, noise-prediction MSE, the context encoder
trained jointly with drop_path_rate 0.05, guarded Adam. The small-shape gradient tests (test_gpu_training.py, test_gpu_encoder_training.py)
never reach what only this shape and this entry point run: the 256-cout convolution workgroups with two-level accumulation (64 x 64 level),
the encoder's contraction split with Z = 1 and BatchNorm over 16 H W samples, weight gradients over two full batch groups of 8, GroupNorm
sweeps at HW >= 4096, the trainer's largest scratch arenas and the joint step's deferred join of the side stream.

The step is captured with wrappers on the trainers' instances (no product code changes) and checked link by link at the HIP step's own
inputs, so that errors do not compound and the small-shape bounds apply unchanged: the context and running statistics, the UNet's output at
the HIP context, the loss and dL/d(out), every UNet gradient plus dL/d(context) as the oracle's VJP of the HIP dL/d(out), every encoder
gradient as the encoder oracle's VJP of the HIP dL/d(context). Then other arithmetic and plans against the same reference (child processes)
and the step's run-to-run and stream-to-stream determinism.

The float64 reference costs about 4 GB and 10-20 s per sample on 8 CPU threads (a graph of 2 samples takes more than twice that), so the
UNet's VJP is taken one sample at a time (the UNet couples no samples) and computed once per module."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg
from test_gpu_training import _inputs, _loss_of

B, H, W, T, SEED = 16, 128, 128, 1000, 1


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n{__name__}: module wall time {time.perf_counter() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------- the step under test
def run_step(overlap_wgrad=None, capture=None):
    """one training.training_step exactly as bench.py's training_rate calls it, from freshly built trainers and a seeded device RNG
    (the drop-path scales are torch.rand draws on the device). capture: a dict that receives the model output, dL/d(out) and the loss
    scale, the context, the encoder's ReLU masks and drop scales -- device copies taken on the stream, no synchronisation inside the step.
    Returns (trainer, encoder, loss)."""
    tr, et, synth = load_pkg("training"), load_pkg("encoder_training"), load_pkg("synth")
    dev = torch.device("cuda", 0)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0).items()}, device=dev, overlap_wgrad=overlap_wgrad)
    enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, trainer, drop_path_rate=0.05)
    x01, _cond, noise, t = (v.to(dev) for v in _inputs(synth, B, H, W, T, SEED))
    if capture is not None:
        loss_and_grad, forward, backward = trainer.loss_and_grad, enc.forward, enc.backward

        def cap_loss_and_grad(out, target, p2w=None, loss_type="l1", grad_scale=None):
            loss, dout = loss_and_grad(out, target, p2w, loss_type, grad_scale)
            capture.update(out=out.clone(), dout=dout.clone(), S=trainer.grad_scale)
            return loss, dout

        def cap_forward(x, drop_scales=None):
            ctx = forward(x, drop_scales)
            capture["context"] = ctx.clone()
            return ctx

        def cap_backward(dcond, buckets=None):
            sv = enc.saved                         # freed by the backward pass: masks and scales are taken before it runs
            masks, scales = {"bn1": sv["a0"] > 0}, {}
            for bk in enc.blocks:
                r = sv[bk["name"]]
                for key, act in (("bn1", "a1"), ("bn2", "a2"), ("out", "out")):
                    masks[bk["name"] + "." + key] = r[act] > 0
                if r["ss"] is not None:
                    scales[bk["name"]] = r["ss"].clone()
            capture.update(masks=masks, drop_scales=scales)
            return backward(dcond, buckets)

        trainer.loss_and_grad, enc.forward, enc.backward = cap_loss_and_grad, cap_forward, cap_backward
    torch.manual_seed(SEED)
    loss = tr.training_step(trainer, x01, None, t=t, noise=noise, objective="pred_noise", loss_type="l2", encoder=enc)
    torch.cuda.synchronize(dev)
    return trainer, enc, loss


def step_gradients(trainer, enc):
    """{"u:<name>": dL/dp, "e:<name>": dL/dp, "dcond": dL/d(context)} of a finished step as float32 arrays (the loss scale is a power of
    two: dividing by it is exact); Adam leaves the gradient buffers as the backward pass wrote them"""
    S = trainer.grad_scale
    out = {"u:" + k: (v / S).cpu().numpy() for k, v in trainer.g.items()}
    out.update({"e:" + k: (v / S).cpu().numpy() for k, v in enc.g.items()})
    out["dcond"] = (trainer.dcond / S).cpu().numpy()
    return out


def _bits(trainer, enc):
    """what a bitwise comparison of two steps looks at: both gradient buffers, the parameters after Adam, the running statistics"""
    return dict(gflat=trainer.gflat.cpu(), enc_gflat=enc.gflat.cpu(), flat=trainer.flat.cpu(), enc_flat=enc.flat.cpu(),
                running=torch.cat([v.reshape(-1) for v in enc.buf.values()]).cpu())


def save_step(path, overlap_wgrad=None):
    """child-process entry point: one step, its gradients to `path` (.npz)"""
    trainer, enc, loss = run_step(overlap_wgrad)
    np.savez(path, loss=np.float64(float(loss)), **step_gradients(trainer, enc))
    trainer.close()


def _child_step(tmp_path, env_extra):
    """run_step in a fresh process (the convolution plan and the training arithmetic are chosen per process from the environment)"""
    path = str(tmp_path / "step.npz")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport test_gpu_training_config5 as m\nm.save_step(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def hip():
    """the captured step: its inputs, captured intermediates, gradients, running statistics and raw gradient buffers, on the host"""
    cap = {}
    trainer, enc, loss = run_step(capture=cap)
    synth = load_pkg("synth")
    x01, _cond, noise, t = _inputs(synth, B, H, W, T, SEED)
    nchw = lambda m: m.permute(0, 3, 1, 2).cpu()
    res = dict(x01=x01, noise=noise, t=t, loss=float(loss), S=cap["S"], out=cap["out"].double().cpu(), dout=cap["dout"].double().cpu(),
               context=cap["context"].double().cpu(), masks={k: nchw(m) for k, m in cap["masks"].items()},
               drop_scales={k: v.cpu() for k, v in cap["drop_scales"].items()}, grads=step_gradients(trainer, enc),
               running={k: v.double().cpu() for k, v in enc.buf.items()}, bits=_bits(trainer, enc))
    assert trainer.step_count == 1 and trainer.skipped_steps == 0
    n_dropped = sum(int((v == 0).sum()) for v in res["drop_scales"].values())
    print(f"\nHIP step 16x128x128: loss {res['loss']:.6f}, loss scale {res['S']:.0f}, {len(res['drop_scales'])} blocks with drop path, "
          f"{n_dropped} residual branches dropped")
    trainer.close()
    del trainer, enc, cap
    torch.cuda.empty_cache()
    return res


# ---------------------------------------------------------------------------------------------- the float64 reference
def unet_vjp(oracle, sd_np, x, t, cond, v, chunk=1):
    """float64 output of the oracle's UNet and its vector-Jacobian product for the cotangent v: (out, {name: dL/dp}, dL/d(cond)), the
    autograd graph built for `chunk` samples at a time. The UNet couples no samples (GroupNorm, attention and the embeddings act per
    sample), so the parameter gradients of the chunks sum to the batch's."""
    sd = {k: torch.from_numpy(a).double().requires_grad_(True) for k, a in sd_np.items()}
    outs, dconds = [], []
    for i in range(0, x.shape[0], chunk):
        c = cond[i:i + chunk].detach().clone().requires_grad_(True)
        out = oracle.unet_forward(x[i:i + chunk], t[i:i + chunk], c, sd)
        out.backward(v[i:i + chunk])
        outs.append(out.detach())
        dconds.append(c.grad)
        del out
    return torch.cat(outs), {k: p.grad for k, p in sd.items()}, torch.cat(dconds)


@pytest.fixture(scope="module")
def ref64(hip, oracle, sd_np, synth):
    return reference64(hip, oracle, sd_np, synth)


def reference64(hip, oracle, sd_np, synth):
    """float64 autograd of every link at the HIP step's own inputs: the encoder on all 16 samples at once (BatchNorm couples the batch),
    the loss at the HIP output, the UNet's VJP of the HIP dL/d(out) at the HIP context one sample at a time"""
    import encoder_oracle as eo
    t0 = time.perf_counter()
    S = hip["S"]
    enc_np = synth.synth_encoder_state_dict(0)
    sde = {k: torch.from_numpy(v).double() for k, v in enc_np.items()}
    for k, v in sde.items():
        if "running" not in k:
            v.requires_grad_(True)
    stats = {}
    ctx = eo.resnet50_forward(hip["x01"].double(), sde, training=True, drop_scales=hip["drop_scales"], stats=stats, relu_masks=hip["masks"])
    ctx.backward(torch.from_numpy(hip["grads"]["dcond"]).double())
    enc_grads = {k: v.grad for k, v in sde.items() if v.grad is not None}
    t_enc = time.perf_counter() - t0
    buf64 = oracle.to_float64(oracle.schedule_buffers(T))
    t = hip["t"]
    o64 = hip["out"].clone().requires_grad_(True)
    loss = _loss_of(o64, hip["noise"].double(), buf64["p2_loss_weight"][t], "l2")
    loss.backward()
    xt = oracle.q_sample(hip["x01"].double() * 2 - 1, t, hip["noise"].double(), buf64)
    out, grads, dcond = unet_vjp(oracle, sd_np, xt, t, hip["context"], hip["dout"] / S)
    print(f"\nfloat64 reference: encoder {t_enc:.1f} s, UNet VJP {time.perf_counter() - t0 - t_enc:.1f} s")
    return dict(context=ctx.detach(), running=stats, enc_grads=enc_grads, loss=float(loss.detach()), dout=o64.grad, out=out, grads=grads, dcond=dcond)


def _rel(got, ref):
    """max |got - ref| relative to ref's largest entry"""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _summary(link, errs):
    """prints the worst and median relative errors of a link; returns (worst, median)"""
    errs = sorted(errs, reverse=True)
    med = float(np.median([e for e, _ in errs]))
    print(f"\n{link}: worst {errs[0][0]:.2e} ({errs[0][1]}), then {[(f'{e:.1e}', k) for e, k in errs[1:4]]}; median {med:.2e} over {len(errs)}")
    return errs[0][0], med


def unet_errors(grads, ref):
    """relative error of all 316 UNet gradients and of dL/d(context)"""
    errs = [(_rel(grads["u:" + k], r), k) for k, r in ref["grads"].items()]
    errs.append((_rel(grads["dcond"], ref["dcond"]), "dL/d(context)"))
    assert len(errs) == 317
    return errs


def encoder_errors(grads, ref):
    errs = [(_rel(grads["e:" + k], r), k) for k, r in ref["enc_grads"].items()]
    assert len(errs) == sum(1 for k in grads if k.startswith("e:"))
    return errs


# ---------------------------------------------------------------------------------------------- the reference's own check (CPU)
def test_chunked_vjp_equals_the_batched_one(oracle, sd_np, synth):
    """the per-sample decomposition the reference relies on: at 2 x 32 x 32 the VJP taken one sample at a time equals the batched one to
    rounding of the float64 sums (output, every parameter gradient, dL/d(cond))"""
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, T, 3)
    buf64 = oracle.to_float64(oracle.schedule_buffers(T))
    xt = oracle.q_sample(x01.double() * 2 - 1, t, noise.double(), buf64)
    v = torch.from_numpy(synth.noise_xT(4, 0, 2, 32, 32)).reshape(2, 1, 32, 32).double()
    o1, g1, c1 = unet_vjp(oracle, sd_np, xt, t, cond.double(), v, chunk=1)
    o2, g2, c2 = unet_vjp(oracle, sd_np, xt, t, cond.double(), v, chunk=2)
    assert len(g1) == 316
    errs = [(_rel(g1[k], g2[k]), k) for k in g2] + [(_rel(c1, c2), "cond"), (_rel(o1, o2), "out")]
    worst, _med = _summary("chunked vs batched VJP", errs)
    assert worst < 1e-12


# ---------------------------------------------------------------------------------------------- the links against the float64 reference
@pytest.mark.gpu
def test_context_and_running_statistics(hip, ref64):
    e_ctx = _rel(hip["context"], ref64["context"])
    e_run = max((_rel(hip["running"][k], v), k) for k, v in ref64["running"].items())
    print(f"\ncontext: rel err {e_ctx:.2e}; running statistics: worst {e_run[0]:.2e} ({e_run[1]})")
    assert len(ref64["running"]) == len(hip["running"])
    assert e_ctx < 2e-4 and e_run[0] < 5e-5


@pytest.mark.gpu
def test_unet_output_and_loss(hip, ref64):
    e_out = float((hip["out"] - ref64["out"]).abs().max())
    e_loss = abs(hip["loss"] - ref64["loss"])
    e_dout = float((hip["dout"] / hip["S"] - ref64["dout"]).abs().max() / ref64["dout"].abs().max())
    print(f"\nUNet output at the HIP context: max abs err {e_out:.2e}; loss {hip['loss']:.7f} vs {ref64['loss']:.7f} (abs err {e_loss:.2e}); "
          f"dL/d(out): rel err {e_dout:.2e}")
    S = hip["S"]
    assert S == 2 ** round(np.log2(S)) and S >= B * H * W
    assert e_out < 2e-5
    assert e_loss < 2e-6 * max(1.0, abs(ref64["loss"]))
    assert e_dout <= 1e-6


@pytest.mark.gpu
def test_unet_gradients(hip, ref64):
    worst, med = _summary("UNet gradients + dL/d(context), fp32-grade", unet_errors(hip["grads"], ref64))
    assert worst < 1e-4 and med < 1e-5


@pytest.mark.gpu
def test_encoder_gradients(hip, ref64):
    worst, med = _summary("encoder gradients, fp32-grade", encoder_errors(hip["grads"], ref64))
    assert worst < 1e-3 and med < 3e-4


# ---------------------------------------------------------------------------------------------- ordering and races: bitwise determinism
@pytest.mark.gpu
def test_a_repeated_step_is_bitwise_identical(hip):
    """the same step from freshly built trainers with the same seeds: every gradient, updated parameter and running statistic the same
    bits (a race between the main stream, the side stream and the deferred join, or an early reuse of a buffer, would show here at this
    shape)"""
    trainer, enc, loss = run_step()
    same = {k: torch.equal(v, hip["bits"][k]) for k, v in _bits(trainer, enc).items()}
    print(f"\nrepeated step: bitwise identical {same}, loss {float(loss):.7f}")
    trainer.close()
    assert all(same.values()) and float(loss) == hip["loss"]


@pytest.mark.gpu
def test_serial_weight_gradients_are_bitwise_identical(hip):
    """overlap_wgrad=False: the weight gradients on the main stream and its handle instead of the side stream and the second handle. The
    kernels and their plans depend on the call, not the handle (conv_wgrad_plan), so the bits are the same"""
    trainer, enc, loss = run_step(overlap_wgrad=False)
    assert trainer.side is None
    same = {k: torch.equal(v, hip["bits"][k]) for k, v in _bits(trainer, enc).items()}
    print(f"\nserial weight gradients: bitwise identical {same}")
    trainer.close()
    assert all(same.values()) and float(loss) == hip["loss"]


# ---------------------------------------------------------------------------------------------- other arithmetic and plans against the same reference
@pytest.mark.gpu
def test_precision16_step(tmp_path, hip, ref64):
    """the step bench.py reports as config.training_step_precision16: plain fp16 operands with fp32 accumulation in the UNet's
    convolutions (the encoder keeps its arithmetic, its gradients inherit the UNet's dL/d(context)). Bounds of
    test_precision16_mode_gradients_are_fp16_grade."""
    g = _child_step(tmp_path, {"CDDPM_TRAIN_PRECISION": "16"})
    uw, um = _summary("UNet gradients + dL/d(context), precision 16", unet_errors(g, ref64))
    ew, em = _summary("encoder gradients, precision 16", encoder_errors(g, ref64))
    print(f"loss precision 16 {float(g['loss']):.7f}, fp32-grade {hip['loss']:.7f}")
    assert uw < 2e-2 and um < 3e-3 and um > 1e-5          # (the mode is really on: fp32-grade arithmetic is far below 1e-5)
    assert ew < 2e-2 and em < 3e-3


@pytest.mark.gpu
def test_step_without_256_cout_workgroups(tmp_path, hip, ref64):
    """CDDPM_NB2=0: every convolution in the 128-cout form. fp32-grade bounds hold, and the gradients differ bitwise from the default run:
    the evidence that the default step really ran the 256-cout workgroups (two-level accumulation sums in another order)"""
    g = _child_step(tmp_path, {"CDDPM_NB2": "0"})
    uw, um = _summary("UNet gradients + dL/d(context), CDDPM_NB2=0", unet_errors(g, ref64))
    ew, em = _summary("encoder gradients, CDDPM_NB2=0", encoder_errors(g, ref64))
    differ = [k for k in g if k.startswith("u:") and not np.array_equal(g[k], hip["grads"][k])]
    print(f"{len(differ)} of 316 UNet gradient tensors differ bitwise from the default plan's")
    assert uw < 1e-4 and um < 1e-5
    assert ew < 1e-3 and em < 3e-4
    assert differ
