"""GPU: the training step at descriptors other than the experiment's (tests/arch_cases.py) -- 256 and 512 channels (the head and the
device weight packer at Cout 512, E = 2048, no label_emb), four levels (15 tokens in the attention backward), channel_mult[0] = 2 --
against float64 autograd through the oracle, with the limits of tests/test_gpu_training.py::test_loss_and_all_gradients_vs_autograd."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arch_cases as A
from conftest import load_pkg

pytestmark = pytest.mark.gpu
T = 1000
GRAD_CASES = [("w256", "pred_x0", "l1"), ("deep4", "pred_x0", "l1"), ("mult0_2", "pred_x0", "l1"), ("w512_uncond", "pred_x0", "l1"),
              ("w256", "pred_noise", "l2")]


def _inputs(synth, case, seed):
    B, H, W = case["geometry"]
    x01 = torch.from_numpy(synth.synth_slices(seed, 0, B, H, W)).reshape(B, 1, H, W)
    cond = torch.from_numpy(synth.synth_cond(seed, 0, B, case["cond_dim"])) if case["cond_dim"] else None
    noise = torch.from_numpy(synth.noise_xT(seed, 0, B, H, W)).reshape(B, 1, H, W)
    t = torch.tensor([(137 * (i + 1) + seed) % T for i in range(B)], dtype=torch.long)
    return x01, cond, noise, t


def _loss_of(out, target, p2w, loss_type):
    d = out - target
    per = (d.abs() if loss_type == "l1" else d ** 2).reshape(d.shape[0], -1).mean(dim=1) * p2w
    return per.mean()


def _to(v, dev):
    return None if v is None else v.to(dev)


def _oracle_forward(oracle, case, sd, x0, t, noise, cond, buf, dtype):
    c = None if cond is None else cond.to(dtype)
    return oracle.unet_forward(oracle.q_sample(x0.to(dtype), t, noise.to(dtype), buf), t, c, sd, **A.unet_kw(case))


@pytest.mark.parametrize("name,objective,loss_type", GRAD_CASES, ids=[f"{n}-{o}-{l}" for n, o, l in GRAD_CASES])
def test_loss_and_all_gradients_vs_autograd(oracle, synth, name, objective, loss_type):
    """test_gpu_training.py::test_loss_and_all_gradients_vs_autograd, link for link and limit for limit, at another descriptor. Should a
    parameter exceed a limit, the fp32 oracle's own autograd error on that parameter is measured and reported beside it."""
    tr = load_pkg("training")
    case = A.CASES[name]
    B, H, W = case["geometry"]
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    x01, cond, noise, t = _inputs(synth, case, 3)
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
    buf64 = oracle.to_float64(oracle.schedule_buffers(T))
    x0 = x01 * 2 - 1
    ref_out = _oracle_forward(oracle, case, sd, x0, t, noise, cond, buf64, torch.float64)
    target = noise if objective == "pred_noise" else x0
    ref_loss = float(_loss_of(ref_out.detach(), target.double(), buf64["p2_loss_weight"][t], loss_type))

    dev = torch.device("cuda", 0)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **A.trainer_kw(case))
    try:
        buf = load_pkg("schedule").schedule_buffers(T)
        xt = (buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise)
        out = trainer.forward(xt.to(dev), t.to(dev), _to(cond, dev))
        fwd = float((out.double().cpu() - ref_out.detach()).abs().max())
        print(f"{name}: forward max|delta| vs float64 {fwd:.3e}")
        assert fwd < 2e-5
        # link 1: the loss kernel
        loss, dout = trainer.loss_and_grad(out, target.to(dev), buf["p2_loss_weight"][t].to(dev).contiguous(), loss_type)
        assert abs(float(loss) - ref_loss) < 2e-6 * max(1.0, abs(ref_loss))
        o64 = out.double().cpu().requires_grad_(True)
        _loss_of(o64, target.double(), buf64["p2_loss_weight"][t], loss_type).backward()
        S = trainer.grad_scale
        assert S == 2 ** round(np.log2(S)) and S >= B * H * W
        assert float((dout.double().cpu() / S - o64.grad).abs().max()) <= 1e-6 * float(o64.grad.abs().max())
        # link 2: the backward pass
        grads = trainer.backward(dout)
        torch.cuda.synchronize()
        dout_host = dout.double().cpu() / S
        ref_out.backward(dout_host)
        ref_g = {k: v.grad for k, v in sd.items()}
        assert set(grads) == set(ref_g), (set(ref_g) - set(grads), set(grads) - set(ref_g))
        worst = []
        for k in sorted(ref_g):
            r = ref_g[k]
            g = grads[k].double().cpu().reshape(r.shape) / S
            assert torch.isfinite(g).all(), k
            worst.append((float((g - r).abs().max() / (r.abs().max() + 1e-30)), k))
        worst.sort(reverse=True)
        median = float(np.median([e for e, _ in worst]))
        print(f"{name} {objective}/{loss_type}: worst relative gradient errors", [(f"{e:.2e}", k) for e, k in worst[:5]], "median", median)
        over = [(e, k) for e, k in worst if not e < 1e-4]
        if over:        # the fp32 oracle's own autograd on the same vector-Jacobian product, for the parameters over the limit
            sd32 = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sd_np.items()}
            _oracle_forward(oracle, case, sd32, x0, t, noise, cond, oracle.schedule_buffers(T), torch.float32).backward(dout_host.float())
            over = [(f"HIP {e:.2e}", f"fp32 autograd {float((sd32[k].grad.double() - ref_g[k]).abs().max() / (ref_g[k].abs().max() + 1e-30)):.2e}", k)
                    for e, k in over]
        assert not over, over
        assert median < 1e-5
    finally:
        trainer.close()


def test_precision16_mode_gradients_are_fp16_grade_at_256_channels():
    """test_gpu_training.py::test_precision16_mode_gradients_are_fp16_grade (its rule, its limits) on `w256`: contractions over up to
    1024 x 9 fp16 products. Own process (the arithmetic is chosen once per process)."""
    case = A.CASES["w256"]
    B, H, W = case["geometry"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    desc = json.dumps({k: case[k] for k in ("model_channels", "channel_mult", "num_res_blocks", "cond_dim")})
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_grad_check.py"), str(B), str(H), str(W), desc],
                       env=dict(os.environ, CDDPM_TRAIN_PRECISION="16"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("precision 16, w256:", res)
    n = len(load_pkg("synth").unet_param_shapes(**A.synth_kw(case)))
    assert res["finite"] and res["n"] == n
    assert res["forward_max_abs_err"] < 5e-3 and res["worst"] < 2e-2 and res["median"] < 3e-3
    assert res["median"] > 1e-5


def test_level_attention_state_dict_is_refused(synth):
    """a state dict with attention inside the resolution levels (`attn_levels`): the trainer's program has attention in the middle block
    only, so those parameters would silently keep zero gradients -- UNetTrainer names the blocks instead of building such a program"""
    tr = load_pkg("training")
    case = A.CASES["attn_levels"]
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    assert "input_blocks.1.1.qkv.weight" in sd_np and "output_blocks.1.2.in_layers.2.weight" in sd_np
    with pytest.raises(NotImplementedError, match=r"input_blocks\.1\.1.*output_blocks\.1\.1") as ei:
        tr.UNetTrainer({k: torch.from_numpy(v) for k, v in sd_np.items()}, device=torch.device("cuda", 0), **A.trainer_kw(case))
    assert "attention" in str(ei.value)


def test_adam_step_repacks_512_cout_weights(oracle, synth):
    """one optimisation step on `w256` moves every parameter, and the forward on the re-packed weight images (the device packer at
    Cout 512 and Cin 1024) still meets the forward bound against the float64 oracle evaluated at the UPDATED weights"""
    tr = load_pkg("training")
    case = A.CASES["w256"]
    dev = torch.device("cuda", 0)
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **A.trainer_kw(case))
    try:
        x01, cond, noise, t = _inputs(synth, case, 5)
        loss = float(tr.training_step(trainer, x01.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev), timesteps=T, lr=1e-4))
        assert np.isfinite(loss) and trainer.step_count == 1 and trainer.skipped_steps == 0
        still = [k for k, v in sd_np.items() if not float((trainer.p[k].cpu() - torch.from_numpy(v)).abs().max()) > 0]
        assert not still, still
        step = max(float((trainer.p[k].cpu() - torch.from_numpy(v)).abs().max()) for k, v in sd_np.items())
        assert step <= 1.01e-4, step                       # Adam's first step: lr * sign(g)
        sd64 = {k: trainer.p[k].detach().double().cpu() for k in sd_np}
        x2, cond2, noise2, t2 = _inputs(synth, case, 7)
        buf = load_pkg("schedule").schedule_buffers(T)
        x0 = x2 * 2 - 1
        xt = (buf["sqrt_alphas_cumprod"][t2].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t2].reshape(-1, 1, 1, 1) * noise2)
        with torch.no_grad():
            ref = oracle.unet_forward(xt.double(), t2, cond2.double(), sd64, **A.unet_kw(case))
            old = oracle.unet_forward(xt.double(), t2, cond2.double(), oracle.to_float64(oracle.to_torch_sd(sd_np)), **A.unet_kw(case))
        out = trainer.forward(xt.to(dev), t2.to(dev), cond2.to(dev))
        err = float((out.double().cpu() - ref).abs().max())
        moved = float((old - ref).abs().max())
        print(f"w256 after one Adam step: forward max|delta| vs float64 at the updated weights {err:.3e}; the update moved the output by {moved:.3e}")
        assert moved > 10 * 2e-5     # the check discriminates: stale weight images would miss the bound below by an order of magnitude
        assert err < 2e-5
    finally:
        trainer.close()
