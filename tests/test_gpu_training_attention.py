"""GPU: training a UNet that has attention inside its resolution levels (`attention_resolutions` matching a down-sampling factor: the
`attn_levels` descriptor of tests/arch_cases.py, and a descriptor with attention at one level only) against float64 autograd through
the oracle, with the limits of tests/test_gpu_training_descriptors.py::test_loss_and_all_gradients_vs_autograd; one optimisation step,
the finality of the gradient buckets, dropout together with level attention, precision 16 and the DDPM_2D mirror with `att_res`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arch_cases as A
from conftest import load_pkg
from test_gpu_training_dropout import _MaskedOracle

pytestmark = pytest.mark.gpu
T = 1000
SEED = 20240611
# attention at ONE level only (ds = 2): 128 x (1, 2, 2), two ResBlocks per level
ONE_LEVEL = dict(model_channels=128, channel_mult=(1, 2, 2), num_res_blocks=2, attention_resolutions=(2,), cond_dim=128, geometry=(2, 16, 24))
DESCRIPTORS = {"attn_levels": A.CASES["attn_levels"], "one_level": ONE_LEVEL}
GRAD_CASES = [("attn_levels", "pred_x0", "l1"), ("attn_levels", "pred_noise", "l2"), ("one_level", "pred_x0", "l1")]
LEVEL_ATTENTION = ("input_blocks.1.1", "input_blocks.3.1", "output_blocks.1.1", "output_blocks.5.1")


def _trainer_kw(case):
    return dict(A.trainer_kw(case), attention_resolutions=case["attention_resolutions"])


def _inputs(synth, case, seed):
    B, H, W = case["geometry"]
    x01 = torch.from_numpy(synth.synth_slices(seed, 0, B, H, W)).reshape(B, 1, H, W)
    cond = torch.from_numpy(synth.synth_cond(seed, 0, B, case["cond_dim"]))
    noise = torch.from_numpy(synth.noise_xT(seed, 0, B, H, W)).reshape(B, 1, H, W)
    t = torch.tensor([(137 * (i + 1) + seed) % T for i in range(B)], dtype=torch.long)
    return x01, cond, noise, t


def _loss_of(out, target, p2w, loss_type):
    d = out - target
    per = (d.abs() if loss_type == "l1" else d ** 2).reshape(d.shape[0], -1).mean(dim=1) * p2w
    return per.mean()


def _oracle_forward(oracle, case, sd, x0, t, noise, cond, buf, dtype):
    return oracle.unet_forward(oracle.q_sample(x0.to(dtype), t, noise.to(dtype), buf), t, cond.to(dtype), sd, **A.unet_kw(case))


_REF = {}


def _reference(oracle, synth, name):
    """per descriptor, once: the synthetic weights, the inputs, and the float64 oracle forward with its autograd graph (every test that
    differentiates it asks for its own vector-Jacobian product and leaves the graph as it is)"""
    if name not in _REF:
        case = DESCRIPTORS[name]
        sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
        x01, cond, noise, t = _inputs(synth, case, 3)
        sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
        buf64 = oracle.to_float64(oracle.schedule_buffers(T))
        ref_out = _oracle_forward(oracle, case, sd, x01 * 2 - 1, t, noise, cond, buf64, torch.float64)
        _REF[name] = dict(case=case, sd_np=sd_np, sd=sd, buf64=buf64, ref_out=ref_out, inputs=(x01, cond, noise, t))
    return _REF[name]


def _check(oracle, synth, name, objective, loss_type, p=0.0):
    """test_gpu_training_descriptors.py::test_loss_and_all_gradients_vs_autograd, link for link, with the trainer built for the case's
    `attention_resolutions` (and dropout p on both sides). Forward within 2e-5 of float64, loss within 2e-6, median relative gradient
    error below 1e-5, every parameter's below 1e-4 of its largest entry -- a limit measured on programs without level attention: a
    parameter over it is held against YARD_FACTOR x the fp32 oracle's own autograd error on that parameter instead, reported beside it."""
    tr = load_pkg("training")
    ref = _reference(oracle, synth, name)
    case, sd_np, sd, buf64 = ref["case"], ref["sd_np"], ref["sd"], ref["buf64"]
    B, H, W = case["geometry"]
    x01, cond, noise, t = ref["inputs"]
    x0 = x01 * 2 - 1
    dev = torch.device("cuda", 0)
    kw = dict(dropout=p, dropout_seed=SEED) if p else {}
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **_trainer_kw(case), **kw)
    try:
        masked = None
        if p:
            masked = _MaskedOracle(oracle, synth, trainer.program, SEED, trainer.dropout_step, 0, p)
            with masked:
                ref_out = _oracle_forward(oracle, case, sd, x0, t, noise, cond, buf64, torch.float64)
        else:
            ref_out = ref["ref_out"]
        target = noise if objective == "pred_noise" else x0
        ref_loss = float(_loss_of(ref_out.detach(), target.double(), buf64["p2_loss_weight"][t], loss_type))
        buf = load_pkg("schedule").schedule_buffers(T)
        xt = (buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise)
        out = trainer.forward(xt.to(dev), t.to(dev), cond.to(dev))
        fwd = float((out.double().cpu() - ref_out.detach()).abs().max())
        print(f"{name} p={p}: forward max|delta| vs float64 {fwd:.3e}")
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
        names = list(sd)
        ref_g = dict(zip(names, torch.autograd.grad(ref_out, [sd[k] for k in names], dout_host, retain_graph=not p)))
        assert set(grads) == set(sd_np), (set(sd_np) - set(grads), set(grads) - set(sd_np))
        worst = []
        for k in sorted(ref_g):
            r = ref_g[k]
            g = grads[k].double().cpu().reshape(r.shape) / S
            assert torch.isfinite(g).all(), k
            worst.append((float((g - r).abs().max() / (r.abs().max() + 1e-30)), k))
        worst.sort(reverse=True)
        median = float(np.median([e for e, _ in worst]))
        print(f"{name} {objective}/{loss_type} p={p}: worst relative gradient errors", [(f"{e:.2e}", k) for e, k in worst[:5]], "median", median)
        print("   level attention:", [(f"{e:.2e}", k) for e, k in worst if k.startswith(LEVEL_ATTENTION) and k.endswith("weight")][:12])
        over = [(e, k) for e, k in worst if not e < 1e-4]
        if over:        # the fp32 oracle's own autograd on the same vector-Jacobian product, for the parameters over the limit
            sd32 = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sd_np.items()}
            if p:
                with masked:
                    o32 = _oracle_forward(oracle, case, sd32, x0, t, noise, cond, oracle.schedule_buffers(T), torch.float32)
            else:
                o32 = _oracle_forward(oracle, case, sd32, x0, t, noise, cond, oracle.schedule_buffers(T), torch.float32)
            o32.backward(dout_host.float())
            yard = {k: float((sd32[k].grad.double() - ref_g[k]).abs().max() / (ref_g[k].abs().max() + 1e-30)) for _e, k in over}
            print("   over 1e-4:", [(f"HIP {e:.2e}", f"fp32 autograd {yard[k]:.2e}", k) for e, k in over])
            over = [(f"HIP {e:.2e}", f"fp32 autograd {yard[k]:.2e}", k) for e, k in over if not e <= A.YARD_FACTOR * yard[k]]
        assert not over, over
        assert median < 1e-5
        return worst
    finally:
        trainer.close()


@pytest.mark.parametrize("name,objective,loss_type", GRAD_CASES, ids=[f"{n}-{o}-{l}" for n, o, l in GRAD_CASES])
def test_loss_and_all_gradients_vs_autograd(oracle, synth, name, objective, loss_type):
    worst = _check(oracle, synth, name, objective, loss_type)
    seen = {k for _e, k in worst}
    if name == "attn_levels":
        assert all(b + s in seen for b in LEVEL_ATTENTION for s in (".norm.weight", ".qkv.weight", ".qkv.bias", ".proj_out.weight"))
    else:
        assert "input_blocks.4.1.qkv.weight" in seen and "output_blocks.5.2.in_layers.2.weight" in seen and "output_blocks.2.1.in_layers.2.weight" in seen


def test_dropout_together_with_level_attention(oracle, synth):
    """`attn_levels` with dropout 0.1, the masks of the trainer given to the oracle (tests/test_gpu_training_dropout.py's route): the
    ResBlock ordinals that key the masks count ResBlocks only, whatever attention sits between them"""
    _check(oracle, synth, "attn_levels", "pred_x0", "l1", p=0.1)


def test_adam_step_moves_the_level_attention_and_repacks(oracle, synth):
    """one optimisation step at `attn_levels` moves every parameter -- the level attention's qkv, proj_out and norm included -- by at most
    Adam's first step, and the forward on the re-packed weight images meets the forward bound against the float64 oracle evaluated at the
    UPDATED weights (tests/test_gpu_training_descriptors.py::test_adam_step_repacks_512_cout_weights)"""
    tr = load_pkg("training")
    case = DESCRIPTORS["attn_levels"]
    dev = torch.device("cuda", 0)
    sd_np = _reference(oracle, synth, "attn_levels")["sd_np"]
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **_trainer_kw(case))
    try:
        x01, cond, noise, t = _inputs(synth, case, 5)
        loss = float(tr.training_step(trainer, x01.to(dev), cond.to(dev), t=t.to(dev), noise=noise.to(dev), timesteps=T, lr=1e-4))
        assert np.isfinite(loss) and trainer.step_count == 1 and trainer.skipped_steps == 0
        moved_by = {k: float((trainer.p[k].cpu() - torch.from_numpy(v)).abs().max()) for k, v in sd_np.items()}
        still = [k for k, m in moved_by.items() if not m > 0]
        assert not still, still
        for b in LEVEL_ATTENTION:
            for s in (".norm.weight", ".norm.bias", ".qkv.weight", ".qkv.bias", ".proj_out.weight", ".proj_out.bias"):
                assert moved_by[b + s] > 0, b + s
        assert max(moved_by.values()) <= 1.01e-4, max(moved_by.values())                       # Adam's first step: lr * sign(g)
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
        print(f"attn_levels after one Adam step: forward max|delta| vs float64 at the updated weights {err:.3e}; the update moved the output by {moved:.3e}")
        assert moved > 10 * 2e-5     # the check discriminates: stale weight images would miss the bound below by an order of magnitude
        assert err < 2e-5
    finally:
        trainer.close()


def test_gradient_buckets_are_final_with_attention_inside_the_levels(oracle, synth):
    """tests/test_gpu_training.py::test_gradient_buckets_are_final_when_they_are_handed_to_the_collective at `attn_levels`: the flat
    buffer is in forward order with the attention blocks inside it, so after `mark_final(lo)` of any backward operator -- an attention
    included -- [lo, end) does not change any more"""
    tr = load_pkg("training")
    case = DESCRIPTORS["attn_levels"]
    dev = torch.device("cuda", 0)
    sd_np = _reference(oracle, synth, "attn_levels")["sd_np"]
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **_trainer_kw(case))

    class Recorder:
        def __init__(self, flat):
            self.flat, self.marks = flat, []

        def mark_final(self, lo):
            self.marks.append((int(lo), self.flat[int(lo):].clone()))

    try:
        x01, cond, noise, t = (v.to(dev) for v in _inputs(synth, case, 5))
        out = trainer.forward(x01 * 2 - 1, t, cond)
        _loss, dout = trainer.loss_and_grad(out, noise, None, "l2")
        trainer.gflat.fill_(float("nan"))
        rec = Recorder(trainer.gflat)
        trainer.backward(dout, rec)
        torch.cuda.synchronize()
        assert len(rec.marks) == len(trainer.program)
        los = [lo for lo, _ in rec.marks]
        assert los == sorted(los, reverse=True) and los[0] < rec.flat.numel()          # the final region grows from the tail
        # every attention block owns an offset of its own: its mark moves the final region
        at = [i for i, (kind, _n, _a) in enumerate(reversed(trainer.program)) if kind == "attn"]
        assert len(at) == 10 and all(los[i] < los[i - 1] for i in at)
        for lo, snap in rec.marks:
            now = rec.flat[lo:]
            same = (snap == now) | (torch.isnan(snap) & torch.isnan(now))               # padding between tensors stays NaN-filled
            assert bool(same.all()), lo
            assert not bool(torch.isnan(now[: 64]).all())                               # ... and the region really holds gradients
    finally:
        trainer.close()


def test_precision16_mode_gradients_are_fp16_grade_with_level_attention():
    """test_gpu_training_descriptors.py::test_precision16_mode_gradients_are_fp16_grade_at_256_channels (its rule, its limits) at
    `attn_levels`: no contraction is longer than at `w256`. Own process (the arithmetic is chosen once per process)."""
    case = DESCRIPTORS["attn_levels"]
    B, H, W = case["geometry"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    desc = json.dumps({k: case[k] for k in ("model_channels", "channel_mult", "num_res_blocks", "cond_dim", "attention_resolutions")})
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_grad_check.py"), str(B), str(H), str(W), desc],
                       env=dict(os.environ, CDDPM_TRAIN_PRECISION="16"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("precision 16, attn_levels:", res)
    n = len(load_pkg("synth").unet_param_shapes(**A.synth_kw(case)))
    assert res["finite"] and res["n"] == n
    assert res["forward_max_abs_err"] < 5e-3 and res["worst"] < 2e-2 and res["median"] < 3e-3
    assert res["median"] > 1e-5


def test_mirror_trains_and_evaluates_with_att_res(synth):
    """DDPM_2D with `att_res: [1, 2, 4]` (the one cfg key the reference changes): training_step runs on the HIP operators and moves a
    level attention's weights, state_dict() sees them, and validation_step / test_step run on the trained weights"""
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], num_res_blocks=1, att_res=[1, 2, 4], condition=True,
               test_timesteps=500, timesteps=1000, lr=1e-4, noise_ensemble=False)

    class Enc(torch.nn.Module):          # stand-in for the context encoder (not updated by training_step)
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous() * 2 - 1

    mod = M.DDPM_2D(cfg, encoder=Enc())
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(DESCRIPTORS["attn_levels"]))
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    mod = mod.cuda()
    try:
        vol = torch.from_numpy(synth.synth_slices(4, 0, 2, 32, 32)).reshape(2, 1, 32, 32, 1).cuda()
        w0 = mod.diffusion.model.state_dict()["input_blocks.1.1.qkv.weight"].clone()
        torch.manual_seed(0)
        loss = float(mod.training_step({"vol": {"data": vol}}, 0)["loss"])
        assert np.isfinite(loss)
        assert mod.hip_trainer(vol.device).att_res == (1, 2, 4)
        w1 = mod.diffusion.model.state_dict()["input_blocks.1.1.qkv.weight"]
        assert 0 < float((w1 - w0).abs().max()) <= 1.01e-4
        val = mod.validation_step({"vol": {"data": vol}}, 0)
        assert torch.isfinite(val["loss"])
        vol3d = torch.from_numpy(synth.synth_slices(2, 0, 6, 32, 32)).permute(1, 2, 3, 0).unsqueeze(0).contiguous().cuda()     # [1,1,H,W,D]
        out = mod.test_step({"vol": {"data": vol3d}}, 0)
        assert torch.isfinite(out["final_volume"]).all()
    finally:
        mod.hip_trainer(vol.device).close()
        mod.diffusion.model._hip.close()
