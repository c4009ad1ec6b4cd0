"""GPU: dynamic loss scaling of the training step (torch's GradScaler with the scale on the device: cddpm_op_loss_scaled,
cddpm_op_adam_scaled, cddpm_op_scaler_update; UNetTrainer.enable_loss_scaling; the DDPM_2D mirror at precision 16). The scale and growth
tracker follow torch._amp_update_scale_ bit for bit, a step at device scale S is bitwise the fixed-scale step with grad_scale=S, a real
fp16 overflow backs the scale off until a step goes through. Every test that selects precision 16 restores 32 when it ends."""
import functools
import math
import warnings

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture
def tr():
    return load_pkg("training")


@pytest.fixture
def prec16(tr):
    tr.set_precision(16)
    yield tr
    tr.set_precision(32)


def _inputs(synth, B, H, W, T, seed):
    x01 = torch.from_numpy(synth.synth_slices(seed, 0, B, H, W)).reshape(B, 1, H, W)
    cond = torch.from_numpy(synth.synth_cond(seed, 0, B))
    noise = torch.from_numpy(synth.noise_xT(seed, 0, B, H, W)).reshape(B, 1, H, W)
    t = torch.tensor([(137 * (i + 1) + seed) % T for i in range(B)], dtype=torch.long)
    return tuple(v.to(DEV) for v in (x01, cond, noise, t))


def _trainer(tr, sd_np, **scaling):
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(DEV) for k, v in sd_np.items()}, device=DEV)
    if scaling:
        trainer.enable_loss_scaling(**{k: v for k, v in scaling.items() if v is not None})
    return trainer


def _fixed_at(trainer, S):
    """the fixed-scale path at loss scale S (training_step's own loss_and_grad call with grad_scale=S)"""
    trainer.loss_and_grad = functools.partial(trainer.loss_and_grad, grad_scale=S)
    return trainer


def _state(trainer):
    return trainer.flat.clone(), trainer.state["m"].clone(), trainer.state["v"].clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _device_scale(trainer):
    return trainer.scaler[:1].view(torch.float32).cpu()


def test_trajectory_follows_torch_amp_update_scale(prec16, synth, sd_np):
    """10 steps at precision 16, growth interval 3, an inf written into dL/d(out) at steps 1 and 5: after every step the device scale and
    growth tracker are bitwise torch._amp_update_scale_'s on the same found-inf sequence; skipped steps leave flat, m, v as they were"""
    tr = prec16
    trainer = _trainer(tr, sd_np, growth_interval=3)
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, 1000, 5)
    x0 = x01 * 2 - 1
    inject = {1, 5}
    scale_ref = torch.tensor([float(2 ** math.ceil(math.log2(2 * 32 * 32)))], dtype=torch.float32)
    tracker_ref = torch.zeros(1, dtype=torch.int32)
    steps = skipped = 0
    seen_scales = set()
    for i in range(10):
        out = trainer.forward(x0, t, cond)
        _loss, dout = trainer.loss_and_grad(out, noise, None, "l2")
        if i in inject:
            dout[0, 0, 3, 3] = float("inf")
        trainer.backward(dout)
        before = _state(trainer) if "m" in trainer.state else None
        trainer.adam_step(lr=1e-4)                 # unguarded: guard, scaled Adam, scale update
        torch._amp_update_scale_(scale_ref, tracker_ref, torch.tensor([1.0 if i in inject else 0.0]), 2.0, 0.5, 3)
        steps += i not in inject
        skipped += i in inject
        assert torch.equal(_device_scale(trainer), scale_ref), (i, _device_scale(trainer), scale_ref)
        assert trainer.growth_tracker == int(tracker_ref[0]), i
        assert trainer.step_count == steps and trainer.skipped_steps == skipped, i
        assert trainer.consecutive_skips == (1 if i in inject else 0)
        if i in inject:
            assert _same(_state(trainer), before), i
        else:
            assert bool(torch.isfinite(trainer.flat).all())
        seen_scales.add(float(scale_ref[0]))
    assert {1024.0, 2048.0} <= seen_scales                 # the sequence really backed off and grew
    assert trainer.loss_scale == float(scale_ref[0])


@pytest.mark.parametrize("S", [2.0 ** 8, 2.0 ** 14])
def test_a_step_at_device_scale_is_the_fixed_step_at_that_scale(prec16, synth, sd_np, S):
    """one clean training_step with the device scale at S: parameters, m, v bitwise those of the fixed path with grad_scale=S"""
    tr = prec16
    dyn, fix = _trainer(tr, sd_np, init_scale=S), _fixed_at(_trainer(tr, sd_np), S)
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, 1000, 7)
    for trainer in (dyn, fix):
        tr.training_step(trainer, x01, cond, t=t, noise=noise, objective="pred_noise", loss_type="l2")
    assert fix.grad_scale == S and dyn.grad_scale is None
    assert dyn.step_count == fix.step_count == 1 and dyn.skipped_steps == 0
    assert _same(_state(dyn), _state(fix))
    assert dyn.loss_scale == S and dyn.growth_tracker == 1


def test_joint_encoder_step_at_device_scale_is_the_fixed_step(prec16, synth, sd_np):
    """the same with the context encoder trained jointly: one scale, one decision, both Adam updates bitwise the fixed path's"""
    tr, et = prec16, load_pkg("encoder_training")
    S = 2.0 ** 15
    sde = synth.synth_encoder_state_dict(0)
    runs = []
    for scaling in (True, False):
        trainer = _trainer(tr, sd_np, init_scale=S) if scaling else _fixed_at(_trainer(tr, sd_np), S)
        enc = et.EncoderTrainer({k: torch.from_numpy(v) for k, v in sde.items()}, trainer, drop_path_rate=0.0)
        x01, _cond, noise, t = _inputs(synth, 2, 64, 64, 1000, 11)
        tr.training_step(trainer, x01, None, t=t, noise=noise, objective="pred_x0", loss_type="l1", encoder=enc)
        runs.append((trainer, enc))
    (dyn, dyn_enc), (fix, fix_enc) = runs
    assert dyn.step_count == fix.step_count == 1
    assert _same(_state(dyn), _state(fix))
    assert _same(_state(dyn_enc), _state(fix_enc))
    assert not torch.equal(dyn_enc.state["m"], torch.zeros_like(dyn_enc.state["m"]))     # the encoder really stepped


def test_default_start_is_unchanged(prec16, synth, sd_np):
    """default settings, no overflow: the first three steps bitwise those of training_step with the scaler off"""
    tr = prec16
    dyn, fix = _trainer(tr, sd_np, init_scale=None), _trainer(tr, sd_np)
    assert dyn.loss_scaling and not fix.loss_scaling
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, 1000, 5)
    for _ in range(3):
        for trainer in (dyn, fix):
            tr.training_step(trainer, x01, cond, t=t, noise=noise, lr=1e-4)
        assert _same(_state(dyn), _state(fix))
    assert dyn.loss_scale == fix.grad_scale == 2048.0 and dyn.growth_tracker == 3 and dyn.skipped_steps == 0


def test_a_real_overflow_backs_off_until_a_step_goes_through(prec16, synth, sd_np):
    """init scale 2^40 at precision 16, no injection: the fp16 operands of the backward pass overflow, steps are skipped while the scale
    halves, then a step goes through -- bitwise the fixed path's step at the scale reached. A fixed-scale trainer at 2^40 skips as many
    steps and keeps skipping."""
    tr = prec16
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, 1000, 5)
    dyn = _trainer(tr, sd_np, init_scale=2.0 ** 40)
    flat0 = dyn.flat.clone()
    k = 0
    while dyn.step_count == 0:
        assert k < 40, "no step went through"
        S = dyn.loss_scale                              # the scale this step's loss is formed with
        tr.training_step(dyn, x01, cond, t=t, noise=noise, lr=1e-4)
        if dyn.step_count == 0:
            k += 1
            assert torch.equal(dyn.flat, flat0) and dyn.loss_scale == S / 2 and dyn.consecutive_skips == k
    print(f"skipped {k} steps: 2^40 -> 2^{int(math.log2(S))}")
    assert k >= 1 and dyn.skipped_steps == k and dyn.consecutive_skips == 0 and S == 2.0 ** (40 - k)
    ref = _fixed_at(_trainer(tr, sd_np), S)
    tr.training_step(ref, x01, cond, t=t, noise=noise, lr=1e-4)
    assert ref.step_count == 1 and _same(_state(dyn), _state(ref))
    stuck = _fixed_at(_trainer(tr, sd_np), 2.0 ** 40)
    for _ in range(k + 2):
        tr.training_step(stuck, x01, cond, t=t, noise=noise, lr=1e-4)
    assert stuck.step_count == 0 and stuck.skipped_steps == k + 2 and torch.equal(stuck.flat, flat0)


def test_optimizer_state_carries_the_scaler(prec16, synth, sd_np):
    """optimizer_state / load_optimizer_state: the scaler's settings and device block travel under "scaler" and the resumed trainer
    continues bitwise; a state saved without that key leaves a trainer's scaler as it was"""
    tr = prec16
    x01, cond, noise, t = _inputs(synth, 2, 32, 32, 1000, 5)
    a = _trainer(tr, sd_np, init_scale=2.0 ** 12, growth_interval=2)
    for _ in range(3):
        tr.training_step(a, x01, cond, t=t, noise=noise)
    st = a.optimizer_state()
    assert st["scaler"]["growth_interval"] == 2 and a.loss_scale == 2.0 ** 13 and a.growth_tracker == 1
    b = _trainer(tr, sd_np)
    b.flat.copy_(a.flat); b.parameters_changed()
    b.load_optimizer_state(st)
    assert b.loss_scaling and b.loss_scale == 2.0 ** 13 and b.growth_tracker == 1 and b.step_count == 3
    for trainer in (a, b):
        tr.training_step(trainer, x01, cond, t=t, noise=noise)
    assert a.loss_scale == b.loss_scale == 2.0 ** 14 and _same(_state(a), _state(b))
    old = {k: v for k, v in st.items() if k != "scaler"}
    c = _trainer(tr, sd_np)
    c.load_optimizer_state(old)
    assert not c.loss_scaling and c.scaler is None and c.step_count == 3
    d = _trainer(tr, sd_np, init_scale=2.0 ** 9)
    d.load_optimizer_state(old)
    assert d.loss_scaling and d.loss_scale == 2.0 ** 9 and d.scaler is None


# ---------------------------------------------------------------------------------------------- the DDPM_2D mirror
class _Enc(torch.nn.Module):           # a frozen stand-in context encoder: the mirror runs it as a feature extractor
    def forward(self, x):
        return x.flatten(1)[:, :128].contiguous() * 2 - 1


def _mirror(sd_np, **over):
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=1000,
               lr=1e-4)
    cfg.update(over)
    mod = M.DDPM_2D(cfg, encoder=_Enc())
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return mod.cuda()


def _vol(synth, B=2):
    return torch.from_numpy(synth.synth_slices(4, 0, B, 32, 32)).reshape(B, 1, 32, 32, 1).cuda()


def _steps(mod, vol, n, seed=0):
    torch.manual_seed(seed)
    return [mod.training_step({"vol": {"data": vol}}, i)["loss"] for i in range(n)]


@pytest.fixture
def restore32(tr):
    yield
    tr.set_precision(32)


@pytest.mark.parametrize("precision", [16, "16-mixed", "bf16"])
def test_mirror_precision16_turns_the_scaler_on(restore32, sd_np, synth, precision):
    mod = _mirror(sd_np, precision=precision)
    _steps(mod, _vol(synth), 2)
    trainer = mod._hip_unet_trainer
    assert trainer.loss_scaling and trainer.scaler_cfg == (2.0, 0.5, 2000)
    assert trainer.loss_scale == 2048.0 and trainer.growth_tracker == 2 and trainer.step_count == 2


def test_mirror_precision32_is_unchanged(restore32, sd_np, synth):
    """at 32 the scaler stays off: the steps are those of a module without a precision setting, bit for bit"""
    vol = _vol(synth)
    runs = []
    for over in ({"precision": 32}, {}):
        mod = _mirror(sd_np, **over)
        runs.append((mod, torch.stack(_steps(mod, vol, 2))))
    (a, la), (b, lb) = runs
    assert not a._hip_unet_trainer.loss_scaling and a._hip_unet_trainer.scaler is None
    assert torch.equal(la, lb) and torch.equal(a._hip_unet_trainer.flat, b._hip_unet_trainer.flat)


def test_mirror_checkpoint_round_trip_restores_the_scaler(restore32, sd_np, synth):
    vol = _vol(synth)
    mod = _mirror(sd_np, precision=16)
    _steps(mod, vol, 3)
    src = mod._hip_unet_trainer
    ck = {"state_dict": mod.state_dict()}
    mod.on_save_checkpoint(ck)
    sc = ck["hip_optimizer_state"]["unet"]["scaler"]
    assert sc["state"].device.type == "cpu"
    fresh = _mirror(sd_np, precision=16)
    fresh.load_state_dict(ck["state_dict"])
    fresh.on_load_checkpoint(ck)
    dst = fresh.hip_trainer(DEV)
    assert dst.loss_scaling and torch.equal(dst.scaler.cpu(), src.scaler.cpu())
    assert dst.loss_scale == src.loss_scale == 2048.0 and dst.growth_tracker == src.growth_tracker == 3
    _steps(fresh, vol, 1, seed=9)
    assert dst.growth_tracker == 4 and dst.step_count == 4


def test_mirror_seeds_the_scale_from_a_native_amp_checkpoint(restore32, sd_np, synth):
    """a reference checkpoint (no hip_optimizer_state, Lightning 1.5's native_amp_scaling_state): the run resumes with its scale and
    growth tracker"""
    mod = _mirror(sd_np, precision=16)
    mod.on_load_checkpoint({"native_amp_scaling_state": {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                                                         "growth_interval": 2000, "_growth_tracker": 7}})
    _steps(mod, _vol(synth), 1)
    trainer = mod._hip_unet_trainer
    assert trainer.loss_scale == 1024.0 and trainer.growth_tracker == 8 and trainer.step_count == 1


def test_mirror_warns_once_when_every_step_is_skipped(restore32, sd_np, synth):
    """a batch holding a NaN: every step is skipped; the counters are read every 50 steps and the first read that sees >= 30 skips in a
    row warns, once"""
    mod = _mirror(sd_np, precision=16)
    vol = _vol(synth)
    vol[0, 0, 5, 5, 0] = float("nan")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _steps(mod, vol, 49)
        ours = [w for w in seen if issubclass(w.category, RuntimeWarning) and "skipped" in str(w.message)]
        assert ours == []
        _steps(mod, vol, 1)
        ours = [w for w in seen if issubclass(w.category, RuntimeWarning) and "skipped" in str(w.message)]
        assert len(ours) == 1, [str(w.message) for w in seen]
    trainer = mod._hip_unet_trainer
    assert trainer.step_count == 0 and trainer.skipped_steps == 50 and trainer.consecutive_skips == 50
    assert trainer.loss_scale == 2048.0 * 2.0 ** -50
