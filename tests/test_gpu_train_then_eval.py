"""GPU: the seam between training and evaluation. The optimiser kernels write the parameters (and the encoder's BatchNorm kernels the
running statistics) in place, outside torch's version counters, so everything the evaluation side derived from them has to be dropped
by hand: the UNet engine's packed weights (HipBackend.invalidate), the exact-family rescue engine (_close_fallback), the precision-16
pack with its pre-scale exponents, the native ResNet-50's inference handle (ResNet50Encoder.invalidate, called by the EncoderTrainer).

The instrument needs no tolerance: an evaluation call of a module that has trained equals, with torch.equal, the same call of a FRESH
module built from a deep CPU copy of the trained module's state_dict(). The plan of a convolution is part of its bits, so both modules
only ever see one (B, H, W) -- 4 x 64 x 64, the size of the joint-training tests of test_gpu_mirror.py, whose builder is used -- and
the trained module makes the evaluation call once BEFORE its first step, so that an engine and an encoder handle exist to go stale.
numpy and torch are reseeded before every step and every evaluation call. One float64 anchor (oracles on the trained state dict) keeps
"both stale in the same way" from passing."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_pkg
from test_gpu_mirror import _experiment_module

pytestmark = pytest.mark.gpu

B, H, W = 4, 64, 64


def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


def _module(sd_np, synth, spark=False, **over):
    """test_gpu_mirror._experiment_module (native ResNet-50, pred_x0, l1); spark: the same cfg with the experiment's SparK-wrapped
    encoder, built by the module itself (state dict keys encoder.encoder.*)"""
    over.setdefault("noisetype", None)
    if not spark:
        return _experiment_module(sd_np, synth, **over)
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[128, 128, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=1000,
               lr=1e-4, backbone="Spark_Encoder_2D", version="resnet50", cond_dim=128, objective="pred_x0", loss="l1")
    cfg.update(over)
    mod = M.DDPM_2D(cfg)
    mod.encoder.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, strict=False)
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return mod.cuda()


def _close(mod):
    if getattr(mod, "_hip_unet_trainer", None) is not None:
        mod._hip_unet_trainer.close()
    mod.diffusion.model._hip.close()
    enc = getattr(mod, "encoder", None)
    enc = getattr(enc, "encoder", enc)
    if hasattr(enc, "close"):
        enc.close()


@pytest.fixture(scope="module")
def data(synth):
    vol = torch.from_numpy(synth.synth_slices(4, 0, B, H, W)).reshape(B, 1, H, W, 1).cuda()
    inp = vol.squeeze(-1).contiguous()
    big = inp.clone()
    big[2] *= 3.0e5              # test_gpu_conv_family.py::test_ddpm2d_conv_fallback_key: slice 2 leaves the fp16 range on the single-step path
    return dict(vol=vol, inp=inp, big=big, noise=torch.from_numpy(synth.noise_z(3, 0, 0, B, H, W)).cuda())


def _train(mod, data, first, steps):
    for i in range(first, first + steps):
        _seed(100 + i)
        loss = float(mod.training_step({"vol": {"data": data["vol"]}}, i)["loss"])
        assert np.isfinite(loss)


def _state(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}


def _evaluate(mod, data, overflow=False):
    """the three evaluation calls, each under its own fixed seed: the context, the reconstruction with explicit noise (overflow: of the
    batch whose slice 2 overflows, with the context of the plain batch) and validation_step. RuntimeWarnings are collected."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _seed(21)
        ctx = mod(data["inp"]).clone()
        _seed(22)
        loss, reco = mod.reconstruct(data["big"] if overflow else data["inp"], ctx, data["noise"], mod.test_timesteps)
        _seed(23)
        val = mod.validation_step({"vol": {"data": data["vol"]}}, 0)["loss"]
    out = dict(ctx=ctx, loss=loss, reco=reco, val=val)
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    out["warnings"] = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
    return out


def _same(got, want, what):
    for k in want:
        if k == "warnings":
            assert got[k] == want[k], (what, got[k], want[k])
            continue
        assert bool(torch.isfinite(got[k]).all()), (what, k)
        assert torch.equal(got[k], want[k]), (what, k, float((got[k].double() - want[k].double()).abs().max()))


def _moved(before, after, what, least=1e-4):
    """two evaluations with training in between differ (by test_gpu_mirror.py's 1e-4 after three steps): the comparison with the fresh
    module is not vacuous"""
    assert float((after["ctx"] - before["ctx"]).abs().max()) > least, what
    assert float((after["reco"] - before["reco"]).abs().max()) > least, what


def _fresh_eval(sd_np, synth, data, state, *, spark=False, overflow=False, **over):
    fresh = _module(sd_np, synth, spark, **over)
    try:
        fresh.load_state_dict(state)
        return _evaluate(fresh, data, overflow)
    finally:
        _close(fresh)


# ---- joint training, plain evaluation: shared by the bit-for-bit case and the float64 anchor ---------------------------------------------
@pytest.fixture(scope="module")
def trained_plain(sd_np, synth, data):
    mod = _module(sd_np, synth)
    initial = _state(mod)
    probe = _evaluate(mod, data)
    _train(mod, data, 0, 3)
    state = _state(mod)
    got = _evaluate(mod, data)
    yield dict(mod=mod, initial=initial, probe=probe, state=state, got=got)
    _close(mod)


def test_joint_training_then_evaluation_equals_a_fresh_module(trained_plain, sd_np, synth, data):
    r = trained_plain
    _moved(r["probe"], r["got"], "plain")
    assert r["got"]["warnings"] == []
    _same(r["got"], _fresh_eval(sd_np, synth, data, r["state"]), "plain")


def test_trained_module_against_the_float64_oracles(trained_plain, synth, oracle):
    """the trained module against the oracles on its OWN state dict: the context against encoder_oracle.resnet50_forward (eval mode on
    the trained running statistics) with test_gpu_encoder.py's rule, the UNet's output at t = 500 against oracle.unet_forward with
    test_gpu_unet.py::test_rounding_yardstick_fp64's; e_ref is the fp32 oracle's own distance from float64, computed here"""
    import encoder_oracle as EO
    r = trained_plain
    state, initial = r["state"], r["initial"]
    rm = [k for k in state if k.startswith("encoder.") and (k.endswith("running_mean") or k.endswith("running_var"))]
    assert len(rm) == 2 * 53
    for k in rm:                                                         # every BatchNorm's statistics moved in training
        assert float((state[k] - initial[k]).abs().max()) > 1e-7, k
    assert float((state["encoder.layer3.2.conv2.weight"] - initial["encoder.layer3.2.conv2.weight"]).abs().max()) > 1e-5
    _moved(r["probe"], r["got"], "anchor")
    enc_sd = {k[len("encoder."):]: v for k, v in state.items() if k.startswith("encoder.") and v.is_floating_point()}
    x = torch.from_numpy(synth.synth_slices(4, 0, B, H, W))              # data["inp"], on the host
    with torch.no_grad():
        ref32 = EO.resnet50_forward(x, enc_sd)
        ref64 = EO.resnet50_forward(x.double(), {k: v.double() for k, v in enc_sd.items()})
    e_ref, e_hip = float((ref32.double() - ref64).abs().max()), float((r["got"]["ctx"].double() - ref64).abs().max())
    print(f"trained context vs float64: torch fp32 {e_ref:.3e}, HIP {e_hip:.3e}")
    assert e_hip < 10 * e_ref + 1e-6
    # the UNet on its trained weights, one slice at the trained size
    unet_sd = {k[len("diffusion.model."):]: v for k, v in state.items() if k.startswith("diffusion.model.")}
    xt = torch.from_numpy(synth.noise_xT(2, 0, 1, H, W))
    t = torch.tensor([500])
    cond = r["got"]["ctx"][:1].clone()
    out = r["mod"].diffusion.model(xt.cuda(), t.cuda(), cond=cond.cuda()).cpu()
    with torch.no_grad():
        u32 = oracle.unet_forward(xt, t, cond, unet_sd)
        u64 = oracle.unet_forward(xt.double(), t, cond.double(), oracle.to_float64(unet_sd))
    e_ref, e_hip = float((u32.double() - u64).abs().max()), float((out.double() - u64).abs().max())
    print(f"trained UNet at t=500 vs float64: torch fp32 {e_ref:.3e}, HIP {e_hip:.3e}")
    assert e_hip < 4 * e_ref + 1e-6


# ---- every engine the backend can hold, and the SparK-wrapped encoder -------------------------------------------------------------------
CASES = {
    "plain": dict(),
    "spark_simplex": dict(spark=True, noisetype="simplex"),
    "eval_precision16": dict(eval_precision=16),
    "attention_h3": dict(attention_family="h3"),
    "conv_fallback_x6": dict(conv_fallback="x6"),
    "reverse_sampling": dict(reverse_sampling=True, reverse_start_t=3),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_then_evaluate_under_every_engine(sd_np, synth, data, name):
    """probe, 3 steps, evaluate = a fresh module's evaluation. Here the trainers are created BEFORE the probe: creating them re-points
    the module's parameters at the trainers' flat buffers, and an engine or encoder handle built before that is rebuilt on the next
    call for the new data pointers alone, whether or not anybody invalidated it (the order of trained_plain above). Built on the
    aliased tensors, the probe's engines see neither a pointer nor a version change in three steps: only the hand-made invalidations
    keep them from going stale. conv_fallback: the evaluation input carries one overflowing slice, so the rescue engine is created
    before training and needed again after it -- the rescued slice equals the fresh module's and the evaluation issues the same
    single RuntimeWarning"""
    over = dict(CASES[name])
    spark = over.pop("spark", False)
    overflow = name == "conv_fallback_x6"
    mod = _module(sd_np, synth, spark, **over)
    try:
        dev = data["inp"].device
        assert mod.hip_trainer(dev) is not None and mod.hip_encoder_trainer(dev) is not None
        probe = _evaluate(mod, data, overflow)
        if overflow:
            assert mod.diffusion.model._hip._fallback_engine is not None
        _train(mod, data, 0, 3)
        state = _state(mod)
        got = _evaluate(mod, data, overflow)
    finally:
        _close(mod)
    _moved(probe, got, name)
    want = _fresh_eval(sd_np, synth, data, state, spark=spark, overflow=overflow, **over)
    if overflow:
        for ev in (probe, got, want):
            assert len(ev["warnings"]) == 1 and "1 of 4 slices" in ev["warnings"][0] and "x6" in ev["warnings"][0], ev["warnings"]
        assert bool(torch.isfinite(got["reco"][2]).all()) and torch.equal(got["reco"][2], want["reco"][2])
    else:
        assert got["warnings"] == []
    _same(got, want, name)


# ---- interleaving -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interleaved(sd_np, synth, data):
    """probe, train 2, evaluate, train 1, evaluate -- with the state dict at each evaluation"""
    mod = _module(sd_np, synth)
    try:
        _evaluate(mod, data)
        _train(mod, data, 0, 2)
        state2, eval2 = _state(mod), _evaluate(mod, data)
        _train(mod, data, 2, 1)
        state3, eval3 = _state(mod), _evaluate(mod, data)
    finally:
        _close(mod)
    return dict(state2=state2, eval2=eval2, state3=state3, eval3=eval3)


def test_interleaved_evaluations_each_equal_a_fresh_module(interleaved, sd_np, synth, data):
    """an invalidation that works only once shows at the second evaluation"""
    r = interleaved
    _moved(r["eval2"], r["eval3"], "between the two evaluations", least=1e-5)          # one step apart
    _same(r["eval2"], _fresh_eval(sd_np, synth, data, r["state2"]), "after 2 steps")
    _same(r["eval3"], _fresh_eval(sd_np, synth, data, r["state3"]), "after 2 + 1 steps")


def test_evaluation_between_steps_does_not_disturb_training(interleaved, sd_np, synth, data):
    """train 2, evaluate, train 1 leaves the parameters, running statistics and counters of an uninterrupted train 3 with the same
    per-step seeds, bit for bit: evaluation touches neither the trainers' handles nor their scratch nor their packed images"""
    mod = _module(sd_np, synth)
    try:
        _train(mod, data, 0, 3)
        want = _state(mod)
    finally:
        _close(mod)
    got = interleaved["state3"]
    assert set(got) == set(want)
    worst = {k: float((got[k].double() - want[k].double()).abs().max()) for k in want if not torch.equal(got[k], want[k])}
    assert not worst, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


# ---- the patched mirror -------------------------------------------------------------------------------------------------------------------
def _patched(synth):
    P = load_pkg("DDPM_2D_patched")
    cfg = dict(imageDim=[96, 96, 5], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], patch_size=16, grid_boxes=True, inpaint=True,
               objective="pred_x0", loss="l1", test_timesteps=351, lr=1e-4, num_eval_slices=3)           # test_gpu_patched.py::_mirror
    mod = P.DDPM_2D(cfg)
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, num_classes=None).items()}, strict=True)
    return mod.cuda()


def test_patched_mirror_train_then_evaluate_equals_a_fresh_module(synth):
    x01 = torch.from_numpy(synth.synth_slices(2, 0, 2, 32, 32)).reshape(2, 1, 32, 32).cuda()
    batch = {"vol": {"data": x01.unsqueeze(-1)}}
    vol5 = torch.from_numpy(synth.synth_slices(2, 0, 5, 32, 32)).cuda()
    tb = {"vol": {"data": vol5[:, 0].permute(1, 2, 0)[None, None].contiguous()}}            # [1,1,32,32,5]

    def evaluate(mod):
        _seed(31)
        val = mod.validation_step(batch, 0)["loss"].detach().cpu().clone()
        _seed(32)
        out = mod.test_step(tb, 0)
        return dict(val=val, loss=out["loss"].detach().cpu().clone(), volume=out["final_volume"].detach().cpu().clone())

    mod = _patched(synth)
    try:
        mod.hip_trainer(x01.device)            # before the probe, as above: the probe's engine is built on the aliased parameters
        _seed(31)
        probe =mod.validation_step(batch, 0)["loss"].detach().cpu().clone()
        for i in range(3):
            _seed(100 + i)
            assert np.isfinite(float(mod.training_step(batch, i)["loss"]))
        state = _state(mod)
        got = evaluate(mod)
    finally:
        _close(mod)
    assert float((got["val"] - probe).abs()) > 1e-6
    fresh = _patched(synth)
    try:
        fresh.load_state_dict(state)
        want = evaluate(fresh)
    finally:
        _close(fresh)
    assert got["volume"].shape == (1, 1, 32, 32, 3)
    _same(got, want, "patched")


# ---- parameters written after the engines exist, without a training step ---------------------------------------------------------------
def test_load_state_dict_after_evaluation_equals_a_fresh_module(sd_np, synth, data):
    unet = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(3).items()}
    enc = {k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(1).items()}

    def load(mod):
        mod.diffusion.model.load_state_dict(unet)
        mod.encoder.load_state_dict(enc, strict=False)

    mod = _module(sd_np, synth)
    try:
        probe = _evaluate(mod, data)
        load(mod)
        got = _evaluate(mod, data)
    finally:
        _close(mod)
    _moved(probe, got, "other weights")
    fresh = _module(sd_np, synth)
    try:
        load(fresh)
        want = _evaluate(fresh, data)
    finally:
        _close(fresh)
    _same(got, want, "load_state_dict")


# ---- the trainers driven directly -----------------------------------------------------------------------------------------------------------
def test_encoder_handle_follows_a_directly_driven_training_step(sd_np, synth, data):
    """training.training_step(trainer, ..., encoder=enc_trainer) called by hand, not through DDPM_2D.training_step: the module's
    encoder, whose handle was built on the aliased tensors BEFORE the step (their data pointers and versions do not change any more),
    must still return the context of the updated weights and running statistics -- after the first such step and after the second"""
    tr = load_pkg("training")
    mod = _module(sd_np, synth)
    try:
        dev = data["inp"].device
        trainer, enc_trainer = mod.hip_trainer(dev), mod.hip_encoder_trainer(dev)
        d = mod.diffusion
        _seed(21)
        before = mod(data["inp"]).clone()
        for i in range(2):
            _seed(100 + i)
            t = torch.randint(0, d.num_timesteps, (B,), device=dev).long()
            tr.training_step(trainer, data["inp"], None, t=t, noise=torch.randn_like(data["inp"]), timesteps=d.num_timesteps,
                             encoder=enc_trainer, objective=d.objective, loss_type=d.loss_type, lr=1e-4)
            state = _state(mod)
            _seed(21)
            got = mod(data["inp"]).clone().cpu()
            fresh = _module(sd_np, synth)
            try:
                fresh.load_state_dict(state)
                _seed(21)
                want = fresh(data["inp"]).clone().cpu()
            finally:
                _close(fresh)
            assert float((got - before.cpu()).abs().max()) > 1e-5, i
            assert torch.equal(got, want), (i, float((got - want).abs().max()))
            before = got
    finally:
        _close(mod)
