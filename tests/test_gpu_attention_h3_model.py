"""GPU: the h3 attention family inside the model. An engine built with attention_family="h3" meets the block-by-block comparison with
the oracle (tests/test_gpu_unet.py::test_unet_blocks_vs_oracle on the middle-attention model, tests/test_gpu_unet_descriptors.py's rule on
`attn_levels`, where every block has an attention) and the golden reverse loops under their own bound; a trainer built with
attention_family="h3" meets tests/test_gpu_training_attention.py's check of the loss and every parameter gradient against float64
autograd, unchanged; and precision 16 wins: a precision-16 engine and an attention_precision=16 trainer compute the same bits whatever
the family says."""
import numpy as np
import pytest
import torch

import arch_cases as A
import test_gpu_training_attention as TA
import test_gpu_unet as U
import test_gpu_unet_descriptors as D
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu


def _engine(sd_np, timesteps, max_batch=4, max_h=128, max_w=128, **kw):
    e = load_pkg("engine").CddpmEngine(timesteps=timesteps, max_batch=max_batch, max_h=max_h, max_w=max_w, **kw)
    e.load_weights(sd_np)
    e.set_schedule(load_pkg("schedule").schedule_buffers(timesteps, "cosine"), "pred_x0")
    return e


@pytest.fixture(scope="module")
def h3_engines(sd_np):
    made = {T: _engine(sd_np, T, attention_family="h3") for T in (1000, 50)}
    yield made
    for e in made.values():
        e.close()


def test_unet_blocks_vs_oracle_with_h3_attention(h3_engines, synth, oracle, sd_torch):
    eng = h3_engines[1000]
    assert eng.attention_family == "h3" and eng.precision == 32
    U.test_unet_blocks_vs_oracle(eng, synth, oracle, sd_torch)


def test_level_attention_blocks_vs_float64_oracle_with_h3_attention(synth, oracle):
    case = A.CASES["attn_levels"]
    mb, mh, mw = case["geometry"]
    eng = load_pkg("engine").CddpmEngine(timesteps=1000, max_batch=mb, max_h=mh, max_w=mw, attention_family="h3", **A.engine_kw(case))
    try:
        eng.load_weights(D.weights(synth, "attn_levels"))
        eng.set_schedule(load_pkg("schedule").schedule_buffers(1000, "cosine"), "pred_x0")
        D.check_blocks(eng, synth, oracle, "attn_levels", "h3 attention")
        # the switch reaches every attention block: the exact family computes other bits on the same handle
        x, cond, t, _r64, _r32 = D.references(synth, oracle, "attn_levels", "tmixed")
        split = eng.unet_forward(x.cuda(), t, cond.cuda())
        eng.set_attention_family("f32")
        assert not torch.equal(eng.unet_forward(x.cuda(), t, cond.cuda()), split)
    finally:
        eng.close()


@pytest.mark.parametrize("name,T,start_t,B,H,W,slice0", U.LOOPS, ids=[l[0] for l in U.LOOPS])
def test_reverse_loop_golden_with_h3_attention(h3_engines, synth, name, T, start_t, B, H, W, slice0):
    """tests/test_gpu_unet.py::test_reverse_loop_golden's explicit-noise run and bound (1e-4 of the reference's own output, and of the
    float64 chain where one is recorded), reverse / reverse_range / p_sample going through the h3 kernel at every step"""
    eng = h3_engines[T]
    steps = T if start_t == 0 else start_t
    x, cond = U.inputs(synth, B, H, W, slice0)
    noise = np.zeros((steps, B, 1, H, W), np.float32)
    for t in range(1, steps):
        noise[t] = synth.noise_z(3, t, slice0, B, H, W)
    out = eng.reverse(x.cuda(), cond.cuda(), steps, noise=torch.from_numpy(noise).cuda()).cpu().numpy()
    ref = golden(name)["out"]
    err = np.abs(out - ref).max()
    print(name, f"h3 attention: max|delta| vs reference golden: {err:.3e}  rms {np.sqrt(np.mean((out - ref) ** 2)):.3e}")
    assert out.min() >= 0.0 and out.max() <= 1.0
    assert err < U.TOL, err
    import os
    from conftest import GOLD
    if os.path.exists(os.path.join(GOLD, name + "_fp64.npz")):
        truth = golden(name + "_fp64")["out"]
        e_ref, e_hip = np.abs(ref - truth).max(), np.abs(out - truth).max()
        print(name, f"vs fp64: reference {e_ref:.3e}, HIP with h3 attention {e_hip:.3e}")
        assert e_hip < U.TOL


def test_training_with_h3_attention_vs_autograd(oracle, synth, monkeypatch):
    """tests/test_gpu_training_attention.py::_check at its smallest case, `attn_levels` (2 x 16 x 24, attention in every block), with the
    trainer built for attention_family="h3": forward, loss and every parameter gradient under that file's limits, unchanged"""
    plain = TA._trainer_kw
    monkeypatch.setattr(TA, "_trainer_kw", lambda case: dict(plain(case), attention_family="h3"))
    worst = TA._check(oracle, synth, "attn_levels", "pred_x0", "l1")
    seen = {k for _e, k in worst}
    assert all(b + s in seen for b in TA.LEVEL_ATTENTION for s in (".norm.weight", ".qkv.weight", ".qkv.bias", ".proj_out.weight"))


def _train_once(synth, case, **kw):
    """(forward output, every parameter gradient) of one forward / backward of a trainer built with `kw`, cloned"""
    tr = load_pkg("training")
    dev = torch.device("cuda", 0)
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    x01, cond, noise, t = TA._inputs(synth, case, 3)
    x0 = x01 * 2 - 1
    buf = load_pkg("schedule").schedule_buffers(TA.T)
    xt = (buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **TA._trainer_kw(case), **kw)
    try:
        out = trainer.forward(xt.to(dev), t.to(dev), cond.to(dev))
        _loss, dout = trainer.loss_and_grad(out, x0.to(dev), buf["p2_loss_weight"][t].to(dev).contiguous(), "l1")
        grads = trainer.backward(dout)
        torch.cuda.synchronize()
        return out.clone(), {k: g.clone() for k, g in grads.items()}
    finally:
        trainer.close()


def test_precision_16_wins_over_the_family(synth, sd_np):
    """a precision-16 engine and an attention_precision=16 trainer give the same bits with the family set to h3 as without"""
    B, H, W = 2, 32, 32
    x, cond = U.inputs(synth, B, H, W)
    outs = []
    for kw in (dict(precision=16), dict(precision=16, attention_family="h3")):
        eng = _engine(sd_np, 50, max_batch=B, max_h=H, max_w=W, **kw)
        try:
            assert eng.precision == 16 and eng.attention_family == kw.get("attention_family", "f32")
            outs.append(eng.unet_forward(x.cuda(), 25, cond.cuda()))
        finally:
            eng.close()
    assert torch.equal(outs[0], outs[1])
    case = A.CASES["attn_levels"]
    out16, g16 = _train_once(synth, case, attention_precision=16)
    out16h, g16h = _train_once(synth, case, attention_precision=16, attention_family="h3")
    assert torch.equal(out16, out16h) and all(torch.equal(g16[k], g16h[k]) for k in g16)


def test_the_trainers_family_changes_forward_and_backward_together(synth):
    case = A.CASES["attn_levels"]
    out32, g32 = _train_once(synth, case)
    out32h, g32h = _train_once(synth, case, attention_family="h3")
    assert not torch.equal(out32, out32h)
    assert not torch.equal(g32["input_blocks.1.1.qkv.weight"], g32h["input_blocks.1.1.qkv.weight"])
