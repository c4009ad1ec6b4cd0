"""GPU: the convolution family as a property of the handle (cddpm_set_conv_family), the per-slice status kernel
(cddpm_slice_status) and the per-slice fallback of `reverse` / `unet_forward` out of the fp16 range of the default family.

All on the synthetic weights (seed 0), at 32x32 or 64x96 (the status kernel also at its B = 64 x 128 x 128 geometry), T <= 50.

The overflowing batch. Four slices; slice 2's x / x_T is multiplied by SCALE = 3e4. The input convolution is linear in x, so the
residual stream of that slice reaches 8.26e4 in the fp32 oracle (input_blocks.0 .. 2: max |activation| 82608 against 2.8 .. 4.6 of
the other slices), above the 65504 the h3 family's fp16 split can carry: the 1x1 skip convolution of input_blocks.4 reads it
unnormalised. GroupNorm makes everything behind it scale-free, so the exact arithmetic has no trouble. Measured on the CPU with
oracle/cddpm_oracle.py, explicit noise, T = 50, 32x32, fp32 oracle against the float64 oracle on the same input:
    slice 0  max 5.31e-6  rms 7.17e-7        slice 2 (x 3e4)  max 2.84e-6  rms 4.04e-7
    slice 1  max 7.87e-6  rms 9.63e-7        slice 3          max 3.92e-6  rms 6.94e-7
i.e. the fp32 oracle's result for the scaled slice is finite and agrees with float64 as the unscaled slices do.
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, load_pkg

pytestmark = pytest.mark.gpu

SCALE = 3.0e4          # see the module docstring
T, H, W = 50, 32, 32


@pytest.fixture(scope="module")
def make_engine(sd_np):
    eng_mod, sched = load_pkg("engine"), load_pkg("schedule")
    made = []

    def make(family, timesteps=T, max_batch=4, max_h=H, max_w=W, load=True):
        e = eng_mod.CddpmEngine(timesteps=timesteps, max_batch=max_batch, max_h=max_h, max_w=max_w, conv_family=family)
        made.append(e)
        if load:
            e.load_weights(sd_np)
            e.set_schedule(sched.schedule_buffers(timesteps), "pred_x0")
        return e

    yield make
    for e in made:
        e.close()


@pytest.fixture(scope="module")
def h3(make_engine):
    return make_engine("h3")


@pytest.fixture(scope="module")
def x6(make_engine):
    return make_engine("x6")


def explicit_noise(synth, steps, slice0, B, h=H, w=W):
    noise = np.zeros((steps, B, 1, h, w), np.float32)
    for t in range(1, steps):
        noise[t] = synth.noise_z(3, t, slice0, B, h, w)
    return torch.from_numpy(noise)


def overflowing_batch(synth, slice0=0, B=4):
    x = torch.from_numpy(synth.noise_xT(2, slice0, B, H, W))
    x[2] *= SCALE
    return x.cuda(), torch.from_numpy(synth.synth_cond(1, slice0, B)).cuda()


# ---------------------------------------------------------------------------------------------- a. two families, one process
CHILD = r"""
import importlib, sys, numpy as np, torch
sys.path.insert(0, %r)
PKG = "conditioned-diffusion-models-uad_amd"
synth = importlib.import_module(PKG + ".synth"); eng_mod = importlib.import_module(PKG + ".engine"); sched = importlib.import_module(PKG + ".schedule")
B, H, W, T = 2, 32, 32, 50
e = eng_mod.CddpmEngine(timesteps=T, max_batch=2, max_h=H, max_w=W)          # no conv_family: the process default (CDDPM_CONV)
e.load_weights(synth.synth_state_dict(0)); e.set_schedule(sched.schedule_buffers(T), "pred_x0")
x = torch.from_numpy(synth.noise_xT(2, 0, B, H, W)).cuda(); cond = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
noise = np.zeros((T, B, 1, H, W), np.float32)
for t in range(1, T): noise[t] = synth.noise_z(3, t, 0, B, H, W)
fwd = e.unet_forward(x, 25, cond).cpu().numpy()
rev = e.reverse(x, cond, T, noise=torch.from_numpy(noise).cuda()).cpu().numpy()
np.savez(sys.argv[1], fwd=fwd, rev=rev, family=e.conv_family)
"""


def test_two_families_interleaved_equal_their_single_family_processes(make_engine, synth, tmp_path):
    """an h3 and an x6 handle used in alternation on one stream: each call equals, bit for bit, the same call in a process whose
    only family is that one (chosen by CDDPM_CONV, as before), and each chain meets the reference golden at 1e-4"""
    B = 2
    a, b = make_engine("h3", max_batch=B), make_engine("x6", max_batch=B)
    assert (a.conv_family, b.conv_family) == ("h3", "x6")
    x = torch.from_numpy(synth.noise_xT(2, 0, B, H, W)).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
    noise = explicit_noise(synth, T, 0, B).cuda()
    got = {"h3": {}, "x6": {}}
    got["h3"]["fwd"] = a.unet_forward(x, 25, cond)
    got["x6"]["fwd"] = b.unet_forward(x, 25, cond)
    got["h3"]["rev"] = a.reverse(x, cond, T, noise=noise)
    got["x6"]["rev"] = b.reverse(x, cond, T, noise=noise)
    assert torch.equal(a.unet_forward(x, 25, cond), got["h3"]["fwd"])        # and back again after the other family ran
    assert torch.equal(b.unet_forward(x, 25, cond), got["x6"]["fwd"])
    assert not torch.equal(got["h3"]["fwd"], got["x6"]["fwd"])               # two arithmetics, not one handle twice
    ref = golden("loop_B2_32x32_T50_start0")["out"]
    for fam in ("h3", "x6"):
        env = dict(os.environ, CDDPM_CONV=fam)
        out = str(tmp_path / f"{fam}.npz")
        r = subprocess.run([sys.executable, "-c", CHILD % ROOT, out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, fam + ": " + r.stdout[-2000:] + r.stderr[-2000:]
        child = np.load(out)
        assert str(child["family"]) == fam
        for key in ("fwd", "rev"):
            assert np.array_equal(got[fam][key].cpu().numpy(), child[key]), (fam, key)
        err = float(np.abs(got[fam]["rev"].cpu().numpy() - ref).max())
        print(f"{fam}: 50-step chain vs reference golden max|delta| {err:.3e}")
        assert err < 1e-4, (fam, err)


# ---------------------------------------------------------------------------------------------- b. family change after load
def test_set_conv_family_after_load_drops_the_weights(make_engine, x6, synth, sd_np):
    sched = load_pkg("schedule")
    e = make_engine("h3")
    x = torch.from_numpy(synth.noise_xT(2, 0, 2, H, W)).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, 2)).cuda()
    before = e.unet_forward(x, 25, cond)
    e.set_conv_family("h3")                                # the current family: nothing happens
    assert torch.equal(e.unet_forward(x, 25, cond), before)
    with pytest.raises(ValueError):
        e.set_conv_family("h4")
    e.set_conv_family("x6")
    assert e.conv_family == "x6"
    for call in (lambda: e.unet_forward(x, 25, cond), lambda: e.reverse(x, cond, 2), lambda: e.p_sample(x, 3, cond)):
        with pytest.raises(RuntimeError, match="convolution family was changed after cddpm_load_weights"):
            call()
    e.load_weights(sd_np)
    e.set_schedule(sched.schedule_buffers(T), "pred_x0")
    assert torch.equal(e.unet_forward(x, 25, cond), x6.unet_forward(x, 25, cond))
    assert torch.equal(e.reverse(x, cond, 5, seed=3), x6.reverse(x, cond, 5, seed=3))
    with pytest.raises(RuntimeError, match="unknown family"):
        e._ck(e.lib.cddpm_set_conv_family(e._h, 3), "cddpm_set_conv_family")


# ---------------------------------------------------------------------------------------------- c. slice status
@pytest.mark.parametrize("B,h,w", [(5, 32, 32), (4, 64, 96), (64, 128, 128)])
def test_slice_status_flags_exactly_the_non_finite_slices(h3, B, h, w):
    g = torch.Generator().manual_seed(B * h + w)
    x = (torch.randn((B, 1, h, w), generator=g) * 1e4).cuda()
    assert h3.slice_status(x).cpu().tolist() == [0] * B
    inf, nan = float("inf"), float("nan")
    plants = [(0, 0, 0, inf), (B - 1, h - 1, w - 1, nan), (B // 2, h // 2, w // 3, -inf), (0, 0, w - 1, nan), (0, h - 1, 0, inf)]
    for b, yy, xx, v in plants:
        x[b, 0, yy, xx] = v
    x[min(3, B - 1), 0, 1, 1] = 3.4e38                     # the largest finite magnitudes are finite
    x[min(3, B - 1), 0, 1, 2] = -3.4e38
    want = (~torch.isfinite(x).flatten(1).all(1)).to(torch.int32)
    got = h3.slice_status(x)
    assert got.dtype == torch.int32 and got.shape == (B,)
    assert torch.equal(got, want), (got.cpu().tolist(), want.cpu().tolist())
    assert 0 < int(want.sum()) < B
    for b, yy, xx, v in plants:                            # each plant on its own, the rest of the tensor clean
        y = torch.zeros((B, 1, h, w), device="cuda")
        y[b, 0, yy, xx] = v
        assert h3.slice_status(y).cpu().tolist() == [int(i == b) for i in range(B)], (b, yy, xx, v)


# ---------------------------------------------------------------------------------------------- d. the fallback run
def one_warning(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn()
    assert len(rec) == 1 and issubclass(rec[0].category, RuntimeWarning), [str(w.message) for w in rec]
    assert "1 of 4 slices" in str(rec[0].message) and "x6" in str(rec[0].message), str(rec[0].message)
    return out


@pytest.mark.parametrize("noise_mode", ["philox", "explicit"])
def test_reverse_fallback_reruns_only_the_overflowing_slice(h3, x6, synth, noise_mode):
    s0 = 5 if noise_mode == "philox" else 0                # device Philox: a non-zero slice0 checks the slice0 + i of the re-run
    x, cond = overflowing_batch(synth, s0)
    noise = explicit_noise(synth, T, s0, 4).cuda() if noise_mode == "explicit" else None
    sub = lambda i, j: None if noise is None else noise[:, i:j].contiguous()
    kw = dict(seed=3, slice0=s0)
    with pytest.raises(FloatingPointError, match="CDDPM_CONV"):                  # today's behaviour, unchanged
        h3.reverse(x, cond, T, noise=noise, **kw)
    assert h3.slice_status(h3.reverse_unchecked(x, cond, T, noise=noise, **kw)).cpu().tolist() == [0, 0, 1, 0]
    out = one_warning(lambda: h3.reverse(x, cond, T, noise=noise, fallback=x6, **kw))
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0 and float(out.max()) <= 1
    # slices 0, 1, 3: the plain h3 run of those slices
    assert torch.equal(out[0:2], h3.reverse(x[0:2], cond[0:2].contiguous(), T, noise=sub(0, 2), seed=3, slice0=s0))
    assert torch.equal(out[3:4], h3.reverse(x[3:4], cond[3:4].contiguous(), T, noise=sub(3, 4), seed=3, slice0=s0 + 3))
    # slice 2: its result in a whole-batch run of the exact family
    whole = x6.reverse(x, cond, T, noise=noise, **kw)
    assert torch.equal(out[2], whole[2])
    assert not torch.equal(out[0], whole[0])               # (the kept slices are h3's, not x6's)
    # a callable is resolved on the first flagged slice only
    calls = []
    clean = x.clone()
    clean[2] /= SCALE
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ok = h3.reverse(clean, cond, T, noise=noise, fallback=lambda: calls.append(1) or x6, **kw)
    assert not calls and torch.equal(ok, h3.reverse(clean, cond, T, noise=noise, **kw))


def test_unet_forward_fallback_reruns_only_the_overflowing_slice(h3, x6, synth):
    x, cond = overflowing_batch(synth)
    for t in (25, torch.tensor([3, 25, 40, 49])):
        plain = h3.unet_forward(x, t, cond)
        assert h3.slice_status(plain).cpu().tolist() == [0, 0, 1, 0]
        out = one_warning(lambda: h3.unet_forward(x, t, cond, fallback=x6))
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out[[0, 1, 3]], plain[[0, 1, 3]])
        assert torch.equal(out[2], x6.unet_forward(x, t, cond)[2])


def test_fallback_engine_must_match(h3, x6, make_engine, synth):
    x, cond = overflowing_batch(synth)
    with pytest.raises(RuntimeError, match="same geometry"):
        h3.reverse(x, cond, 2, fallback=make_engine("x6", max_batch=8, load=False))
    with pytest.raises(RuntimeError, match="exact convolution family"):
        h3.reverse(x, cond, 2, fallback=make_engine("h3", load=False))


# ---------------------------------------------------------------------------------------------- e. accuracy of the rescued slice
def test_rescued_slice_is_as_close_to_float64_as_the_fp32_oracle(h3, x6, synth, oracle, sd_torch):
    """The slice re-run in the x6 family against the float64 oracle on the same (scaled) input. Yardstick: the fp32 oracle's own
    error against float64 on that input, computed here; acceptance max and rms <= 2 x yardstick (the rule of _accept_final_image,
    tests/test_gpu_headline.py: two fp32 executions with different summation orders, each as far from the exact chain as the
    other, can be twice that apart)."""
    x, cond = overflowing_batch(synth)
    noise = explicit_noise(synth, T, 0, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = h3.reverse(x, cond, T, noise=noise.cuda(), fallback=x6)[2:3].cpu().double()
    xs, cs = x[2:3].cpu(), cond[2:3].cpu()
    buf = oracle.schedule_buffers(T)
    with torch.no_grad():
        r32 = oracle.p_sample_loop(xs, cs, sd_torch, buf, lambda t: noise[t, 2:3], start_t=0).double()
        r64 = oracle.p_sample_loop(xs.double(), cs.double(), oracle.to_float64(sd_torch), oracle.to_float64(buf),
                                   lambda t: noise[t, 2:3].double(), start_t=0)
    assert bool(torch.isfinite(r32).all())
    rms = lambda d: float((d ** 2).mean().sqrt())
    y_max, y_rms = float((r32 - r64).abs().max()), rms(r32 - r64)
    e_max, e_rms = float((out - r64).abs().max()), rms(out - r64)
    print(f"rescued slice (x {SCALE:g}) vs float64: HIP x6 max {e_max:.3e} rms {e_rms:.3e}; fp32 oracle (yardstick) max {y_max:.3e} rms {y_rms:.3e}")
    assert e_max <= 2 * y_max and e_rms <= 2 * y_rms, (e_max, e_rms, y_max, y_rms)


# ---------------------------------------------------------------------------------------------- f. still-bad input
def test_nan_input_raises_after_one_rerun(h3, x6, synth, monkeypatch):
    x, cond = overflowing_batch(synth)
    x[1, 0, 5, 7] = float("nan")
    reruns = []
    real = x6.reverse_unchecked
    monkeypatch.setattr(x6, "reverse_unchecked", lambda *a, **k: reruns.append(a[0].shape[0]) or real(*a, **k))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(FloatingPointError, match=r"slices \[1\] are still non-finite"):
            h3.reverse(x, cond, 3, seed=3, fallback=x6)
    assert reruns == [2]                                   # slices 1 and 2 as ONE run, once


# ---------------------------------------------------------------------------------------------- g. the mirror
def test_ddpm2d_conv_fallback_key(sd_np, synth):
    """cfg.conv_fallback through DDPM_2D.reconstruct. reverse_sampling off: a batch like (d)'s as the input, slice 2 scaled. The
    single step feeds the UNet q_sample(input, t = 25), i.e. 0.7 x the input: at 3e4 the stream of the fp32 oracle stays at 6.06e4,
    just inside the fp16 range, so this input is scaled by 3e5 (stream 6.06e5, oracle finite). reverse_sampling on: the loop starts from the engine's own N(0,1) draw and the
    input reaches the UNet through the context only, so there slice 2's context is scaled -- by 1e6, which takes the residual
    stream of that slice to 2.5e5 in the fp32 oracle (finite)."""
    M = load_pkg("DDPM_2D")
    base = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=26, timesteps=T)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous()

    def module(**over):
        mod = M.DDPM_2D(dict(base, **over), encoder=Enc())
        mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        return mod.cuda()

    plain, fb = module(), module(conv_fallback="x6")
    assert set(fb.state_dict()) == set(plain.state_dict())
    with pytest.raises(ValueError):
        module(conv_fallback="x5")
    inp = torch.from_numpy(synth.synth_slices(2, 0, 4, H, W)).cuda()
    inp[2] *= 3.0e5
    feats = torch.from_numpy(synth.synth_cond(1, 0, 4)).cuda()
    noise = torch.from_numpy(synth.noise_z(3, 1, 0, 4, H, W)).cuda()
    # single step (the reference's default evaluation call): no finiteness check there today, the overflow comes back as NaN
    _loss, reco = plain.reconstruct(inp, features=feats, noise=noise)
    assert (~torch.isfinite(reco).flatten(1).all(1)).cpu().tolist() == [False, False, True, False]
    _loss, reco_fb = one_warning(lambda: fb.reconstruct(inp, features=feats, noise=noise))
    assert bool(torch.isfinite(reco_fb).all()) and torch.equal(reco_fb[[0, 1, 3]], reco[[0, 1, 3]])
    assert fb.diffusion.model._hip._fallback_engine is not None
    # the reverse loop
    feats_big = feats.clone()
    feats_big[2] *= 1.0e6
    for mod in (plain, fb):
        mod.cfg["reverse_sampling"], mod.cfg["reverse_start_t"] = True, 3
    torch.manual_seed(11)
    with pytest.raises(FloatingPointError, match="CDDPM_CONV"):
        plain.reconstruct(inp, features=feats_big)
    torch.manual_seed(11)
    _loss, reco2 = one_warning(lambda: fb.reconstruct(inp, features=feats_big))
    assert bool(torch.isfinite(reco2).all()) and float(reco2.min()) >= 0 and float(reco2.max()) <= 1
    # without an overflow the key changes nothing
    torch.manual_seed(11)
    a = plain.reconstruct(inp / inp.amax(), features=feats)[1]
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = fb.reconstruct(inp / inp.amax(), features=feats)[1]
    assert torch.equal(a, b)
    hip = fb.diffusion.model._hip
    fb_eng = hip._fallback_engine
    hip.close()
    assert hip._fallback_engine is None and fb_eng._h is None      # closed together with the main engine
    plain.diffusion.model._hip.close()
