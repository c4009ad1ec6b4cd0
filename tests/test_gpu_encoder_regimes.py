"""GPU: the inference encoder (csrc/encoder.hip behind DDPM_encoder.ResNet50Encoder) on weights that look like a trained network
(tests/encoder_regime_cases.py: running_var over eleven decades, bn3.weight = 0, |running_mean| / sqrt(running_var) ~ 1e2, dead
channels with running_var = 0, heads of 1, 7, 130 outputs) against the float64 oracle, and the handle's reuse across sizes, batch
limits and streams, bit for bit.

The bound is tests/test_gpu_encoder.py's, relative to the output: e_hip <= 10 e_ref + 1e-6 max(1, max|ref64|), e_ref = the fp32
oracle's own distance from float64 on the same weights and input.

Measured on an MI355X, worst e_hip / e_ref per regime over (2, 64, 64), (1, 33, 47), (3, 32, 32):
    eps 0.977 (33x47: 0.884, 32x32: 0.974)    bn3_zero 1.657 (e_hip 8.5e-07)    offset 1.237    dead 1.939 (at 33x47)
    nc1 1.786    nc7 1.557    nc130 0.977
With `1e-5` replaced by `0` in load_convbn every one of the 21 cases fails.
"""
import pytest
import torch

import encoder_regime_cases as RC
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SHAPES = [(2, 64, 64), (1, 33, 47), (3, 32, 32)]       # | odd feature maps at every level | the smallest size the handle takes


def _encoder(regime):
    E = load_pkg("DDPM_encoder")
    enc = E.ResNet50Encoder(num_classes=RC.num_classes(regime))
    missing, unexpected = enc.load_state_dict(RC.build(regime), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    return enc


@pytest.fixture(scope="module")
def encoders():
    made = {}

    def get(regime):
        if regime not in made:
            made[regime] = _encoder(regime)
        return made[regime]

    yield get
    for enc in made.values():
        enc.close()


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("regime", RC.REGIMES)
def test_encoder_regime_vs_float64(encoders, synth, regime, B, H, W):
    x = torch.from_numpy(synth.synth_slices(4, 0, B, H, W))
    ref32, ref64 = RC.oracles(regime, x)
    out = encoders(regime)(x.cuda()).cpu()
    assert out.shape == ref64.shape and bool(torch.isfinite(out).all())
    top = float(ref64.abs().max())
    e_ref, e_hip = float((ref32.double() - ref64).abs().max()), float((out.double() - ref64).abs().max())
    print(f"{regime} {B}x{H}x{W}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  e_hip/e_ref {e_hip / e_ref:.3f}  max|ref64| {top:.3e}")
    assert e_hip <= 10 * e_ref + 1e-6 * max(1.0, top)


# ---- one handle, many calls ------------------------------------------------------------------------------------------------------------
def _x(synth, B, H, W, seed=4):
    return torch.from_numpy(synth.synth_slices(seed, 0, B, H, W)).cuda()


def test_one_handle_across_sizes_equals_fresh_handles(synth):
    """128x128, 33x47, 96x96, 32x32, 128x128 on ONE module: every result is a fresh module's at that size, the last is the first
    (stale activation buffers, size bookkeeping)"""
    enc = _encoder("eps")
    try:
        outs = []
        for H, W in [(128, 128), (33, 47), (96, 96), (32, 32), (128, 128)]:
            x = _x(synth, 2, H, W)
            got = enc(x).clone()
            fresh = _encoder("eps")
            try:
                want = fresh(x).clone()
            finally:
                fresh.close()
            assert torch.equal(got, want), (H, W, float((got - want).abs().max()))
            outs.append(got)
        assert torch.equal(outs[0], outs[-1])
    finally:
        enc.close()


def test_batch_limit_and_rebuild_slices_equal_single_calls(synth):
    """B = 64 is the handle's default limit, B = 65 forces a rebuild: every slice equals the B = 1 call of that slice (the kernels have
    no cross-slice arithmetic)"""
    enc = _encoder("eps")
    try:
        x = _x(synth, 65, 32, 32)
        singles = torch.cat([enc(x[i:i + 1]) for i in range(65)])
        first = enc._h
        got64 = enc(x[:64]).clone()
        assert enc._h is first                                   # within the limit: the same handle
        got65 = enc(x).clone()
        assert enc._h is not first and enc._key[1] == 65         # rebuilt for the larger batch
        assert torch.equal(got64, singles[:64]) and torch.equal(got65, singles)
        assert torch.equal(enc(x[64:65]), singles[64:65])        # and the rebuilt handle on one slice
    finally:
        enc.close()


def test_non_default_stream_equals_default_stream(synth):
    enc = _encoder("eps")
    try:
        base = _x(synth, 3, 48, 40)
        want = enc(base * 0.5 + 0.25).clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            x = base * 0.5 + 0.25                                # produced on the side stream: the call must be ordered behind it
            got = enc(x)
        side.synchronize()
        assert torch.equal(got, want)
    finally:
        enc.close()
