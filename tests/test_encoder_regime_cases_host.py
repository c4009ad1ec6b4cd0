"""CPU: the conditions on the trained-like encoder weights of tests/encoder_regime_cases.py that the REFERENCE alone must meet, before
any kernel is compared on them: both oracles finite, the float64 output inside a stated band, the regime's own property (shares of
channels) present, and the fp32 oracle's own distance from float64 -- the yardstick of tests/test_gpu_encoder_regimes.py -- recorded."""
import numpy as np
import pytest
import torch

import encoder_regime_cases as RC
from conftest import load_pkg

B, H, W = 2, 64, 64


@pytest.mark.parametrize("regime", RC.REGIMES)
def test_reference_conditions(regime):
    synth = load_pkg("synth")
    sd = RC.build(regime)
    shapes = synth.encoder_param_shapes(RC.num_classes(regime))
    assert set(sd) == set(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) and sd[k].dtype == torch.float32 for k in shapes)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    x = torch.from_numpy(synth.synth_slices(4, 0, B, H, W))
    ref32, ref64 = RC.oracles(regime, x)
    assert ref64.shape == (B, RC.num_classes(regime))
    assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(ref64).all())
    top = float(ref64.abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    shares = RC.property_shares(regime, sd)
    var, _ratio = RC.channel_stats(sd)
    print(f"{regime}: max|ref64| {top:.3e}  e_ref {e_ref:.3e}  running_var {var.min():.1e} .. {var.max():.1e}  "
          + "  ".join(f"share({k}) {got:.3f}" for k, (got, _least) in shares.items()))
    assert RC.OUT_BAND[0] <= top <= RC.OUT_BAND[1]
    for label, (got, least) in shares.items():
        assert got >= least, (regime, label, got, least)
    assert e_ref > 0.0                      # a yardstick of zero would turn the GPU bound into its absolute floor
    assert np.isfinite(var).all() and (var >= 0).all()


def test_cases_are_seeded_and_calibrated_on_their_own_input():
    """built twice, the same bits; and the statistics ARE those of the calibration batch: in a float64 run of the oracle on that batch
    the stem's BatchNorm output has per-channel mean = beta and variance = gamma^2 var / (var + eps)"""
    import encoder_oracle as EO
    synth = load_pkg("synth")
    sd = RC.build("eps")
    again = RC._trained_like("eps")
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(synth.synth_slices(7, 0, 4, 64, 64)).double()
    z = torch.nn.functional.conv2d(x, sd64["conv1.weight"], None, stride=2, padding=3)
    y = EO._bn(z, sd64, "bn1")
    var = sd64["bn1.running_var"]
    want_var = sd64["bn1.weight"] ** 2 * var / (var + 1e-5)
    assert float((y.mean(dim=(0, 2, 3)) - sd64["bn1.bias"]).abs().max()) < 1e-5          # float32 storage of the statistics
    assert float((y.var(dim=(0, 2, 3), unbiased=False) / want_var - 1).abs().max()) < 1e-5
