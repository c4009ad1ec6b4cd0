"""CPU: the host side of training with dropout (`dropout_unet`; nn.Dropout between the SiLU and the second convolution of every ResBlock,
reference OpenAI_Unet.py:255) -- synth.dropout_mask, the host restatement of the device mask of csrc/train_kernels.hip, and the
{seed, step} state that travels in UNetTrainer.optimizer_state()["dropout"]."""
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg

SEED = 20240611


def test_dropout_mask_is_deterministic_and_keyed_by_layer_step_and_slice(synth):
    a = synth.dropout_mask(SEED, 3, 5, 7, 2, 8, 12, 32, 0.3)
    assert a.dtype == np.uint8 and a.shape == (2, 8, 12, 32) and set(np.unique(a)) == {0, 1}
    assert np.array_equal(a, synth.dropout_mask(SEED, 3, 5, 7, 2, 8, 12, 32, 0.3))
    for other in (synth.dropout_mask(SEED, 3, 6, 7, 2, 8, 12, 32, 0.3),        # another ResBlock
                  synth.dropout_mask(SEED, 4, 5, 7, 2, 8, 12, 32, 0.3),        # another step
                  synth.dropout_mask(SEED, 3, 5, 8, 2, 8, 12, 32, 0.3),        # other slices
                  synth.dropout_mask(SEED + 1, 3, 5, 7, 2, 8, 12, 32, 0.3)):   # another seed
        assert 0.3 < float((a != other).mean()) < 0.55                         # two independent p = 0.3 masks differ at 2 p (1 - p) = 0.42
    assert not np.array_equal(a[0], a[1])
    # the streams of the masks stay clear of every stream the noise and the synthetic weights use
    taken = {synth.STREAM_XT, synth.STREAM_Z, synth.STREAM_COND, synth.STREAM_INPUT}
    n_w, n_e = len(synth.unet_param_shapes()), len(synth.synth_encoder_state_dict(0))
    assert synth.STREAM_DROPOUT > max(max(taken), synth.STREAM_WEIGHT + 4 * n_w, synth.STREAM_ENC_WEIGHT + 4 * n_e)


def test_dropout_mask_is_the_philox_word_against_the_threshold(synth):
    p, step, layer, sl = 0.25, 9, 2, 11
    m = synth.dropout_mask(SEED, step, layer, sl, 1, 2, 2, 8, p).reshape(-1)
    q = np.arange(8, dtype=np.uint32)
    words = np.stack(synth.philox4x32(q, np.uint32(step), np.uint32(sl), np.uint32(synth.STREAM_DROPOUT + layer), SEED & 0xFFFFFFFF, SEED >> 32),
                     axis=-1).reshape(-1)
    assert synth.dropout_threshold(p) == 1 << 30
    assert np.array_equal(m, (words >= np.uint32(1 << 30)).astype(np.uint8))
    assert synth.dropout_scale(0.5) == np.float32(2.0) and synth.dropout_scale(0.1) == np.float32(1.0 / 0.9)


def test_dropout_zero_keeps_everything_and_bad_probabilities_are_refused(synth):
    assert synth.dropout_mask(SEED, 0, 0, 0, 2, 8, 8, 32, 0.0).all()
    assert synth.dropout_threshold(0.0) == 0 and synth.dropout_scale(0.0) == np.float32(1.0)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            synth.dropout_mask(SEED, 0, 0, 0, 1, 8, 8, 32, bad)


def test_a_batch_of_four_is_two_batches_of_two(synth):
    full = synth.dropout_mask(SEED, 2, 4, 0, 4, 8, 12, 32, 0.1)
    halves = [synth.dropout_mask(SEED, 2, 4, s0, 2, 8, 12, 32, 0.1) for s0 in (0, 2)]
    assert np.array_equal(full, np.concatenate(halves, axis=0))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction_is_binomial(synth, p):
    """n = 2 * 32 * 32 * 128 draws: the kept fraction lies within five standard deviations of 1 - p (a binomial bound on a fixed seed)"""
    B, H, W, C = 2, 32, 32, 128
    n = B * H * W * C
    kept = float(synth.dropout_mask(SEED, 0, 0, 0, B, H, W, C, p).mean())
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
    print(f"p {p}: kept {kept:.6f}, expected {1 - p}, deviation {kept - (1 - p):+.2e}, bound {bound:.2e}")
    assert abs(kept - (1.0 - p)) <= bound


def test_dropout_state_round_trips_through_the_state_helpers():
    tr = load_pkg("training")
    st = tr.dropout_state(2 ** 63 + 5, 17)
    assert st == {"seed": 2 ** 63 + 5, "step": 17} and tr.dropout_from_state(st) == (2 ** 63 + 5, 17)
    # what a checkpoint hands back after torch.save / torch.load of nested tensors
    assert tr.dropout_from_state({"seed": torch.tensor(12345), "step": torch.tensor(3)}) == (12345, 3)
    for bad in ({"seed": 1}, {"seed": -1, "step": 0}, {"seed": 1, "step": -2}, {"seed": 1.5, "step": 0}, None):
        with pytest.raises(ValueError):
            tr.dropout_from_state(bad)
    # the constructor's arguments: the default seed is torch.initial_seed(), as the diffusion mirror seeds its noise
    torch.manual_seed(4242)
    assert tr.dropout_settings(0.1, None) == (0.1, 4242) and tr.dropout_settings(0, 7) == (0.0, 7) and tr.dropout_settings(None, 7)[0] == 0.0
    for bad in (1.0, -0.5, float("nan"), "much"):
        with pytest.raises(ValueError):
            tr.dropout_settings(bad, 1)
    with pytest.raises(ValueError):
        tr.dropout_settings(0.1, 1.5)
