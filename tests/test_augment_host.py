"""CPU: what the augmented-slice path rests on. The live numpy / scipy restatement (tests/augment_reference.py) against the literal
forms it restates -- the ghosting comb against the 3-D FFT rule, the bias coordinates against torchio's meshgrid form, the repeated
reflection against np.pad -- and the host side of augment.py: the counter-RNG draws, the cfg keys that are refused, the loader's
row arithmetic, the host arithmetic of cddpm_aug_workspace_bytes and the header against the library's exports."""
import os
import re

import numpy as np
import pytest

import augment_reference as AR
from conftest import ROOT, load_pkg

A = load_pkg("augment")


@pytest.mark.parametrize("shape", [(16, 12, 4), (15, 9, 5), (8, 70, 1), (6, 1, 10)])
def test_comb_equals_the_fft_rule(shape):
    """g > L, L // 2 a multiple of g (the restored plane is one of the scaled ones), L = 1, odd and even axes"""
    rng = np.random.Generator(np.random.PCG64(sum(shape)))
    vol = rng.random(shape) - 0.02
    worst = 0.0
    for axis in range(3):
        for g in (1, 2, 3, 4, 5, 7, 10, 80):
            for I in (0.5, 1.0):
                a, b = AR.ghost_fft(vol, g, axis, I), AR.ghost_comb(vol, g, axis, I)
                worst = max(worst, float(np.abs(a - b).max()))
    print(f"{shape}: max |comb - fft| = {worst:.2e}")
    assert worst < 1e-13                       # float64 rounding of an FFT pair over <= 768 voxels of size <= 1; measured <= 1.6e-15
    assert np.array_equal(AR.ghost_fft(vol, 0, 1, 1.0), vol) and np.array_equal(AR.ghost_fft(vol, 4, 1, 0.0), vol)
    for L in shape:                            # c has no DC term (its sum is the coefficient of the plane s = L // 2): that plane is restored
        for g in (1, 2, 4):                    # whether or not it is one of the scaled ones (L // 2 a multiple of g)
            assert abs(AR.comb_kernel(L, g).sum()) < 1e-12


@pytest.mark.parametrize("shape", [(16, 12, 4), (15, 9, 5), (8, 70, 1), (1, 1, 1), (2, 3, 1)])
def test_bias_coordinates_equal_the_meshgrid_form(shape):
    want = AR.bias_coords_meshgrid(shape)
    got = np.meshgrid(*[AR.bias_coords(L) for L in shape], indexing="ij")
    for w, g in zip(want, got):
        assert w.shape == tuple(shape) and np.array_equal(w, g)        # bit for bit in float64


@pytest.mark.parametrize("L,r", [(4, 4), (4, 9), (1, 3), (5, 32), (7, 2)])
def test_repeated_reflection_equals_symmetric_padding(L, r):
    want = np.pad(np.arange(L), r, mode="symmetric")
    assert np.array_equal(AR.reflect_index(np.arange(-r, L + r), L), want)
    # and scipy's own filter, at a radius beyond the axis: the line sum over reflected indices
    rng = np.random.Generator(np.random.PCG64(L * 100 + r))
    x = rng.random(L)
    sigma = (r - 0.4) / 4.0
    rr, w = AR.gaussian_weights(sigma)
    assert rr == r
    manual = np.array([sum(w[k + r] * x[AR.reflect_index(i + k, L)] for k in range(-r, r + 1)) for i in range(L)])
    assert np.abs(manual - AR.blur(x.reshape(L, 1, 1), (sigma, 0, 0)).reshape(L)).max() < 1e-14


def test_draw_ranges_and_flag_frequencies():
    aug = A.IntensityAugment()
    n, D = 20000, 50
    meta, par = aug.draw(7, 3, np.arange(n), D, spacing=(2.0, 2.0, 2.0))
    assert meta.dtype == np.int32 and meta.shape == (n, 4) and par.dtype == np.float32 and par.shape == (n, 28)
    assert meta[:, 1].min() == 0 and meta[:, 1].max() == D - 1
    g, axis = meta[:, 3] & 0xff, meta[:, 3] >> 8
    assert set(np.unique(g)) == set(range(4, 11)) and set(np.unique(axis)) == {0, 1, 2}
    assert np.exp(-0.3) <= par[:, 0].min() and par[:, 0].max() <= np.float32(np.exp(0.3))
    assert 0 <= par[:, 1:4].min() and par[:, 1:4].max() <= 1.0                     # std in [0, 2] mm at 2 mm spacing
    assert 0.5 <= par[:, 4].min() and par[:, 4].max() <= 1.0
    assert -0.5 <= par[:, 5:25].min() and par[:, 5:25].max() <= 0.5 and not par[:, 25:].any()
    assert (meta[:, 2] & ~15 == 0).all()
    for bit, p in aug.p.items():
        k = int(((meta[:, 2] & bit) != 0).sum())
        assert abs(k - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (bit, k)
    for lo, hi, col in ((np.exp(-0.3), np.exp(0.3), par[:, 0]), (0.5, 1.0, par[:, 4]), (0, 1, par[:, 2])):     # spread over the range
        assert col.min() < lo + 0.01 * (hi - lo) and col.max() > hi - 0.01 * (hi - lo)
    m4, p4 = aug.draw(7, 3, np.arange(100), D, spacing=(1.0, 2.0, 4.0))
    assert np.array_equal(m4, meta[:100]) and np.allclose(p4[:, 1:4] * np.float32([1, 2, 4]), par[:100, 1:4] * 2, rtol=1e-6)


def test_draw_is_a_function_of_seed_epoch_and_position_alone():
    aug = A.IntensityAugment()
    whole = aug.draw(11, 2, np.arange(37), 9)
    for split in ((0, 5, 37), (0, 1, 2, 30, 37), (0, 36, 37)):
        parts = [aug.draw(11, 2, np.arange(a, b), 9) for a, b in zip(split[:-1], split[1:])]
        assert np.array_equal(np.concatenate([m for m, _ in parts]), whole[0])
        assert np.array_equal(np.concatenate([p for _, p in parts]), whole[1])
    back = aug.draw(11, 2, np.arange(37)[::-1], 9)
    assert np.array_equal(back[0][::-1], whole[0]) and np.array_equal(back[1][::-1], whole[1])
    assert not np.array_equal(aug.draw(12, 2, np.arange(37), 9)[1], whole[1])
    assert not np.array_equal(aug.draw(11, 3, np.arange(37), 9)[1], whole[1])


class _Bank:
    """the host side of a VolumeBank: what the loader's row arithmetic reads"""
    def __init__(self, n, shape=(16, 12, 4)):
        self.n, self.shape, self.spacing, self.device = n, shape, (2.0, 2.0, 2.0), "cpu"

    def __len__(self):
        return self.n


def test_two_ranks_of_B_equal_one_rank_of_2B():
    aug = A.IntensityAugment()
    for n, B, drop in ((19, 4, True), (19, 4, False), (8, 4, True), (5, 4, False)):
        one = A.DeviceSliceLoader(_Bank(n), 2 * B, 5, aug, drop_last=drop, engine=object())
        ranks = [A.DeviceSliceLoader(_Bank(n), B, 5, aug, drop_last=drop, rank=r, world=2, engine=object()) for r in (0, 1)]
        for ld in (one, *ranks):
            ld.set_epoch(3)
        rows = [ld._rows() for ld in ranks]
        assert len(one) == len(one._rows()) == (n // (2 * B) if drop else -(-n // (2 * B)))
        for k, (first, count) in enumerate(one._rows()):
            want = one.tables(first, count)
            got = [ld.tables(*r[k]) for ld, r in zip(ranks, rows) if k < len(r)]
            assert np.array_equal(np.concatenate([m for m, _ in got]), want[0])
            assert np.array_equal(np.concatenate([p for _, p in got]), want[1])
        seen = np.concatenate([one.tables(f, c)[0][:, 0] for f, c in one._rows()])
        assert len(set(seen.tolist())) == len(seen) and (drop or sorted(seen.tolist()) == list(range(n)))      # a permutation's prefix
    a, b = A.epoch_order(5, 0, 50), A.epoch_order(5, 1, 50)
    assert sorted(a.tolist()) == list(range(50)) and not np.array_equal(a, b) and np.array_equal(a, A.epoch_order(5, 0, 50))
    assert np.array_equal(A.epoch_order(5, 0, 50, shuffle=False), np.arange(50))


@pytest.mark.parametrize("key", A.REFUSED_KEYS + ("unique_slice",))
def test_refused_cfg_keys_raise(key):
    assert len(A.REFUSED_KEYS) == 9
    with pytest.raises(NotImplementedError, match=key):
        A.IntensityAugment.from_cfg({"aug_intensity": True, key: True})
    assert A.IntensityAugment.from_cfg({"aug_intensity": True, key: False}).stages == (1, 2, 4, 8)


def test_refused_vol2slice_variants_and_the_unaugmented_recipe():
    for kw in (dict(onlyBrain=True), dict(slice=20), dict(seq_slices=3)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            A.IntensityAugment.from_cfg({"aug_intensity": True}, **kw)
    for cfg in ({}, {"aug_intensity": False}):
        none = A.IntensityAugment.from_cfg(cfg)
        assert none.stages == ()
        meta, par = none.draw(1, 0, np.arange(500), 7)
        assert not meta[:, 2].any() and meta[:, 1].max() == 6          # no stage is built; the slice is still drawn
    full = A.IntensityAugment.from_cfg({"aug_intensity": True})
    assert full.p == {1: 0.5, 2: 0.25, 4: 0.25, 8: 0.5}


def test_table_check_names_the_bad_row():
    E = load_pkg("engine").CddpmEngine
    meta, par = A.IntensityAugment().draw(1, 0, np.arange(6), 4, volumes=np.arange(6) % 3)
    E.check_augment_tables(meta, par, 3, 4)
    for what, col, val, table in (("volume", 0, 3, "meta"), ("z outside", 1, 4, "meta"), ("axis", 3, 4 | (3 << 8), "meta"), ("flag", 2, 16, "meta"),
                                  ("sigma", 2, 9.0, "par"), ("sigma", 1, -1.0, "par"), ("non-finite", 0, np.nan, "par"), ("non-finite", 7, np.inf, "par")):
        m, p = meta.copy(), par.copy()
        (m if table == "meta" else p)[4, col] = val
        with pytest.raises(RuntimeError, match=f"sample 4: .*{what}"):
            E.check_augment_tables(m, p, 3, 4)
    with pytest.raises(RuntimeError, match="int32"):
        E.check_augment_tables(meta.astype(np.int64), par, 3, 4)


def test_workspace_bytes_host_arithmetic():
    lib = load_pkg("_lib").load_library()
    one = lib.cddpm_aug_workspace_bytes(1, 16, 12, 4)
    assert one >= 2 * 16 * 12 * 4 * 4
    b32 = lib.cddpm_aug_workspace_bytes(32, 96, 96, 50)
    assert 32 * 2 * 96 * 96 * 50 * 4 <= b32 <= 32 * 2 * 96 * 96 * 50 * 4 + 32 * 16384      # two work volumes per sample and small tables
    for bad in ((0, 16, 12, 4), (1, 0, 12, 4), (1, 16, 1025, 4), (1, 16, 12, -1), (65536, 1, 1, 1)):
        assert lib.cddpm_aug_workspace_bytes(*bad) == 0
        assert "cddpm_aug_workspace_bytes" in lib.cddpm_last_error(None).decode()


def test_header_declares_what_the_library_exports():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    declared = set(re.findall(r"\b(cddpm_[a-z0-9_]+)\s*\(", header)) - {"cddpm_ctx"}
    assert {"cddpm_aug_slices", "cddpm_aug_workspace_bytes"} <= declared
    assert declared == set(lib_mod.SYMBOLS), declared ^ set(lib_mod.SYMBOLS)
    lib = lib_mod.load_library()
    for name in ("cddpm_aug_slices", "cddpm_aug_workspace_bytes"):
        assert getattr(lib, name) is not None
    E = load_pkg("engine").CddpmEngine                                   # the Python constants are the header's
    for name, val in (("CDDPM_AUG_META", E.AUG_META), ("CDDPM_AUG_PAR", E.AUG_PAR), ("CDDPM_AUG_ALL", E.AUG_ALL), ("CDDPM_AUG_MAX_SIGMA", 8),
                      ("CDDPM_AUG_GAMMA", A.GAMMA), ("CDDPM_AUG_BIAS", A.BIAS), ("CDDPM_AUG_BLUR", A.BLUR), ("CDDPM_AUG_GHOST", A.GHOST)):
        assert re.search(rf"#define {name} {int(val)}\b", header), name
