"""CPU: what the augmentation pipeline rests on. The host side of augment.SliceAugment -- get_augment's keys, order and probabilities, the
refusals that remain, the draws that must equal IntensityAugment's, the affine's matrix -- CddpmEngine.check_pipeline_tables, the host
arithmetic of cddpm_aug_pipeline_workspace_bytes, and the new rules of tests/augment_pipeline_reference.py against what numpy, scipy
and synth already state: the trilinear resample against scipy.ndimage.map_coordinates, the flip against np.flip, the restated Philox
and normals against synth's."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import augment_pipeline_reference as PR
from conftest import ROOT, load_pkg

A = load_pkg("augment")
KEYS = {"random_bias": (1, 0.25), "random_noise": (2, 0.5), "random_ghosting": (4, 0.5), "random_blur": (8, 0.5), "random_gamma": (16, 0.5),
        "random_affine": (32, 0.5), "random_flip": (64, 0.5)}
POLICY = {128: 0.5, 256: 0.25, 512: 0.25, 1024: 0.5}


@pytest.mark.parametrize("key", sorted(KEYS))
def test_from_cfg_maps_each_key_alone_and_with_the_policy(key):
    bit, p = KEYS[key]
    alone = A.SliceAugment.from_cfg({key: True})
    assert alone.p == {bit: p} and alone.stages == (bit,)
    both = A.SliceAugment.from_cfg({key: True, "aug_intensity": True})
    assert both.p == {bit: p, **POLICY} and both.stages == (bit, 128, 256, 512, 1024)
    assert A.SliceAugment.from_cfg({key: False, "aug_intensity": True}).stages == (128, 256, 512, 1024)


def test_from_cfg_order_and_the_header_constants():
    """all keys together: get_augment's order, bias . noise . ghosting . blur . gamma . affine . flip . the policy group"""
    full = A.SliceAugment.from_cfg({**{k: True for k in KEYS}, "aug_intensity": True})
    assert full.stages == tuple(1 << k for k in range(11)) == A.SLOTS == PR.SLOTS
    assert full.p == {**{b: p for b, p in KEYS.values()}, **POLICY} == A.SliceAugment().p
    assert A.SliceAugment.from_cfg({}).stages == () and A.SliceAugment.from_cfg({"aug_intensity": False}).stages == ()
    assert {A.POLICY_GAMMA >> 7: 0.5, A.POLICY_BIAS >> 7: 0.25, A.POLICY_BLUR >> 7: 0.25, A.POLICY_GHOST >> 7: 0.5} == A.IntensityAugment.DEFAULT_P
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    E = load_pkg("engine").CddpmEngine
    names = ("BIAS", "NOISE", "GHOST", "BLUR", "GAMMA", "AFFINE", "FLIP", "POLICY_GAMMA", "POLICY_BIAS", "POLICY_BLUR", "POLICY_GHOST")
    for name, val in (*zip(names, A.SLOTS), ("ALL", E.PIPE_ALL), ("META", E.PIPE_META), ("PAR", E.PIPE_PAR), ("META", A.PIPE_META), ("PAR", A.PIPE_PAR),
                      ("META_GHOST", E.PIPE_META_GHOST), ("META_POLICY_GHOST", E.PIPE_META_POLICY_GHOST), ("PAR_SLOT", E.PIPE_PAR_SLOT),
                      ("PAR_POLICY", E.PIPE_PAR_POLICY), ("PAR_NOISE_STD", E.PIPE_PAR_NOISE_STD), ("PAR_MATRIX", E.PIPE_PAR_MATRIX),
                      ("PAR_POLICY", PR.SET), ("PAR_NOISE_STD", PR.COL_STD), ("PAR_MATRIX", PR.COL_M)):
        assert re.search(rf"#define CDDPM_PIPE_{name} {int(val)}\b", header), name
    assert "cddpm_aug_pipeline" in load_pkg("_lib").SYMBOLS and "cddpm_aug_pipeline_workspace_bytes" in load_pkg("_lib").SYMBOLS
    assert A.STREAM_AUG_NOISE == PR.NOISE_STREAM == 0x6002


@pytest.mark.parametrize("key", ("random_elastic", "random_motion", "unique_slice"))
def test_the_refusals_that_remain(key):
    with pytest.raises(NotImplementedError, match=key):
        A.SliceAugment.from_cfg({"aug_intensity": True, "random_flip": True, key: True})
    assert A.SliceAugment.from_cfg({"random_flip": True, key: False}).stages == (64,)
    assert len(A.REFUSED_KEYS) == 9 and set(A.PIPELINE_REFUSED_KEYS) | set(A.PIPELINE_KEYS) == set(A.REFUSED_KEYS)


def test_refused_vol2slice_variants():
    for kw in (dict(onlyBrain=True), dict(slice=20), dict(seq_slices=3)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            A.SliceAugment.from_cfg({"random_noise": True}, **kw)
    with pytest.raises(ValueError):
        A.SliceAugment(p={3: 0.5})
    with pytest.raises(ValueError):
        A.SliceAugment(p={64: 1.5})


@pytest.mark.parametrize("spacing", [(2.0, 2.0, 2.0), (1.0, 1.5, 3.0)])
def test_policy_draws_equal_the_intensity_recipe_column_for_column(spacing):
    pos, vols = np.arange(300), np.arange(300) % 7
    m4, p28 = A.IntensityAugment().draw(9, 2, pos, 11, spacing, volumes=vols)
    for recipe in (A.SliceAugment.from_cfg({"aug_intensity": True}), A.SliceAugment()):
        m8, p64 = recipe.draw(9, 2, pos, 11, spacing, volumes=vols)
        assert m8.dtype == np.int32 and m8.shape == (300, 8) and p64.dtype == np.float32 and p64.shape == (300, 64)
        assert np.array_equal(m8[:, 0], m4[:, 0]) and np.array_equal(m8[:, 1], m4[:, 1]) and np.array_equal(m8[:, 4], m4[:, 3])
        assert np.array_equal((m8[:, 2] >> 7) & 15, m4[:, 2])
        assert np.array_equal(p64[:, 25:50], p28[:, :25])
        assert not m8[:, 7].any() and not p64[:, 60:].any()
    only_policy = A.SliceAugment.from_cfg({"aug_intensity": True}).draw(9, 2, pos, 11, spacing, volumes=vols)[0]
    assert not (only_policy[:, 2] & 127).any()


def test_draw_ranges_and_slot_frequencies():
    aug = A.SliceAugment()
    n, D = 20000, 50
    meta, par = aug.draw(7, 3, np.arange(n), D, spacing=(2.0, 2.0, 2.0))
    assert (meta[:, 2] & ~2047 == 0).all()
    for bit, p in aug.p.items():
        p = p * 0.5 if bit == A.SLOT_FLIP else p                  # the gate and RandomFlip's own draw
        k = int(((meta[:, 2] & bit) != 0).sum())
        assert abs(k - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (bit, k)
    g, axis = meta[:, 3] & 0xff, meta[:, 3] >> 8
    assert set(np.unique(g)) == set(range(4, 11)) and set(np.unique(axis)) == {0, 1, 2}
    assert np.exp(-0.3) <= par[:, 0].min() and par[:, 0].max() <= np.float32(np.exp(0.3))
    assert 0 <= par[:, 1:4].min() and par[:, 1:4].max() <= 1.0 and 0.5 <= par[:, 4].min() and par[:, 4].max() <= 1.0
    assert -0.5 <= par[:, 5:25].min() and par[:, 5:25].max() <= 0.5
    assert 0 <= par[:, 50].min() < 0.0025 and 0.2475 < par[:, 50].max() <= 0.25
    assert len(np.unique(meta[:, 5])) > 0.99 * n and len(np.unique(meta[:, 6])) > 0.99 * n
    # the slot set is drawn apart from the policy set
    assert not np.array_equal(par[:, 0:25], par[:, 25:50]) and abs(np.corrcoef(par[:, 0], par[:, 25])[0, 1]) < 0.05
    # the matrix: singular values 1 / scales at isotropic spacing, within the drawn ranges
    sv = np.linalg.svd(par[:200, 51:60].reshape(-1, 3, 3).astype(np.float64), compute_uv=False)
    assert 1 / 1.1 - 1e-6 <= sv.min() and sv.max() <= 1 / 0.9 + 1e-6
    # every value is a function of (seed, epoch, position) alone
    for split in ((0, 5, 37), (0, 36, 37)):
        parts = [aug.draw(7, 3, np.arange(a, b), D) for a, b in zip(split[:-1], split[1:])]
        assert np.array_equal(np.concatenate([m for m, _ in parts]), meta[:37]) and np.array_equal(np.concatenate([p for _, p in parts]), par[:37])
    assert not np.array_equal(aug.draw(8, 3, np.arange(37), D)[1], par[:37]) and not np.array_equal(aug.draw(7, 4, np.arange(37), D)[1], par[:37])


class _Bank:
    """the host side of a VolumeBank: what the loader's row arithmetic reads"""
    def __init__(self, n, shape=(16, 12, 4)):
        self.n, self.shape, self.spacing, self.device = n, shape, (1.0, 1.5, 3.0), "cpu"

    def __len__(self):
        return self.n


def test_two_ranks_of_B_equal_one_rank_of_2B_on_the_new_tables():
    aug = A.SliceAugment()
    for n, B, drop in ((19, 4, True), (19, 4, False), (5, 4, False)):
        one = A.DeviceSliceLoader(_Bank(n), 2 * B, 5, aug, drop_last=drop, engine=object())
        ranks = [A.DeviceSliceLoader(_Bank(n), B, 5, aug, drop_last=drop, rank=r, world=2, engine=object()) for r in (0, 1)]
        for ld in (one, *ranks):
            ld.set_epoch(3)
        rows = [ld._rows() for ld in ranks]
        for k, (first, count) in enumerate(one._rows()):
            want = one.tables(first, count)
            assert want[0].shape == (count, 8) and want[1].shape == (count, 64)
            got = [ld.tables(*r[k]) for ld, r in zip(ranks, rows) if k < len(r)]
            assert np.array_equal(np.concatenate([m for m, _ in got]), want[0])
            assert np.array_equal(np.concatenate([p for _, p in got]), want[1])


def test_rotation_is_orthogonal_and_the_identity_draw_gives_the_identity_matrix():
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(20):
        deg = rng.uniform(-10, 10, 3)
        R = A.euler_matrix(deg)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    for spacing in ((2.0, 2.0, 2.0), (1.0, 1.5, 3.0), (0.7, 4.0, 1.0)):
        assert np.array_equal(A.affine_matrix((0, 0, 0), (1, 1, 1), spacing), np.eye(3))
    # R = Rz Rx Ry: a rotation about one axis leaves that axis alone, and scales divide along their own axis
    assert np.allclose(A.euler_matrix((7, 0, 0))[0], (1, 0, 0)) and np.allclose(A.euler_matrix((0, 7, 0))[1], (0, 1, 0))
    assert np.allclose(A.euler_matrix((0, 0, 7))[2], (0, 0, 1))
    a, b, c = A.euler_matrix((3, 0, 0)), A.euler_matrix((0, 5, 0)), A.euler_matrix((0, 0, -8))
    assert np.allclose(A.euler_matrix((3, 5, -8)), c @ a @ b, atol=1e-15)
    assert np.allclose(A.affine_matrix((0, 0, 0), (0.9, 1.0, 1.1), (1.0, 1.5, 3.0)), np.diag([1 / 0.9, 1.0, 1 / 1.1]))
    # anisotropic spacing: the rotation acts in mm
    M = A.affine_matrix((0, 0, 10), (1, 1, 1), (1.0, 2.0, 3.0))
    assert np.allclose(M, np.diag([1, 0.5, 1 / 3]) @ A.euler_matrix((0, 0, 10)).T @ np.diag([1, 2, 3]))


def test_table_check_names_the_bad_row():
    E = load_pkg("engine").CddpmEngine
    meta, par = A.SliceAugment().draw(1, 0, np.arange(6), 4, volumes=np.arange(6) % 3)
    E.check_pipeline_tables(meta, par, 3, 4)
    for what, col, val, table in (("volume", 0, 3, "meta"), ("z outside", 1, 4, "meta"), ("slot ghosting word.*axis", 3, 4 | (3 << 8), "meta"),
                                  ("policy ghosting word.*axis", 4, 4 | (3 << 8), "meta"), ("slot ghosting word", 3, -1, "meta"),
                                  ("flag", 2, 2048, "meta"), ("slot sigma", 2, 9.0, "par"), ("policy sigma", 26, -1.0, "par"),
                                  ("non-finite slot", 0, np.nan, "par"), ("non-finite policy", 32, np.inf, "par"),
                                  ("non-finite noise std", 50, np.nan, "par"), ("non-finite affine matrix", 55, np.inf, "par")):
        m, p = meta.copy(), par.copy()
        (m if table == "meta" else p)[4, col] = val
        with pytest.raises(RuntimeError, match=f"cddpm_aug_pipeline: sample 4: .*{what}"):
            E.check_pipeline_tables(m, p, 3, 4)
    with pytest.raises(RuntimeError, match="int32"):
        E.check_pipeline_tables(meta.astype(np.int64), par, 3, 4)
    with pytest.raises(RuntimeError, match=r"\[6, 64\]"):
        E.check_pipeline_tables(meta, par[:, :28].copy(), 3, 4)


def test_workspace_bytes_host_arithmetic():
    lib = load_pkg("_lib").load_library()
    one = lib.cddpm_aug_pipeline_workspace_bytes(1, 16, 12, 4)
    assert one >= 2 * 16 * 12 * 4 * 4
    b32 = lib.cddpm_aug_pipeline_workspace_bytes(32, 96, 96, 50)
    # two work volumes per sample and small tables: two combs of 1024 doubles, two sets of blur weights, the plan, a few words
    assert 32 * 2 * 96 * 96 * 50 * 4 <= b32 <= 32 * 2 * 96 * 96 * 50 * 4 + 32 * 2 * 16384
    assert b32 > lib.cddpm_aug_workspace_bytes(32, 96, 96, 50)
    for bad in ((0, 16, 12, 4), (1, 0, 12, 4), (1, 16, 1025, 4), (1, 16, 12, -1), (65536, 1, 1, 1)):
        assert lib.cddpm_aug_pipeline_workspace_bytes(*bad) == 0
        assert "cddpm_aug_pipeline_workspace_bytes" in lib.cddpm_last_error(None).decode()


@pytest.mark.parametrize("shape", [(16, 12, 4), (15, 9, 5)])
def test_trilinear_resample_equals_map_coordinates_at_interior_points(shape):
    rng = np.random.Generator(np.random.PCG64(sum(shape)))
    vol = rng.random(shape) - 0.02
    M = A.affine_matrix((6.0, -9.0, 4.0), (0.93, 1.08, 1.02), (1.0, 1.5, 3.0)).astype(np.float32)
    q = PR.source_coords(shape, M)
    L = np.asarray(shape)
    interior = ((q >= 0) & (q <= L - 1)).all(axis=-1)
    assert 50 < interior.sum() < interior.size
    want = ndimage.map_coordinates(vol, q[interior].T, order=1)
    got = PR.affine(vol, M)[interior]
    assert np.abs(got - want).max() < 1e-14
    # outside the half-voxel border: the minimum; the identity matrix: the volume, bit for bit, in both variants
    out = PR.affine(vol, M)
    outside = ~((q >= -0.5) & (q <= L - 0.5)).all(axis=-1)
    assert outside.any() and (out[outside] == vol.min()).all()
    assert np.array_equal(PR.affine(vol, np.eye(3).reshape(9)), vol)
    assert np.array_equal(PR.affine(vol.astype(np.float32), np.eye(3).reshape(9), np.float32), vol.astype(np.float32))
    assert PR.boundary_distance(shape, np.eye(3).reshape(9)) == 0.5


def test_flip_equals_np_flip_and_the_pipeline_composes_in_order():
    rng = np.random.Generator(np.random.PCG64(5))
    vol = (rng.random((16, 12, 4)) - 0.02).astype(np.float32)
    assert np.array_equal(PR.flip(vol), np.flip(vol, axis=0))
    meta, par = A.SliceAugment().draw(2, 0, np.arange(1), 4, (1.0, 1.5, 3.0))
    meta[0, 1], meta[0, 2] = 2, PR.FLIP
    assert np.array_equal(PR.pipeline_slice(vol, meta[0], par[0]), np.flip(vol, axis=0)[:, :, 2])
    meta[0, 2] = 0
    assert np.array_equal(PR.pipeline_slice(vol, meta[0], par[0], np.float32), vol[:, :, 2])
    # affine then flip, in sequence
    meta[0, 2] = PR.AFFINE | PR.FLIP
    assert np.array_equal(PR.pipeline_slice(vol, meta[0], par[0]), np.flip(PR.affine(vol, par[0, 51:60]), axis=0)[:, :, 2])
    # noise of std 0 is the identity, bit for bit
    meta[0, 2], par[0, 50] = PR.NOISE, 0.0
    assert np.array_equal(PR.pipeline_slice(vol, meta[0], par[0], np.float32), vol[:, :, 2])


def test_restated_philox_and_normals_equal_synth():
    synth = load_pkg("synth")
    k0, k1 = 0x9abcdef1, 0x12345678
    q = np.arange(40, dtype=np.uint32)
    want = synth.philox4x32(q, np.uint32(0), np.uint32(0), np.uint32(0x6002), k0, k1)
    got = PR.philox4x32_10(q, 0, 0, 0x6002, k0, k1)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    shape = (5, 4, 3)                                             # 60 voxels: 15 quads
    n = PR.noise_normals(shape, k0, k1).transpose(2, 0, 1).reshape(-1)       # back to memory order
    f32 = synth.normal_quads(15, 0, 0, 0x6002, k0 | (k1 << 32))
    assert np.abs(n - f32).max() < 4e-6                           # synth's fp32 Box-Muller of the same uniforms, |n| < 6
    big = PR.noise_normals((96, 96, 50), 1, 2)
    assert abs(big.mean()) < 4 / np.sqrt(big.size) and abs(big.std() - 1) < 0.005
