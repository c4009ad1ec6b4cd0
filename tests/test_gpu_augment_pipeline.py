"""GPU: the eleven-slot augmentation pipeline (cddpm_aug_pipeline, csrc/augment.hip, through CddpmEngine.augment_pipeline and
augment.DeviceSliceLoader) against the live numpy / scipy restatement of tests/augment_pipeline_reference.py.

The bound is the project's own. Every case is compared with the float64 restatement, normalised by max |ref| of the case, and the
device's error may be at most max(4 x the error of the float32 restatement IN THE SAME CASE, 2^-23): the 4 is the margin of
tests/test_gpu_augment.py, the floor one fp32 rounding of a value of size max |ref| with its neighbour's (tests/test_gpu_preprocess.py).
No voxel is left out. Instead the test asserts about its own inputs that no source coordinate of an affine case lies within 1e-6 of
-0.5 or L - 0.5 -- the device forms q with fused multiply-adds, numpy without, and only a voxel that close could fall on the other
side of the inside test -- and takes the next seed for a row's angles and scales when one does.

The shapes are the smallest at which the passes can go wrong: (16, 12, 4) has D below the blur radius and W below a wave, (15, 9, 5) is
odd everywhere, (8, 70, 1) has D = 1, where the affine sends most voxels outside and the minimum fills them, and (96, 96, 50), the
experiments' volume, runs once with a batch of 4. Spacings (2, 2, 2) and (1, 1.5, 3). Volumes are rand - 0.02, as in
tests/test_gpu_augment.py. At (16, 12, 4) the masks are each slot alone, every pair, all on and 64 random ones; every z and every
ghosting axis occur in each of these groups, the product z x axis thinned to four rows per mask."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import augment_pipeline_reference as PR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

A = load_pkg("augment")
MARGIN, FLOOR = 4.0, 2.0 ** -23
SIGMAS = ((1.0, 0.5, 1.0), (0.05, 0.9, 0.3), (1.0, 1.0, 0.0))      # radius 4 >= D = 4; radius 0 on axis 0; axis 2 skipped
SPACINGS = ((2.0, 2.0, 2.0), (1.0, 1.5, 3.0))
ALL = 2047
SINGLES = [1 << k for k in range(11)]
PAIRS = [a | b for a, b in itertools.combinations(SINGLES, 2)]


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


def volumes(shape, n, seed):
    """n volumes [H, W, D] fp32 (torchio's layout) with negatives"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(rng.random(shape) - 0.02).astype(np.float32) for _ in range(n)]


def tables(rows, shape, spacing, seed=0, identity=False):
    """rows: (volume, z, flags, slot axis, policy axis) -> meta, par. Per row: both parameter sets as tests/test_gpu_augment.py draws
    them (gamma around 1, coefficients U(-0.5, 0.5), sigmas from SIGMAS, g in {4, 10}, I in {0.5, 1}), std ~ U(0, 0.25), two key words,
    and the affine's M from degrees ~ U(-10, 10) and scales ~ U(0.9, 1.1), redrawn while a source coordinate lies within 1e-6 of the
    border of the inside test."""
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    meta = np.zeros((len(rows), 8), np.int32)
    par = np.zeros((len(rows), 64), np.float32)
    for b, (v, z, flags, axis_s, axis_p) in enumerate(rows):
        g = ((4, 10)[b % 2], (10, 4)[(b // 2) % 2])
        meta[b, :5] = (v, z, flags, g[0] | (axis_s << 8), g[1] | (axis_p << 8))
        meta[b, 5:7] = rng.integers(-2 ** 31, 2 ** 31, 2)
        for s, par0 in enumerate((0, 25)):
            par[b, par0] = np.exp(rng.uniform(-0.3, 0.3))
            par[b, par0 + 1:par0 + 4] = SIGMAS[(b + s) % 3]
            par[b, par0 + 4] = (0.5, 1.0)[(b // 3 + s) % 2]
            par[b, par0 + 5:par0 + 25] = rng.uniform(-0.5, 0.5, 20)
        par[b, 50] = rng.uniform(0.0, 0.25)
        for _attempt in range(20):
            M = np.eye(3) if identity else A.affine_matrix(rng.uniform(-10, 10, 3), rng.uniform(0.9, 1.1, 3), spacing)
            par[b, 51:60] = M.reshape(9)
            if identity or PR.boundary_distance(shape, par[b, 51:60]) > 1e-6:
                break
        assert identity or PR.boundary_distance(shape, par[b, 51:60]) > 1e-6, "no clean draw of the affine"
    return meta, par


def rows_for(masks, shape, nvol, per_mask=4):
    """per mask `per_mask` rows; over them z runs through 0 .. D-1 and both ghosting axes through 0 .. 2"""
    D = shape[2]
    return [(i % nvol, (i + k) % D, flags, k % 3, (k + i) % 3) for i, flags in enumerate(masks) for k in range(per_mask)]


def compare(eng, vols, meta, par, tag, spacing=SPACINGS[0]):
    """every row against the float64 restatement under the bound of the module docstring; prints the largest ratio per flag mask group"""
    bank = A.VolumeBank(vols, "cuda", spacing)
    got = eng.augment_pipeline(bank, meta, par).cpu().numpy()
    worst_dev, worst_f32, worst_ratio, fails = 0.0, 0.0, 0.0, []
    for b in range(len(meta)):
        vol = vols[meta[b, 0]]
        ref = PR.pipeline_slice(vol, meta[b], par[b], np.float64)
        f32 = PR.pipeline_slice(vol, meta[b], par[b], np.float32)
        assert f32.dtype == np.float32 and ref.dtype == np.float64
        scale = float(np.abs(ref).max())
        e_dev = float(np.abs(got[b].astype(np.float64) - ref).max()) / scale
        e_f32 = float(np.abs(f32.astype(np.float64) - ref).max()) / scale
        worst_dev, worst_f32 = max(worst_dev, e_dev), max(worst_f32, e_f32)
        worst_ratio = max(worst_ratio, e_dev / max(MARGIN * e_f32, FLOOR))
        if not e_dev <= max(MARGIN * e_f32, FLOOR):
            fails.append((b, meta[b].tolist(), e_dev, e_f32))
    print(f"{tag}: {len(meta)} cases, device error <= {worst_dev:.2e}, float32 restatement <= {worst_f32:.2e}; largest device error / bound "
          f"{worst_ratio:.3f}")
    assert not fails, fails[:5]


@pytest.mark.parametrize("spacing", SPACINGS)
def test_each_slot_alone_and_all_on(eng, spacing):
    """each of the 11 slots alone and all on at (16, 12, 4): every z x every axis of both ghosting slots"""
    shape = (16, 12, 4)
    vols = volumes(shape, 3, 1)
    rows = [(i % 3, z, flags, ax, (ax + z) % 3) for i, (flags, z, ax) in enumerate(itertools.product(SINGLES + [ALL], range(4), range(3)))]
    compare(eng, vols, *tables(rows, shape, spacing, 1), f"(16, 12, 4) singles and all, spacing {spacing}", spacing)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_every_pair_of_slots(eng, spacing):
    shape = (16, 12, 4)
    vols = volumes(shape, 3, 2)
    assert len(PAIRS) == 55
    compare(eng, vols, *tables(rows_for(PAIRS, shape, 3), shape, spacing, 2), f"(16, 12, 4) pairs, spacing {spacing}", spacing)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_random_masks(eng, spacing):
    shape = (16, 12, 4)
    vols = volumes(shape, 3, 3)
    masks = np.random.Generator(np.random.PCG64(33)).integers(0, 2048, 64).tolist()
    compare(eng, vols, *tables(rows_for(masks, shape, 3), shape, spacing, 3), f"(16, 12, 4) 64 random masks, spacing {spacing}", spacing)


@pytest.mark.parametrize("shape,spacing", [((15, 9, 5), SPACINGS[1]), ((8, 70, 1), SPACINGS[0])])
def test_odd_and_flat_shapes(eng, shape, spacing):
    vols = volumes(shape, 2, 4)
    masks = SINGLES + [ALL, 32 | 64, 2 | 32, 4 | 32 | 64, 1 | 2 | 4 | 8 | 16] + np.random.Generator(np.random.PCG64(44)).integers(0, 2048, 16).tolist()
    meta, par = tables(rows_for(masks, shape, 2, per_mask=3), shape, spacing, 4)
    if shape[2] == 1:                       # the affine sends most voxels of a one-slice volume outside: the minimum fills them
        q = PR.source_coords(shape, par[SINGLES.index(32) * 3, 51:60])
        assert (np.abs(q[..., 2]) > 0.5).mean() > 0.5
    compare(eng, vols, meta, par, str(shape), spacing)


def test_experiment_volume_one_batch_of_four(eng):
    shape = (96, 96, 50)
    vols = volumes(shape, 2, 5)
    rows = [(0, 0, ALL, 0, 2), (1, 49, ALL & ~8, 2, 1), (1, 24, 2 | 4 | 32 | 1024, 1, 0), (0, 31, 1 | 16 | 64 | 128 | 512, 0, 1)]
    compare(eng, vols, *tables(rows, shape, SPACINGS[0], 5), str(shape))


def test_identities_are_bit_exact(eng):
    """flags 0 is the slice; flip alone is the mirrored slice; the affine with the identity matrix is the slice; noise with std 0 leaves
    what the earlier slots made"""
    shape = (16, 12, 4)
    vols = volumes(shape, 2, 6)
    bank = A.VolumeBank(vols, "cuda")
    rows = [(b % 2, b % 4, 0, b % 3, (b + 1) % 3) for b in range(8)]
    got = eng.augment_pipeline(bank, *tables(rows, shape, SPACINGS[0], 6)).cpu().numpy()
    for b, r in enumerate(rows):
        assert np.array_equal(got[b], vols[r[0]][:, :, r[1]])
    got = eng.augment_pipeline(bank, *tables([(v, z, 64, a, p) for v, z, _f, a, p in rows], shape, SPACINGS[0], 6)).cpu().numpy()
    for b, r in enumerate(rows):
        assert np.array_equal(got[b], vols[r[0]][::-1, :, r[1]])
    for flags, mirrored in ((32, False), (32 | 64, True)):
        got = eng.augment_pipeline(bank, *tables([(v, z, flags, a, p) for v, z, _f, a, p in rows], shape, SPACINGS[1], 6, identity=True)).cpu().numpy()
        for b, r in enumerate(rows):
            vol = np.flip(vols[r[0]], axis=0) if mirrored else vols[r[0]]
            assert np.array_equal(got[b], vol[:, :, r[1]])
    for before in (0, 1, 1 | 4, 1 | 8 | 16 | 32 | 64, ALL & ~2):
        with_noise = [(v, z, before | 2, a, p) for v, z, _f, a, p in rows]
        meta, par = tables(with_noise, shape, SPACINGS[0], 7)
        par[:, 50] = 0.0
        a = eng.augment_pipeline(bank, meta, par).clone()
        meta[:, 2] = before
        b = eng.augment_pipeline(bank, meta, par)
        assert torch.equal(a, b)
        if before:
            assert not torch.equal(b[0], torch.from_numpy(vols[0][:, :, 0]).cuda())


def test_policy_bits_alone_give_the_slices_entry_bit_for_bit(eng):
    """a table with only policy bits against cddpm_aug_slices on the corresponding four-bit rows, at every mask, z and axis"""
    for shape in ((16, 12, 4), (15, 9, 5)):
        vols = volumes(shape, 3, 8)
        bank = A.VolumeBank(vols, "cuda")
        rows = [(i % 3, z, f4 << 7, (i + 1) % 3, ax) for i, (f4, z, ax) in enumerate(itertools.product(range(16), range(shape[2]), range(3)))]
        meta, par = tables(rows, shape, SPACINGS[0], 8)
        m4, p28 = np.zeros((len(rows), 4), np.int32), np.zeros((len(rows), 28), np.float32)
        m4[:, :2], m4[:, 2], m4[:, 3] = meta[:, :2], meta[:, 2] >> 7, meta[:, 4]
        p28[:, :25] = par[:, 25:50]
        want = eng.augment_slices(bank, m4, p28).clone()
        assert torch.equal(eng.augment_pipeline(bank, meta, par), want)


def test_batch_and_order_invariance_bit_for_bit(eng):
    shape = (15, 9, 5)
    vols = volumes(shape, 3, 9)
    bank = A.VolumeBank(vols, "cuda", SPACINGS[1])
    rows = [(2, 4, ALL, 0, 1), (0, 0, 2 | 32 | 1024, 2, 2), (1, 2, 0, 1, 1), (2, 1, 4 | 8 | 64 | 256, 1, 0), (0, 3, 1 | 16 | 32 | 64 | 128 | 512, 2, 1)]
    meta, par = tables(rows, shape, SPACINGS[1], 9)
    whole = eng.augment_pipeline(bank, meta, par).clone()
    for b in range(5):
        assert torch.equal(eng.augment_pipeline(bank, meta[b:b + 1], par[b:b + 1])[0], whole[b]), b
    perm = np.array([3, 0, 4, 2, 1])
    assert torch.equal(eng.augment_pipeline(bank, meta[perm], par[perm]), whole[torch.from_numpy(perm).cuda()])
    assert torch.equal(eng.augment_pipeline(bank, meta, par), whole)


def test_refusals_leave_the_output_untouched(eng):
    """bad table rows are refused on the host before anything is copied and name themselves; the library refuses a short workspace before
    anything is enqueued; rows that reach the device bad are flagged by the first kernel and no kernel writes the output for them, while
    the good rows of the same call are computed"""
    shape = (16, 12, 4)
    N = 2
    vols = volumes(shape, N, 10)
    bank = A.VolumeBank(vols, "cuda")
    good = [(b % 2, b % 4, ALL, b % 3, (b + 1) % 3) for b in range(6)]
    gmeta, gpar = tables(good, shape, SPACINGS[0], 10)

    def spoil(what):
        meta, par = gmeta.copy(), gpar.copy()
        for w in what:
            b, table, col, val, _match, _bit = BAD[w]
            (meta if table == "meta" else par)[b, col] = val
        return meta, par

    BAD = {"volume": (1, "meta", 0, N, "volume", 1), "z": (2, "meta", 1, 4, "z outside", 2), "axis": (3, "meta", 3, 4 | (3 << 8), "axis", 4),
           "sigma": (4, "par", 27, 9.0, "sigma", 8), "std": (1, "par", 50, np.nan, "non-finite noise std", 32),
           "matrix": (2, "par", 59, np.inf, "non-finite affine matrix", 32), "flags": (3, "meta", 2, 4096, "flag", 16)}
    out = torch.full((6, 16, 12), -7.0, device="cuda")
    for what, (b, _t, _c, _v, match, _bit) in BAD.items():
        with pytest.raises(RuntimeError, match=f"cddpm_aug_pipeline: sample {b}: .*{match}"):
            eng.augment_pipeline(bank, *spoil([what]), out=out)
        assert bool((out == -7.0).all())
    want = eng.augment_pipeline(bank, gmeta, gpar).clone()
    lib = eng.lib
    need = lib.cddpm_aug_pipeline_workspace_bytes(6, 16, 12, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda mm, pp, nbytes: lib.cddpm_aug_pipeline(eng._h, bank.data.data_ptr(), N, 16, 12, 4, mm.data_ptr(), pp.data_ptr(), 6, ws.data_ptr(),
                                                         nbytes, out.data_ptr(), stream)
    m, p = torch.from_numpy(gmeta).cuda(), torch.from_numpy(gpar).cuda()
    assert call(m, p, need - 1) == -1 and "workspace" in lib.cddpm_last_error(eng._h).decode()
    assert lib.cddpm_aug_pipeline(eng._h, bank.data.data_ptr(), N, 16, 12, 4, m.data_ptr(), None, 6, ws.data_ptr(), need, out.data_ptr(), stream) == -1
    assert lib.cddpm_aug_pipeline(eng._h, bank.data.data_ptr(), N, 16, 1025, 4, m.data_ptr(), p.data_ptr(), 6, ws.data_ptr(), need, out.data_ptr(),
                                  stream) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the device: bad rows 1 .. 4 in one call, flagged; rows 0 and 5 are good and computed
    for group, status in ((("volume", "z", "axis", "sigma"), [0, 1, 2, 4, 8, 0]), (("std", "matrix", "flags", "sigma"), [0, 32, 32, 16, 8, 0])):
        meta, par = spoil(group)
        m, p = torch.from_numpy(meta).cuda(), torch.from_numpy(par).cuda()
        out.fill_(-7.0)
        assert call(m, p, need) == 0
        torch.cuda.synchronize()
        assert ws[:24].view(torch.int32).cpu().tolist() == status
        assert bool((out[1:5] == -7.0).all())
        assert torch.equal(out[0], want[0]) and torch.equal(out[5], want[5])


def test_loader_over_the_policy_recipe_yields_the_intensity_loader_tensors(eng):
    shape = (16, 12, 4)
    bank = A.VolumeBank(np.stack(volumes(shape, 10, 11)), "cuda", SPACINGS[1])
    cfg = {"aug_intensity": True}
    old = A.DeviceSliceLoader(bank, 4, 3, A.IntensityAugment.from_cfg(cfg), drop_last=False, engine=eng)
    new = A.DeviceSliceLoader(bank, 4, 3, A.SliceAugment.from_cfg(cfg), drop_last=False, engine=eng)
    for epoch in (0, 1):
        old.set_epoch(epoch), new.set_epoch(epoch)
        a = [b["vol"]["data"].clone() for b in old]
        b = [b["vol"]["data"].clone() for b in new]
        assert [x.shape for x in b] == [(4, 1, 16, 12, 1), (4, 1, 16, 12, 1), (2, 1, 16, 12, 1)]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # and the full recipe runs, reproduces under its seed and differs from the policy alone
    full = A.DeviceSliceLoader(bank, 4, 3, A.SliceAugment(), drop_last=False, engine=eng)
    full.set_epoch(1)
    c = [b["vol"]["data"].clone() for b in full]
    d = [b["vol"]["data"].clone() for b in full]
    assert all(torch.equal(x, y) for x, y in zip(c, d)) and all(bool(torch.isfinite(x).all()) for x in c)
    assert not all(torch.equal(x, y) for x, y in zip(c, b))
