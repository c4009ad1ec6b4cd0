"""GPU: augmented training slices from a resident bank (csrc/augment.hip through CddpmEngine.augment_slices and augment.DeviceSliceLoader)
against the live numpy / scipy restatement of tests/augment_reference.py.

The bound. Every case is compared with the float64 restatement, normalised by max |ref| of the case, and the device's error may be at
most 4 x the error the float32 restatement (the same rules on float32 arrays) makes IN THE SAME CASE: the yardstick is the reference's own
fp32 error, never the code under test; 4 x is the margin the SparK tests give over torch's fp32 error and covers another, equally valid
fp32 order of evaluation and another `pow`. Where the float32 restatement is exact (flags = 0) the device must be.

The shapes are the smallest at which the kernels can go wrong: (16, 12, 4) has D below the blur radius and W below a wave, (15, 9, 5) is odd
everywhere, (8, 70, 1) has D = 1 and a W that straddles 64, and (96, 96, 50), the experiments' volume, runs once with a batch of 4.
Volumes are rand - 0.02: they have negatives, as the percentile-rescaled, B-spline-resampled volumes do."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import augment_reference as AR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

A = load_pkg("augment")
MARGIN = 4.0
SIGMAS = ((1.0, 0.5, 1.0), (0.05, 0.9, 0.3), (1.0, 1.0, 0.0))      # radius 4 >= D = 4; radius 0 on axis 0; axis 2 skipped
STAGE = {0: "copy", 1: "gamma", 2: "bias", 4: "blur", 8: "ghost", 15: "all"}


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


def volumes(shape, n, seed):
    """n volumes [H, W, D] fp32 (torchio's layout) with negatives"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(rng.random(shape) - 0.02).astype(np.float32) for _ in range(n)]


def tables(cases, seed=0):
    """cases: (volume, z, flags, g, axis, sigmas, I) -> meta, par; gamma alternates around 1, the bias coefficients are U(-0.5, 0.5)"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    meta = np.zeros((len(cases), 4), np.int32)
    par = np.zeros((len(cases), 28), np.float32)
    for b, (v, z, flags, g, axis, sig, I) in enumerate(cases):
        meta[b] = (v, z, flags, g | (axis << 8))
        par[b, 0] = np.exp(rng.uniform(-0.3, 0.3))
        par[b, 1:4] = sig
        par[b, 4] = I
        par[b, 5:25] = rng.uniform(-0.5, 0.5, 20)
    return meta, par


def compare(eng, vols, meta, par, tag):
    """every row against the float64 restatement under the bound of the module docstring; prints the largest ratio per flag mask"""
    bank = A.VolumeBank(vols, "cuda")
    got = eng.augment_slices(bank, meta, par).cpu().numpy()
    ratio, worst_dev, worst_f32, fails = {}, 0.0, 0.0, []
    for b in range(len(meta)):
        vol = vols[meta[b, 0]]
        ref = AR.augment_slice(vol, meta[b], par[b], np.float64)
        f32 = AR.augment_slice(vol, meta[b], par[b], np.float32)
        assert f32.dtype == np.float32 and ref.dtype == np.float64
        scale = float(np.abs(ref).max())
        e_dev = float(np.abs(got[b].astype(np.float64) - ref).max()) / scale
        e_f32 = float(np.abs(f32.astype(np.float64) - ref).max()) / scale
        worst_dev, worst_f32 = max(worst_dev, e_dev), max(worst_f32, e_f32)
        fl = int(meta[b, 2])
        if e_f32 > 0:
            ratio[fl] = max(ratio.get(fl, 0.0), e_dev / e_f32)
        if not e_dev <= MARGIN * e_f32:
            fails.append((b, meta[b].tolist(), par[b, :5].tolist(), e_dev, e_f32))
    print(f"{tag}: {len(meta)} cases, device error <= {worst_dev:.2e}, float32 restatement <= {worst_f32:.2e}; largest device / float32 ratio per "
          "mask: " + ", ".join(f"{STAGE.get(k, k)} {v:.2f}" for k, v in sorted(ratio.items())))
    assert not fails, fails[:5]


@pytest.mark.parametrize("sig", SIGMAS)
def test_every_stage_and_mask(eng, sig):
    """each stage alone and all 16 flag masks at (16, 12, 4), for every z and every ghost axis, g in {4, 10} (10 > D), I in {0.5, 1}"""
    shape = (16, 12, 4)
    vols = volumes(shape, 3, 1)
    cases = [(i % 3, z, flags, g, axis, sig, I)
             for i, (flags, z, axis, g, I) in enumerate(itertools.product(range(16), range(4), range(3), (4, 10), (0.5, 1.0)))]
    assert len(cases) == 16 * 4 * 3 * 2 * 2
    compare(eng, vols, *tables(cases, 1), f"(16, 12, 4) sigma {sig}")


@pytest.mark.parametrize("shape", [(15, 9, 5), (8, 70, 1)])
def test_odd_and_flat_shapes(eng, shape):
    vols = volumes(shape, 2, 2)
    cases = [(i % 2, z, flags, g, axis, SIGMAS[i % 3], (0.5, 1.0)[(i // 3) % 2])
             for i, (flags, z, axis, g) in enumerate(itertools.product(range(16), range(shape[2]), range(3), (4, 10)))]
    compare(eng, vols, *tables(cases, 2), str(shape))


def test_experiment_volume_one_batch_of_four(eng):
    shape = (96, 96, 50)
    vols = volumes(shape, 2, 3)
    cases = [(0, 0, 15, 4, 0, (1.0, 0.5, 1.0), 1.0), (1, 49, 15, 7, 2, (0.3, 1.0, 0.9), 0.5), (1, 24, 12, 10, 1, (1.0, 1.0, 0.0), 0.75),
             (0, 31, 3, 4, 0, (0.0, 0.0, 0.0), 0.5)]
    compare(eng, vols, *tables(cases, 3), str(shape))


def test_identities_are_bit_exact(eng):
    """flags = 0 is a copy of the slice; g = 0 and I = 0 leave what the stages before the ghosting made"""
    shape = (16, 12, 4)
    vols = volumes(shape, 2, 4)
    bank = A.VolumeBank(vols, "cuda")
    cases = [(b % 2, b % 4, 0, 4, b % 3, SIGMAS[0], 1.0) for b in range(8)]
    got = eng.augment_slices(bank, *tables(cases, 4)).cpu().numpy()
    for b, c in enumerate(cases):
        assert np.array_equal(got[b], vols[c[0]][:, :, c[1]])
    for before in (0, 1, 2, 4, 7):
        with_ghost = [(0, z, before | 8, g, axis, SIGMAS[0], I) for z in range(4) for axis in range(3) for g, I in ((0, 1.0), (4, 0.0), (0, 0.0))]
        without = [(v, z, before, 4, axis, s, 1.0) for v, z, _f, _g, axis, s, _I in with_ghost]
        a = eng.augment_slices(bank, *tables(with_ghost, 5)).clone()
        b = eng.augment_slices(bank, *tables(without, 5))
        assert torch.equal(a, b)
        if before:
            assert not torch.equal(b[0], torch.from_numpy(vols[0][:, :, 0]).cuda())


def test_batch_and_order_invariance_bit_for_bit(eng):
    shape = (15, 9, 5)
    vols = volumes(shape, 3, 6)
    bank = A.VolumeBank(vols, "cuda")
    cases = [(2, 4, 15, 4, 0, SIGMAS[0], 1.0), (0, 0, 13, 10, 2, SIGMAS[1], 0.5), (1, 2, 0, 4, 1, SIGMAS[2], 0.5), (2, 1, 6, 7, 1, SIGMAS[2], 1.0),
             (0, 3, 11, 5, 1, SIGMAS[0], 0.7)]
    meta, par = tables(cases, 6)
    whole = eng.augment_slices(bank, meta, par).clone()
    for b in range(5):
        assert torch.equal(eng.augment_slices(bank, meta[b:b + 1], par[b:b + 1])[0], whole[b]), b
    perm = np.array([3, 0, 4, 2, 1])
    assert torch.equal(eng.augment_slices(bank, meta[perm], par[perm]), whole[torch.from_numpy(perm).cuda()])
    assert torch.equal(eng.augment_slices(bank, meta, par), whole)


def test_refusals_leave_the_output_untouched(eng):
    """bad table rows are refused on the host before anything is copied; the library refuses a short workspace before anything is enqueued;
    and rows that reach the device bad are flagged by the first kernel, which reads the two tables only -- no kernel reads the bank or
    writes the output for them, while the good rows of the same call are computed"""
    shape = (16, 12, 4)
    N = 2
    vols = volumes(shape, N, 7)
    bank = A.VolumeBank(vols, "cuda")
    good = [(b % 2, b % 4, 15, 4, b % 3, SIGMAS[0], 1.0) for b in range(6)]
    bad_rows = {"volume": (1, (N, 0, 15, 4, 0, SIGMAS[0], 1.0), 1), "z outside": (2, (0, 4, 15, 4, 0, SIGMAS[0], 1.0), 2),
                "axis": (3, (0, 0, 15, 4, 3, SIGMAS[0], 1.0), 4), "sigma": (4, (0, 0, 15, 4, 0, (1.0, 9.0, 1.0), 1.0), 8)}
    out = torch.full((6, 16, 12), -7.0, device="cuda")
    for what, (b, row, _bit) in bad_rows.items():
        cases = list(good)
        cases[b] = row
        with pytest.raises(RuntimeError, match=f"sample {b}: .*{what}"):
            eng.augment_slices(bank, *tables(cases, 7), out=out)
        assert bool((out == -7.0).all())
    want = eng.augment_slices(bank, *tables(good, 7)).clone()
    # the library: a short workspace
    lib, dev = eng.lib, out.device
    meta, par = tables(good, 7)
    m, p = torch.from_numpy(meta).cuda(), torch.from_numpy(par).cuda()
    need = lib.cddpm_aug_workspace_bytes(6, 16, 12, 4)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda mm, pp, nbytes: lib.cddpm_aug_slices(eng._h, bank.data.data_ptr(), N, 16, 12, 4, mm.data_ptr(), pp.data_ptr(), 6, ws.data_ptr(),
                                                       nbytes, out.data_ptr(), stream)
    assert call(m, p, need - 1) == -1 and "workspace" in lib.cddpm_last_error(eng._h).decode()
    assert lib.cddpm_aug_slices(eng._h, bank.data.data_ptr(), N, 16, 12, 4, m.data_ptr(), None, 6, ws.data_ptr(), need, out.data_ptr(), stream) == -1
    assert lib.cddpm_aug_slices(eng._h, bank.data.data_ptr(), N, 16, 1025, 4, m.data_ptr(), p.data_ptr(), 6, ws.data_ptr(), need, out.data_ptr(),
                                stream) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the device: the four bad rows in one call, flagged; rows 0 and 5 are good and computed
    cases = list(good)
    for what, (b, row, _bit) in bad_rows.items():
        cases[b] = row
    meta, par = tables(cases, 7)
    m, p = torch.from_numpy(meta).cuda(), torch.from_numpy(par).cuda()
    assert call(m, p, need) == 0
    torch.cuda.synchronize()
    status = ws[:24].view(torch.int32).cpu().tolist()
    assert status == [0, 1, 2, 4, 8, 0]
    assert bool((out[1:5] == -7.0).all())
    assert torch.equal(out[0], want[0]) and torch.equal(out[5], want[5])


def loader_epochs(bank, eng, seed, epochs, **kw):
    ld = A.DeviceSliceLoader(bank, kw.pop("B", 4), seed, A.IntensityAugment(), engine=eng, **kw)
    out = []
    for e in epochs:
        ld.set_epoch(e)
        batches = [b["vol"]["data"].clone() for b in ld]
        assert len(batches) == len(ld)
        out.append(batches)
    return out


def test_loader_reproduces_under_a_seed(eng):
    shape = (16, 12, 4)
    bank = A.VolumeBank(np.stack(volumes(shape, 6, 8)), "cuda")
    assert len(bank) == 6 and bank.shape == shape and bank.data.shape == (6, 4, 16, 12)
    a = loader_epochs(bank, eng, 3, (0, 1), drop_last=False)
    b = loader_epochs(bank, eng, 3, (0, 1), drop_last=False)
    c = loader_epochs(bank, eng, 4, (0, 1), drop_last=False)
    assert [x.shape for x in a[0]] == [(4, 1, 16, 12, 1), (2, 1, 16, 12, 1)] and a[0][0].dtype == torch.float32 and a[0][0].is_cuda
    for e in range(2):
        assert all(torch.equal(x, y) for x, y in zip(a[e], b[e]))
        assert not all(torch.equal(x, y) for x, y in zip(a[e], c[e]))
    assert not torch.equal(a[0][0], a[1][0])
    assert len(loader_epochs(bank, eng, 3, (0,), drop_last=True)[0]) == 1
    # without a recipe and without shuffling: the drawn slice of volumes 0 .. 3, bit for bit
    plain = A.DeviceSliceLoader(bank, 4, 3, None, shuffle=False, engine=eng)
    x = next(iter(plain))["vol"]["data"]
    meta, _ = plain.tables(0, 4)
    assert meta[:, 0].tolist() == [0, 1, 2, 3] and not meta[:, 2].any()
    for i in range(4):
        assert torch.equal(x[i, 0, :, :, 0], bank.data[i, int(meta[i, 1])])


def test_two_ranks_concatenate_to_the_one_rank_run(eng):
    shape = (16, 12, 4)
    bank = A.VolumeBank(volumes(shape, 16, 9), "cuda")
    one = loader_epochs(bank, eng, 5, (0, 1), B=8)
    r0 = loader_epochs(bank, eng, 5, (0, 1), B=4, rank=0, world=2)
    r1 = loader_epochs(bank, eng, 5, (0, 1), B=4, rank=1, world=2)
    for e in range(2):
        assert len(one[e]) == len(r0[e]) == len(r1[e]) == 2
        for k in range(2):
            assert torch.equal(torch.cat([r0[e][k], r1[e][k]]), one[e][k])


def test_ddpm2d_training_step_reads_a_loader_batch(eng, sd_np):
    """one DDPM_2D.training_step on a loader batch (synthetic weights, 32 x 32 slices, precision 32) returns the loss, bit for bit, of the
    same step given the identical tensor by hand"""
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=1000,
               lr=1e-4, aug_intensity=True)

    class Enc(torch.nn.Module):          # stand-in for the context encoder
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous() * 2 - 1

    bank = A.VolumeBank(volumes((32, 32, 3), 2, 10), "cuda")
    loader = A.DeviceSliceLoader(bank, 2, 1, A.IntensityAugment.from_cfg(cfg), engine=eng)
    batch = next(iter(loader))
    x = batch["vol"]["data"]
    assert x.shape == (2, 1, 32, 32, 1)
    by_hand = x.cpu().clone().cuda()
    losses = []
    for b in (batch, {"vol": {"data": by_hand}}):
        mod = M.DDPM_2D(cfg, encoder=Enc())
        mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        mod = mod.cuda()
        np.random.seed(5); torch.manual_seed(5)
        losses.append(mod.training_step(b, 0)["loss"].detach().cpu().clone())
        mod.diffusion.model._hip.close()
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1]), losses
