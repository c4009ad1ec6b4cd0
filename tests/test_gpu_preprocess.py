"""GPU: raw volumes preprocessed on the device (csrc/preprocess.hip through CddpmEngine.preprocess_volume / preprocess_labels,
preprocess.VolumePreprocess, VolumeBank.from_raw and EvalVolumes) against the live numpy / scipy restatement of
tests/preprocess_reference.py.

The bound. Every case is compared with the float64 restatement, normalised by max |ref| of the case, and the device's error may be at most
the larger of 4 x the error the float32 restatement (the same rules with the reference's own float32 stores) makes IN THE SAME CASE, and
2^-23: the yardstick is the reference's arithmetic, never the code under test; 4 x is the margin test_gpu_augment.py and the SparK tests
use; 2^-23 is one fp32 unit of the largest stored output (what a correctly rounded fp32 store may be off where the float32 restatement
happens to be exact). Crop / pad, every label output, the order statistics and the statuses are bit exact.

The curvature flow switches its update off where |grad|^2 < 1e-9. A rounding difference must not be able to flip that branch in a
compared case, so every smoothing case asserts that no voxel-iteration of its input has 1e-10 <= |grad|^2 < 1e-8 (random volumes satisfy
this), and the zero branch is tested on its own with a constant volume that must come back bit for bit.

Inputs are rand - 0.02 fp32 volumes with masks vol > 0.1 unless stated otherwise. The shapes: (13, 10, 7) -> (12, 12, 8), f = 2 crops,
pads odd and even and runs below a wave; (9, 8, 6), f = 1.5 has 24 sample points outside the extent; (6, 6, 6), f = 3; (80, 12, 10) has a
line longer than a wave; (3, 2, 5) -> (4, 2, 3), f = 1 has axes shorter than the spline's support; (48, 40, 20) -> (24, 20, 10) runs several
workgroups per pass; (2, 1024, 45) has the longest contiguous line the library takes (5 lines per LDS tile, 18 tiles) and lines along W
and D beyond the horizon of the mirror initial sum."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as EC
import preprocess_reference as PR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

A = load_pkg("augment")
P = load_pkg("preprocess")
MARGIN, FLOOR = 4.0, 2.0 ** -23
STAGE = {15: "all", 1: "smooth", 2: "croppad", 4: "rescale", 8: "resample"}
# shape, imageDim, f
CASES = [((13, 10, 7), (12, 12, 8), 2.0), ((9, 8, 6), (9, 8, 6), 1.5), ((6, 6, 6), (6, 6, 6), 3.0), ((80, 12, 10), (80, 12, 10), 2.0),
         ((3, 2, 5), (4, 2, 3), 1.0), ((48, 40, 20), (48, 40, 20), 2.0), ((2, 1024, 45), (2, 1024, 45), 2.0)]
PERC = (1.0, 99.0)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


def raw(shape, seed):
    """(vol fp32, mask uint8 = vol > 0.1, seg uint8 with labels 0 .. 3), torchio's layout [H, W, D]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    vol = (rng.random(shape) - 0.02).astype(np.float32)
    return vol, (vol > 0.1).astype(np.uint8), (rng.random(shape) * 4).astype(np.uint8)


def hwd(t):
    """a slice-major device result [D, H, W] -> numpy [H, W, D]"""
    return t.permute(1, 2, 0).contiguous().cpu().numpy()


def device_run(eng, vol, mask, stages, target, f, perc=PERC):
    res = eng.preprocess_volume(torch.from_numpy(vol).cuda(), None if mask is None else torch.from_numpy(mask).cuda(), stages=stages,
                                target=target, perc=perc, f=f)
    torch.cuda.synchronize()
    return hwd(res["vol"]), hwd(res["mask"]), P.record_dict(res["record"])


@pytest.mark.parametrize("shape,target,f", CASES)
def test_pipeline_and_every_stage_alone(eng, shape, target, f):
    vol, mask, seg = raw(shape, sum(shape))
    _, smallest, near = PR.curvature_flow(vol, condition=True)
    print(f"{shape}: smallest non-zero |grad|^2 = {smallest:.3e}, voxel-iterations near the branch: {near}")
    assert near == 0
    fails = []
    for stages in (15, 1, 2, 4, 8):
        ref = PR.preprocess(vol, mask, seg, stages, target, PERC, f, dtype=np.float64)
        f32 = PR.preprocess(vol, mask, seg, stages, target, PERC, f, dtype=np.float32)
        assert ref["vol"].dtype == np.float64 and f32["vol"].dtype == np.float32
        got, got_mask, rec = device_run(eng, vol, mask, stages, target, f)
        assert got.shape == ref["vol"].shape and rec["status"] == 0
        scale = float(np.abs(ref["vol"]).max())
        e_dev = float(np.abs(got.astype(np.float64) - ref["vol"]).max()) / scale
        e_f32 = float(np.abs(f32["vol"].astype(np.float64) - ref["vol"]).max()) / scale
        bound = max(MARGIN * e_f32, FLOOR)
        print(f"{shape} {STAGE[stages]}: device error {e_dev:.3e}, float32 restatement {e_f32:.3e}, ratio "
              f"{e_dev / e_f32 if e_f32 > 0 else float('nan'):.2f}, bound {bound:.3e}")
        if not e_dev <= bound:
            fails.append((STAGE[stages], e_dev, e_f32))
        # labels: bit for bit, the mask of the call and the segmentation through cddpm_prep_labels
        assert np.array_equal(got_mask, ref["mask"]), STAGE[stages]
        got_seg = hwd(eng.preprocess_labels(torch.from_numpy(seg).cuda(), stages=stages, target=target, f=f))
        assert np.array_equal(got_seg, ref["seg"]), STAGE[stages]
        if stages == 2:
            assert np.array_equal(got, PR.crop_pad(vol, target))
        if stages & 4:
            assert rec["count"] == ref["info"]["count"]
            assert abs(rec["cut_lo"] - ref["info"]["cut"][0]) <= 1e-6 and abs(rec["cut_hi"] - ref["info"]["cut"][1]) <= 1e-6
    assert not fails, fails
    if f == 1.5:
        assert PR.outside_count(target, f) == 24
        full = device_run(eng, vol, mask, 8, target, f)[0]
        assert int((full == 0).sum()) >= 24 and not full[:, -1, :].any() and full[:, :-1, :].all()


def test_no_stage_is_a_copy_into_the_output_layout(eng):
    vol, mask, seg = raw((13, 10, 7), 3)
    vol[0, 0, 0], vol[1, 2, 3] = -0.0, np.float32(1e-42)          # the copy keeps a negative zero and a denormal
    got, got_mask, rec = device_run(eng, vol, mask, 0, None, 1.0)
    assert got.tobytes() == vol.tobytes() and np.array_equal(got_mask, mask) and rec["status"] == 0


def test_constant_volume_takes_the_zero_branch_bit_for_bit(eng):
    vol = np.full((7, 9, 5), 0.3125, np.float32)
    got, _m, rec = device_run(eng, vol, None, 1, None, 1.0)
    assert got.tobytes() == vol.tobytes() and rec["status"] == 0


def order_case(kind, n, seed):
    """(11, 10, 10) volume whose mask holds n voxels at scattered places"""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (11, 10, 10)
    if kind == "normal":
        vol = rng.standard_normal(shape).astype(np.float32)
    elif kind == "ties":
        vol = (np.floor(rng.random(shape) * 16) / 16 - 0.25).astype(np.float32)
    else:                                                          # negatives and both zeros
        vol = rng.standard_normal(shape).astype(np.float32)
        vol[rng.random(shape) < 0.3] = 0.0
        vol[rng.random(shape) < 0.3] = -0.0
    mask = np.zeros(vol.size, np.uint8)
    mask[rng.permutation(vol.size)[:n]] = 1
    return vol, mask.reshape(shape)


@pytest.mark.parametrize("kind", ["normal", "ties", "zeros"])
def test_order_statistics_are_exact(eng, kind):
    for n in (1, 2, 101, 1000):
        vol, mask = order_case(kind, n, n)
        values = vol[mask > 0]
        assert values.size == n
        for perc in ((0.0, 100.0), (1.0, 99.0), (50.0, 50.0)):
            _got, _m, rec = device_run(eng, vol, mask, 4, None, 1.0, perc)
            want = []
            for p in perc:
                k, k1, _t = PR.ranks(n, p)
                part = np.partition(values, (k, k1))
                want += [float(part[k]), float(part[k1])]
            have = [rec[s] for s in ("stat_lo_k", "stat_lo_k1", "stat_hi_k", "stat_hi_k1")]
            assert rec["count"] == n and have == want, (kind, n, perc, have, want)
            cut = np.percentile(values.astype(np.float64), perc)
            assert abs(rec["cut_lo"] - cut[0]) <= 1e-15 * max(1.0, abs(cut[0])) and abs(rec["cut_hi"] - cut[1]) <= 1e-15 * max(1.0, abs(cut[1]))
            clipped = np.clip(vol.astype(np.float64), cut[0], cut[1])
            assert abs(rec["min"] - clipped.min()) <= 1e-15 and abs(rec["max"] - clipped.max()) <= 1e-15


def test_unchanged_statuses_equal_the_unrescaled_pipeline(eng):
    shape, target, f = (13, 10, 7), (12, 12, 8), 2.0
    vol, _mask, _seg = raw(shape, 5)
    plain = device_run(eng, vol, np.ones(shape, np.uint8), 2 | 8, target, f)[0]
    got, got_mask, rec = device_run(eng, vol, np.zeros(shape, np.uint8), 2 | 4 | 8, target, f)
    assert rec["status"] == P.BAD_MASK | P.UNCHANGED and rec["count"] == 0
    assert np.array_equal(got, plain) and not got_mask.any()
    two = np.where(np.arange(vol.size).reshape(shape) % 3 == 0, np.float32(0.25), np.float32(0.75))
    plain = device_run(eng, two, np.ones(shape, np.uint8), 8, None, f)[0]
    got, _m, rec = device_run(eng, two, np.ones(shape, np.uint8), 4 | 8, None, f, (50.0, 50.0))
    assert rec["status"] == P.BAD_RANGE | P.UNCHANGED and rec["cut_lo"] == rec["cut_hi"] == 0.75 and rec["min"] == rec["max"]
    assert np.array_equal(got, plain)


def test_null_mask_is_vol_above_zero_after_smoothing(eng):
    shape, target, f = (13, 10, 7), (12, 12, 8), 2.0
    vol, _mask, _seg = raw(shape, 6)
    assert (vol <= 0).any()
    a = device_run(eng, vol, None, 2 | 4 | 8, target, f)
    b = device_run(eng, vol, (vol > 0).astype(np.uint8), 2 | 4 | 8, target, f)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    smoothed = device_run(eng, vol, None, 1, None, 1.0)[0]
    a = device_run(eng, vol, None, 15, target, f)
    b = device_run(eng, vol, (smoothed > 0).astype(np.uint8), 15, target, f)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert (a[1] != 0).sum() < a[1].size


def test_the_same_call_twice_and_a_bank_slot(eng):
    shape, cfg = (13, 10, 7), dict(imageDim=(12, 12, 8), rescaleFactor=2, resizedEvaluation=True)
    raws = [raw(shape, 20 + i) for i in range(3)]
    pre = P.VolumePreprocess.from_cfg(cfg, smoothed=False, engine=eng)
    assert pre.stages == 15 and pre.output_shape(shape) == (6, 6, 4)
    singles = [pre.run(v, m) for v, m, _s in raws]
    singles = [{k: (t.clone() if t is not None else None) for k, t in r.items()} for r in singles]
    again = pre.run(raws[1][0], raws[1][1])
    assert torch.equal(again["vol"], singles[1]["vol"]) and torch.equal(again["mask"], singles[1]["mask"])
    assert torch.equal(again["record"], singles[1]["record"])
    bank = A.VolumeBank.from_raw([v for v, _m, _s in raws], [m for _v, m, _s in raws], "cuda", pre)
    assert len(bank) == 3 and bank.shape == (6, 6, 4) and bank.spacing == (2.0, 2.0, 2.0) and bank.data.shape == (3, 4, 6, 6)
    for n in range(3):
        assert torch.equal(bank.data[n], singles[n]["vol"]) and torch.equal(bank.masks[n], singles[n]["mask"])
        assert torch.equal(bank.records[n], singles[n]["record"])
    # the torchio view of __call__, from host arrays and from device tensors
    view = pre(torch.from_numpy(raws[2][0]).cuda(), torch.from_numpy(raws[2][1]).cuda(), raws[2][2])
    assert view["vol"].shape == (1, 6, 6, 4) and torch.equal(view["vol"][0].permute(2, 0, 1), singles[2]["vol"])
    assert view["seg"].dtype == torch.uint8 and view["seg"].shape == (1, 6, 6, 4)
    # from_raw against the bank of the preprocessed volumes, through one loader batch
    by_hand = A.VolumeBank([s["vol"].permute(1, 2, 0).cpu() for s in singles], "cuda", spacing=(2.0, 2.0, 2.0))
    assert torch.equal(by_hand.data, bank.data)
    batches = [next(iter(A.DeviceSliceLoader(b, 3, 4, A.IntensityAugment(), engine=eng)))["vol"]["data"].clone() for b in (bank, by_hand)]
    assert batches[0].shape == (3, 1, 6, 6, 1) and torch.equal(batches[0], batches[1])


def test_refusals_leave_the_outputs_untouched(eng):
    shape, target = (13, 10, 7), (12, 12, 8)
    vol, mask, _seg = raw(shape, 7)
    v, m = torch.from_numpy(vol).cuda(), torch.from_numpy(mask).cuda()
    lib, h = eng.lib, eng._h
    out = torch.full((4, 6, 6), -7.0, device="cuda")
    mout = torch.full((4, 6, 6), 9, dtype=torch.uint8, device="cuda")
    rec = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    need = lib.cddpm_prep_workspace_bytes(13, 10, 7, 15, 12, 12, 8, 2.0)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(vol_p=v.data_ptr(), H=13, stages=15, th=12, lo=1.0, hi=99.0, f=2.0, nbytes=need, out_p=out.data_ptr(), iterations=3, par=True):
        p = (ctypes.c_double * 8)(0.125, 1.0, 1.0, 1.0, lo, hi, f, 0.0)
        return lib.cddpm_prep_volume(h, vol_p, m.data_ptr(), H, 10, 7, stages, iterations, th, 12, 8, ctypes.addressof(p) if par else None,
                                     ws.data_ptr(), nbytes, out_p, mout.data_ptr(), rec.data_ptr(), stream)

    for kw, what in ((dict(vol_p=None), "NULL"), (dict(par=False), "NULL"), (dict(H=0), "outside"), (dict(H=1025), "outside"),
                     (dict(th=1025), "target"), (dict(stages=16), "stage"), (dict(lo=-1.0), "percentiles"), (dict(lo=60.0, hi=40.0), "percentiles"),
                     (dict(hi=100.5), "percentiles"), (dict(f=0.5), "f < 1"), (dict(f=float("nan")), "f < 1"), (dict(iterations=-1), "iterations"),
                     (dict(nbytes=need - 256), "workspace"), (dict(out_p=v.data_ptr()), "equal to input")):
        assert call(**kw) == -1, kw
        assert what in lib.cddpm_last_error(h).decode(), (kw, lib.cddpm_last_error(h).decode())
    flat = torch.zeros(5, 1, 4, device="cuda")
    with pytest.raises(RuntimeError, match="length 1"):
        eng.preprocess_volume(flat, stages=8, f=2.0)
    lab = torch.zeros(13, 10, 7, dtype=torch.uint8, device="cuda")
    assert lib.cddpm_prep_labels(h, lab.data_ptr(), 13, 10, 7, 4, 12, 12, 8, 2.0, mout.data_ptr(), stream) == -1
    assert lib.cddpm_prep_labels(h, lab.data_ptr(), 13, 10, 7, 10, 12, 12, 8, 0.5, mout.data_ptr(), stream) == -1
    assert lib.cddpm_prep_labels(h, None, 13, 10, 7, 10, 12, 12, 8, 2.0, mout.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((mout == 9).all()) and bool((rec == -7.0).all())
    assert bool((v.cpu() == torch.from_numpy(vol)).all())
    # a NaN reaches the device: the status bit stands in the record, no output is written
    for bad in (np.nan, np.inf):
        nv = vol.copy()
        nv[5, 4, 3] = bad
        nvd = torch.from_numpy(nv).cuda()
        assert call(vol_p=nvd.data_ptr()) == 0
        torch.cuda.synchronize()
        assert int(rec[0]) == P.BAD_VALUE and bool((out == -7.0).all()) and bool((mout == 9).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(rec[0]) == 0 and bool((out != -7.0).all()) and bool((mout != 9).all())


def same(a, b):
    """equal, NaN where NaN, lists and tensors element by element"""
    a, b = (x.tolist() if isinstance(x, (torch.Tensor, np.ndarray, np.generic)) else x for x in (a, b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def test_ddpm2d_test_step_reads_an_eval_batch(eng, sd_np):
    """one EvalVolumes batch through DDPM_2D.on_test_start / test_step (synthetic weights, 32 x 32 slices, the geometry of
    test_gpu_augment.py's training-step check) fills eval_dict exactly as the same tensors given by hand do"""
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 8], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=1000,
               noise_ensemble=False, **EC.CFG)

    class Enc(torch.nn.Module):          # stand-in for the context encoder
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous() * 2 - 1

    vol, mask, seg = raw((60, 66, 7), 11)
    pre = P.VolumePreprocess.from_cfg(cfg, smoothed=True, engine=eng)
    items = [dict(vol=vol, mask=mask, seg=(seg > 2), ID=["v0"], label=torch.tensor([1]), Dataset=["Brats21"], stage="val"),
             dict(vol=vol, ID=["v1"], label=torch.tensor([0]), Dataset=["Brats21"], stage="val")]
    ev = P.EvalVolumes(items, "cuda", pre)
    batches = list(ev)
    assert len(ev) == 2 and batches[0]["seg_available"] is True and batches[1]["seg_available"] is False and "seg_orig" not in batches[1]
    b = batches[0]
    assert b["vol"]["data"].shape == (1, 1, 32, 32, 4) and b["vol_orig"]["data"] is b["vol"]["data"]
    assert b["mask_orig"]["data"].shape == (1, 1, 32, 32, 4) and b["mask_orig"]["data"].dtype == torch.float32
    ref = PR.preprocess(vol, mask, (seg > 2), 2 | 4 | 8, (64, 64, 8), PERC, 2.0)
    assert np.array_equal(b["seg_orig"]["data"][0, 0].cpu().numpy(), ref["seg"]) and np.array_equal(b["mask_orig"]["data"][0, 0].cpu().numpy(), ref["mask"])
    hand = {k: ({"data": v["data"].cpu().clone().cuda().contiguous()} if isinstance(v, dict) else v) for k, v in b.items() if k != "record"}
    mod = M.DDPM_2D(cfg, encoder=Enc())
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    mod = mod.cuda()
    try:
        mod.on_test_start()
        outs = []
        for i, batch in enumerate((b, hand)):
            np.random.seed(5); torch.manual_seed(5)
            outs.append(mod.test_step(batch, i))
        assert torch.isfinite(outs[0]["final_volume"]).all() and torch.equal(outs[0]["final_volume"], outs[1]["final_volume"])
        filled = 0
        for k, v in mod.eval_dict.items():
            if isinstance(v, list) and len(v) == 2:
                assert same(v[0], v[1]), (k, v)
                filled += 1
        assert filled > 0
    finally:
        mod.diffusion.model._hip.close()
