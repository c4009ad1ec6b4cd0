"""CPU: what the device preprocessing rests on. The live numpy / scipy restatement (tests/preprocess_reference.py) against independent
forms -- the resampler against the identity and the half-position rule on spline_filter1d coefficients, the vectorised curvature flow
against a literal per-voxel loop, the crop / pad bounds against hand-written cases, the percentile against np.percentile -- and the host
side of preprocess.py: from_cfg's defaults and refusals, the header against the library's exports, the host arithmetic of
cddpm_prep_workspace_bytes, output sizes and the sample points outside the extent."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import preprocess_reference as PR
from conftest import ROOT, load_pkg

P = load_pkg("preprocess")


@pytest.mark.parametrize("shape", [(9, 8, 6), (3, 2, 5), (13, 10, 7)])
def test_resampler_at_integer_positions_is_the_identity(shape):
    rng = np.random.Generator(np.random.PCG64(sum(shape)))
    vol = rng.random(shape) - 0.02
    back = PR.sample_bspline(vol, [np.arange(N, dtype=np.float64) for N in shape])
    err = float(np.abs(back - vol).max())
    print(f"{shape}: max |spline(i) - v[i]| = {err:.2e}")
    assert err < 1e-13                                   # float64 rounding of three recursions and 64 taps on values below 1
    assert PR.resample_image(vol, 1.0) is not None and np.array_equal(PR.resample_image(vol, 1.0), vol)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_resampler_at_half_positions_equals_the_four_coefficient_rule(axis):
    """B3(1.5) = 1/48, B3(0.5) = 23/48: the spline at i + 1/2 is (c[i-1] + 23 c[i] + 23 c[i+1] + c[i+2]) / 48 on the line's coefficients"""
    shape = (9, 8, 7)
    rng = np.random.Generator(np.random.PCG64(axis))
    vol = rng.random(shape) - 0.02
    xs = [np.arange(N, dtype=np.float64) for N in shape]
    i = np.arange(1, shape[axis] - 2)
    xs[axis] = i + 0.5
    got = PR.sample_bspline(vol, xs)
    c = np.moveaxis(ndimage.spline_filter1d(vol, order=3, axis=axis, mode="mirror"), axis, 0)
    want = np.moveaxis((c[i - 1] + 23.0 * c[i] + 23.0 * c[i + 1] + c[i + 2]) / 48.0, 0, axis)
    err = float(np.abs(got - want).max())
    print(f"axis {axis}: max |spline(i + 1/2) - rule| = {err:.2e}")
    assert err < 1e-13


@pytest.mark.parametrize("shape", [(5, 4, 3), (2, 3, 5)])
def test_curvature_flow_equals_the_per_voxel_loop(shape):
    rng = np.random.Generator(np.random.PCG64(sum(shape)))
    vol = rng.random(shape) - 0.02
    for spacing in ((1.0, 1.0, 1.0), (1.0, 0.5, 2.0)):
        err = float(np.abs(PR.curvature_flow(vol, spacing=spacing) - PR.curvature_flow_loop(vol, spacing=spacing)).max())
        print(f"{shape} spacing {spacing}: max |vectorised - loop| = {err:.2e}")
        assert err < 1e-14
    assert np.array_equal(PR.curvature_flow(np.full(shape, 0.25)), np.full(shape, 0.25))        # the m < 1e-9 branch
    v32 = PR.curvature_flow(vol.astype(np.float32), dtype=np.float32)
    assert v32.dtype == np.float32 and 0 < np.abs(v32 - PR.curvature_flow(vol.astype(np.float32))).max() < 1e-6
    _v, smallest, near = PR.curvature_flow(vol, condition=True)
    assert smallest > 1e-8 and near == 0


def test_crop_pad_bounds_by_hand():
    assert PR.crop_pad_bounds(10, 13) == (2, 1)          # odd padding: ceil in front
    assert PR.crop_pad_bounds(10, 14) == (2, 2)
    assert PR.crop_pad_bounds(13, 10) == (-2, -1)        # odd crop: ceil removed in front
    assert PR.crop_pad_bounds(12, 8) == (-2, -2)
    assert PR.crop_pad_bounds(7, 7) == (0, 0)
    vol = np.arange(1, 1 + 5 * 4 * 3, dtype=np.float32).reshape(5, 4, 3)
    out = PR.crop_pad(vol, (2, 7, 3))                    # crop on one axis while another pads
    assert out.shape == (2, 7, 3)
    assert np.array_equal(out[:, 2:6, :], vol[2:4]) and not out[:, :2].any() and not out[:, 6:].any()
    line = np.arange(1, 8).reshape(7, 1, 1)
    assert PR.crop_pad(line, (4, 1, 1)).reshape(-1).tolist() == [3, 4, 5, 6]
    assert PR.crop_pad(line, (10, 1, 1)).reshape(-1).tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 0]


@pytest.mark.parametrize("n", [1, 2, 101])
def test_percentile_matches_numpy(n):
    rng = np.random.Generator(np.random.PCG64(n))
    x = rng.standard_normal(n)
    for p in (0, 1, 5, 33.3, 50, 99, 100):
        assert abs(PR.percentile(x, p) - np.percentile(x, p)) <= 1e-15 * max(1.0, abs(np.percentile(x, p))), (n, p)
    k, k1, t = PR.ranks(n, 50)
    assert 0 <= k <= k1 <= n - 1 and 0 <= t < 1


def test_rescale_statuses_and_the_affine_map():
    rng = np.random.Generator(np.random.PCG64(4))
    vol = rng.random((6, 5, 4)) - 0.02
    out, info = PR.rescale(vol, vol > 0.1, 1, 99)
    assert info["status"] == 0 and out.min() == 0.0 and out.max() == 1.0
    same, info = PR.rescale(vol, np.zeros_like(vol), 1, 99)
    assert info["status"] == PR.BAD_MASK | PR.UNCHANGED and np.array_equal(same, vol)
    two = np.where(np.arange(120).reshape(6, 5, 4) % 3 == 0, 0.25, 0.75)
    same, info = PR.rescale(two, np.ones_like(two), 50, 50)
    assert info["status"] == PR.BAD_RANGE | PR.UNCHANGED and np.array_equal(same, two)


def test_output_sizes_and_points_outside_the_extent():
    assert [PR.output_size(N, 2.0) for N in (12, 13, 7, 1)] == [6, 7, 4, 1]
    assert [PR.output_size(N, 1.5) for N in (9, 8, 6)] == [6, 6, 4]
    assert [PR.output_size(N, 3.0) for N in (6, 160, 192)] == [2, 54, 64]
    assert PR.outside_count((9, 8, 6), 1.5) == 24        # the last index along W samples 7.75 >= 7.5
    assert PR.outside_count((12, 12, 8), 2.0) == 0 and PR.outside_count((6, 6, 6), 3.0) == 0
    E = load_pkg("engine").CddpmEngine
    for shape, stages, target, f in (((13, 10, 7), 15, (12, 12, 8), 2.0), ((9, 8, 6), 8, None, 1.5), ((9, 8, 6), 2, (3, 20, 6), 1.5),
                                      ((9, 8, 6), 4, (3, 3, 3), 2.0), ((192, 192, 100), 10, (192, 192, 100), 2.0)):
        after = target if stages & 2 else shape
        want = tuple(PR.output_size(N, f) for N in after) if stages & 8 else tuple(after)
        assert E.prep_output_shape(shape, stages, target, f) == want
    labels = (np.arange(9 * 8 * 6).reshape(9, 8, 6) % 5).astype(np.uint8)
    out = PR.resample_labels(labels, 1.5)
    assert out.shape == (6, 6, 4) and not out[:, -1, :].any() and out[0, 0, 0] == labels[0, 0, 0] and out[1, 1, 1] == labels[2, 2, 2]
    with pytest.raises(ValueError, match="length 1"):
        PR.resample_image(np.zeros((4, 1, 4)), 2.0)


def test_from_cfg_defaults_and_refusals():
    pre = P.VolumePreprocess.from_cfg({"resizedEvaluation": True}, smoothed=False)
    assert pre.stages == 15 and pre.target == (160, 192, 160) and pre.perc == (1.0, 99.0) and pre.factor == 3.0
    assert pre.dt == 0.125 and pre.iterations == 3 and pre.output_shape((170, 180, 150)) == (54, 64, 54)
    pre = P.VolumePreprocess.from_cfg(dict(resizedEvaluation=True, imageDim=[192, 192, 100], rescaleFactor=2, perc_low=2, perc_high=98,
                                           unisotropic_sampling=False), smoothed=True)
    assert pre.stages == P.RESCALE | P.RESAMPLE and pre.perc == (2.0, 98.0) and pre.factor == 2.0
    assert pre.output_shape((160, 192, 160)) == (80, 96, 80)
    with pytest.raises(NotImplementedError, match="resizedEvaluation"):
        P.VolumePreprocess.from_cfg({"resizedEvaluation": False}, smoothed=True)
    with pytest.raises(KeyError, match="resizedEvaluation"):
        P.VolumePreprocess.from_cfg({}, smoothed=True)
    with pytest.raises(TypeError):
        P.VolumePreprocess.from_cfg({"resizedEvaluation": True})              # `smoothed` has no default
    for kw in (dict(perc=(60, 40)), dict(perc=(-1, 99)), dict(factor=0.5), dict(stages=16)):
        with pytest.raises(ValueError):
            P.VolumePreprocess(**{"stages": 15, "target": (4, 4, 4), **kw})
    with pytest.raises(ValueError, match="target"):
        P.VolumePreprocess(P.CROPPAD)


def test_workspace_bytes_host_arithmetic():
    lib = load_pkg("_lib").load_library()
    n0, n1 = 160 * 192 * 160, 192 * 192 * 100
    small = lib.cddpm_prep_workspace_bytes(160, 192, 160, 2, 192, 192, 100, 1.0)
    assert 0 < small <= 1 << 20                           # state words and tap tables alone
    flow = lib.cddpm_prep_workspace_bytes(160, 192, 160, 1, 0, 0, 0, 1.0)
    assert flow - small in range(2 * 4 * n0, 2 * 4 * n0 + 1024)                  # two fp32 work volumes
    full = lib.cddpm_prep_workspace_bytes(160, 192, 160, 15, 192, 192, 100, 2.0)
    assert full - flow in range(8 * n1, 8 * n1 + 1024)                           # one float64 coefficient volume
    assert lib.cddpm_prep_workspace_bytes(160, 192, 160, 15, 192, 192, 100, 1.0) == flow       # f = 1 skips the stage
    for bad in ((0, 8, 8, 0, 0, 0, 0, 1.0), (8, 1025, 8, 0, 0, 0, 0, 1.0), (8, 8, 8, 2, 8, 0, 8, 1.0), (8, 8, 8, 2, 8, 8, 1025, 1.0),
                (8, 8, 8, 16, 8, 8, 8, 1.0), (8, 8, 8, 8, 0, 0, 0, 0.5), (8, 1, 8, 8, 0, 0, 0, 2.0), (8, 8, 8, 10, 8, 8, 1, 2.0)):
        assert lib.cddpm_prep_workspace_bytes(*bad) == 0, bad
        assert "cddpm_prep_workspace_bytes" in lib.cddpm_last_error(None).decode()
    assert lib.cddpm_prep_workspace_bytes(8, 1, 8, 8, 0, 0, 0, 1.0) > 0           # an axis of length 1 is fine where nothing resamples


def test_header_declares_what_the_library_exports():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    declared = set(re.findall(r"\b(cddpm_[a-z0-9_]+)\s*\(", header)) - {"cddpm_ctx"}
    new = {"cddpm_prep_workspace_bytes", "cddpm_prep_volume", "cddpm_prep_labels"}
    assert new <= declared and new <= set(lib_mod.SYMBOLS)
    lib = lib_mod.load_library()
    for name in new:
        assert getattr(lib, name) is not None
    E = load_pkg("engine").CddpmEngine
    for name, val in (("CDDPM_PREP_SMOOTH", P.SMOOTH), ("CDDPM_PREP_CROPPAD", P.CROPPAD), ("CDDPM_PREP_RESCALE", P.RESCALE),
                      ("CDDPM_PREP_RESAMPLE", P.RESAMPLE), ("CDDPM_PREP_ALL", E.PREP_ALL), ("CDDPM_PREP_RECORD", E.PREP_RECORD),
                      ("CDDPM_PREP_BAD_VALUE", P.BAD_VALUE), ("CDDPM_PREP_BAD_MASK", P.BAD_MASK), ("CDDPM_PREP_BAD_RANGE", P.BAD_RANGE),
                      ("CDDPM_PREP_UNCHANGED", P.UNCHANGED), ("CDDPM_PREP_MAX_AXIS", 1024), ("CDDPM_PREP_PAR", 8)):
        assert re.search(rf"#define {name} {int(val)}\b", header), name
    assert (P.SMOOTH, P.CROPPAD, P.RESCALE, P.RESAMPLE) == (PR.SMOOTH, PR.CROPPAD, PR.RESCALE, PR.RESAMPLE)
    for i, slot in enumerate(("STATUS", "COUNT", "STAT", None, None, None, "CUT_LO", "CUT_HI", "MIN", "MAX")):
        if slot:
            assert re.search(rf"#define CDDPM_PREP_REC_{slot} {i}\b", header), slot
    assert len(P.RECORD_SLOTS) == 10
