"""The preprocessing of a raw volume -- sitk_reader's CurvatureFlow and get_transform's CropOrPad, RescaleIntensity and Resample of the
reference's datamodule (src/datamodules/create_dataset.py:252-258, :196-218) -- restated live in numpy / scipy (no fixtures): the rules of
include/cddpm.h, "Preprocessed volumes", as torchio >=0.18.90,<0.19 and ITK are recalled -- neither is available to compare with (PINNED TO
NUMPY / SCIPY, UNPINNED TO TORCHIO AND SIMPLEITK). Volumes are in torchio's layout [H, W, D]; axis numbers are torchio's (0 = H, 1 = W,
2 = D).

dtype=np.float64 is the reference. dtype=np.float32 is the fair fp32 yardstick, the same rules with the reference's own float32 stores: the
curvature flow evaluates its update in double and stores the volume as float32 after every iteration (as ITK does on a float image), the
rescale runs on float32 arrays, and the resampler holds its B-spline coefficients in float64 (as scipy and ITK do) and stores a float32
result. Its distance from the float64 form is the error an fp32 implementation of the same rules makes; the device is held to a multiple
of it."""
import math

import numpy as np
from scipy import ndimage

SMOOTH, CROPPAD, RESCALE, RESAMPLE = 1, 2, 4, 8
BAD_VALUE, BAD_MASK, BAD_RANGE, UNCHANGED = 1, 2, 4, 8


# ---- 1. curvature flow ----------------------------------------------------------------------------------------------------------------
def _speed(v, spacing):
    """u and m = |grad|^2 of a float64 volume: central differences, neighbours clamped to the edge"""
    s = [1.0 / float(x) for x in spacing]
    p = np.pad(v, 1, mode="edge")
    c = (slice(1, -1),) * 3

    def sh(*off):
        return p[tuple(slice(1 + o, p.shape[a] - 1 + o) for a, o in enumerate(off))]

    def e(axis, k):
        off = [0, 0, 0]
        off[axis] = k
        return off

    dx, dxx = [], []
    for i in range(3):
        plus, minus = sh(*e(i, 1)), sh(*e(i, -1))
        dx.append(0.5 * (plus - minus) * s[i])
        dxx.append((plus - 2.0 * p[c] + minus) * s[i] * s[i])
    dxy = {}
    for i in range(3):
        for j in range(i + 1, 3):
            def o(a, b):
                off = [0, 0, 0]
                off[i], off[j] = a, b
                return sh(*off)
            dxy[i, j] = 0.25 * (o(1, 1) - o(1, -1) - o(-1, 1) + o(-1, -1)) * s[i] * s[j]
    q = [d * d for d in dx]
    m = q[0] + q[1] + q[2]
    num = (dxx[0] * (q[1] + q[2]) + dxx[1] * (q[0] + q[2]) + dxx[2] * (q[0] + q[1])
           - 2.0 * (dx[0] * dx[1] * dxy[0, 1] + dx[0] * dx[2] * dxy[0, 2] + dx[1] * dx[2] * dxy[1, 2]))
    zero = m < 1e-9
    u = np.where(zero, 0.0, num / np.where(zero, 1.0, m))
    return u, m


def curvature_flow(vol, dt=0.125, iterations=3, spacing=(1.0, 1.0, 1.0), dtype=np.float64, condition=False):
    """sitk.CurvatureFlow(timeStep=dt, numberOfIterations=iterations): per iteration v <- v + dt u, stored as `dtype`. condition=True
    returns (v, smallest non-zero m met, number of voxel-iterations with 1e-10 <= m < 1e-8): how far the inputs stay from the m < 1e-9
    branch, which a rounding difference must not be able to flip"""
    v = np.asarray(vol, dtype=dtype)
    smallest, near = np.inf, 0
    for _ in range(int(iterations)):
        u, m = _speed(v.astype(np.float64), spacing)
        v = (v.astype(np.float64) + float(dt) * u).astype(dtype)
        if (m > 0).any():
            smallest = min(smallest, float(m[m > 0].min()))
        near += int(((m >= 1e-10) & (m < 1e-8)).sum())
    return (v, smallest, near) if condition else v


def curvature_flow_loop(vol, dt=0.125, iterations=3, spacing=(1.0, 1.0, 1.0)):
    """the same rule, voxel by voxel in float64: the literal form the vectorised one is tied to"""
    v = np.asarray(vol, dtype=np.float64).copy()
    H, W, D = v.shape
    s = [1.0 / float(x) for x in spacing]
    n = (H, W, D)
    for _ in range(int(iterations)):
        out = np.empty_like(v)
        for h in range(H):
            for w in range(W):
                for d in range(D):
                    pos = (h, w, d)

                    def at(*off):
                        return v[tuple(min(max(pos[a] + off[a], 0), n[a] - 1) for a in range(3))]

                    def unit(i, k, j=None, l=0):
                        off = [0, 0, 0]
                        off[i] = k
                        if j is not None:
                            off[j] = l
                        return at(*off)

                    dx = [0.5 * (unit(i, 1) - unit(i, -1)) * s[i] for i in range(3)]
                    dxx = [(unit(i, 1) - 2.0 * v[pos] + unit(i, -1)) * s[i] ** 2 for i in range(3)]
                    m = sum(x * x for x in dx)
                    if m < 1e-9:
                        out[pos] = v[pos]
                        continue
                    num = sum(dxx[i] * sum(dx[j] ** 2 for j in range(3) if j != i) for i in range(3))
                    for i in range(3):
                        for j in range(i + 1, 3):
                            dxy = 0.25 * (unit(i, 1, j, 1) - unit(i, 1, j, -1) - unit(i, -1, j, 1) + unit(i, -1, j, -1)) * s[i] * s[j]
                            num -= 2.0 * dx[i] * dx[j] * dxy
                    out[pos] = v[pos] + dt * num / m
        v = out
    return v


# ---- 2. crop or pad -------------------------------------------------------------------------------------------------------------------
def crop_pad_bounds(size, target):
    """-> (front, back): voxels added (positive) or removed (negative) in front of and behind one axis"""
    delta = int(target) - int(size)
    front, back = math.ceil(abs(delta) / 2), math.floor(abs(delta) / 2)
    return (front, back) if delta >= 0 else (-front, -back)


def crop_pad(vol, target):
    """tio.CropOrPad(target, padding_mode=0)"""
    out = np.asarray(vol)
    for axis, t in enumerate(target):
        front, back = crop_pad_bounds(out.shape[axis], t)
        if front < 0 or back < 0:
            index = [slice(None)] * 3
            index[axis] = slice(-front, out.shape[axis] + back)
            out = out[tuple(index)]
        else:
            pad = [(0, 0)] * 3
            pad[axis] = (front, back)
            out = np.pad(out, pad, mode="constant", constant_values=0)
    return np.ascontiguousarray(out)


# ---- 3. rescale -----------------------------------------------------------------------------------------------------------------------
def ranks(n, p):
    """the two order statistics of percentile p among n values and the fraction between them: v = p (n - 1) / 100"""
    v = float(p) * float(n - 1) / 100.0
    k = min(int(math.floor(v)), n - 1)
    return k, min(k + 1, n - 1), v - k


def percentile(values, p):
    """np.percentile(values, p) (linear) stated on order statistics, in the dtype of `values`"""
    values = np.asarray(values).reshape(-1)
    k, k1, t = ranks(values.size, p)
    part = np.partition(values, (k, k1))
    a, b = part[k], part[k1]
    t = values.dtype.type(t)
    return b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t


def rescale(vol, mask, lo, hi, dtype=np.float64):
    """tio.RescaleIntensity((0, 1), percentiles=(lo, hi), masking_method=mask) -> (volume, info). info: status, count, the four order
    statistics, the cutoffs, min and max of the clipped volume"""
    x = np.asarray(vol, dtype=dtype)
    values = x[np.asarray(mask) > 0]
    info = dict(status=0, count=int(values.size), stats=[0.0] * 4, cut=(0.0, 0.0), min=float(x.min()), max=float(x.max()))
    if values.size == 0:
        info["status"] = BAD_MASK | UNCHANGED
        return x, info
    stats = []
    for p in (lo, hi):
        k, k1, _ = ranks(values.size, p)
        part = np.partition(values, (k, k1))
        stats += [float(part[k]), float(part[k1])]
    cut = (percentile(values, lo), percentile(values, hi))
    y = np.clip(x, dtype(cut[0]), dtype(cut[1]))
    mn, mx = y.min(), y.max()
    info.update(stats=stats, cut=(float(cut[0]), float(cut[1])), min=float(mn), max=float(mx))
    if mx == mn:
        info["status"] = BAD_RANGE | UNCHANGED
        return x, info
    return ((y - mn) / (mx - mn)).astype(dtype), info


# ---- 4. resample ----------------------------------------------------------------------------------------------------------------------
def output_size(N, f):
    return int(math.ceil(N / float(f)))


def sample_points(N, f):
    """-> (x, inside): the input coordinate of every output voxel of one axis, and whether it lies in [-1/2, N - 1/2)"""
    x = (np.arange(output_size(N, f), dtype=np.float64) + 0.5) * float(f) - 0.5
    return x, (x >= -0.5) & (x < N - 0.5)


def outside_count(shape, f):
    """how many output voxels sample outside the input's extent"""
    inside = [sample_points(N, f)[1] for N in shape]
    grid = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    return int((~grid).sum())


def sample_bspline(vol, xs, dtype=np.float64):
    """the cubic B-spline of `vol` (mirror boundaries, scipy's prefilter, float64 coefficients) at the outer product of the three
    coordinate lists `xs`, stored as `dtype`"""
    grid = np.meshgrid(*xs, indexing="ij")
    return ndimage.map_coordinates(np.asarray(vol, dtype=dtype), grid, output=dtype, order=3, mode="mirror", prefilter=True)


def resample_image(vol, f, dtype=np.float64):
    """tio.Resample(f, image_interpolation='bspline') of an image at spacing 1; outside the extent: 0"""
    vol = np.asarray(vol, dtype=dtype)
    if float(f) == 1.0:
        return vol
    if min(vol.shape) == 1:
        raise ValueError("an axis of length 1 is not resampled with f != 1")
    pts = [sample_points(N, f) for N in vol.shape]
    out = sample_bspline(vol, [x for x, _ in pts], dtype)
    inside = pts[0][1][:, None, None] & pts[1][1][None, :, None] & pts[2][1][None, None, :]
    return np.where(inside, out, dtype(0))


def resample_labels(lab, f):
    """tio.Resample(f) of a label map: the nearest voxel floor(x + 1/2); outside the extent: 0"""
    lab = np.asarray(lab)
    if float(f) == 1.0:
        return lab
    if min(lab.shape) == 1:
        raise ValueError("an axis of length 1 is not resampled with f != 1")
    pts = [sample_points(N, f) for N in lab.shape]
    idx = [np.clip(np.floor(x + 0.5).astype(np.int64), 0, N - 1) for (x, _), N in zip(pts, lab.shape)]
    out = lab[np.ix_(*idx)]
    inside = pts[0][1][:, None, None] & pts[1][1][None, :, None] & pts[2][1][None, None, :]
    return np.where(inside, out, 0).astype(lab.dtype)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
def preprocess(vol, mask=None, seg=None, stages=15, target=None, perc=(1.0, 99.0), f=1.0, dt=0.125, iterations=3,
               spacing=(1.0, 1.0, 1.0), dtype=np.float64):
    """-> dict(vol, mask, seg, info) in torchio's layout [H', W', D']; mask None: vol > 0 after the smoothing"""
    v = np.asarray(vol, dtype=dtype)
    if stages & SMOOTH:
        v = curvature_flow(v, dt, iterations, spacing, dtype)
    m = (v > 0).astype(np.uint8) if mask is None else np.asarray(mask).astype(np.uint8)
    s = None if seg is None else np.asarray(seg).astype(np.uint8)
    if stages & CROPPAD:
        v, m = crop_pad(v, target), crop_pad(m, target)
        s = None if s is None else crop_pad(s, target)
    info = dict(status=0, count=0, stats=[0.0] * 4, cut=(0.0, 0.0), min=0.0, max=0.0)
    if stages & RESCALE:
        v, info = rescale(v, m, perc[0], perc[1], dtype)
    if stages & RESAMPLE:
        v, m = resample_image(v, f, dtype), resample_labels(m, f)
        s = None if s is None else resample_labels(s, f)
    return dict(vol=np.ascontiguousarray(v), mask=m, seg=s, info=info)
