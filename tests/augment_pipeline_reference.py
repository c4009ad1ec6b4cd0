"""The eleven slots of the augmentation pipeline restated live in numpy / scipy (no fixtures): the rules of include/cddpm.h, "The
augmentation pipeline". The bias, blur, gamma and ghosting slots and the policy group are tests/augment_reference.py's functions with
the slot's own parameters; new here are the noise (a Philox4x32-10 restated on its own, Box-Muller in float64), the affine (a trilinear
resample padded with the volume's minimum) and the flip. PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO AND SIMPLEITK.
Volumes are in torchio's layout [H, W, D]; axis numbers are torchio's (0 = H, 1 = W, 2 = D).

dtype=np.float64 is the reference, dtype=np.float32 the fair fp32 yardstick (see tests/augment_reference.py). In BOTH variants the
geometry -- source coordinates, the inside test, the trilinear weights -- and the noise's uniforms and normals are computed in
float64: a float32 inside test would flip voxels between the interpolated value and the minimum on its own and loosen the bound by
orders of magnitude. The float32 variant rounds what torchio holds in float32: the volume between stages, the noise tensor, the
interpolation weights and the arithmetic on values."""
import numpy as np

import augment_reference as AR

BIAS, NOISE, GHOST, BLUR, GAMMA, AFFINE, FLIP, POLICY_GAMMA, POLICY_BIAS, POLICY_BLUR, POLICY_GHOST = (1 << k for k in range(11))
SLOTS = tuple(1 << k for k in range(11))
META, PAR, SET, COL_STD, COL_M = 8, 64, 25, 50, 51
NOISE_STREAM = 0x6002


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    mask = np.uint64(0xFFFFFFFF)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def noise_normals(shape, key0, key1):
    """n(v) for every voxel, float64 [H, W, D]: v = (d H + h) W + w, the counter (v / 4, 0, 0, 0x6002), u = ((word >> 9) + 0.5) 2^-23,
    the quad's normals r_a cos, r_a sin, r_b cos, r_b sin"""
    H, W, D = shape
    v = np.arange(H * W * D, dtype=np.int64)
    words = np.stack(philox4x32_10(v // 4, 0, 0, NOISE_STREAM, key0, key1), axis=-1)          # [n, 4]
    u = ((words >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0
    lane = v % 4
    ua, ub = u[v, lane & 2], u[v, (lane & 2) + 1]
    r = np.sqrt(-2.0 * np.log(ua))
    n = r * np.where(lane & 1, np.sin(2.0 * np.pi * ub), np.cos(2.0 * np.pi * ub))
    return n.reshape(D, H, W).transpose(1, 2, 0)


def noise(vol, std, key0, key1, dtype=np.float64):
    """x + std n(v); std = 0 is the identity"""
    x = np.asarray(vol, dtype=dtype)
    if not float(std):
        return x
    return (x + dtype(std) * noise_normals(x.shape, key0, key1).astype(dtype)).astype(dtype)


def source_coords(shape, M):
    """q = c + M (p - c) in float64 for every output voxel p, c = (L - 1) / 2: [H, W, D, 3]. M: nine fp32 values, row-major"""
    M = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(3, 3)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    p = np.stack(np.meshgrid(*[np.arange(L, dtype=np.float64) for L in shape], indexing="ij"), axis=-1) - c
    return c + p @ M.T


def boundary_distance(shape, M):
    """the least distance of a source coordinate from -0.5 or L - 0.5, over all voxels and axes"""
    q = source_coords(shape, M)
    L = np.asarray(shape, dtype=np.float64)
    return float(min(np.abs(q + 0.5).min(), np.abs(q - (L - 0.5)).min()))


def trilinear(vol, q, dtype=np.float64):
    """trilinear interpolation of vol at the points q [..., 3]: floor(q) and floor(q) + 1 clamped to [0, L - 1]; weights in float64,
    rounded to `dtype` with the values"""
    x = np.asarray(vol, dtype=dtype)
    f = np.floor(q)
    t = q - f
    lo = [np.clip(f[..., a], 0, x.shape[a] - 1).astype(np.int64) for a in range(3)]
    hi = [np.clip(f[..., a] + 1, 0, x.shape[a] - 1).astype(np.int64) for a in range(3)]
    w1 = [t[..., a].astype(dtype) for a in range(3)]
    w0 = [(1.0 - t[..., a]).astype(dtype) for a in range(3)]
    out = np.zeros(q.shape[:-1], dtype=dtype)
    for i0, u0 in ((lo[0], w0[0]), (hi[0], w1[0])):
        for i1, u1 in ((lo[1], w0[1]), (hi[1], w1[1])):
            for i2, u2 in ((lo[2], w0[2]), (hi[2], w1[2])):
                out += x[i0, i1, i2] * u0 * u1 * u2
    return out


def affine(vol, M, dtype=np.float64):
    """y(p) = trilinear(x, q(p)) where -0.5 <= q_a <= L_a - 0.5 on all axes, min(x) elsewhere"""
    x = np.asarray(vol, dtype=dtype)
    q = source_coords(x.shape, M)
    L = np.asarray(x.shape, dtype=np.float64)
    inside = ((q >= -0.5) & (q <= L - 0.5)).all(axis=-1)
    return np.where(inside, trilinear(x, q, dtype), x.min()).astype(dtype)


def flip(vol):
    """y[h] = x[H - 1 - h]"""
    return vol[::-1]


def pipeline_slice(vol, meta_row, par_row, dtype=np.float64):
    """slice z of the volume after the slots the row's flags select, in get_augment's order. vol [H, W, D]; meta_row {volume, z, flags,
    slot g | axis << 8, policy g | axis << 8, key0, key1, -}; par_row {slot set [25], policy set [25], std, M[9], -}. Parameters are
    read as the float32 values the table holds."""
    flags = int(meta_row[2])
    g, axis = int(meta_row[3]) & 0xff, int(meta_row[3]) >> 8
    p = np.asarray(par_row, dtype=np.float32)
    x = np.asarray(vol, dtype=dtype)
    if flags & BIAS:
        x = AR.bias(x, p[5:25], dtype)
    if flags & NOISE:
        x = noise(x, p[COL_STD], int(meta_row[5]), int(meta_row[6]), dtype)
    if flags & GHOST:
        x = AR.ghost_fft(x, g, axis, p[4], dtype)
    if flags & BLUR:
        x = AR.blur(x, p[1:4], dtype)
    if flags & GAMMA:
        x = AR.gamma(x, p[0], dtype)
    if flags & AFFINE:
        x = affine(x, p[COL_M:COL_M + 9], dtype)
    if flags & FLIP:
        x = flip(x)
    policy_meta = (meta_row[0], meta_row[1], (flags >> 7) & 15, meta_row[4])
    return AR.augment_slice(x, policy_meta, p[SET:2 * SET], dtype)
