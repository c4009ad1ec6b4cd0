"""The four intensity augmentations of the training datamodule and the slice extraction, restated live in numpy / scipy (no fixtures):
the rules of include/cddpm.h, "Augmented training slices", as torchio 0.18.9x's RandomGamma, RandomBiasField, RandomBlur and
RandomGhosting are recalled -- torchio itself is not available to compare with (PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO).
Volumes are in torchio's layout [H, W, D]; axis numbers are torchio's (0 = H, 1 = W, 2 = D).

dtype=np.float64 is the reference. dtype=np.float32 is the fair fp32 yardstick: what torchio computes on its float32 tensors -- every
intermediate volume is stored as float32, numpy's power and scipy's filter run on float32 arrays, and the bias field and the Fourier
transform, which torchio evaluates in double, are rounded to float32 where torchio rounds them. Its distance from the float64 form is the
error an fp32 implementation of the same rules makes; the device is held to a multiple of it.

The ghosting is stated twice: `ghost_fft`, the literal rule on the fft-shifted 3-D spectrum, and `ghost_comb`, the circular convolution
along the axis that the device evaluates; tests/test_augment_host.py ties the two."""
import numpy as np
from scipy import ndimage

GAMMA, BIAS, BLUR, GHOST = 1, 2, 4, 8


def gamma(vol, g, dtype=np.float64):
    """sign(x) |x|^gamma"""
    x = np.asarray(vol, dtype=dtype)
    return (np.sign(x) * np.abs(x) ** dtype(g)).astype(dtype)


def bias_coords(L):
    """u(i) = (2 i - L + 1) / (L - 1), 0 where L = 1"""
    if L == 1:
        return np.zeros(1)
    return (2.0 * np.arange(L) - L + 1.0) / (L - 1.0)


def bias_coords_meshgrid(shape):
    """torchio's form: arange(-L/2, L/2) + 0.5 per axis, np.meshgrid, each mesh divided by its maximum where that is positive, and the
    transpose(1, 0, 2) its maps get -> the three coordinate volumes X, Y, Z of shape `shape`"""
    ranges = [np.arange(-n, n) + 0.5 for n in np.array(shape) / 2]
    meshes = np.asarray(np.meshgrid(*ranges))
    for mesh in meshes:
        m = mesh.max()
        if m > 0:
            mesh[:] = mesh / m
    return [np.transpose(m, (1, 0, 2)) for m in meshes]


def bias_field(shape, coef):
    """exp(sum_i c_i X^a Y^b Z^c) in float64, i counting a in 0..3, b in 0..3-a, c in 0..3-a-b"""
    X, Y, Z = np.meshgrid(*[bias_coords(L) for L in shape], indexing="ij")
    field = np.zeros(shape)
    i = 0
    for a in range(4):
        for b in range(4 - a):
            for c in range(4 - a - b):
                field += float(coef[i]) * X ** a * Y ** b * Z ** c
                i += 1
    assert i == 20
    return np.exp(field)


def bias(vol, coef, dtype=np.float64):
    x = np.asarray(vol, dtype=dtype)
    return (x * bias_field(x.shape, coef).astype(dtype)).astype(dtype)      # torchio rounds the field to float32, then multiplies


def blur(vol, sigmas, dtype=np.float64):
    """scipy.ndimage.gaussian_filter with its defaults (reflect, truncate 4, axes with sigma <= 1e-15 skipped) on an array of `dtype`:
    on float32 scipy sums each line in double and stores float32 between the passes"""
    return ndimage.gaussian_filter(np.asarray(vol, dtype=dtype), [float(s) for s in sigmas])


def reflect_index(i, L):
    """scipy's `reflect` (d c b a | a b c d | d c b a) as repeated reflection"""
    m = np.mod(i, 2 * L)
    return np.where(m >= L, 2 * L - 1 - m, m)


def gaussian_weights(sigma):
    r = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * k ** 2)
    return r, w / w.sum()


def ghost_fft(vol, g, axis, intensity, dtype=np.float64):
    """the literal rule: scale the planes s = 0, g, 2 g, ... of the fft-shifted spectrum along `axis` by 1 - I, restore the plane
    s = L // 2, invert, keep the real part. The transform runs in double (as numpy's did under torchio 0.18.9x); the result is `dtype`."""
    x = np.asarray(vol, dtype=dtype)
    if not g or not intensity:
        return x
    spectrum = np.fft.fftshift(np.fft.fftn(x.astype(np.float64)))
    sl = [slice(None)] * 3
    mid = list(sl)
    mid[axis] = x.shape[axis] // 2
    restore = spectrum[tuple(mid)].copy()
    sl[axis] = slice(None, None, int(g))
    spectrum[tuple(sl)] *= 1.0 - float(intensity)
    spectrum[tuple(mid)] = restore
    return np.fft.ifftn(np.fft.ifftshift(spectrum)).real.astype(dtype)


def comb_kernel(L, g):
    """c[d] = (1 / L) sum over s = 0, g, 2 g, ... < L, s != L // 2 of cos(2 pi (s - L // 2) d / L), the argument reduced in integers"""
    d = np.arange(L)
    c = np.zeros(L)
    for s in range(0, L, int(g)):
        if s != L // 2:
            c += np.cos(2.0 * np.pi * (((s - L // 2) * d) % L) / L)
    return c / L


def ghost_comb(vol, g, axis, intensity):
    """y = x - I (c (*) x): the circular convolution along `axis`, float64"""
    x = np.asarray(vol, dtype=np.float64)
    if not g or not intensity:
        return x
    L = x.shape[axis]
    c = comb_kernel(L, g)
    idx = (np.arange(L)[:, None] - np.arange(L)[None, :]) % L          # [i, j] -> (i - j) mod L
    conv = np.moveaxis(np.tensordot(c[idx], np.moveaxis(x, axis, 0), axes=(1, 0)), 0, axis)
    return x - float(intensity) * conv


def augment_slice(vol, meta_row, par_row, dtype=np.float64):
    """slice z of the volume after the stages the row's flags select, in Compose's order. vol [H, W, D]; meta_row {volume, z, flags,
    g | axis << 8}; par_row {gamma, sigma0, sigma1, sigma2, I, c[20], ...} (the sigmas in voxels). Parameters are read as the float32
    values the table holds."""
    z, flags, g, axis = int(meta_row[1]), int(meta_row[2]), int(meta_row[3]) & 0xff, int(meta_row[3]) >> 8
    p = np.asarray(par_row, dtype=np.float32)
    x = np.asarray(vol, dtype=dtype)
    if flags & GAMMA:
        x = gamma(x, p[0], dtype)
    if flags & BIAS:
        x = bias(x, p[5:25], dtype)
    if flags & BLUR:
        x = blur(x, p[1:4], dtype)
    if flags & GHOST:
        x = ghost_fft(x, g, axis, p[4], dtype)
    return np.ascontiguousarray(x[:, :, z])
