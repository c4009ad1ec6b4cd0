"""Inputs for the evaluation-metric kernels (csrc/eval_metrics.hip) beyond the 96 x 96 x 4 geometry of tests/eval_cases.py,
shared by tests/test_metrics_oracle_host.py (which asserts the conditions each case is chosen for) and
tests/test_gpu_eval_metrics_shapes.py (which compares the device with oracle/metrics_oracle.py). Everything is regenerated
from numpy PCG64 seeds; nothing is stored.

Shapes are (R, D1, D2): R rows of C = D1 * D2 voxels. The kernels take a row in steps of 256 voxels, the rows in steps of
256, the distinct curve points in steps of 65 536 and everything else in steps of 4096 * 256 = 1 048 576 items."""
import itertools
from collections import deque

import numpy as np

EB = 256                      # block size of the wide kernels
CURVE_STRIDE = 256 * EB       # distinct points per round of the curve kernels
GRID_STRIDE = 4096 * EB       # items per round of the grid-stride kernels

SMALL = [(70, 9, 1),          # C = 9 < 256; D2 = 1
         (3, 64, 4),          # C = 256 exactly
         (3, 257, 1),         # C = 257
         (1, 40, 37),         # R = 1: 2-D labelling, a row curve over one item
         (33, 19, 4),         # everything odd
         (300, 5, 4)]         # R > 256: second round over the rows; a 300-point row curve
MID = (20, 64, 64)            # 81 920 > 65 536: second round of the curve loops
BIG = (65, 128, 128)          # 1 064 960 > 1 048 576: second round of every grid-stride loop

REGIMES = ("continuous", "quantised", "constant", "zero", "nolesion", "alllesion", "rowmask", "nomask")


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _lesion(shape):
    """a box of lesion in the middle rows, so that (for R > 2) there are rows with and rows without lesion"""
    R, D1, D2 = shape
    seg = np.zeros(shape, np.float32)
    r0, r1 = (0, 1) if R == 1 else (R // 3, R // 3 + max(1, R // 4))
    seg[r0:r1, D1 // 4:D1 // 4 + max(1, D1 // 2), :] = 2.0          # raw labels: binarised as > 0 inside
    if R > EB:
        seg[R - 20:R - 10, 0:max(1, D1 // 2), :] = 1.0              # and some among the rows beyond the first 256
    return seg


def volume(shape, regime, seed):
    """dict of float32 [R, D1, D2] arrays recon, orig, seg, mask, diff. `diff` is the score map the metrics read: the entry
    point takes it apart from recon / orig (it is post-processed in the evaluation step), so each regime shapes it freely."""
    assert regime in REGIMES
    R, D1, D2 = shape
    rng = _rng(seed, R, D1, D2)
    orig = rng.random(shape, dtype=np.float32)
    seg = _lesion(shape)
    if regime == "nolesion":
        seg[:] = 0
    if regime == "alllesion":
        seg[:] = 1
    mask = np.ones(shape, np.float32)
    mask[:, 0, :] = 0
    if regime == "rowmask" and R > 1:
        mask[1::3] = 0                                              # rows without mask, among them rows with lesion
    if regime == "nomask":
        mask[:] = 0
    les = (seg > 0).astype(np.float64)
    recon = orig + np.float32(0.05) * rng.standard_normal(shape).astype(np.float32) \
        - (0.35 * les * rng.random(shape)).astype(np.float32)
    # log-uniform over 12 binades (few fp32 collisions, so nearly every voxel is a distinct curve point) and a lesion that
    # raises the scores, as in eval_cases.volume
    c = 0.2 * np.exp2(-12.0 * rng.random(shape)) + 0.35 * les * rng.random(shape)
    if regime == "quantised":
        diff = np.round(c * 128.0) / 32.0                           # k / 32: heavy ties, a few dozen distinct points
    elif regime == "constant":
        diff = np.full(shape, 0.5)
    elif regime == "zero":
        diff = np.zeros(shape)
    else:
        diff = c
    return dict(recon=recon.astype(np.float32), orig=orig, seg=seg, mask=mask, diff=diff.astype(np.float32))


# (shape, regime, seed) of the score cases, in an order that takes n up, down and up again through one workspace
SCORE_CASES = [(s, g, 100 + 10 * i + j) for i, s in enumerate(SMALL[:3]) for j, g in enumerate(REGIMES)] \
    + [(MID, "continuous", 301), (MID, "quantised", 302)] \
    + [(s, g, 400 + 10 * i + j) for i, s in enumerate(SMALL[3:]) for j, g in enumerate(REGIMES)] \
    + [(BIG, "continuous", 501)]


# ---- sets ------------------------------------------------------------------------------------------------------------
SET_SIZES = (257, 81920, 1064960)
SET_REGIMES = ("continuous", "quantised", "constant", "zero", "nolesion", "alllesion", "signedzero", "negative")


def score_set(n, regime, seed):
    """(x float32 [n], y int8 [n]) for cddpm_eval_set"""
    assert regime in SET_REGIMES
    rng = _rng(seed, n)
    y = (rng.random(n) < 0.08).astype(np.int8)
    if regime == "nolesion":
        y[:] = 0
    if regime == "alllesion":
        y[:] = 1
    c = 0.2 * np.exp2(-12.0 * rng.random(n)) + 0.35 * y * rng.random(n)
    if regime == "quantised":
        c = np.round(c * 128.0) / 32.0
    elif regime == "constant":
        c = np.full(n, 0.5)
    elif regime == "zero":
        c = np.zeros(n)
    elif regime == "signedzero":                                    # both zeros, which are one score, among positive scores
        c = np.round(c * 128.0) / 32.0
        c[(c == 0) & (rng.random(n) < 0.5)] = -0.0
    elif regime == "negative":                                      # scores on both sides of zero
        c = c - 0.05
    return c.astype(np.float32), y


# (n, regime, seed): all regimes at the small size, "continuous" at the two large ones plus one quantised run at 81 920
SET_CASES = [(SET_SIZES[0], g, 600 + j) for j, g in enumerate(SET_REGIMES)] \
    + [(SET_SIZES[1], "continuous", 611), (SET_SIZES[1], "quantised", 612), (SET_SIZES[2], "continuous", 621)]


# ---- component regimes: the foreground is diff > threshold, with the threshold passed as the override ---------------
def _random_foreground(shape, density, seed):
    v = volume(shape, "continuous", seed)
    v["diff"] = _rng(seed, 7).random(shape, dtype=np.float32)
    return v, float(np.float32(1.0 - density))


def _binary(shape, fg, seed):
    v = volume(shape, "continuous", seed)
    v["diff"] = fg.astype(np.float32)
    return v, 0.5


def serpentine(shape=(16, 16, 16), planes=6):
    """One voxel wide path: in every second plane x it runs along z through every second line y, forwards and backwards in
    turn, joined at alternating line ends through the line between and from plane to plane through the plane between: one
    long thin component whose links alternate in memory direction. Beside it (two empty planes away): single voxels and a
    corner chain of 7. Returns (foreground, path length)."""
    D0, D1, D2 = shape
    assert 2 * planes + 2 <= D0 and D1 % 2 == 0
    fg = np.zeros(shape, bool)
    for p in range(planes):
        x = 2 * p
        fg[x, 0:D1:2, :] = True
        for k, y in enumerate(range(1, D1 - 1, 2)):                 # line ends: z = D2 - 1 after a forward line, 0 after a backward one
            fg[x, y, D2 - 1 if k % 2 == 0 else 0] = True
        if p + 1 < planes:                                          # to the next plane: at the last line and the first in turn
            fg[x + 1, D1 - 2 if p % 2 == 0 else 0, 0] = True
    length = int(fg.sum())
    x = 2 * planes + 1
    for i in range(7):
        fg[x + (i % 2), 2 + i, 2 + i] = True                        # corner chain of 7: removed
    fg[x, 12, 2] = fg[x + 1, 14, 12] = fg[x, 2, 13] = True          # single voxels: removed
    return fg, length


def line_end_pairs(shape=(10, 9, 10)):
    """Clusters of 4 voxels whose nearest voxels are adjacent in memory, or a whole line / plane apart, without being
    neighbours: joined by mistake a pair would be one component of 8 and survive the filter. Returns (foreground, list of
    (voxel a, voxel b) with a, b the nearest voxels of two clusters that must stay apart, the 8-voxel control's voxels)."""
    D0, D1, D2 = shape
    fg = np.zeros(shape, bool)
    pairs = []
    # (x, y, D2 - 1) and (x, y + 1, 0): consecutive in memory. The clusters run along y, away from each other.
    fg[0, 0:4, D2 - 1] = True
    fg[0, 4:8, 0] = True
    pairs.append(((0, 3, D2 - 1), (0, 4, 0)))
    # (x, D1 - 1, z) and (x + 1, 0, z): one line apart in memory. The clusters run along z in the two lines.
    fg[2, D1 - 1, 3:7] = True
    fg[3, 0, 3:7] = True
    pairs.append(((2, D1 - 1, 3), (3, 0, 3)))
    # the two ends of one line, (x, y, 0) and (x, y, D2 - 1): what (x, y - 1, D2) would alias
    fg[5, 2:6, 0] = True
    fg[5, 2:6, D2 - 1] = True
    pairs.append(((5, 2, 0), (5, 2, D2 - 1)))
    # the two ends of one plane, (x, 0, z) and (x, D1 - 1, z): what (x - 1, D1, z) would alias
    fg[7, 0, 2:6] = True
    fg[7, D1 - 1, 2:6] = True
    pairs.append(((7, 0, 2), (7, D1 - 1, 2)))
    control = [(9, 1 + i, 3 + i % 2) for i in range(8)]
    for v in control:                                               # an edge chain of 8: kept
        fg[v] = True
    return fg, pairs, control


def component_case(name):
    """(volume dict, threshold override) of a component case"""
    if name == "sparse_odd":
        return _random_foreground((33, 19, 4), 0.07, 709)
    if name == "sparse_mid":
        return _random_foreground(MID, 0.03, 703)
    if name == "sparse_plane":
        return _random_foreground((1, 40, 37), 0.20, 704)            # R = 1: 8-connectivity in the plane, so denser
    if name == "sparse_column":
        return _random_foreground((70, 9, 1), 0.20, 701)             # D2 = 1: the same
    if name == "dense_odd":
        return _random_foreground((33, 19, 4), 0.30, 706)
    if name == "dense_big":
        # the last plane is the second round of the grid-stride kernels. Its lower half stays dense and joined to the large
        # component; its upper half is cut off by an empty band and thinned to 0.20 in the plane, so that components of 7, 8
        # and more voxels lie wholly in the second round
        v, thr = _random_foreground(BIG, 0.30, 707)
        R, D1, _ = BIG
        v["diff"][R - 2, :D1 // 2 + 2, :] = 0
        v["diff"][R - 1, D1 // 2:D1 // 2 + 2, :] = 0
        v["diff"][R - 1, :D1 // 2, :] *= np.float32(0.875)           # P(0.875 u > 0.7) = 0.2
        return v, thr
    if name == "serpentine":
        return _binary((16, 16, 16), serpentine()[0], 708)
    if name == "line_ends":
        return _binary((10, 9, 10), line_end_pairs()[0], 709)
    if name == "full":
        return _binary((33, 19, 4), np.ones((33, 19, 4), bool), 710)
    if name == "empty":
        return _binary((33, 19, 4), np.zeros((33, 19, 4), bool), 711)
    raise KeyError(name)


SPARSE = ("sparse_odd", "sparse_mid", "sparse_plane", "sparse_column")
# n up, down and up again
COMPONENT_CASES = ("sparse_odd", "sparse_plane", "sparse_mid", "sparse_column", "serpentine", "line_ends", "dense_odd", "full",
                   "empty", "dense_big")


# ---- a labelling that owes nothing to scipy ---------------------------------------------------------------------------
def brute_force_components(v):
    """26-connected components by breadth-first search: list of voxel sets"""
    seen, comps = np.zeros(v.shape, bool), []
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    for start in zip(*np.nonzero(v)):
        if seen[start]:
            continue
        comp, q = set(), deque([start])
        seen[start] = True
        while q:
            p = q.popleft()
            comp.add(p)
            for o in offs:
                n = tuple(a + b for a, b in zip(p, o))
                if all(0 <= c < s for c, s in zip(n, v.shape)) and v[n] and not seen[n]:
                    seen[n] = True
                    q.append(n)
        comps.append(comp)
    return comps


# ---- whole evaluation steps at a shape with H != W --------------------------------------------------------------------
STEP_SHAPES = ((48, 40, 5), (40, 48, 3))      # (H, W, D): W // 25 = 1 erosion; the row axis is H


def step_volume(H, W, D, seed):
    """(final_volume, data_orig, data_seg, data_mask) as float32 [H, W, D] arrays: an elliptic brain that leaves the first
    and last rows empty, a lesion off the centre that spans some rows and not others"""
    rng = _rng(seed, H, W, D)
    yy, xx = np.mgrid[0:H, 0:W]
    brain = ((yy - H / 2) / (0.42 * H)) ** 2 + ((xx - W / 2) / (0.40 * W)) ** 2 < 1.0
    mask = np.repeat(brain[:, :, None], D, axis=2).astype(np.float32)
    les = (yy - 0.4 * H) ** 2 + (xx - 0.55 * W) ** 2 < (0.17 * min(H, W)) ** 2
    seg = np.repeat(les[:, :, None], D, axis=2).astype(np.float32) * mask
    orig = rng.random((H, W, D), dtype=np.float32)
    recon = orig + np.float32(0.05) * rng.standard_normal((H, W, D)).astype(np.float32) \
        - np.float32(0.35) * seg * rng.random((H, W, D), dtype=np.float32)
    return recon.astype(np.float32), orig, seg, mask
