"""The Hausdorff distance of the evaluation step restated live in numpy / scipy (no fixtures): the rules of include/cddpm.h,
"Hausdorff distance", as monai 1.0.1's get_mask_edges / get_surface_distance / compute_hausdorff_distance are recalled --
crop to the union's bounding box, np.squeeze, binary_erosion with the cross, distance_transform_edt, the maximum over the other
edge set. Pinned to scipy, unpinned to monai. Shared by the host tests (which tie it to brute force and to hand-computed cases)
and the GPU tests (which compare the device's edges, fields and record with it exactly)."""
import math
from collections import namedtuple

import numpy as np
from scipy import ndimage

FAR = 1 << 28            # CDDPM_HAUSDORFF_FAR: the squared field of an empty edge set

Result = namedtuple("Result", "distance d2_pred_to_seg d2_seg_to_pred edge_pred edge_seg dist2_pred dist2_seg active")


def _edge(m):
    """m & ~erode(m) with the cross over every axis of m (border_value = 0); a 0-d array is its own edge"""
    if m.ndim == 0:
        return m.copy()
    return m & ~ndimage.binary_erosion(m, structure=ndimage.generate_binary_structure(m.ndim, 1), border_value=0)


def _dist2(edge):
    """squared distance of every voxel to the nearest edge voxel, as exact integers (scipy takes the square root of an integer sum)"""
    if not edge.any():
        return np.full(edge.shape, FAR, np.int64)
    d = ndimage.distance_transform_edt(~edge)
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), d)        # the square root of the integer field IS scipy's EDT
    return d2


def hausdorff(pred, seg, squeeze=True):
    """pred, seg: [R, D1, D2] arrays, foreground where != 0. Returns Result: the distance (NaN: both empty, inf: one empty), the two
    directed squared distances (None unless both masks are non-empty), both edge masks and both squared fields in the volume's shape,
    the active axes."""
    P, G = np.asarray(pred) != 0, np.asarray(seg) != 0
    assert P.ndim == 3 and P.shape == G.shape
    U = P | G
    edges = [np.zeros(P.shape, bool), np.zeros(P.shape, bool)]
    active = (False,) * 3 if squeeze else (True,) * 3
    if U.any():
        idx = np.nonzero(U)
        lo, hi = [int(i.min()) for i in idx], [int(i.max()) for i in idx]
        if squeeze:
            active = tuple(h > l for l, h in zip(lo, hi))
            box = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
            for e, m in zip(edges, (P, G)):
                c = np.squeeze(m[box])                                  # monai: crop to the box, squeeze, erode
                e[box] = _edge(c).reshape(m[box].shape)
        else:
            edges = [_edge(P), _edge(G)]
    ep, eg = edges
    assert ep.any() == P.any() and eg.any() == G.any()                  # a non-empty mask always has an edge
    d2p, d2g = _dist2(ep), _dist2(eg)
    if not P.any() and not G.any():
        return Result(math.nan, None, None, ep, eg, d2p, d2g, active)
    if not P.any() or not G.any():
        return Result(math.inf, None, None, ep, eg, d2p, d2g, active)
    # the distance the way monai takes it: distance_transform_edt of the cropped (and squeezed) complement, read on the other edge
    box = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
    cp, cg = (np.squeeze(e[box]) if squeeze else e for e in (ep, eg))
    if cp.ndim == 0:
        dist = 0.0 if (cp and cg) else math.inf
    else:
        dist = float(max(ndimage.distance_transform_edt(~cg)[cp].max(), ndimage.distance_transform_edt(~cp)[cg].max()))
    pg, gp = int(d2g[ep].max()), int(d2p[eg].max())
    assert dist == math.sqrt(max(pg, gp))                               # the crop selects the axes and changes nothing else
    return Result(dist, pg, gp, ep, eg, d2p, d2g, active)


def brute_force(edge_a, edge_b):
    """max over a in edge_a of min over b in edge_b of the squared index distance: O(|A| |B|), no transform"""
    a = np.argwhere(edge_a).astype(np.int64)
    b = np.argwhere(edge_b).astype(np.int64)
    return int(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1).min(1).max())


def brute_force_edge(m, active=(True, True, True)):
    """edge(M) voxel by voxel from the definition"""
    out = np.zeros(m.shape, bool)
    for v in np.argwhere(m):
        inner = any(active)
        for a in range(3):
            if not active[a]:
                continue
            for s in (-1, 1):
                w = v.copy()
                w[a] += s
                if w[a] < 0 or w[a] >= m.shape[a] or not m[tuple(w)]:
                    inner = False
        out[tuple(v)] = not inner
    return out
