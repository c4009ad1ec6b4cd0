"""CPU: what the Hausdorff tests rest on. The live numpy / scipy restatement (tests/hausdorff_reference.py) against an independent
brute-force computation and against hand-computed cases; the host arithmetic of cddpm_hausdorff_workspace_bytes; and the default of
the native _test_step, which stays NaN unless cfg.evalHausdorff is set."""
import math

import numpy as np
import pytest
import torch

import eval_cases as EC
import hausdorff_reference as HR
from conftest import load_pkg


def rng_masks(shape, density, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random(shape) < density, rng.random(shape) < density


@pytest.mark.parametrize("shape", [(7, 5, 3), (4, 4, 4), (1, 9, 6), (6, 1, 1), (3, 8, 1), (10, 9, 2)])
@pytest.mark.parametrize("density", [0.05, 0.3, 0.8])
def test_reference_against_brute_force(shape, density):
    for seed in range(3):
        P, G = rng_masks(shape, density, 1000 * seed + shape[0])
        for squeeze in (True, False):
            r = HR.hausdorff(P, G, squeeze)
            U = P | G
            if squeeze and U.any():
                idx = np.nonzero(U)
                assert r.active == tuple(int(i.max()) > int(i.min()) for i in idx)
            # with no active axis the union is one voxel, which is its own edge: the rule for that is "all axes"
            act = r.active if any(r.active) else (True, True, True)
            assert np.array_equal(r.edge_pred, HR.brute_force_edge(P, act))
            assert np.array_equal(r.edge_seg, HR.brute_force_edge(G, act))
            for e, d2 in ((r.edge_pred, r.dist2_pred), (r.edge_seg, r.dist2_seg)):
                if e.any():
                    pts = np.argwhere(e)
                    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 1, 3)
                    want = ((grid - pts[None]) ** 2).sum(-1).min(1).reshape(shape)
                    assert np.array_equal(d2, want)
                else:
                    assert (d2 == HR.FAR).all()
            if P.any() and G.any():
                pg, gp = HR.brute_force(r.edge_pred, r.edge_seg), HR.brute_force(r.edge_seg, r.edge_pred)
                assert (r.d2_pred_to_seg, r.d2_seg_to_pred) == (pg, gp)
                assert r.distance == math.sqrt(max(pg, gp))
            elif P.any() or G.any():
                assert math.isinf(r.distance) and r.d2_pred_to_seg is None
            else:
                assert math.isnan(r.distance)


def ring_case():
    """a 9 x 9 one-voxel-thick square against its own perimeter ring, in one slice of a 12 x 12 x 4 volume"""
    P = np.zeros((12, 12, 4), bool)
    P[1:10, 2:11, 2] = True
    G = P.copy()
    G[2:9, 3:10, 2] = False
    return P, G


def test_ring_case_pins_the_squeeze_rule():
    P, G = ring_case()
    with_flag, without = HR.hausdorff(P, G, True), HR.hausdorff(P, G, False)
    assert with_flag.distance == 0.0 and with_flag.active == (True, True, False)
    assert np.array_equal(with_flag.edge_pred, G) and np.array_equal(with_flag.edge_seg, G)      # both edge sets are the perimeter
    assert without.distance == 4.0 and without.active == (True, True, True)
    assert np.array_equal(without.edge_pred, P)                                                  # every voxel of the flat square


@pytest.mark.parametrize("shape", [(1, 1, 2), (5, 3, 2), (1, 40, 3), (30, 1, 1), (12, 12, 4), (2, 3, 65)])
def test_opposite_corners(shape):
    P, G = np.zeros(shape, bool), np.zeros(shape, bool)
    P[0, 0, 0] = G[-1, -1, -1] = True
    want = math.sqrt(sum((s - 1) ** 2 for s in shape))
    for squeeze in (True, False):
        r = HR.hausdorff(P, G, squeeze)
        assert r.distance == want and r.d2_pred_to_seg == r.d2_seg_to_pred == sum((s - 1) ** 2 for s in shape)


def test_identical_masks_and_the_empty_rules():
    P, _ = rng_masks((9, 8, 4), 0.3, 3)
    Z = np.zeros_like(P)
    one = np.zeros((1, 1, 1), bool)
    one[0, 0, 0] = True
    single = np.zeros((6, 5, 4), bool)
    single[2, 3, 1] = True
    for squeeze in (True, False):
        assert HR.hausdorff(P, P, squeeze).distance == 0.0
        assert HR.hausdorff(one, one, squeeze).distance == 0.0
        r = HR.hausdorff(single, single, squeeze)                  # one voxel: no active axis under the flag, its own edge
        assert r.distance == 0.0 and np.array_equal(r.edge_pred, single) and r.active == ((False,) * 3 if squeeze else (True,) * 3)
        assert math.isnan(HR.hausdorff(Z, Z, squeeze).distance)
        for a, b in ((P, Z), (Z, P)):
            r = HR.hausdorff(a, b, squeeze)
            assert math.isinf(r.distance) and r.distance > 0 and r.d2_pred_to_seg is None and r.d2_seg_to_pred is None
    seg = np.zeros((9, 8, 4), np.float32)                          # foreground is != 0: 2.0 and 0.5 count
    seg[P] = 2.0
    seg[0, 0, 0] = 0.5
    Q = P.copy()
    Q[0, 0, 0] = True
    assert HR.hausdorff(Q, seg).distance == 0.0


def test_workspace_bytes_is_host_arithmetic():
    lib = load_pkg("_lib").load_library()
    for shape in ((1, 1, 1), (96, 96, 4), (128, 128, 128), (1024, 1024, 1024), (1024, 1, 7)):
        n = shape[0] * shape[1] * shape[2]
        b = lib.cddpm_hausdorff_workspace_bytes(*shape)
        assert 9 * n <= b <= 9 * n + 4096, (shape, b)              # the edge byte and two int32 fields per voxel, a stats line, padding
    for shape in ((0, 4, 4), (4, -1, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025)):
        assert lib.cddpm_hausdorff_workspace_bytes(*shape) == 0
        msg = lib.cddpm_last_error(None).decode()
        assert "cddpm_hausdorff_workspace_bytes" in msg and "x".join(str(s) for s in shape) in msg and "1024" in msg


class StubEngine:
    """an engine that computes nothing: shapes and dtypes of CddpmEngine's results, on the CPU; records the hausdorff calls"""

    def __init__(self):
        self.calls = []

    def _engine(self, B, H, W, device):
        return self

    def residual_postprocess(self, orig, recon, mask=None, **kw):
        return torch.zeros_like(orig)

    def eval_volume(self, recon, orig, seg, mask, diff, **kw):
        R, D1, D2 = diff.shape
        rec = torch.zeros(24, dtype=torch.float64)
        rec[8] = R * D1 * D2
        self.pred = torch.zeros(R, D1, D2, dtype=torch.uint8)
        return dict(record=rec, row_score=torch.zeros(R), row_label=torch.zeros(R, dtype=torch.int32),
                    row_counts=torch.zeros(R, 3, dtype=torch.int32), pred=self.pred)

    def eval_set(self, x, y, **kw):
        return torch.zeros(8, dtype=torch.float64)

    def hausdorff(self, pred, seg, **kw):
        self.calls.append((pred, seg, kw))
        return dict(record=torch.tensor([2.5, 4.0, 6.25, 1.0, 1.0, 1.0, 1.0, 1.0], dtype=torch.float64))


@pytest.mark.parametrize("key, want", [(None, None), (False, None), (True, 2.5)])
def test_test_step_default_stays_nan(key, want):
    UE = load_pkg("utils_eval")
    cfg = dict(EC.CFG) if key is None else dict(EC.CFG, evalHausdorff=key)
    stub = StubEngine()
    host = EC.Host("Brats21", cfg, diffusion=stub)
    host.stage, host.eval_dict = "val", UE.get_eval_dictionary()
    fv, orig, seg, mask = EC.volume("lesion", 11)
    UE._test_step(host, fv, orig, seg, mask, 0, ["v0"], torch.tensor(1))
    (h,) = host.eval_dict["HausPerVol"]
    if want is None:
        assert math.isnan(h) and stub.calls == []
    else:
        assert h == want and len(stub.calls) == 1
        pred, s, kw = stub.calls[0]
        assert pred is stub.pred and torch.equal(s, seg.squeeze()) and kw == {}      # the filtered prediction, raw data_seg, squeeze on
    UE._test_end(host)
    assert math.isnan(host.eval_dict["HausPerVolMean"]) if want is None else host.eval_dict["HausPerVolMean"] == want
