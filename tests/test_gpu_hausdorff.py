"""GPU: the device Hausdorff distance (csrc/eval_hausdorff.hip through CddpmEngine.hausdorff and cfg.evalHausdorff of the native
_test_step) against the live scipy restatement of tests/hausdorff_reference.py. Every comparison is exact: the edge byte and both
squared fields voxel for voxel, the record with ==. The shapes sit at the kernels' loop edges: a line pass stages K = 2048 // L
neighbouring lines of length L per 256-thread block and walks at most 128 tiles per grid round."""
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_cases as EC
import hausdorff_reference as HR
from conftest import GOLD, load_pkg
from test_gpu_eval_metrics import Recorder, close, unpack_mask

pytestmark = pytest.mark.gpu

BIG = (128, 128, 32)
# file order: the workspace grows up to BIG and is then reused at smaller sizes
SHAPES = ([(96, 96, 4), (1, 1, 1), (5, 3, 2), (1, 40, 3), (30, 1, 1), (12, 12, 4)]
          + [s for L in (63, 64, 65, 255, 256, 257) for s in ((L, 3, 2), (3, L, 2), (2, 3, L))]
          + [(1, 1, 255), (1, 1, 256), (1, 1, 257),           # one tile of 255 / 256 / 257 elements for 256 threads
             (1024, 3, 2), (2, 1024, 3), (3, 2, 1024),        # the longest line: two lines per tile, the largest distances
             (200, 37, 3),                                    # 200 tiles along axis 1: a second, partial grid round; partial tiles
             BIG,                                             # 256 tiles along every axis: two grid rounds
             (7, 6, 5), (2, 2, 2)])


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=10, max_batch=1, max_h=32, max_w=32)


def layouts(shape):
    """(name, pred uint8, seg float32) for one shape; the same masks are run with the flag set and clear"""
    R, D1, D2 = shape
    n = R * D1 * D2
    rng = np.random.Generator(np.random.PCG64(n * 7 + R))
    zero = np.zeros(shape, bool)
    out = []
    dens = (0.05,) if shape == BIG else (0.002, 0.05, 0.5)
    for d in dens:
        out.append((f"random{d}", rng.random(shape) < d, rng.random(shape) < d))
    # solid blocks (interiors are no edges where the block is 3 wide), overlapping, the second touching the far faces
    a, b = zero.copy(), zero.copy()
    a[: max(1, R * 2 // 3), : max(1, D1 * 2 // 3), : max(1, D2 * 2 // 3)] = True
    b[R // 3:, D1 // 3:, D2 // 3:] = True
    out.append(("blocks", a, b))
    corner_p, corner_g = zero.copy(), zero.copy()
    corner_p[0, 0, 0] = corner_g[-1, -1, -1] = True
    out.append(("corners", corner_p, corner_g))               # the largest distance: FAR + (L - 1)^2 terms in every pass
    if shape == BIG:
        return out
    full = ~zero
    out.append(("full_vs_random", full, rng.random(shape) < 0.5))       # touches every face
    out.append(("full_vs_full", full, full))
    r5 = rng.random(shape) < 0.05
    out += [("pred_empty", zero, r5 | corner_p), ("seg_empty", r5 | corner_p, zero), ("both_empty", zero, zero)]
    out.append(("identical", r5 | corner_g, r5 | corner_g))
    out.append(("single_voxel", corner_g, corner_g))
    for ax in range(3):                                       # a union confined to one slice / one line, in the three orientations
        sl = [slice(None)] * 3
        sl[ax] = shape[ax] // 2
        p, g = zero.copy(), zero.copy()
        p[tuple(sl)] = rng.random(p[tuple(sl)].shape) < 0.6
        g[tuple(sl)] = rng.random(g[tuple(sl)].shape) < 0.6
        out.append((f"slice{ax}", p, g))
        ln = [s // 2 for s in shape]
        ln[ax] = slice(None)
        p, g = zero.copy(), zero.copy()
        p[tuple(ln)] = rng.random(shape[ax]) < 0.7
        g[tuple(ln)] = rng.random(shape[ax]) < 0.7
        out.append((f"line{ax}", p, g))
    seg = np.where(rng.random(shape) < 0.3, np.float32(2.0), np.float32(0.0))     # 2.0 and 0.5 are foreground
    seg[rng.random(shape) < 0.1] = 0.5
    out.append(("seg_values", rng.random(shape) < 0.3, seg.astype(np.float32)))
    return out


def run(eng, pred, seg, squeeze):
    p = torch.from_numpy(np.ascontiguousarray(pred).astype(np.uint8)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(seg).astype(np.float32)).cuda()
    return {k: v.cpu().numpy() for k, v in eng.hausdorff(p, s, squeeze=squeeze, fields=True).items()}


def check(got, ref, tag):
    rec = got["record"]
    assert np.array_equal(got["edges"], ref.edge_pred.astype(np.uint8) | (ref.edge_seg.astype(np.uint8) << 1)), tag
    assert np.array_equal(got["dist2"][0], ref.dist2_pred), tag
    assert np.array_equal(got["dist2"][1], ref.dist2_seg), tag
    if math.isnan(ref.distance):
        assert math.isnan(rec[0]), tag
    elif math.isinf(ref.distance):
        assert math.isinf(rec[0]) and rec[0] > 0, tag
    else:
        assert rec[0] == ref.distance, (tag, rec[0], ref.distance)
    if ref.d2_pred_to_seg is None:
        assert math.isnan(rec[1]) and math.isnan(rec[2]), tag
    else:
        assert (rec[1], rec[2]) == (ref.d2_pred_to_seg, ref.d2_seg_to_pred), (tag, rec[1], rec[2])
    assert (rec[3], rec[4]) == (ref.edge_pred.sum(), ref.edge_seg.sum()), tag
    assert tuple(rec[5:8]) == tuple(float(a) for a in ref.active), (tag, rec[5:8], ref.active)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edges_fields_and_record_against_scipy(eng, shape):
    ran = 0
    for name, pred, seg in layouts(shape):
        for squeeze in (True, False):
            check(run(eng, pred, seg, squeeze), HR.hausdorff(pred, seg, squeeze), (shape, name, squeeze))
            ran += 1
    assert ran >= 6
    if shape == BIG:
        assert eng._hausdorff_ws.numel() >= 9 * 128 * 128 * 32
    if shape == (2, 2, 2):                                    # after BIG in file order: the grown workspace is reused
        assert eng._hausdorff_ws.numel() >= 9 * 128 * 128 * 32


def test_ring_case(eng):
    P = np.zeros((12, 12, 4), bool)
    P[1:10, 2:11, 2] = True
    G = P.copy()
    G[2:9, 3:10, 2] = False
    for squeeze, want, axes in ((True, 0.0, (1.0, 1.0, 0.0)), (False, 4.0, (1.0, 1.0, 1.0))):
        got = run(eng, P, G, squeeze)
        check(got, HR.hausdorff(P, G, squeeze), ("ring", squeeze))
        assert got["record"][0] == want and tuple(got["record"][5:8]) == axes


def test_record_only_call_and_second_run_bitwise_identical(eng):
    rng = np.random.Generator(np.random.PCG64(99))
    p = torch.from_numpy((rng.random((96, 96, 4)) < 0.05).astype(np.uint8)).cuda()
    s = torch.from_numpy((rng.random((96, 96, 4)) < 0.05).astype(np.float32)).cuda()
    a, b = eng.hausdorff(p, s, fields=True), eng.hausdorff(p, s, fields=True)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    c = eng.hausdorff(p, s)                                   # squeeze is the default; without fields only the record
    assert set(c) == {"record"} and torch.equal(c["record"].view(torch.uint8), a["record"].view(torch.uint8))
    assert c["record"][0].item() == HR.hausdorff(p.cpu().numpy(), s.cpu().numpy(), True).distance


def test_distance_is_the_correctly_rounded_square_root(eng):
    """two single voxels d apart: the record holds math.sqrt(|d|^2) for squared distances from 1 to over 10^6, few of them squares"""
    shape = (1024, 4, 3)
    s = torch.zeros(shape, device="cuda")
    s[0, 0, 0] = 1.0
    recs, want = [], []
    for i, r in enumerate(list(range(1, 60)) + list(range(61, 1024, 13)) + [1023]):
        y, z = i % 4, (i // 4) % 3
        p = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        p[r, y, z] = 1
        recs.append(eng.hausdorff(p, s, squeeze=bool(i & 1))["record"])
        want.append(r * r + y * y + z * z)
    recs = torch.stack(recs).cpu().numpy()
    assert len({math.isqrt(w) ** 2 == w for w in want}) == 2
    for rec, w in zip(recs, want):
        assert rec[0] == math.sqrt(w) and rec[1] == rec[2] == w, (rec, w)


def test_engine_rejects_bad_inputs(eng):
    p = torch.zeros(4, 8, 8, dtype=torch.uint8, device="cuda")
    s = torch.zeros(4, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="uint8"):
        eng.hausdorff(p.float(), s)
    with pytest.raises(RuntimeError, match="float32"):
        eng.hausdorff(p, s.double())
    with pytest.raises(RuntimeError, match="shape"):
        eng.hausdorff(p, torch.zeros(4, 8, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="shape"):
        eng.hausdorff(p.reshape(-1), s.reshape(-1))
    with pytest.raises(RuntimeError, match="1024"):
        eng.hausdorff(torch.zeros(1025, 2, 1, dtype=torch.uint8, device="cuda"), torch.zeros(1025, 2, 1, device="cuda"))
    with pytest.raises(RuntimeError, match="HIP device"):
        eng.hausdorff(p, s.cpu())


class Capture(Recorder):
    """keeps the residual each eval_volume call was given, beside what it returned"""

    def __init__(self, eng):
        super().__init__(eng)
        self.diffs = []

    def eval_volume(self, recon, orig, seg, mask, diff, **k):
        self.diffs.append(diff)
        return super().eval_volume(recon, orig, seg, mask, diff, **k)


@pytest.mark.parametrize("name", ["val_then_test", "components", "node"])
def test_test_step_fills_hausdorff_end_to_end(eng, name):
    UE = load_pkg("utils_eval")
    with open(os.path.join(GOLD, "eval_metrics.json")) as f:
        ref = json.load(f)["cases"][name]
    case = EC.CASES[name]
    rec = Capture(eng)
    host = EC.Host(case["dataset"], dict(case["cfg"], evalHausdorff=True), diffusion=rec)
    res = EC.run_case(UE, case, host, to_device=lambda t: t.cuda())
    segs = [EC.volume(kind, seed)[2][0, 0].numpy() for _stage, vols in case["phases"] for kind, seed in vols]
    if name == "node":          # no component filter: the reference hands monai diff > threshold as it is (float32 comparison)
        masks = [d.cpu().numpy() > np.float32(v["record"][13].item()) for d, v in zip(rec.diffs, rec.volumes)]
    else:
        masks = [unpack_mask(m) for m in ref["filtered_masks"]]
    assert len(masks) == len(segs) == len(rec.volumes)
    got = [h for ed, _thr in res for h in ed["HausPerVol"]]
    want = [HR.hausdorff(m, s, True).distance for m, s in zip(masks, segs)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w or (math.isnan(g) and math.isnan(w)), (got, want)
    checked = 0
    for (ed, _thr), phase in zip(res, ref["phases"]):         # every other key as recorded: the switch changes nothing else
        for key, w in phase["eval_dict"].items():
            if key.startswith("HausPerVol"):
                continue
            assert close(key, EC.plain(ed[key]), w), (name, phase["stage"], key)
            checked += 1
        finite = [h for h in ed["HausPerVol"] if math.isfinite(h)]
        assert finite and math.isfinite(ed["HausPerVolMean"]) and ed["HausPerVolMean"] == np.mean(finite)
    assert checked > 40
