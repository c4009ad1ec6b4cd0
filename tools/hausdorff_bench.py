"""Times the device Hausdorff distance (CddpmEngine.hausdorff: cddpm_eval_hausdorff, csrc/eval_hausdorff.hip) at the experiment's
96 x 96 x 4 evaluation volume and at 128 x 128 x 128, on seeded blob masks (a thresholded residual and a lesion have surfaces, not
salt and pepper). Method: warm-up calls, then `--reps` calls each between two device events on the engine's stream, the median and
the minimum of those; the workspace is sized by the warm-up, so a timed call allocates only its 64-byte record. Needs an MI355X: no
device, no number. The wall time of the scipy restatement of the same semantics (tests/hausdorff_reference.py) on this host's CPU is
printed beside it for scale only: another algorithm on another processor, no comparison of kernels.

    python tools/hausdorff_bench.py [--reps 50] [--out profiles/hausdorff_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "conditioned-diffusion-models-uad_amd"

SHAPES = [(96, 96, 4), (128, 128, 128)]


def blobs(shape, seed, count):
    """a union of `count` balls with seeded centres and radii: a mask with interiors and a surface"""
    rng = np.random.Generator(np.random.PCG64(seed))
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1)
    m = np.zeros(shape, bool)
    for _ in range(count):
        c = rng.random(3) * np.array(shape)
        r = 2 + rng.random() * max(shape) / 8
        m |= ((grid - c) ** 2).sum(-1) < r * r
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hausdorff_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: the Hausdorff distance is timed on an MI355X or not at all")
    import hausdorff_reference as HR
    eng = importlib.import_module(f"{PKG}.engine").CddpmEngine(timesteps=10, max_batch=1, max_h=32, max_w=32)
    stream = torch.cuda.current_stream(eng.device)
    rows = []
    for shape in SHAPES:
        P, G = blobs(shape, 1, 6), blobs(shape, 2, 6)
        p = torch.from_numpy(P.astype(np.uint8)).cuda()
        s = torch.from_numpy(G.astype(np.float32)).cuda()
        t0 = time.perf_counter()
        ref = HR.hausdorff(P, G, True)
        scipy_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(a.warmup):
            rec = eng.hausdorff(p, s)["record"]
        torch.cuda.synchronize()
        same = rec[0].item() == ref.distance
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.hausdorff(p, s)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        row = dict(shape=list(shape), voxels=int(np.prod(shape)), edges_pred=int(ref.edge_pred.sum()), edges_seg=int(ref.edge_seg.sum()),
                   distance=ref.distance, equals_scipy=bool(same), device_ms_median=statistics.median(ts), device_ms_min=min(ts),
                   scipy_host_ms=scipy_ms)
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, method="device events around one call, median",
                       rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
