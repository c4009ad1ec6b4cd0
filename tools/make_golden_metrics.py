"""Fixtures for the device evaluation metrics (tests/golden/eval_metrics.json): the REFERENCE's own _test_step / _test_end
(src/utils/utils_eval.py, imported by path through oracle/ref_harness.py) run over the cases of tests/eval_cases.py.

Build container only (the reference tree does not travel to the GPU machine). Stand-ins are registered only for modules
missing here: skimage.measure (label / regionprops restated with scipy: ndimage.label with a 3x3x3 structure, filled_area
from binary_fill_holes(..., ones((3, 3, 3))) over the component's bounding box, as skimage 0.18.3 computes it), monai (a
Hausdorff distance that returns NaN), wandb, torchvision.transforms. Two version differences from the reference's
environment (numpy 1.22.4, scikit-learn 1.0.1) are handled here and recorded with the fixture:
  * numpy 2 keeps np.float32 probe thresholds in find_best_val; passing val_range as Python floats gives numpy 1.22's
    float64 thresholds compared in float32 (NEP 50 weak scalars);
  * scikit-learn >= 1.3 returns AUPRC 0.0 for labels without a positive; 1.0.1 returns NaN, which is recorded.

    python tools/make_golden_metrics.py          # writes tests/golden/eval_metrics.json
"""
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import scipy
import scipy.ndimage as ndi
import sklearn
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import eval_cases as EC  # noqa: E402
import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "eval_metrics.json")


def sk_label(volume, connectivity=3):
    assert connectivity == 3
    lab, _ = ndi.label(np.asarray(volume), structure=np.ones((3, 3, 3)))
    return lab


def sk_regionprops(lab):
    props = []
    for i, sl in enumerate(ndi.find_objects(lab), 1):
        if sl is None:
            continue
        img = lab[sl] == i
        props.append({"label": i, "area": int(img.sum()),
                      "filled_area": int(ndi.binary_fill_holes(img, np.ones((3, 3, 3))).sum())})
    return props


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference_utils_eval():
    for name in ("skimage", "monai", "wandb", "torchvision"):
        try:
            importlib.import_module(name)
        except ImportError:
            if name == "skimage":
                sk = _stub("skimage")
                sk.measure = _stub("skimage.measure", label=sk_label, regionprops=sk_regionprops)
            elif name == "monai":
                mo = _stub("monai")
                mo.metrics = _stub("monai.metrics", compute_hausdorff_distance=lambda *a, **k: torch.tensor(float("nan")))
            elif name == "wandb":
                _stub("wandb")
            else:
                tv = _stub("torchvision")
                tv.transforms = _stub("torchvision.transforms", ToTensor=object, ToPILImage=object)
    path = os.path.join(ref_harness.REF_ROOT, "src", "utils", "utils_eval.py")
    spec = importlib.util.spec_from_file_location("ref_utils_eval", path)
    ue = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ue)
    fbv = ue.find_best_val

    def find_best_val(x, y, val_range=(0, 1), **kw):        # numpy 1.22's float64 probe thresholds under numpy 2
        return fbv(x, y, val_range=(float(val_range[0]), float(val_range[1])), **kw)
    ue.find_best_val = find_best_val
    masks = []
    filt = ue.filter_3d_connected_components

    def filter_3d_connected_components(volume):
        out = filt(volume)
        masks.append(np.asarray(out).astype(bool))
        return out
    ue.filter_3d_connected_components = filter_3d_connected_components
    return ue, masks


def main():
    ue, masks = import_reference_utils_eval()
    notes = []

    def after_step(host, kind):
        ed = host.eval_dict
        if ed["lesionSizePerVol"] and ed["lesionSizePerVol"][-1] == 0 and ed["AUPRCPerVol"][-1] == 0.0:
            ed["AUPRCPerVol"][-1] = float("nan")
            notes.append(f"{kind}: AUPRCPerVol 0.0 (scikit-learn {sklearn.__version__}) recorded as NaN (1.0.1)")
        labels = ed["labelPerSlice"][-EC.H:]
        if ed["AUPRCAnomalyRecoPerSlice"] and labels and not any(labels) and ed["AUPRCAnomalyRecoPerSlice"][-1] == 0.0:
            ed["AUPRCAnomalyRecoPerSlice"][-1] = float("nan")
            notes.append(f"{kind}: AUPRCAnomalyRecoPerSlice 0.0 recorded as NaN (1.0.1)")

    cases = {}
    for name, case in EC.CASES.items():
        masks.clear()
        host = EC.Host(case["dataset"], case["cfg"])
        phases = run_case_plain(ue, case, host, after_step)
        cases[name] = dict(phases=phases, filtered_masks=[np.packbits(m.reshape(-1)).tobytes().hex() for m in masks])
        print(name, [p["threshold"] for p in phases], len(masks), "filtered masks")
    ref_keys = sorted(ue.get_eval_dictionary())
    doc = dict(provenance=dict(generator="tools/make_golden_metrics.py", reference="src/utils/utils_eval.py",
                               cases="tests/eval_cases.py (inputs from numpy PCG64 seeds)",
                               numpy=np.__version__, scipy=scipy.__version__, sklearn=sklearn.__version__, torch=torch.__version__,
                               stand_ins=["skimage.measure: scipy restatement", "monai: Hausdorff NaN", "wandb", "torchvision.transforms"],
                               version_handling=["find_best_val: val_range passed as Python floats (numpy 1.22 float64 thresholds)",
                                                 "AUPRC of a label set without positives recorded as NaN (scikit-learn 1.0.1)"],
                               notes=sorted(set(notes))),
               eval_dict_keys=ref_keys, cases=cases)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def run_case_plain(ue, case, host, after_step):
    res = EC.run_case(ue, case, host, after_step=after_step)
    phases = []
    for (ed, thr), (stage, vols) in zip(res, case["phases"]):
        d = {k: EC.plain(v) for k, v in ed.items() if not (isinstance(v, list) and not v) and k not in ("IDs",)}
        phases.append(dict(stage=stage, eval_dict=d, threshold={k: EC.plain(v) for k, v in thr.items()}))
    return phases


if __name__ == "__main__":
    main()
