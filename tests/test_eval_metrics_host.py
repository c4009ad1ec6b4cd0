"""CPU: what the evaluation-metric fixtures rest on (tools/make_golden_metrics.py, tests/golden/eval_metrics.json) and the
host-only parts of the native _test_end (utils_eval.py of this package): the aggregates and the test stage's `del threshold`."""
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, load_pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_metrics as MG  # noqa: E402
import eval_cases as EC  # noqa: E402
from metric_shape_cases import brute_force_components  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "eval_metrics.json")) as f:
        return json.load(f)


def test_skimage_restatement_against_brute_force_labelling():
    rng = np.random.default_rng(5)
    for shape, p in (((9, 8, 4), 0.2), ((12, 7, 5), 0.35), ((6, 6, 6), 0.1)):
        v = rng.random(shape) < p
        lab = MG.sk_label(v, connectivity=3)
        props = MG.sk_regionprops(lab)
        want = sorted(sorted(c) for c in brute_force_components(v))
        got = sorted(sorted(zip(*np.nonzero(lab == pr["label"]))) for pr in props)
        assert got == want
        for pr in props:
            assert pr["area"] == int((lab == pr["label"]).sum())
            if pr["area"] <= 7:       # a cavity needs a closed shell of 26 voxels: small components have no holes
                assert pr["filled_area"] == pr["area"]
    shell = np.ones((3, 3, 3), bool)
    shell[1, 1, 1] = False            # the smallest component with a cavity sealed against 26-connected background
    (pr,) = MG.sk_regionprops(MG.sk_label(np.pad(shell, 1)))
    assert pr["area"] == 26 and pr["filled_area"] == 27


def test_the_components_case_pins_the_size_rule():
    v = EC.volume("components", 61)[0][0, 0].numpy() > 0
    sizes = sorted(len(c) for c in brute_force_components(v))
    assert 7 in sizes and 8 in sizes and 1 in sizes


def test_fixture_provenance(fixture):
    p = fixture["provenance"]
    assert p["generator"] == "tools/make_golden_metrics.py" and p["reference"] == "src/utils/utils_eval.py"
    for k in ("numpy", "scipy", "sklearn", "torch"):
        assert p[k]
    assert any("find_best_val" in s for s in p["version_handling"]) and any("AUPRC" in s for s in p["version_handling"])
    assert set(fixture["cases"]) == set(EC.CASES)
    assert os.path.getsize(os.path.join(GOLD, "eval_metrics.json")) < 1 << 20
    # the native eval_dict has the reference's key set and initial values
    UE = load_pkg("utils_eval")
    d = UE.get_eval_dictionary()
    assert sorted(d) == fixture["eval_dict_keys"]
    assert all(d[k] == 0.0 for k in UE._SCALARS) and all(v == [] for k, v in d.items() if k not in UE._SCALARS)


def same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def test_native_aggregates_against_the_fixtures(fixture):
    UE = load_pkg("utils_eval")
    n = 0
    for case in fixture["cases"].values():
        for phase in case["phases"]:
            ref = phase["eval_dict"]
            ed = UE.get_eval_dictionary()
            for k, v in ref.items():
                if isinstance(ed.get(k), list):
                    ed[k] = list(v)
            UE._aggregate(ed)
            for out, _src, _nan in UE._AGGREGATES:
                for suffix in ("Mean", "Std"):
                    assert same(float(ed[out + suffix]), ref[out + suffix]), (out + suffix, ed[out + suffix], ref[out + suffix])
                    n += 1
            assert same(float(ed["HausPerVolMean"]), ref["HausPerVolMean"])
    assert n > 300


def test_native_test_end_deletes_the_threshold_in_the_test_stage(fixture):
    UE = load_pkg("utils_eval")
    host = EC.Host("Brats21", EC.CFG)
    host.stage = "test"
    host.threshold = {"total": 0.06}
    host.eval_dict = UE.get_eval_dictionary()
    UE._test_end(host)
    assert not hasattr(host, "threshold")
    test_phase = fixture["cases"]["val_then_test"]["phases"][1]
    assert test_phase["stage"] == "test" and test_phase["threshold"] == {}
