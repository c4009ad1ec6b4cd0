"""CPU: the split-K rule of the small-batch plan (csrc/cddpm_api.hip::ksplit_rule, exported host-only as cddpm_conv_ksplit_plan) against
the rule written out again in Python (conv_plan_cases.ksplit_rule), its invariants over a grid, and the plane workspace condition of
conv_launch over the descriptors of arch_cases.py. The kernel reads the rule's output as data (ConvArgs::kbound); an empty or
non-monotone range would make a workgroup multiply nothing, or a chunk twice."""
import ctypes as C

import pytest

import arch_cases as A
import conv_plan_cases as P
from conftest import load_pkg

WORKGROUPS = range(1, 130)
MAIN = range(32, 2049, 32)
SKIP = (0, 128, 256, 384, 512, 640, 768, 1024, 1536, 2048)
TAPS = (1, 4, 9)


@pytest.fixture(scope="module")
def query():
    lib = load_pkg("_lib").load_library()

    def run(family, nwg, Cin, Cskip, taps):
        kb = (C.c_int * (P.MAX_KSPLIT + 1))(*([-7] * (P.MAX_KSPLIT + 1)))
        S = lib.cddpm_conv_ksplit_plan(P.FAMILY_CODE[family], nwg, Cin, Cskip, taps, kb)
        return S, list(kb)

    return run


@pytest.mark.parametrize("taps", TAPS)
def test_rule_equals_the_python_port_and_keeps_its_invariants(query, taps):
    n = split = 0
    for nwg in WORKGROUPS:
        for Cin in MAIN:
            for Cskip in SKIP:
                S, kb = query("h3", nwg, Cin, Cskip, taps)
                what = (nwg, Cin, Cskip, taps, S, kb)
                assert (S, kb[:S + 1]) == P.ksplit_rule("h3", nwg, Cin, Cskip, taps), what
                nch_main, nch_skip = Cin // 32, Cskip // 32
                units = nch_main * taps + nch_skip
                assert S in (1, 2, 4, 8) and kb[0] == 0 and kb[S] == nch_main + nch_skip, what
                assert all(kb[j] < kb[j + 1] for j in range(S)), what                    # no empty range, none out of order
                assert all(v == 0 for v in kb[S + 1:]), what
                assert S * nwg <= 256, what
                assert S == 1 or units // S >= 9, what
                n += 1
                split += S > 1
    assert n == len(WORKGROUPS) * len(MAIN) * len(SKIP) and split > n // 20      # the grid does reach the split plans


@pytest.mark.parametrize("family", ["x6", "f32"])
def test_only_the_default_family_splits(query, family):
    for nwg in (1, 2, 8, 32, 129):
        for Cin in (32, 256, 640, 2048):
            for Cskip in (0, 384):
                for taps in TAPS:
                    assert query(family, nwg, Cin, Cskip, taps) == (1, [0, (Cin + Cskip) // 32] + [0] * (P.MAX_KSPLIT - 1))


def test_bad_arguments_are_refused(query):
    lib = load_pkg("_lib").load_library()
    kb = (C.c_int * (P.MAX_KSPLIT + 1))()
    for args in ((3, 8, 256, 0, 9), (2, 0, 256, 0, 9), (2, 8, 0, 0, 9), (2, 8, 48, 0, 9), (2, 8, 256, 16, 9), (2, 8, 256, -32, 9), (2, 8, 256, 0, 3)):
        assert lib.cddpm_conv_ksplit_plan(*args, kb) == -1, args
    assert lib.cddpm_conv_ksplit_plan(2, 8, 256, 0, 9, None) == -1


def test_cases_of_the_gpu_test_have_the_plans_they_were_written_for(query):
    """the expectations of conv_plan_cases.py (which the GPU test asserts against what the launch reports) are the library's rule"""
    for case in P.ALL_CASES:
        nwg, S, kb = P.case_plan(case)
        taps = 4 if case["folded"] else case["k"] ** 2
        assert (S, kb) == (lambda r: (r[0], r[1][:r[0] + 1]))(query("h3", nwg, case["C0"], case["S0"] + case["S1"], taps)), case["name"]
        assert S == case["expect_S"], (case["name"], S)
        assert case["kbound"] is None or kb == case["kbound"], (case["name"], kb)
        assert S * case["B"] * case["H"] * case["W"] * case["Cout"] <= P.PLANE_FLOATS
        P.check_ranges(case, S, kb)
    skip = next(c for c in P.CASES_P if c["S0"])
    kb, nmain = skip["kbound"], skip["C0"] // 32
    s0_end = nmain + skip["S0"] // 32
    assert any(nmain <= kb[j] < s0_end < kb[j + 1] for j in range(8)), "one range also crosses from skip0 into skip1"
    # the 256-cout threshold: 512 workgroups exactly at GEOM_Q, 480 one slice below
    for case in P.CASES_Q:
        taps = 4 if case["folded"] else 9
        assert P.workgroups_at_max(P.GEOM_Q, case["img"], 256, taps, case["H"], case["W"]) == 512
        assert P.workgroups_at_max(P.GEOM_Q15, case["img"], 256, taps, case["H"], case["W"]) == 480
        assert P.nb2_planned("h3", True, 512, 256, taps, 1) and not P.nb2_planned("h3", True, 480, 256, taps, 1)
        assert not P.nb2_planned("h3", False, 512, 256, taps, 1) and not P.nb2_planned("x6", True, 512, 256, taps, 1)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_split_planes_fit_the_workspace_at_every_descriptors_maximum_geometry(query, name):
    """conv_launch refuses a split launch whose S planes exceed the handle's 256 x 256 x 128 floats: no convolution of a descriptor the
    suite runs may get there at its own maximum geometry (the full batch at the full image)"""
    case = A.CASES[name]
    B, H, W = case["geometry"]
    convs = P.unet_convs(**A.unet_kw(case))
    assert len(convs) >= 12 and all(cin % 32 == 0 and cs % 32 == 0 and co % 128 == 0 for _n, cin, cs, co, _t, _d in convs)
    nsplit = 0
    for lname, Cin, Cskip, Cout, taps, ds in convs:
        assert H % ds == 0 and W % ds == 0
        h, w = H // ds, W // ds
        nwg = P.conv_workgroups(Cout, taps, B, h, w)
        S, kb = query("h3", nwg, Cin, Cskip, taps)
        assert S * B * h * w * Cout <= P.PLANE_FLOATS, (lname, S, B, h, w, Cout)
        assert kb[S] == (Cin + Cskip) // 32
        nsplit += S > 1
    assert nsplit > 0, "these descriptors run at small batches: the split plan is what they take"
