"""CPU: the float64 references and bounds of conv_plan_cases.py (what tests/test_gpu_conv_planned.py compares the planned convolution
with) against torch's own operators, and the Python port of the UNet's convolution list against the parameter shapes of the synthetic
weights."""
import pytest
import torch
import torch.nn.functional as F

import conv_plan_cases as P
import test_gpu_kernels as K
from conftest import load_pkg
from conv_p16_reference import folded_classes, folded_conv


def _small(case, **over):
    """a case at a size a CPU runs in a blink, same structure"""
    c = dict(case, B=1, C0=64, Cout=128, H=min(case["H"], 8), W=min(case["W"], 12))
    c.update(over)
    if c["S0"]:
        c.update(S0=64, S1=32)
    return c


def test_two_source_skip_reference_is_conv2d_on_the_concatenation():
    case = _small(next(c for c in P.CASES_P if c["S0"]))
    d = P.make_inputs(case)
    sk0, sk1 = d["skip"][:, :case["S0"]], d["skip"][:, case["S0"]:]
    got = P.skip64(sk0, sk1, d["wskip"])
    want = F.conv2d(torch.cat([sk0, sk1], 1).double(), d["wskip"].double())
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # and the case reference is the plain composition: conv3x3(act(x)) + bias + conv1x1(cat[skip0, skip1])
    ref, _ = P.reference32(case, d, 8)
    v = P.act64(d["x"], d["coef"], True)
    plain = F.conv2d(v, d["wt"].double(), d["bias"].double(), padding=1) + want
    assert float((ref - plain).abs().max()) <= 1e-12 * float(plain.abs().max())
    # one source only: the second is optional
    assert torch.equal(P.skip64(d["skip"], None, d["wskip"]), F.conv2d(d["skip"].double(), d["wskip"].double()))


def test_folded_classes_equal_upsample_then_conv3x3():
    case = _small(next(c for c in P.CASES_P if c["folded"]), H=8, W=12)
    d = P.make_inputs(case)
    assert d["x"].shape[-2:] == (4, 6) and d["res"].shape[-2:] == (4, 6)
    ref, lim = P.reference32(case, d, 2)
    v = P.act64(d["x"], d["coef"], True)
    up = F.conv2d(F.interpolate(v, scale_factor=2, mode="nearest"), d["wt"].double(), d["bias"].double(), padding=1)
    up = up + F.interpolate(d["res"].double(), scale_factor=2, mode="nearest")
    assert float((ref - up).abs().max()) <= 1e-12 * float(up.abs().max())
    # the four 2 x 2 class kernels the packer folds (their sums rounded once to fp32) give the same convolution to fp32 rounding of the
    # weights -- far inside the bound
    cls = folded_conv(v, folded_classes(d["wt"])) + d["bias"].double()[None, :, None, None] + F.interpolate(d["res"].double(), scale_factor=2, mode="nearest")
    assert float(((cls - up).abs() / lim).max()) < 0.1


@pytest.mark.parametrize("case", P.ALL_CASES, ids=[c["name"] for c in P.ALL_CASES])
def test_every_case_has_a_positive_finite_bound(case):
    c = _small(case)
    d = P.make_inputs(c)
    for fam in ("h3", "x6"):
        ref, lim = P.reference32(c, d, c["expect_S"] if fam == "h3" else 1, fam)
        assert ref.shape == (1, c["Cout"], c["H"], c["W"]) == lim.shape
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(lim).all()) and float(lim.min()) > 0
        assert float((lim / (ref.abs() + lim)).median()) < 1e-4          # a bound at the fp32 level, not a vacuous one
    if case["name"] in P.P16_NAMES:
        ref16, lim16 = P.reference16(c, d, 13)
        assert bool(torch.isfinite(ref16).all()) and bool(torch.isfinite(lim16).all()) and float(lim16.min()) > 0
        ref32, _ = P.reference32(c, d, 8)
        assert float((ref16 - ref32).abs().max()) > 0          # fp16 operands are a different function
    # the B = 1 slice of the inputs gives the same slice of the reference
    full = dict(c, B=2)
    dd = P.make_inputs(full)
    r2, l2 = P.reference32(full, dd, 2)
    r1, l1 = P.reference32(c, P.take(dd, 1), 2)
    assert torch.equal(r2[1:2], r1) and torch.equal(l2[1:2], l1)


def test_conv_bound_is_the_kernel_tests_bound():
    torch.manual_seed(0)
    v, w = torch.randn(1, 32, 5, 7).double(), torch.randn(128, 32, 3, 3).double()
    assert torch.equal(P.conv_bound(v, w, 1, K.FAMILY), K.conv_bound(v, w, 1))
    assert float((P.conv_bound(v, w, 1, "h3") - P.conv_bound(v, w, 1, "x6")).min()) > 0          # the absolute term, h3 only


def test_gn_error_is_zero_for_exact_coefficients():
    torch.manual_seed(1)
    o = torch.randn(2, 64, 5, 6) + 3.0
    gamma, beta = 1 + 0.1 * torch.randn(64), 0.1 * torch.randn(64)
    g = o.double().reshape(2, 32, -1)
    mean, rstd = g.mean(-1), 1 / torch.sqrt(g.var(-1, unbiased=False) + 1e-5)
    coef = torch.stack([mean.repeat_interleave(2, 1), rstd.repeat_interleave(2, 1) * gamma.double(), beta.double().expand(2, 64)])
    assert P.gn_error(o, coef, gamma, beta) < 1e-12
    coef[0] += 1e-3
    assert P.gn_error(o, coef, gamma, beta) > 1e-4


def test_convolution_list_matches_the_synthetic_weights():
    """unet_convs (the port of build_program the workspace test walks) names exactly the 3x3 / 1x1 convolutions of the model's state dict,
    with their channel counts; a fused skip segment is the block's skip_connection"""
    synth = load_pkg("synth")
    import arch_cases as A
    for name, case in A.CASES.items():
        shapes = synth.unet_param_shapes(**A.synth_kw(case))
        convs = P.unet_convs(**A.unet_kw(case))
        seen = set()
        for lname, Cin, Cskip, Cout, taps, _ds in convs:
            shp = tuple(shapes[lname + ".weight"])
            assert shp[:2] == (Cout, Cin) and shp[2] == (1 if taps == 1 else 3), (name, lname, shp)
            seen.add(lname + ".weight")
            if Cskip:
                sk = lname.replace("out_layers.3", "skip_connection") + ".weight"
                assert tuple(shapes[sk])[:2] == (Cout, Cskip), (name, sk)
                seen.add(sk)
        planned = {k for k, s in shapes.items() if k.endswith(".weight") and len(s) >= 3 and k not in ("input_blocks.0.0.weight", "out.2.weight")}
        assert planned == seen, (name, sorted(planned ^ seen))
