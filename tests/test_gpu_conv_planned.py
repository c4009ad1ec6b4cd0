"""GPU: the fused convolution as a HANDLE plans it, call by call against float64 (cddpm_op_conv_planned -> cddpm_api.hip::conv_launch):
the split-K range loop of the kernel (ranges inside the main segment, across the main / skip boundary, inside the skip segment and
across its two sources), the plane store, conv_reduce_kernel (fixed-order combine, bias, residual at the same and at half resolution,
its own statistics records with a tail record), hi_only with split-K on a precision-16 handle, and the 256-cout decision of the handle
plan exactly at its threshold. Cases, references and bounds: conv_plan_cases.py.

Every case first asserts the plan the launch REPORTS against the plan the case was written for -- a change of the rule fails here and
never silently moves a case off its path. Then, per case: the output against float64 element by element; batch independence (slice b of
the B = 2 call equals, bit for bit, the B = 1 call of that slice on the same handle); and the output written into the middle of a larger
buffer pre-filled with a sentinel bit pattern, whose two margins must come back untouched.

Lines `PARITY <case> <what> <max err / bound>` are printed for the record (profiles/conv_planned_parity.json)."""
import pytest
import torch

import conv_plan_cases as P
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5      # a quiet-NaN bit pattern no kernel writes
MARGIN = 4096              # floats in front of and behind the output (a multiple of 4: the kernels store float4)


def _engine(geom, **kw):
    mb, mh, mw = geom
    return load_pkg("engine").CddpmEngine(timesteps=50, max_batch=mb, max_h=mh, max_w=mw, **kw)


@pytest.fixture(scope="module")
def engines():
    """handles by (geometry, flavour), made on first use; no weights are loaded: the operator brings its own"""
    made = {}

    def get(geom, flavour="h3"):
        key = (geom, flavour)
        if key not in made:
            kw = {"p16": dict(precision=16), "x6": dict(conv_family="x6"), "h3": {}}[flavour]
            e = _engine(geom, **kw)
            assert e.conv_family == ("x6" if flavour == "x6" else "h3") and e.precision == (16 if flavour == "p16" else 32)
            made[key] = e
        return made[key]

    yield get
    for e in made.values():
        e.close()


def nhwc(x):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def run(eng, case, d, *, t=-1, guarded=False):
    """one cddpm_op_conv_planned call of the case's inputs d -> (out NCHW cpu, coef_out cpu | None, plan); guarded: into the middle of a
    sentinel-filled buffer whose margins are checked"""
    B = d["x"].shape[0]
    H, W, Cout, S0 = case["H"], case["W"], case["Cout"], case["S0"]
    n = B * H * W * Cout
    buf = out = None
    if guarded:
        buf = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        out = buf[MARGIN:MARGIN + n].view(B, H, W, Cout)
    sk = d["skip"]
    got, coef_out, plan = eng.op_conv_planned(
        nhwc(d["x"]), None, d["coef"].cuda().contiguous() if d["coef"] is not None else None, case["silu"], 2 if case["folded"] else 0,
        d["wt"], d["bias"], nhwc(d["res"]), case["res"] == "up", case["k"], img_hw=case["img"], t=t,
        skip0=nhwc(sk[:, :S0]) if S0 else None, skip1=nhwc(sk[:, S0:]) if case["S1"] else None, wskip=d["wskip"],
        gamma=d["gamma"], beta=d["beta"], out=out)
    torch.cuda.synchronize()
    if guarded:
        bits = buf.view(torch.int32)
        assert bool((bits[:MARGIN] == SENTINEL).all()) and bool((bits[MARGIN + n:] == SENTINEL).all()), f"{case['name']}: a margin of the output was written"
        assert not bool((bits[MARGIN:MARGIN + n] == SENTINEL).any()), f"{case['name']}: part of the output was not written"
    return nchw(got), (coef_out.cpu() if coef_out is not None else None), plan


def assert_plan(case, plan, *, family="h3", geom=None, nb2=False):
    """the plan the launch reports is the one the case was written for: S (the port's at this handle), chunk ranges the kernel can run
    with the property the case exists for, and the 256-cout flag. The exact bounds are the host test's business (test_conv_plan_host.py)."""
    nwg, S, _kb = P.case_plan(case, family, geom)
    assert plan["S"] == S, (case["name"], plan, S)
    if family == "h3" and (geom or case["geom"]) == case["geom"]:
        assert plan["S"] == case["expect_S"], (case["name"], plan)
    P.check_ranges(case, plan["S"], plan["kbound"], prop=family == "h3")
    assert plan["nb2"] is nb2, (case["name"], plan, nwg)
    return nwg


def ratio(name, what, got, ref, lim):
    err = (got.double() - ref).abs()
    r = float((err / lim).max())
    print(f"PARITY {name} {what} {r:.4f}")
    assert r <= 1.0, f"{name} {what}: max err/bound {r:.3f} (max err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e})"
    return r


def check_gn(case, d, out, coef_out, what):
    err = P.gn_error(out, coef_out, d["gamma"], d["beta"])
    lim = 1e-5 * (1 + case["gn_ratio"])
    print(f"PARITY {case['name']} {what}_groupnorm {err / lim:.4f}")
    assert err <= lim, f"{case['name']} {what}: normalised-value max err {err:.3e} > {lim:.3e}"


def check_case(eng, case, *, bits=32, family="h3"):
    """the three checks of every case on one handle -> the B = 2 output"""
    d = P.make_inputs(case)
    out, coef_out, plan = run(eng, case, d, guarded=True)
    assert_plan(case, plan, family=family)
    if bits == 16:
        assert plan["scale_exp"] > 0
        ref, lim = P.reference16(case, d, plan["scale_exp"])
    else:
        ref, lim = P.reference32(case, d, plan["S"], family)
    ratio(case["name"], f"p{bits}_{family}", out, ref, lim)
    if coef_out is not None:
        check_gn(case, d, out, coef_out, f"p{bits}_{family}")
    for b in range(case["B"]):
        one, coef_one, plan1 = run(eng, dict(case, B=1), P.take(d, b))
        assert (plan1["S"], plan1["kbound"], plan1["nb2"]) == (plan["S"], plan["kbound"], plan["nb2"]), "the plan is the handle's, not the call's"
        assert torch.equal(one.view(torch.int32), out[b:b + 1].contiguous().view(torch.int32)), f"{case['name']}: slice {b} depends on the batch it is in"
        if coef_out is not None:
            assert torch.equal(coef_one.view(torch.int32), coef_out[:, b:b + 1].contiguous().view(torch.int32)), f"{case['name']}: statistics of slice {b}"
    return out


@pytest.mark.parametrize("case", P.CASES_P, ids=[c["name"] for c in P.CASES_P])
def test_small_batch_plan_against_float64(engines, case):
    """handle P (max_batch 2 at 32 x 32): S = 4 / 8 / 8 with a skip segment of two sources / 2 folded / 2 in the 1x1 loop / 1"""
    check_case(engines(P.GEOM_P), case)


def test_ragged_layer_with_statistics_records_from_the_combine(engines):
    """12 x 20: H % 8, W % 32 and H W % 64 all non-zero, S = 4; the combine's statistics records (three full ones and a tail of 48 pixels)
    under a channel mean of 100 sigma"""
    case = P.CASE_RAGGED
    assert case["H"] % 8 and case["W"] % 32 and (case["H"] * case["W"]) % 64 and case["expect_S"] > 1 and case["gn_ratio"] == 100.0
    check_case(engines(P.GEOM_R), case)


@pytest.mark.parametrize("name", P.P16_NAMES)
def test_precision16_handle_takes_hi_only_through_split_k(engines, name):
    """a precision-16 handle at small batch: plain fp16 operands in every range of the split, against p16_forward_ref; and the result
    differs from the precision-32 handle's, so the mode is known to be on"""
    case = next(c for c in P.CASES_P if c["name"] == name)
    out16 = check_case(engines(P.GEOM_P, "p16"), case, bits=16)
    out32, _, _ = run(engines(P.GEOM_P), case, P.make_inputs(case))
    assert not torch.equal(out16, out32)
    assert float((out16 - out32).abs().max()) > 2.0 ** -14 * float(out32.abs().max())      # operand rounding 2^-11, far above fp32 noise


@pytest.mark.parametrize("case", P.CASES_Q, ids=[c["name"] for c in P.CASES_Q])
def test_handle_plan_takes_256_cout_workgroups_exactly_at_512(engines, case):
    """handle Q (max_batch 16 at 64 x 64): a Cout = 256 full-resolution layer has exactly 512 workgroups of the 128-cout form at the
    maximum geometry. With the accumulation switch at 0 a reverse step (t >= 0) runs the 256-cout form and a single forward (t = -1) the
    128-cout form; a sibling handle of max_batch 15 (480) runs the 128-cout form for both. B = 1 calls: the decision is the handle's."""
    d = P.make_inputs(case)
    ref, lim = P.reference32(case, d, 1)
    outs = {}
    for geom, tag in ((P.GEOM_Q, "q16"), (P.GEOM_Q15, "q15")):
        eng = engines(geom)
        eng.set_accumulation_switch(1 << 30)          # the default: off, no step wants the 256-cout form
        _, _, plan = run(eng, case, d, t=7)
        assert_plan(case, plan, geom=geom, nb2=False)
        eng.set_accumulation_switch(0)
        for t in (7, -1):
            want_nb2 = geom == P.GEOM_Q and t >= 0
            out, coef_out, plan = run(eng, case, d, t=t, guarded=True)
            nwg = assert_plan(case, plan, geom=geom, nb2=want_nb2)
            assert nwg == (512 if geom == P.GEOM_Q else 480) and plan["S"] == 1
            what = f"{tag}_t{t}_{'256' if want_nb2 else '128'}cout"
            ratio(case["name"], what, out, ref, lim)
            check_gn(case, d, out, coef_out, what)
            outs[(tag, t)] = out
    # the three 128-cout launches are one kernel on one input; the 256-cout form accumulates in two levels: other bits
    assert torch.equal(outs[("q16", -1)], outs[("q15", -1)]) and torch.equal(outs[("q15", 7)], outs[("q15", -1)])
    assert not torch.equal(outs[("q16", 7)], outs[("q16", -1)])


ALL_X6 = P.CASES_P + [P.CASE_RAGGED]


@pytest.mark.parametrize("case", ALL_X6, ids=[c["name"] for c in ALL_X6])
def test_x6_handle_never_splits(engines, case):
    """the exact bf16 three-term family through the same entry: S = 1 for every case, and conv_bound without the absolute term"""
    eng = engines(case["geom"], "x6")
    d = P.make_inputs(case)
    out, coef_out, plan = run(eng, case, d, guarded=True)
    assert_plan(case, plan, family="x6")
    assert plan["S"] == 1 and plan["scale_exp"] == 0
    ref, lim = P.reference32(case, d, 1, "x6")
    ratio(case["name"], "p32_x6", out, ref, lim)
    if coef_out is not None:
        check_gn(case, d, out, coef_out, "p32_x6")


def test_x6_handle_at_the_256_cout_threshold_keeps_128_cout_workgroups(engines):
    eng = engines(P.GEOM_Q, "x6")
    eng.set_accumulation_switch(0)
    for case in P.CASES_Q:
        d = P.make_inputs(case)
        out, coef_out, plan = run(eng, case, d, t=7)
        assert_plan(case, plan, family="x6", nb2=False)
        ref, lim = P.reference32(case, d, 1, "x6")
        ratio(case["name"], "q16_t7_x6", out, ref, lim)
        check_gn(case, d, out, coef_out, "q16_t7_x6")


def test_arguments_outside_the_handles_geometry_are_refused(engines):
    eng = engines(P.GEOM_P)
    case = P.CASES_P[0]
    d = P.make_inputs(dict(case, B=3))
    with pytest.raises(RuntimeError, match="outside the handle's geometry"):
        run(eng, dict(case, B=3), d)
    with pytest.raises(RuntimeError, match="outside the handle's geometry"):
        run(eng, dict(case, img=(64, 32)), P.make_inputs(case))
    # and the handle's state came back: the next call plans as before
    _, _, plan = run(eng, case, P.make_inputs(case))
    assert plan["S"] == case["expect_S"]
