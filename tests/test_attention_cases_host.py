"""Host side of the attention operator tests (no GPU): the conditions tests/test_gpu_attention_regimes.py and the three attention files
that share attention_cases.py rest on. `flat` inputs are the ones those files always drew; every yardstick is finite and non-zero; and
every (regime, shape) that a precision-16 acceptance is asserted at is ADMITTED: attention_cases.p16_model -- the kernels' roundings
with exact accumulation -- itself passes precision16_cases.acceptance with rms ratio <= 0.9 and max ratio <= 1.5. That is a condition on
the case, not a tolerance: the device adds only fp32 accumulation and the online softmax's re-rounding to the model, so a case where
the model alone has no headroom would test the random draw and not the kernel.

Model / autocast ratios measured on the CPU, rms and max, over out, dq, dk, dv at (2,240,128), (1,130,64), (2,67,128):
    flat       0.63-0.80   0.29-0.86    admitted       (all eight tile-edge shapes and (2,15,256): 0.63-0.86 / 0.28-0.94, none dropped)
    peaked     0.51-0.66   0.31-0.84    admitted
    shifted    0.07-0.18   0.06-0.32    admitted       autocast rounds fp16 logits near 72, where one ulp is 0.06
    late_key   up to 1.54  up to 1.82   excluded       a near-one-hot softmax: the error is the rounding of one huge key, which the
    first_key  up to 1.13  up to 1.42   excluded       kernel and autocast round alike -- the ratio is a coin toss"""
import pytest
import torch

import attention_cases as AC
import precision16_cases as P

REGIME_SHAPES = [(2, 240, 128), (1, 130, 64), (2, 67, 128)]
EDGE_SHAPES = [(1, 63, 64), (1, 64, 64), (1, 127, 64), (1, 128, 64), (1, 65, 64), (2, 67, 128), (1, 129, 128), (1, 130, 64)]
# every (regime, shape) a precision-16 acceptance is asserted at by test_gpu_attention_regimes.py (peaked, shifted) and, at the tile
# edges, by test_gpu_attention_backward_p16.py and test_gpu_precision16.py (flat)
P16_ADMITTED = [(r, s) for r in ("peaked", "shifted") for s in REGIME_SHAPES] + [("flat", s) for s in EDGE_SHAPES + [(2, 240, 128), (2, 15, 256)]]
ADMIT_RMS, ADMIT_MAX = 0.9, 1.5
_id = lambda c: c[0] + "-" + "x".join(map(str, c[1]))


def model_rows(regime, shape):
    """[(tensor, acceptance row of p16_model against the autocast yardstick)] for out, dq, dk, dv; at `flat` also the forward against
    torch fp16 on the CPU, the yardstick of test_gpu_precision16.py::test_attention_p16_operator"""
    ref = AC.reference(regime, shape)
    out, dqkv = AC.p16_model(ref["qkv"], ref["da"])
    rows = [("out", P.acceptance(out, dict(r64=ref["a64"], amp=ref["amp_a"])))]
    if regime == "flat":
        with torch.no_grad():
            rows.append(("out/fp16", P.acceptance(out, dict(r64=ref["a64"], amp=AC.attention(ref["qkv"].half()).double()))))
    rows += [(n, P.acceptance(dqkv[:, sl], dict(r64=ref["d64"][:, sl], amp=ref["amp_d"][:, sl]))) for n, sl in AC.parts(shape[2])]
    return rows


def test_flat_inputs_are_the_ones_the_attention_tests_always_drew():
    for shape in [(2, 240, 128), (1, 65, 64), (2, 15, 256)]:
        B, N, C = shape
        g = torch.Generator().manual_seed(N + C)
        qkv = torch.randn(B, 3 * C, N, generator=g)
        da = torch.randn(B, C, N, generator=g)
        got = AC.make_inputs("flat", shape)
        assert torch.equal(got[0], qkv) and torch.equal(got[1], da)
        ref = AC.reference("flat", shape)
        assert torch.equal(ref["qkv"], qkv) and torch.equal(ref["da"], da)
        assert AC.reference("flat", shape) is ref                       # computed once


def test_regimes_change_only_what_they_say():
    shape = (2, 67, 128)
    B, N, C = shape
    flat, da = AC.make_inputs("flat", shape)
    for regime in AC.REGIMES[1:]:
        x, d = AC.make_inputs(regime, shape)
        assert torch.equal(d, da) and torch.equal(x[:, 2 * C:], flat[:, 2 * C:]), regime          # dA and v untouched
        assert not torch.equal(x, flat)
    assert torch.equal(AC.make_inputs("peaked", shape)[0][:, :2 * C], flat[:, :2 * C] * 2.0)
    assert torch.equal(AC.make_inputs("shifted", shape)[0][:, :2 * C], flat[:, :2 * C] + 3.0)
    for regime, key in (("late_key", N - 1), ("first_key", 0)):
        x = AC.make_inputs(regime, shape)[0]
        same = torch.ones(N, dtype=torch.bool)
        same[key] = False
        assert torch.equal(x[:, :, same], flat[:, :, same]) and torch.equal(x[:, :C], flat[:, :C])
        assert torch.equal(x[:, C:2 * C, key], flat[:, C:2 * C, key] * 25.0)
    with pytest.raises(AssertionError):
        AC.make_inputs("sharp", shape)


@pytest.mark.parametrize("regime", AC.REGIMES)
def test_every_yardstick_is_finite_and_non_zero(regime):
    for shape in REGIME_SHAPES:
        ref = AC.reference(regime, shape)
        pairs = [("a32", "a64", slice(None)), ("amp_a", "a64", slice(None))]
        pairs += [(y, "d64", sl) for y in ("d32", "amp_d") for _n, sl in AC.parts(shape[2])]
        for y, truth, sl in pairs:
            assert bool(torch.isfinite(ref[y]).all()) and bool(torch.isfinite(ref[truth]).all()), (regime, shape, y)
            d = float((ref[y][:, sl].double() - ref[truth][:, sl]).abs().max())
            assert 0.0 < d < 0.5 * float(ref[truth][:, sl].abs().max()), (regime, shape, y, d)


def test_the_model_is_exact_where_fp16_is():
    """inputs that fp16 holds exactly and a one-key softmax (N = 1): the model's forward is v, its dv is dA, dq = dk = 0"""
    qkv, da = AC.make_inputs("flat", (2, 1, 128))
    qkv, da = qkv.half().float(), da.half().float()
    out, dqkv = AC.p16_model(qkv, da)
    assert torch.equal(out, qkv[:, 256:].double()) and torch.equal(dqkv[:, 256:], da.double())
    assert float(dqkv[:, :256].abs().max()) < 1e-12                     # two float64 summation orders of one 64-term dot product


@pytest.mark.parametrize("case", P16_ADMITTED, ids=_id)
def test_p16_model_admits_the_case(case):
    rows = model_rows(*case)
    print("\n".join(P.format_acceptance(f"model {case[0]} {case[1]} {n}", r) for n, r in rows))
    for n, r in rows:
        assert r[0] <= ADMIT_RMS * r[2] and r[1] <= ADMIT_MAX * r[3], P.format_acceptance(f"{case} {n}", r)


def test_one_key_regimes_are_not_admitted():
    """why test_gpu_attention_regimes.py holds late_key and first_key to no autocast rule under precision 16: at every one of these
    shapes some tensor of the model already misses the admission condition"""
    for regime in AC.ONE_KEY:
        for shape in REGIME_SHAPES:
            rows = model_rows(regime, shape)
            assert any(r[0] > ADMIT_RMS * r[2] or r[1] > ADMIT_MAX * r[3] for _n, r in rows), (regime, shape)
