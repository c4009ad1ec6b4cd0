"""GPU: cddpm_op_attention_h3 and cddpm_op_attention_backward_h3 (csrc/attention.hip), attention at fp32 accuracy on the fp16 matrix
pipe: two-term fp16 splits of q / 8, k, v, dA, P and dS, three products each, fp32 accumulators. The truth is float64 torch autograd of
QKVAttention (attention_cases.reference) throughout, and the bounds are the ones the EXACT fp32 operators are held to:

  tile edges       the 12 SHAPES of test_gpu_attention_shapes.py, flat regime, per tensor err <= YARD_FACTOR x (fp32 torch vs float64)
  regimes          all five of attention_cases.REGIMES at REGIME_SHAPES under arch_cases.block_ratios (test_regime_fp32's rule)
  gradient scale   dA x 2^-30, 2^-20, 2^10 on flat and late_key at (2, 240, 128): the outputs divided by the factor pass the rule of the
                   regimes, and equal the unscaled call's bits (the per-sample normalisation is an exact power of two)
  long rows        (1, 16384, 64), dA zero except on 256 spread query rows, against a float64 256 x 16384 block: the smallest N at
                   which a P operand formed against the row sum would go subnormal in fp16. Rule of the regimes, the yardstick being the
                   same block in fp32 torch; the other rows of dq are exact zeros
  single token     (2, 1, 128): out = v and dv = dA to 2^-20 elementwise (hi + 2^-11 lo carries 22 bits), dq and dk within the bound
                   test_gpu_attention_regimes.py::test_single_token_is_the_identity derives
  contract         guard bands, determinism, batch independence, non-finite isolation, refusals -- as test_gpu_attention_regimes.py
  the switch       h3 differs from the exact operators' bits, is at least 16 x closer to float64 than the p16 operators (a 2^-21-grade
                   and a 2^-11-grade arithmetic are three orders apart), and the family is per handle
The float64 model of the roundings (attention_h3_cases.h3_model, tests/test_attention_h3_host.py) leaves a factor above 5 of every bound
for the device's fp32 accumulation. Every test prints its rows before it asserts."""
import functools

import pytest
import torch

import arch_cases as A
import attention_cases as AC
import attention_h3_cases as H
from conftest import load_pkg
from test_gpu_attention_shapes import SHAPES

pytestmark = pytest.mark.gpu

REGIME_SHAPES = [(2, 240, 128), (1, 130, 64), (2, 67, 128)]
_id = lambda s: "x".join(map(str, s))
FWD, BWD = "cddpm_op_attention_h3", "cddpm_op_attention_backward_h3"


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)


def _fwd(eng, qkv, **kw):
    return eng.op_attention(qkv, family="h3", **kw)


def _bwd(eng, qkv, da, **kw):
    return eng.op_attention_backward(qkv, da, family="h3", **kw)


def _run(eng, backward, qkv, da):
    return _bwd(eng, qkv, da) if backward else _fwd(eng, qkv)


def _host(x):
    return x.cpu().permute(0, 2, 1)


def _got(eng, ref, scale=1.0):
    """{out, dq, dk, dv} of the two h3 operators on a reference's inputs, on the host as [B, channels, N]; dA times `scale`, undone"""
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"] * scale)
    return H.tensors(_host(_fwd(eng, qkv)), _host(_bwd(eng, qkv, da)) / scale, ref["da"].shape[1])


NAMES = ["out", "dq", "dk", "dv"]


# ---------------------------------------------------------------------------------------------- 1. tile edges, regimes, gradient scale
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_tile_edges_under_the_exact_operators_rule(eng, shape):
    ref = AC.reference("flat", shape)
    r64, r32 = H.truths(ref, shape[2])
    rows = H.strict_rows(_got(eng, ref), r64, r32, NAMES)
    print(f"attention h3 flat {shape}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)


@pytest.mark.parametrize("shape", REGIME_SHAPES, ids=_id)
@pytest.mark.parametrize("regime", AC.REGIMES)
def test_regimes(eng, regime, shape):
    ref = AC.reference(regime, shape)
    r64, r32 = H.truths(ref, shape[2])
    rows = A.block_ratios(_got(eng, ref), r64, r32, NAMES)
    print(f"attention h3 {regime} {shape}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)


@pytest.mark.parametrize("exponent", [-30, -20, 10])
@pytest.mark.parametrize("regime", ["flat", "late_key"])
def test_gradient_scale(eng, regime, exponent):
    shape = (2, 240, 128)
    ref = AC.reference(regime, shape)
    r64, r32 = H.truths(ref, shape[2])
    f = 2.0 ** exponent
    got = _got(eng, ref, scale=f)
    rows = A.block_ratios(got, r64, r32, NAMES)[1:]
    print(f"attention h3 backward {regime} {shape}, dA x 2^{exponent}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)
    base = _got(eng, ref)
    for n in NAMES[1:]:
        assert torch.equal(got[n], base[n]), n


# ---------------------------------------------------------------------------------------------- 2. long rows
LONG = (1, 16384, 64)
LONG_ROWS = 256


@functools.lru_cache(maxsize=None)
def _long_reference():
    """qkv, da (zero except on LONG_ROWS spread query rows) of LONG and, per dtype, the attention of those rows only: a 256 x 16384 block"""
    B, N, C = LONG
    qkv, da = AC.make_inputs("flat", LONG)
    rows = torch.arange(LONG_ROWS) * (N // LONG_ROWS) + 13
    keep = torch.zeros(N, dtype=torch.bool)
    keep[rows] = True
    da[:, :, ~keep] = 0.0
    res = {"qkv": qkv, "da": da, "rows": rows}
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        q, k, v = (t[0].to(dt) for t in qkv.chunk(3, dim=1))                 # [C, N]
        qr, dar = q[:, rows] * 0.125, da[0][:, rows].to(dt)                  # [C, R]
        P = torch.softmax(qr.T @ k, dim=-1)                                  # [R, N]
        out = P @ v.T                                                        # [R, C]
        dS = P * (dar.T @ v - (dar.T * out).sum(dim=1, keepdim=True))
        res[key] = {"out": out.T, "dq": (dS @ k.T).T * 0.125, "dk": qr @ dS, "dv": dar @ P}       # [C, R], [C, R], [C, N], [C, N]
    return res


def test_long_rows(engine_factory):
    eng = engine_factory(timesteps=50, max_batch=1, max_h=128, max_w=128)
    ref = _long_reference()
    C, rows = LONG[2], ref["rows"]
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    out, d = _host(_fwd(eng, qkv))[0], _host(_bwd(eng, qkv, da))[0]
    dq = d[:C]
    got = {"out": out[:, rows], "dq": dq[:, rows], "dk": d[C:2 * C], "dv": d[2 * C:]}
    table = A.block_ratios(got, ref["64"], ref["32"], NAMES)
    print(f"attention h3 {LONG}, {LONG_ROWS} live rows:\n" + A.format_ratios(table))
    assert all(r[-1] for r in table), A.format_ratios(table)
    other = torch.ones(LONG[1], dtype=torch.bool)
    other[rows] = False
    assert bool((dq[:, other] == 0).all()), "a query row without an upstream gradient has a non-zero dq"
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------- 3. a single token
def test_single_token(eng):
    """N = 1: P = 1, so out = v and dv = dA up to the split (hi + 2^-11 lo keeps 22 bits: 2^-20 with room); dq and dk are the difference
    of two summations of the same 64 products, as for the exact operator"""
    B, N, C = shape = (2, 1, 128)
    qkv, da = AC.make_inputs("flat", shape)
    dev_qkv, dev_da = AC.nlc(qkv), AC.nlc(da)
    out, d = _host(_fwd(eng, dev_qkv)), _host(_bwd(eng, dev_qkv, dev_da))
    q, k, v = qkv.chunk(3, dim=1)
    dq, dk, dv = d.chunk(3, dim=1)
    print(f"attention h3 {shape}: max|out - v| / |v| {float(((out - v).abs() / v.abs()).max()):.3e}, "
          f"max|dv - dA| / |dA| {float(((dv - da).abs() / da.abs()).max()):.3e}")
    assert bool(((out - v).abs() <= 2.0 ** -20 * v.abs()).all())
    assert bool(((dv - da).abs() <= 2.0 ** -20 * da.abs()).all())
    dS = 2 * 64 * 2.0 ** -24 * (da.double() * v.double()).abs().reshape(B, C // 64, 64, N).sum(dim=2, keepdim=True)
    dS = dS.expand(B, C // 64, 64, N).reshape(B, C, N)
    for name, g, bound in (("dq", dq, dS * k.double().abs() / 8), ("dk", dk, dS * (q.double() * 0.125).abs())):
        worst = float((g.double().abs() / bound).max())
        print(f"attention h3 {shape} {name}: max|{name}| {float(g.abs().max()):.3e}, at most {worst:.3f} of its bound")
        assert bool((g.double().abs() <= bound).all()), (name, worst)


# ---------------------------------------------------------------------------------------------- 4. contract checks
GUARD = 4096
SENTINEL = 0x7FC5A5A5       # a quiet NaN with a payload: no operator computes it


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("shape", [(2, 15, 256), (2, 67, 128), (1, 129, 128)], ids=_id)
def test_operator_writes_its_output_and_nothing_else(eng, backward, shape):
    B, N, C = shape
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    qkv0, da0 = qkv.clone(), da.clone()
    n_out = B * N * (3 * C if backward else C)
    buf = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.int32, device=qkv.device)
    out_ptr = buf.data_ptr() + 4 * GUARD
    stream = load_pkg("engine")._stream_ptr(eng.device)
    fn = getattr(eng.lib, BWD if backward else FWD)
    args = (qkv.data_ptr(), da.data_ptr(), out_ptr) if backward else (qkv.data_ptr(), out_ptr)
    assert fn(eng._h, *args, B, N, C, stream) == 0, eng.lib.cddpm_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()), "a store below the output"
    assert bool((buf[GUARD + n_out:] == SENTINEL).all()), "a store past the output"
    inner = buf[GUARD:GUARD + n_out]
    assert not bool((inner == SENTINEL).any()), "an output element was never written"
    assert torch.equal(qkv.view(torch.int32), qkv0.view(torch.int32)) and torch.equal(da.view(torch.int32), da0.view(torch.int32))
    assert torch.equal(inner.view(torch.float32).view(B, N, -1), _run(eng, backward, qkv, da))


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("shape", [(2, 240, 128), (2, 15, 256)], ids=_id)
def test_operator_is_deterministic_and_a_sample_does_not_depend_on_its_batch(eng, backward, shape):
    """the backward's dA normalisation is per sample: slice 1 alone, and slice 1 next to a slice whose dA is 2^12 times larger, give
    slice 1's bits"""
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    both = _run(eng, backward, qkv, da)
    assert torch.equal(_run(eng, backward, qkv, da), both)
    for i in range(shape[0]):
        assert torch.equal(_run(eng, backward, qkv[i:i + 1].contiguous(), da[i:i + 1].contiguous())[0], both[i]), i
    if backward:
        loud = da.clone()
        loud[0] *= 4096.0
        assert torch.equal(_bwd(eng, qkv, loud)[1], both[1])


POISON_SHAPE = (2, 240, 128)
# name -> (value, tensor, channel, token) in sample 0, head 1 of 2, a token of the second query block / third key tile
POISONS = {"inf_in_q": (float("inf"), "qkv", 70, 130), "nan_in_v": (float("nan"), "qkv", 2 * 128 + 70, 130),
           "inf_in_dA": (float("inf"), "da", 70, 130)}


@functools.lru_cache(maxsize=None)
def _poisoned(poison):
    value, which, channel, token = POISONS[poison]
    qkv, da = AC.make_inputs("flat", POISON_SHAPE)
    (qkv if which == "qkv" else da)[0, channel, token] = value
    a64, d64 = AC.forward_backward(AC.attention, qkv.double(), da.double())
    return qkv, da, a64, d64


@pytest.mark.parametrize("backward, poison", [(b, p) for p in POISONS for b in (False, True) if b or POISONS[p][1] == "qkv"],
                         ids=lambda v: v if isinstance(v, str) else "backward" if v else "forward")
def test_non_finite_sample_stays_in_its_sample_and_never_comes_out_finite(eng, backward, poison):
    """an inf or a NaN in sample 0's qkv, or an inf in its dA (the backward; the forward does not read dA), leaves sample 1's bits as
    they are, and nothing comes out finite where float64 has a non-finite value"""
    clean = AC.reference("flat", POISON_SHAPE)
    qkv, da, a64, d64 = _poisoned(poison)
    want = d64 if backward else a64
    base = _run(eng, backward, AC.nlc(clean["qkv"]), AC.nlc(clean["da"]))
    got = _run(eng, backward, AC.nlc(qkv), AC.nlc(da))
    assert bool(torch.isfinite(base).all())
    assert torch.equal(got[1], base[1])                                   # the neighbour's bits
    bad = ~torch.isfinite(want)                                           # [B, channels, N]
    fin = torch.isfinite(_host(got))
    print(f"attention h3 {'backward' if backward else 'forward'} {poison}: float64 non-finite {int(bad.sum())} of {bad.numel()}, "
          f"device non-finite {int((~fin).sum())}")
    assert bool(bad[0].any()) and not bool(bad[1].any())
    assert not bool((fin & bad).any()), f"{int((fin & bad).sum())} finite values where float64 has none"


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_operator_refuses_bad_arguments_before_any_launch(eng, backward):
    B, N, C = shape = (2, 15, 256)
    sym = BWD if backward else FWD
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    before = _run(eng, backward, qkv, da)
    out = torch.empty_like(before)
    stream = load_pkg("engine")._stream_ptr(eng.device)
    fn = getattr(eng.lib, sym)
    ptrs = [qkv.data_ptr(), da.data_ptr(), out.data_ptr()] if backward else [qkv.data_ptr(), out.data_ptr()]
    bad = [("B = 0", ptrs, (0, N, C)), ("N = 0", ptrs, (B, 0, C)), ("C = 0", ptrs, (B, N, 0)), ("C = 96", ptrs, (B, N, 96))]
    bad += [(f"pointer {i} NULL", ptrs[:i] + [None] + ptrs[i + 1:], (B, N, C)) for i in range(len(ptrs))]
    for what, p, dims in bad:
        assert fn(eng._h, *p, *dims, stream) != 0, what
        msg = eng.lib.cddpm_last_error(eng._h).decode()
        print(f"{sym} {what}: {msg}")
        assert msg.startswith(sym + ":"), (what, msg)
        assert ("NULL" in msg) == ("NULL" in what), (what, msg)
    assert fn(None, *ptrs, B, N, C, stream) == -1                          # no handle: refused, no message to leave
    assert fn(eng._h, *ptrs, B, N, C, stream) == 0, eng.lib.cddpm_last_error(eng._h).decode()
    assert torch.equal(out, before)
    assert torch.equal(_run(eng, backward, qkv, da), before)


# ---------------------------------------------------------------------------------------------- 5. the switch is real
SEPARATION = 16.0


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_h3_is_neither_the_exact_nor_the_p16_arithmetic(eng, regime):
    shape = (2, 240, 128)
    ref = AC.reference(regime, shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    r64 = H.truths(ref, shape[2])[0]
    rms = lambda x: float(x.double().pow(2).mean().sqrt())
    three = {}
    for label, kw in (("f32", {}), ("h3", dict(family="h3")), ("p16", dict(precision=16))):
        three[label] = H.tensors(_host(eng.op_attention(qkv, **kw)), _host(eng.op_attention_backward(qkv, da, **kw)), shape[2])
    for n in NAMES:
        e = {label: rms(three[label][n].double() - r64[n]) for label in three}
        print(f"attention {regime} {shape} {n}: rms error vs float64  f32 {e['f32']:.3e}  h3 {e['h3']:.3e}  p16 {e['p16']:.3e}  "
              f"p16 / h3 {e['p16'] / e['h3']:.0f}")
        assert not torch.equal(three["h3"][n], three["f32"][n]), n
        assert SEPARATION * e["h3"] <= e["p16"], (n, e)
    # precision 16 wins over the family, as on a handle
    assert torch.equal(eng.op_attention(qkv, precision=16, family="h3"), eng.op_attention(qkv, precision=16))
    assert torch.equal(eng.op_attention_backward(qkv, da, precision=16, family="h3"), eng.op_attention_backward(qkv, da, precision=16))


def test_the_family_is_per_handle_and_x6_is_refused(eng, engine_factory, synth):
    B, Hh, W = 2, 16, 24
    x = torch.from_numpy(synth.noise_xT(2, 0, B, Hh, W)).cuda()
    cond = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
    assert eng.attention_family == "f32"
    before = eng.unet_forward(x, 25, cond)
    other = engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)
    other.set_attention_family("h3")
    assert other.attention_family == "h3" and eng.attention_family == "f32"
    split = other.unet_forward(x, 25, cond)
    assert torch.equal(eng.unet_forward(x, 25, cond), before)
    assert not torch.equal(split, before) and float((split - before).abs().max()) < 1e-4
    code = load_pkg("engine").CONV_FAMILIES
    assert other.lib.cddpm_set_attention_family(other._h, code["x6"]) != 0
    msg = other.lib.cddpm_last_error(other._h).decode()
    assert msg.startswith("cddpm_set_attention_family:") and "x6" in msg, msg
    assert other.lib.cddpm_set_attention_family(other._h, 7) != 0 and other.attention_family == "h3"
    other.set_attention_family("f32")
    assert torch.equal(other.unet_forward(x, 25, cond), before)
