"""GPU: the four attention operators (csrc/attention.hip: cddpm_op_attention, cddpm_op_attention_p16, cddpm_op_attention_backward,
cddpm_op_attention_backward_p16) away from N(0,1) inputs and at the edges of what they may touch. Inputs, references and the float64
model of the fp16 kernels come from attention_cases.py; the truth is float64 torch autograd of QKVAttention everywhere.

  regimes, fp32    peaked, shifted, late_key, first_key: per tensor (out; dq, dk, dv) the rule of arch_cases.block_ratios,
                   err <= max(REL_FLOOR max|ref64|, YARD_FACTOR yardstick), the yardstick being fp32 torch on the CPU against float64
  regimes, p16     peaked, shifted: precision16_cases.acceptance against fp16 autocast on the CPU, and the switch stays real (rms error
                   >= SWITCH x the fp32 operator's). late_key and first_key are NOT held to the autocast rule: with a near-one-hot
                   softmax the error is the rounding of one huge key, which the kernel and autocast round alike, so the ratio is a coin
                   toss. The float64 model of the kernels' own roundings (exact accumulation) already reads, model / autocast, at
                   (2,240,128), (1,130,64), (2,67,128):
                       flat 0.63-0.80 rms, 0.29-0.86 max    peaked 0.51-0.66, 0.31-0.84    shifted 0.07-0.18, 0.06-0.32
                       late_key up to 1.54, up to 1.82      first_key up to 1.13, up to 1.42
                   (tests/test_attention_cases_host.py asserts the first three below 0.9 / 1.5 and the last two above). There the p16
                   operators must be finite, deterministic, independent of the batch, and not grossly wrong: rms(err) <= rms(ref64).
  single token     (2,1,128), analytically: out = v, dv = dA bit for bit, dq and dk zero up to the difference of two dot products
  guard bands      every output written into the interior of a larger buffer: the guards keep their bits, every interior element
                   is written, the inputs keep theirs
  determinism, batch independence, non-finite isolation for the operators that had no such test
  refusals         B = 0, N = 0, C = 0, C = 96 and each NULL pointer, per operator: non-zero, a message, and the next call is right

The tile-edge shapes of the `flat` regime run in the SHAPES lists of test_gpu_attention_shapes.py, test_gpu_attention_backward_p16.py
and ATTN_SHAPES of test_gpu_precision16.py, under the rules of those files. Every test prints its rows before it asserts;
profiles/attention_regimes.json holds them as measured on an MI355X."""
import functools

import pytest
import torch

import arch_cases as A
import attention_cases as AC
import precision16_cases as P
from conftest import load_pkg
from test_gpu_precision16 import SWITCH

pytestmark = pytest.mark.gpu

REGIME_SHAPES = [(2, 240, 128), (1, 130, 64), (2, 67, 128)]
_id = lambda s: "x".join(map(str, s))
_cases = lambda regimes: [pytest.param(r, s, id=f"{r}-{_id(s)}") for r in regimes for s in REGIME_SHAPES]
# name -> (C ABI symbol, is backward, precision of the engine's wrapper)
OPERATORS = {"forward_32": ("cddpm_op_attention", False, 32), "forward_16": ("cddpm_op_attention_p16", False, 16),
             "backward_32": ("cddpm_op_attention_backward", True, 32), "backward_16": ("cddpm_op_attention_backward_p16", True, 16)}


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)


def _run(eng, op, qkv, da):
    """operator `op` of OPERATORS on device tensors [B, N, 3C], [B, N, C] -> device [B, N, C] or [B, N, 3C]"""
    _sym, backward, precision = OPERATORS[op]
    return eng.op_attention_backward(qkv, da, precision=precision) if backward else eng.op_attention(qkv, precision=precision)


def _host(x):
    return x.cpu().permute(0, 2, 1)


def _tensors(op, C):
    return AC.parts(C) if OPERATORS[op][1] else [("out", slice(None))]


def _truth(op, ref):
    """(float64 reference, fp32 yardstick, autocast yardstick) of the operator's output"""
    return (ref["d64"], ref["d32"], ref["amp_d"]) if OPERATORS[op][1] else (ref["a64"], ref["a32"], ref["amp_a"])


# ---------------------------------------------------------------------------------------------- 1. regimes
@pytest.mark.parametrize("op", ["forward_32", "backward_32"])
@pytest.mark.parametrize("regime, shape", _cases(["peaked", "shifted", "late_key", "first_key"]))
def test_regime_fp32(eng, op, regime, shape):
    ref = AC.reference(regime, shape)
    got = _host(_run(eng, op, AC.nlc(ref["qkv"]), AC.nlc(ref["da"])))
    r64, r32, _amp = _truth(op, ref)
    names = _tensors(op, shape[2])
    rows = A.block_ratios({n: got[:, sl] for n, sl in names}, {n: r64[:, sl] for n, sl in names}, {n: r32[:, sl] for n, sl in names},
                          [n for n, _sl in names])
    print(f"attention {op} {regime} {shape}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)


@pytest.mark.parametrize("op", ["forward_16", "backward_16"])
@pytest.mark.parametrize("regime, shape", _cases(["peaked", "shifted"]))
def test_regime_p16_is_autocast_grade_and_not_fp32(eng, op, regime, shape):
    ref = AC.reference(regime, shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    got, g32 = _host(_run(eng, op, qkv, da)), _host(_run(eng, op.replace("16", "32"), qkv, da))
    r64, _r32, amp = _truth(op, ref)
    rows, lines = [], []
    for name, sl in _tensors(op, shape[2]):
        row = P.acceptance(got[:, sl], dict(r64=r64[:, sl], amp=amp[:, sl]))
        e32 = P.rms(g32[:, sl].double() - r64[:, sl])
        rows.append((name, row, e32))
        lines.append(P.format_acceptance(f"attention {op} {regime} {shape} {name}", row) +
                     f"   rms / fp32 operator's rms {e32:.3e} = {row[0] / e32:.1f}")
    print("\n".join(lines))
    for name, row, e32 in rows:
        assert row[-1], "\n".join(lines)
        assert row[0] >= SWITCH * e32, (name, row[0], e32)


@pytest.mark.parametrize("op", ["forward_16", "backward_16"])
@pytest.mark.parametrize("regime, shape", _cases(AC.ONE_KEY))
def test_one_key_regime_p16_is_sane(eng, op, regime, shape):
    """not the autocast rule (see the module docstring): finite, deterministic, independent of the batch, rms(err) <= rms(ref64)"""
    ref = AC.reference(regime, shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    dev = _run(eng, op, qkv, da)
    got = _host(dev)
    r64, _r32, amp = _truth(op, ref)
    lines = []
    for name, sl in _tensors(op, shape[2]):
        row = P.acceptance(got[:, sl], dict(r64=r64[:, sl], amp=amp[:, sl]))
        lines.append((name, row[0], P.rms(r64[:, sl])))
        print(f"attention {op} {regime} {shape} {name}: rms {row[0]:.3e} / rms(ref64) {P.rms(r64[:, sl]):.3e}   for the record, not "
              f"asserted: rms / AMP reference {row[2]:.3e} = {row[0] / row[2]:.3f}   max {row[1]:.3e} / {row[3]:.3e} = {row[1] / row[3]:.3f}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(_run(eng, op, qkv, da), dev)
    for i in range(shape[0]):
        assert torch.equal(_run(eng, op, qkv[i:i + 1].contiguous(), da[i:i + 1].contiguous())[0], dev[i]), i
    for name, e, mag in lines:
        assert e <= mag, (name, e, mag)


# ---------------------------------------------------------------------------------------------- 2. a single token
@pytest.mark.parametrize("op", list(OPERATORS))
def test_single_token_is_the_identity(eng, op):
    """N = 1 (one live key, 63 masked; one live query, 127 clamped). The softmax is exactly 1, so out = v and dv = dA bit for bit --
    under precision 16 after their rounding to fp16, which the fp32 accumulators hold exactly. dq and dk are not exactly zero:
        dS = P (dP - D) with P = 1, dP = sum_c dA_c v_c (an MFMA dot product) and D = sum_c dA_c out_c = sum_c dA_c v_c (a VALU one):
        the same 64 products summed in two orders. Each fp32 sum is within 64 u sum_c |dA_c v_c| of the exact one (u = 2^-24: at most
        64 roundings, one per product or addition), so |dS| <= 2 . 64 . 2^-24 sum_c |dA_c v_c|, and with one live row the second
        products are single terms: |dq_c| = |dS k_c| / 8, |dk_c| = |dS q_c / 8|.
    Under precision 16 the products are of the rounded operands (fp16 x fp16 is exact in fp32) and q / 8 is rounded after the scaling."""
    B, N, C = shape = (2, 1, 128)
    qkv, da = AC.make_inputs("flat", shape)
    _sym, backward, precision = OPERATORS[op]
    got = _host(_run(eng, op, AC.nlc(qkv), AC.nlc(da)))
    h = (lambda x: x.half().float()) if precision == 16 else (lambda x: x)
    q, k, v = qkv.chunk(3, dim=1)
    if not backward:
        assert torch.equal(got, h(v))
        return
    dq, dk, dv = got.chunk(3, dim=1)
    assert torch.equal(dv, h(da))
    q8, k, v, dA = h(q * 0.125).double(), h(k).double(), h(v).double(), h(da).double()
    dS = 2 * 64 * 2.0 ** -24 * (dA * v).abs().reshape(B, C // 64, 64, N).sum(dim=2, keepdim=True)      # per (sample, head)
    dS = dS.expand(B, C // 64, 64, N).reshape(B, C, N)
    for name, g, bound in (("dq", dq, dS * k.abs() / 8), ("dk", dk, dS * q8.abs())):
        worst = float((g.double().abs() / bound).max())
        print(f"attention {op} {shape} {name}: max|{name}| {float(g.abs().max()):.3e}, at most {worst:.3f} of its bound")
        assert bool((g.double().abs() <= bound).all()), (name, worst)


# ---------------------------------------------------------------------------------------------- 3. guard bands
GUARD = 4096
SENTINEL = 0x7FC5A5A5       # a quiet NaN with a payload: no operator computes it


@pytest.mark.parametrize("op", list(OPERATORS))
@pytest.mark.parametrize("shape", [(2, 15, 256), (2, 67, 128), (1, 129, 128)], ids=_id)
def test_operator_writes_its_output_and_nothing_else(eng, op, shape):
    B, N, C = shape
    sym, backward, _precision = OPERATORS[op]
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    qkv0, da0 = qkv.clone(), da.clone()
    n_out = B * N * (3 * C if backward else C)
    buf = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.int32, device=qkv.device)
    out_ptr = buf.data_ptr() + 4 * GUARD
    stream = load_pkg("engine")._stream_ptr(eng.device)
    fn = getattr(eng.lib, sym)
    args = (qkv.data_ptr(), da.data_ptr(), out_ptr) if backward else (qkv.data_ptr(), out_ptr)
    assert fn(eng._h, *args, B, N, C, stream) == 0, eng.lib.cddpm_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()), "a store below the output"
    assert bool((buf[GUARD + n_out:] == SENTINEL).all()), "a store past the output"
    inner = buf[GUARD:GUARD + n_out]
    assert not bool((inner == SENTINEL).any()), "an output element was never written"
    assert torch.equal(qkv.view(torch.int32), qkv0.view(torch.int32)) and torch.equal(da.view(torch.int32), da0.view(torch.int32))
    assert torch.equal(inner.view(torch.float32).view(B, N, -1), _run(eng, op, qkv, da))


# ---------------------------------------------------------------------------------------------- 4. determinism, isolation
@pytest.mark.parametrize("op", ["forward_32", "backward_32", "forward_16"])        # backward_16: test_gpu_attention_backward_p16.py
@pytest.mark.parametrize("shape", [(2, 240, 128), (2, 15, 256)], ids=_id)
def test_operator_is_deterministic_and_a_sample_does_not_depend_on_its_batch(eng, op, shape):
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    both = _run(eng, op, qkv, da)
    assert torch.equal(_run(eng, op, qkv, da), both)
    for i in range(shape[0]):
        assert torch.equal(_run(eng, op, qkv[i:i + 1].contiguous(), da[i:i + 1].contiguous())[0], both[i]), i


POISON_SHAPE = (2, 240, 128)
# name -> (value, channel of qkv [B, 3C, N], token), in sample 1, head 1 of 2, a token of the second query block / third key tile
POISONS = {"inf_in_q": (float("inf"), 70, 130), "nan_in_v": (float("nan"), 2 * 128 + 70, 130)}


@functools.lru_cache(maxsize=None)
def _poisoned(poison):
    """(qkv, da, float64 forward, float64 dL/dqkv) of the flat inputs with one non-finite value in sample 1"""
    value, channel, token = POISONS[poison]
    qkv, da = AC.make_inputs("flat", POISON_SHAPE)
    qkv[1, channel, token] = value
    a64, d64 = AC.forward_backward(AC.attention, qkv.double(), da.double())
    return qkv, da, a64, d64


@pytest.mark.parametrize("op", list(OPERATORS))
@pytest.mark.parametrize("poison", list(POISONS))
def test_non_finite_sample_stays_in_its_sample_and_never_comes_out_finite(eng, op, poison):
    """inf in q: that query's logits are +-inf and its softmax is NaN -- its output row, its dq row and, through dS, every dk and dv of
    the head. NaN in v: one output channel of every query, so every D, dS, dq and dk of the head (dv does not read v)."""
    C = POISON_SHAPE[2]
    clean = AC.reference("flat", POISON_SHAPE)
    qkv, da, a64, d64 = _poisoned(poison)
    want = d64 if OPERATORS[op][1] else a64
    base = _run(eng, op, AC.nlc(clean["qkv"]), AC.nlc(clean["da"]))
    got = _run(eng, op, AC.nlc(qkv), AC.nlc(da))
    assert bool(torch.isfinite(base).all())
    assert torch.equal(got[0], base[0])                                   # the neighbour's bits
    bad = ~torch.isfinite(want)                                           # [B, channels, N]
    fin = torch.isfinite(_host(got))
    head1 = torch.zeros_like(bad)
    for t in range(want.shape[1] // C):
        head1[1, t * C + 64:t * C + 128] = True                           # sample 1, head 1 of q / k / v (or of the output)
    print(f"attention {op} {poison}: float64 non-finite {int(bad.sum())} of {bad.numel()}, device non-finite {int((~fin).sum())}")
    assert bool(bad.any()) and not bool((bad & ~head1).any())             # the reference: only there, and something there
    assert not bool((fin & bad).any()), f"{int((fin & bad).sum())} finite values where float64 has none"


# ---------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("op", list(OPERATORS))
def test_operator_refuses_bad_arguments_before_any_launch(eng, op):
    """every refusal returns non-zero with the operator's own message in cddpm_last_error and launches nothing (a NULL pointer or an
    empty grid never reaches the device); the same handle then computes the bits it computed before"""
    B, N, C = shape = (2, 15, 256)
    sym, backward, _precision = OPERATORS[op]
    ref = AC.reference("flat", shape)
    qkv, da = AC.nlc(ref["qkv"]), AC.nlc(ref["da"])
    before = _run(eng, op, qkv, da)
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
    assert torch.equal(_run(eng, op, qkv, da), before)
