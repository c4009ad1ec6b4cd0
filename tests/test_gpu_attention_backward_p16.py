"""GPU: cddpm_op_attention_backward_p16 (csrc/attention.hip: attention_bwd_q_p16_kernel, attention_bwd_kv_p16_kernel), the backward of
the attention core in the arithmetic of fp16 autocast, standalone. Truth is float64 torch autograd of QKVAttention (reference
OpenAI_Unet.py:457-476); the yardstick is the same function under torch.autocast("cpu", dtype=torch.float16) with the reference's
`softmax(weight.float()).type(weight.dtype)`, forward and backward, with the upstream gradient in fp16. dq, dk and dv are each accepted
by the rule of precision16_cases.acceptance (rms error <= 1.0 x the yardstick's, max error <= 2 x the yardstick's: the kernels round a
strict subset of what autocast rounds -- a CPU model of their arithmetic, operands rounded to fp16 and exact accumulation, reads rms
0.64-0.86 x and max 0.28-0.77 x the yardstick at these shapes), and the switch must be real: rms error >= SWITCH x that of the fp32
operator on the same input. Also: determinism, batch independence, the fp16 range of dA, and the unchanged default."""
import functools

import pytest
import torch

import precision16_cases as P
from conftest import load_pkg
from attention_cases import nlc as _nlc, reference      # d64: float64 autograd of attention_cases.attention
from test_gpu_precision16 import SWITCH

pytestmark = pytest.mark.gpu

# (B, N, C): N below one key tile; N a multiple of neither 128 nor 64; two heads, three query tiles; four heads, twelve query tiles; one
# head with two queries past a 128-query workgroup and two keys past a key tile. Then the tile boundaries, where the fp16 staging (4-key
# columns of the transposed images, zero rows past N) has the most to get wrong: one short of a tile and of a workgroup, exactly one and
# two tiles, one past each, N % 4 != 0 in a second tile. tests/test_attention_cases_host.py admits every one (none dropped)
SHAPES = [(2, 15, 256), (2, 240, 128), (2, 384, 128), (1, 1536, 256), (1, 130, 64),
          (1, 63, 64), (1, 64, 64), (1, 127, 64), (1, 128, 64), (1, 65, 64), (2, 67, 128), (1, 129, 128)]
_id = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)


_reference = functools.partial(reference, "flat")


def _yardstick(shape):
    """dL/dqkv [B, 3C, N] of fp16 autocast on the CPU for the inputs of _reference(shape), computed once per shape"""
    return _reference(shape)["amp_d"]


def _parts(C):
    return [("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_backward_p16_is_autocast_grade_and_not_fp32(eng, shape):
    ref, amp = _reference(shape), _yardstick(shape)
    qkv, da = _nlc(ref["qkv"].detach()), _nlc(ref["da"])
    got = eng.op_attention_backward(qkv, da, precision=16).cpu().permute(0, 2, 1)
    g32 = eng.op_attention_backward(qkv, da, precision=32).cpu().permute(0, 2, 1)
    rows, lines = [], []
    for name, sl in _parts(shape[2]):
        r64 = ref["d64"][:, sl]
        row = P.acceptance(got[:, sl], dict(r64=r64, amp=amp[:, sl]))
        e32 = P.rms(g32[:, sl].double() - r64)
        rows.append((name, row, e32))
        lines.append(P.format_acceptance(f"{shape} {name}", row) + f"   rms / fp32 operator's rms {e32:.3e} = {row[0] / e32:.1f}")
    print("\n".join(lines))
    for name, row, e32 in rows:
        assert row[-1], "\n".join(lines)
        assert row[0] >= SWITCH * e32, (name, row[0], e32)


def test_backward_p16_is_deterministic(eng):
    ref = _reference((2, 240, 128))
    qkv, da = _nlc(ref["qkv"].detach()), _nlc(ref["da"])
    a = eng.op_attention_backward(qkv, da, precision=16)
    b = eng.op_attention_backward(qkv, da, precision="16-mixed")
    assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 240, 128), (2, 15, 256)], ids=_id)
def test_backward_p16_sample_does_not_depend_on_its_batch(eng, shape):
    ref = _reference(shape)
    qkv, da = _nlc(ref["qkv"].detach()), _nlc(ref["da"])
    both = eng.op_attention_backward(qkv, da, precision=16)
    for i in range(shape[0]):
        one = eng.op_attention_backward(qkv[i:i + 1].contiguous(), da[i:i + 1].contiguous(), precision=16)
        assert torch.equal(one[0], both[i]), i


def test_backward_p16_leaves_the_fp16_range_as_autocast_does(eng):
    """|dA| >= 65504 rounds to +-inf: that sample's gradients are non-finite (never finite and wrong), the other sample's bits unchanged"""
    ref = _reference((2, 240, 128))
    qkv, da = _nlc(ref["qkv"].detach()), _nlc(ref["da"])
    clean = eng.op_attention_backward(qkv, da, precision=16)
    big = da.clone()
    big[1] = torch.where(da[1] >= 0, 1e5, -1e5)
    got = eng.op_attention_backward(qkv, big, precision=16)
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(got[0], clean[0])
    assert not bool(torch.isfinite(got[1]).any())


def test_default_backward_is_the_fp32_operator(eng):
    ref = _reference((2, 240, 128))
    qkv, da = _nlc(ref["qkv"].detach()), _nlc(ref["da"])
    B, N, C3 = qkv.shape
    direct = torch.empty_like(qkv)
    stream = load_pkg("engine")._stream_ptr(eng.device)
    assert eng.lib.cddpm_op_attention_backward(eng._h, qkv.data_ptr(), da.data_ptr(), direct.data_ptr(), B, N, C3 // 3, stream) == 0
    got = eng.op_attention_backward(qkv, da)
    assert torch.equal(got, direct)
    assert not torch.equal(got, eng.op_attention_backward(qkv, da, precision=16))
