"""GPU: cddpm_op_attention and cddpm_op_attention_backward (csrc/attention.hip) standalone at the token counts an attention inside the
resolution levels has -- N = H W tokens at level 0, not the H W / 16 of the middle block -- against float64 torch autograd of
QKVAttention (reference OpenAI_Unet.py:457-476). No bound fixed in advance: the same forward and the same vector-Jacobian product in
fp32 torch on the CPU give the yardstick (their distance from float64), and the device result is accepted within
arch_cases.YARD_FACTOR of it, tensor by tensor (out; dq, dk, dv)."""
import functools

import pytest

import arch_cases as A
from attention_cases import nlc as _nlc, reference

pytestmark = pytest.mark.gpu

# (B, N, C): `attn_levels` level 0 (16 x 24 tokens, two heads); 12 x 20 tokens (a multiple of neither the 128-query workgroup nor the
# 64-key tile); four heads with 12 query tiles each. Then the edges of the staging, masking and row-store code that the fp32 and the
# fp16 kernels share: below one tile with N % 4 != 0; one key into the second tile (a fully masked 32-key sub-tile); the same with
# N % 4 != 0; a second workgroup with a single live query (the clamped row). fp32-vs-float64 yardsticks there: 2.8e-7 ... 1.2e-6. Then
# the tile boundaries themselves: one key short of a tile and of a workgroup, exactly one and two tiles, two queries and keys past both
SHAPES = [(2, 384, 128), (2, 240, 128), (1, 1536, 256), (2, 15, 256), (1, 65, 64), (2, 67, 128), (1, 129, 128),
          (1, 63, 64), (1, 64, 64), (1, 127, 64), (1, 128, 64), (1, 130, 64)]


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)


_reference = functools.partial(reference, "flat")      # fp32 inputs; the forward and dL/dqkv in float64 and in fp32, once per shape


def _rows(parts, got, ref):
    rows = []
    for name, sl in parts:
        r64, r32, g = ref[0][:, sl], ref[1][:, sl], got[:, sl]
        err, yard = float((g.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
        rows.append((name, err, yard, float(r64.abs().max()), bool(err <= A.YARD_FACTOR * yard)))      # NaN fails
    return rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_forward_at_level_token_counts(eng, shape):
    ref = _reference(shape)
    got = eng.op_attention(_nlc(ref["qkv"])).cpu().permute(0, 2, 1)
    rows = _rows([("out", slice(None))], got, (ref["a64"], ref["a32"]))
    print(f"attention forward {shape}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_backward_at_level_token_counts(eng, shape):
    ref = _reference(shape)
    C = shape[2]
    got = eng.op_attention_backward(_nlc(ref["qkv"]), _nlc(ref["da"])).cpu().permute(0, 2, 1)
    parts = [("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))]
    rows = _rows(parts, got, (ref["d64"], ref["d32"]))
    print(f"attention backward {shape}:\n" + A.format_ratios(rows))
    assert all(r[-1] for r in rows), A.format_ratios(rows)
