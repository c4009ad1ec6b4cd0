"""GPU: cddpm_op_attention and cddpm_op_attention_backward (csrc/attention.hip) standalone at the token counts an attention inside the
resolution levels has -- N = H W tokens at level 0, not the H W / 16 of the middle block -- against float64 torch autograd of
QKVAttention (reference OpenAI_Unet.py:457-476). No bound fixed in advance: the same forward and the same vector-Jacobian product in
fp32 torch on the CPU give the yardstick (their distance from float64), and the device result is accepted within
arch_cases.YARD_FACTOR of it, tensor by tensor (out; dq, dk, dv)."""
import functools

import pytest
import torch

import arch_cases as A

pytestmark = pytest.mark.gpu

# (B, N, C): `attn_levels` level 0 (16 x 24 tokens, two heads); 12 x 20 tokens (a multiple of neither the 128-query workgroup nor the
# 64-key tile); four heads with 12 query tiles each. Then the edges of the staging, masking and row-store code that the fp32 and the
# fp16 kernels share: below one tile with N % 4 != 0; one key into the second tile (a fully masked 32-key sub-tile); the same with
# N % 4 != 0; a second workgroup with a single live query (the clamped row). fp32-vs-float64 yardsticks there: 2.8e-7 ... 1.2e-6
SHAPES = [(2, 384, 128), (2, 240, 128), (1, 1536, 256), (2, 15, 256), (1, 65, 64), (2, 67, 128), (1, 129, 128)]


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=24)


def _attention(qkv, ch=64):
    """QKVAttention.forward on [B, 3C, N]"""
    B, C3, N = qkv.shape
    heads = C3 // 3 // ch
    q, k, v = qkv.chunk(3, dim=1)
    s = 1 / (ch ** 0.25)
    w = torch.softmax(torch.einsum("bct,bcs->bts", (q * s).reshape(B * heads, ch, N), (k * s).reshape(B * heads, ch, N)), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v.reshape(B * heads, ch, N)).reshape(B, -1, N)


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """fp32 inputs; the forward and dL/dqkv for one upstream gradient in float64 and in fp32, computed once per shape"""
    B, N, C = shape
    g = torch.Generator().manual_seed(N + C)
    qkv = torch.randn(B, 3 * C, N, generator=g)
    da = torch.randn(B, C, N, generator=g)
    res = {"qkv": qkv, "da": da}
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        x = qkv.to(dt).requires_grad_(True)
        a = _attention(x)
        a.backward(da.to(dt))
        res["a" + key], res["d" + key] = a.detach(), x.grad
    return res


def _rows(parts, got, ref):
    rows = []
    for name, sl in parts:
        r64, r32, g = ref[0][:, sl], ref[1][:, sl], got[:, sl]
        err, yard = float((g.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
        rows.append((name, err, yard, float(r64.abs().max()), bool(err <= A.YARD_FACTOR * yard)))      # NaN fails
    return rows


def _nlc(x):
    return x.permute(0, 2, 1).contiguous().cuda()


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
