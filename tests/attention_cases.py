"""What the attention operator tests share (tests/test_gpu_attention_shapes.py, test_gpu_attention_backward_p16.py, test_gpu_precision16.py,
test_gpu_attention_regimes.py, test_attention_cases_host.py): QKVAttention (reference OpenAI_Unet.py:457-476) on the CPU, seeded inputs in
five regimes of the logits, per (regime, shape) the references every acceptance is stated in, computed once per process and never
modified, and a float64 model of what the fp16-MFMA kernels round. Nothing here needs a GPU except nlc().

Regimes (the logits are q . k / 8 over 64 channels; `flat` is what every test drew before there were regimes):
    flat       qkv ~ N(0,1): logits ~ N(0,1), an almost flat softmax, the running maximum settles in the first key tile
    peaked     q, k doubled: logits ~ N(0,16)
    shifted    q, k + 3: logits 72 +- 4, a large common offset (cancellation in S - m and S - lse)
    late_key   the LAST key x 25: the dominant key sits in the last (partly masked when N % 64 != 0) tile, the running maximum jumps
               there and alpha underflows
    first_key  the FIRST key x 25: the maximum is settled in tile 0 and every later tile has p near 0
"""
import functools

import torch

REGIMES = ("flat", "peaked", "shifted", "late_key", "first_key")
ONE_KEY = ("late_key", "first_key")


def attention(qkv, ch=64):
    """QKVAttention.forward on [B, 3C, N]"""
    B, C3, N = qkv.shape
    heads = C3 // 3 // ch
    q, k, v = qkv.chunk(3, dim=1)
    s = 1 / (ch ** 0.25)
    w = torch.softmax(torch.einsum("bct,bcs->bts", (q * s).reshape(B * heads, ch, N), (k * s).reshape(B * heads, ch, N)), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v.reshape(B * heads, ch, N)).reshape(B, -1, N)


def attention_autocast(qkv, ch=64):
    """attention() as the reference writes it for autocast: the softmax in fp32, cast back to the weights' dtype"""
    B, C3, N = qkv.shape
    heads = C3 // 3 // ch
    q, k, v = qkv.chunk(3, dim=1)
    s = 1 / (ch ** 0.25)
    w = torch.einsum("bct,bcs->bts", (q * s).reshape(B * heads, ch, N), (k * s).reshape(B * heads, ch, N))
    w = torch.softmax(w.float(), dim=-1).type(w.dtype)
    return torch.einsum("bts,bcs->bct", w, v.reshape(B * heads, ch, N)).reshape(B, -1, N)


def nlc(x):
    """[B, channels, N] on the host -> the operators' [B, N, channels] on the device"""
    return x.permute(0, 2, 1).contiguous().cuda()


def parts(C):
    return [("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))]


def make_inputs(regime, shape):
    """(qkv [B, 3C, N], da [B, C, N]) fp32 for shape = (B, N, C)"""
    B, N, C = shape
    g = torch.Generator().manual_seed(N + C)
    qkv = torch.randn(B, 3 * C, N, generator=g)
    da = torch.randn(B, C, N, generator=g)
    if regime == "peaked":
        qkv[:, :2 * C] *= 2.0
    elif regime == "shifted":
        qkv[:, :2 * C] += 3.0
    elif regime == "late_key":
        qkv[:, C:2 * C, N - 1] *= 25.0
    elif regime == "first_key":
        qkv[:, C:2 * C, 0] *= 25.0
    else:
        assert regime == "flat", regime
    return qkv, da


def forward_backward(fn, qkv, da):
    """(fn(qkv), dL/dqkv for the upstream gradient da) on a leaf of its own"""
    x = qkv.detach().clone().requires_grad_(True)
    a = fn(x)
    a.backward(da.to(a.dtype))
    return a.detach(), x.grad


@functools.lru_cache(maxsize=None)
def reference(regime, shape):
    """fp32 inputs `qkv`, `da`; the forward and dL/dqkv in float64 (`a64`, `d64`: the truth) and in fp32 (`a32`, `d32`: the yardstick of
    the fp32 operators), and under torch.autocast("cpu", dtype=torch.float16) with the upstream gradient in fp16 (`amp_a`, `amp_d`, as
    fp32: the yardstick of the fp16 operators)"""
    qkv, da = make_inputs(regime, shape)
    res = {"qkv": qkv, "da": da}
    for key, dt in (("64", torch.float64), ("32", torch.float32)):
        res["a" + key], res["d" + key] = forward_backward(attention, qkv.to(dt), da.to(dt))

    def amp(x):
        with torch.autocast("cpu", dtype=torch.float16):
            a = attention_autocast(x)
        assert a.dtype == torch.float16
        return a

    a, d = forward_backward(amp, qkv, da.half())
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(d).all()), (regime, shape)
    res["amp_a"], res["amp_d"] = a.float(), d.float()
    return res


def p16_model(qkv, da, ch=64):
    """(out [B, C, N], dqkv [B, 3C, N]) in float64: what attention_p16_kernel and the two p16 backward kernels round, with exact
    accumulation and the softmax against the final row maximum. h(x) is x rounded to fp16:
        q8 = h(q / 8), k16 = h(k), v16 = h(v), dA16 = h(dA);   S = q8 . k16, m = rowmax S, pe = exp(S - m), l = sum pe
        O = (h(pe) . v16) / l;   P = pe / l, D = sum_c dA16 O, dP = dA16 . v16, dS = P (dP - D)
        dv = h(P)^T dA16, dk = h(dS)^T q8, dq = h(dS) k16 / 8
    The device adds fp32 accumulation and the online softmax's re-rounding (P against the running maximum) on top of it."""
    def h(x):
        return x.float().half().double()

    B, C3, N = qkv.shape
    C = C3 // 3
    G = B * (C // ch)
    q, k, v = (t.reshape(G, ch, N) for t in qkv.chunk(3, dim=1))
    q8, k16, v16, dA16 = h(q * 0.125), h(k), h(v), h(da.reshape(G, ch, N))
    S = torch.einsum("bct,bcs->bts", q8, k16)
    pe = torch.exp(S - S.amax(dim=-1, keepdim=True))
    l = pe.sum(dim=-1, keepdim=True)                                   # [G, t, 1]
    O = torch.einsum("bts,bcs->bct", h(pe), v16) / l.transpose(1, 2)
    P = pe / l
    D = (dA16 * O).sum(dim=1)                                          # [G, t]
    dP = torch.einsum("bct,bcs->bts", dA16, v16)
    dS = P * (dP - D.unsqueeze(-1))
    dv = torch.einsum("bts,bct->bcs", h(P), dA16)
    dk = torch.einsum("bts,bct->bcs", h(dS), q8)
    dq = torch.einsum("bts,bcs->bct", h(dS), k16) / 8
    return O.reshape(B, C, N), torch.cat([t.reshape(B, C, N) for t in (dq, dk, dv)], dim=1)
