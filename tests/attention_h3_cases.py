"""What the tests of the h3 attention operators share (tests/test_attention_h3_host.py, test_gpu_attention_h3.py): a float64 model of
what attention_h3_kernel and the two h3 backward kernels (csrc/attention.hip) round, next to attention_cases.p16_model, and the
acceptance rows every h3 test is stated in. The model accumulates exactly and takes the softmax against the final row maximum; the
device adds fp32 accumulation and the online softmax on top of it. Nothing here needs a GPU.

    h(x) is x rounded to fp16 (RNE, gradual underflow).
    an operand of unknown scale (q / 8, k, v, the normalised dA):   x  ~  xh + 2^-11 xl,   xh = h(x), xl = h((x - xh) 2^11)
    first product  a . b  ->  ah . bh + 2^-11 (ah . bl + al . bh)
    second product x . y, y = P 2^15 or dS 2^10 formed in registers  ->  xh . h(y) + xh . h(y - h(y)) + xl . h(y 2^-11)
    dA is normalised per sample by 2^-e, e the exponent of that sample's largest |dA|; 2^e and the lifts leave with the outputs.

Two mutations show what each device of the arithmetic is for (test_attention_h3_host.py asserts that either one alone fails):
    raw_lo=True        lo = h(x - hi) as it is and no lift of P and dS: lo terms fall into fp16's subnormal range
    normalise=False    dA as it comes: at dA 2^-20 its hi terms underflow
"""
import math

import torch

import arch_cases as A
import attention_cases as AC

P_LIFT, DS_LIFT, LO_LIFT = 15, 10, 11


def h(x):
    return x.float().half().double()


def split(x, raw_lo=False):
    """(hi, lo, weight of lo) of an operand of unknown scale"""
    hi = h(x)
    if raw_lo:
        return hi, h(x - hi), 1.0
    return hi, h((x - hi) * 2.0 ** LO_LIFT), 2.0 ** -LO_LIFT


def first_product(eq, a, b, raw_lo):
    ah, al, wa = split(a, raw_lo)
    bh, bl, wb = split(b, raw_lo)
    return torch.einsum(eq, ah, bh) + wb * torch.einsum(eq, ah, bl) + wa * torch.einsum(eq, al, bh)


def second_product(eq, x, y, lift, raw_lo):
    """x (unknown scale) against y (P or dS), y lifted by 2^lift; the lift is taken out again"""
    xh, xl, wx = split(x, raw_lo)
    if raw_lo:
        yh = h(y)
        return torch.einsum(eq, xh, yh) + torch.einsum(eq, xh, h(y - yh)) + torch.einsum(eq, xl, yh)
    yl = y * 2.0 ** lift
    yh = h(yl)
    return (torch.einsum(eq, xh, yh) + torch.einsum(eq, xh, h(yl - yh)) + torch.einsum(eq, xl, h(yl * wx))) * 2.0 ** -lift


def sample_exponent(da):
    """[B] exponents e with max|dA_b| 2^-e in [1, 2) (0 for an all-zero sample), as the device takes them from the magnitude bits"""
    m = da.reshape(da.shape[0], -1).abs().amax(dim=1).double()
    return [0 if float(v) == 0.0 else max(math.frexp(float(v))[1] - 1, -126) for v in m]


def h3_model(qkv, da, ch=64, raw_lo=False, normalise=True):
    """(out [B, C, N], dqkv [B, 3C, N]) in float64 for fp32 qkv [B, 3C, N] and da [B, C, N]"""
    B, C3, N = qkv.shape
    C = C3 // 3
    heads = C // ch
    G = B * heads
    q, k, v = (t.double().reshape(G, ch, N) for t in qkv.chunk(3, dim=1))
    q8 = q * 0.125
    e = sample_exponent(da) if normalise else [0] * B
    unit = torch.tensor([2.0 ** x for x in e], dtype=torch.float64).repeat_interleave(heads).reshape(G, 1, 1)
    dan = da.double().reshape(G, ch, N) / unit
    S = first_product("bct,bcs->bts", q8, k, raw_lo)
    pe = torch.exp(S - S.amax(dim=-1, keepdim=True))
    l = pe.sum(dim=-1, keepdim=True)                                    # [G, t, 1]
    O = second_product("bcs,bts->bct", v, pe, P_LIFT, raw_lo) / l.transpose(1, 2)
    P = pe / l
    D = (dan * O).sum(dim=1)                                            # [G, t]
    dP = first_product("bct,bcs->bts", dan, v, raw_lo)
    dS = P * (dP - D.unsqueeze(-1))
    dv = second_product("bct,bts->bcs", dan, P, P_LIFT, raw_lo) * unit
    dk = second_product("bct,bts->bcs", q8, dS, DS_LIFT, raw_lo) * unit
    dq = second_product("bcs,bts->bct", k, dS, DS_LIFT, raw_lo) * unit / 8
    return O.reshape(B, C, N), torch.cat([t.reshape(B, C, N) for t in (dq, dk, dv)], dim=1)


def tensors(out, dqkv, C):
    """{name: tensor} of out, dq, dk, dv"""
    got = {"out": out}
    got.update({n: dqkv[:, sl] for n, sl in AC.parts(C)})
    return got


def truths(ref, C):
    """({name: float64}, {name: fp32 torch}) of a reference of attention_cases.reference"""
    return tensors(ref["a64"], ref["d64"], C), tensors(ref["a32"], ref["d32"], C)


def strict_rows(got, r64, r32, names):
    """the rule of test_gpu_attention_shapes.py: per tensor err <= YARD_FACTOR x (fp32 torch vs float64), no relative floor"""
    rows = []
    for n in names:
        err, yard = float((got[n].double().cpu() - r64[n]).abs().max()), float((r32[n].double() - r64[n]).abs().max())
        rows.append((n, err, yard, float(r64[n].abs().max()), bool(err <= A.YARD_FACTOR * yard)))      # NaN fails
    return rows
