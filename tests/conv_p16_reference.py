"""Float64 reference of the fused convolution under precision 16, by its definition, and its error bound -- shared by the tests of the
training operators (tests/test_gpu_train_ops_edges.py: cddpm_op_conv_packed under cddpm_set_train_precision(16)) and of the handle's
plan (tests/test_gpu_conv_planned.py: cddpm_op_conv_planned on a handle at cddpm_set_precision(h, 16)). Pure torch on the CPU.

Precision 16: float64 sums of fp16(a) fp16(b), fp16 = torch's .half() (round to nearest even, gradual underflow); the weight operand of
a packed image is fp16(w 2^e) 2^-e with e the image's pre-scale exponent. Accumulation bound: fp32 accumulation of exact fp32 products
(a product of two fp16 values has at most 22 significant bits), 2^-20 sum |a||b| over the contraction -- the allowance of the forward
family (tests/test_gpu_kernels.py::conv_bound)."""
import torch
import torch.nn.functional as F

U20, U24, U25 = 2.0 ** -20, 2.0 ** -24, 2.0 ** -25


def f16(x):
    """fp16 value of an fp32 operand, as float64 (torch's .half(): RNE, gradual underflow, inf above 65504)"""
    return x.float().half().double()


def f16_ulp(v):
    """spacing of the fp16 grid at |v| (2^-24 in the subnormal range)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def near_f16_midpoint(v, scale):
    """elements whose float64 value lies within `scale` of a rounding midpoint of the fp16 grid (there the device's fp32 value of the
    same expression may round to the other neighbour)"""
    u = f16_ulp(v)
    r = torch.remainder(v.abs(), u)
    return (r - u / 2).abs() <= scale


def fused_act(x, coef, silu):
    """float64 act(v) = silu?((v - mean) a + d) of the fp32 inputs, and the tolerance of the device's fp32 evaluation: the affine takes
    three roundings, each <= 2^-24 of its operand; SiLU's exp2 / rcp form ~1.5 ulp -- 2^-20 of the largest intermediate covers them with
    room (16 fp32 ulp)"""
    v = x.double()
    if coef is None:
        return v, torch.zeros_like(v)
    m, a, d = (coef[i].double()[:, :, None, None] for i in range(3))
    t = (v - m) * a
    u = t + d
    tol = U20 * torch.maximum(torch.maximum(t.abs(), d.abs().expand_as(t)), (v - m).abs() * a.abs())
    return (F.silu(u) if silu else u), tol


def w16(w, e):
    """the precision-16 weight operand of a forward / input-gradient image: fp16(w 2^e) 2^-e"""
    return (w.float() * 2.0 ** e).half().double() * 2.0 ** -e


def folded_classes(w, e=None):
    """the four 2 x 2 class kernels of 'nearest x2 upsample -> conv3x3' (class (pa, pb) = output pixel (2 gy + pa, 2 gx + pb); tap (ty, tx)
    reads the low-resolution pixel (gy + ty + pa - 1, gx + tx + pb - 1)), summed in float64 and rounded once to fp32 as the packer does;
    e given: the precision-16 operand fp16(sum 2^e) 2^-e"""
    w64 = w.double()
    out = {}
    for pa in (0, 1):
        for pb in (0, 1):
            rows = [(0, 0), (1, 2)] if pa == 0 else [(0, 1), (2, 2)]
            cols = [(0, 0), (1, 2)] if pb == 0 else [(0, 1), (2, 2)]
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2, dtype=torch.float64)
            for ty, (y0, y1) in enumerate(rows):
                for tx, (x0, x1) in enumerate(cols):
                    k[:, :, ty, tx] = w64[:, :, y0:y1 + 1, x0:x1 + 1].sum(dim=(2, 3)).float().double()
            out[(pa, pb)] = k if e is None else w16(k, e)
    return out


def folded_conv(a, classes):
    """out[2 gy + pa, 2 gx + pb] = sum over the class's 2 x 2 taps of the low-resolution input a [B, C, h, w]"""
    B, _, h, w_ = a.shape
    ap = F.pad(a, (1, 1, 1, 1))
    out = None
    for (pa, pb), k in classes.items():
        o = F.conv2d(ap[:, :, pa:pa + h + 1, pb:pb + w_ + 1], k)
        if out is None:
            out = torch.zeros(B, o.shape[1], 2 * h, 2 * w_, dtype=torch.float64)
        out[:, :, pa::2, pb::2] = o
    return out


def p16_forward_ref(x, coef, silu, w, e, k, bias, folded=False, x1=None, skip=None, ws=None, res=None, res_up=False):
    """float64 reference of a precision-16 fused convolution (cddpm_op_conv_packed, cddpm_op_conv_planned) and its bound:
    out = 2^-e sum fp16(act) fp16(w 2^e) (fp32 accumulation: 2^-20 sum |.||.|) + bias [+ res] (two fp32 adds in the epilogue: 2^-23 of the
    larger of the sum and the addends); elements of the fused transform's output within a few fp32 ulp of an fp16 rounding midpoint may round
    either way: one fp16 ulp on exactly those"""
    xin = torch.cat([x, x1], 1) if x1 is not None else x
    v, tol = fused_act(xin, coef, silu)
    fa = f16(v)
    slack = near_f16_midpoint(v, tol).double() * f16_ulp(v) if coef is not None else torch.zeros_like(v)
    if folded:
        cls = folded_classes(w, e)
        s, sabs, sx = folded_conv(fa, cls), folded_conv(fa.abs(), {c: t.abs() for c, t in cls.items()}), folded_conv(slack, {c: t.abs() for c, t in cls.items()})
    else:
        fw = w16(w, e)
        s, sabs, sx = F.conv2d(fa, fw, None, padding=k // 2), F.conv2d(fa.abs(), fw.abs(), None, padding=k // 2), F.conv2d(slack, fw.abs(), None, padding=k // 2)
    if skip is not None:
        fs, fws = f16(skip), w16(ws, e)
        s, sabs = s + F.conv2d(fs, fws), sabs + F.conv2d(fs.abs(), fws.abs())
    add = bias.double()[None, :, None, None].expand_as(s)
    if res is not None:
        add = add + (F.interpolate(res.double(), scale_factor=2, mode="nearest") if res_up else res.double())
    ref = s + add
    lim = U20 * sabs + sx + 2.0 ** -23 * (s.abs() + add.abs() + ref.abs()) + 1e-300
    return ref, lim
