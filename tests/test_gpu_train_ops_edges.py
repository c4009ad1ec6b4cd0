"""GPU: the training step's convolution operators at the edges of their arithmetic and of their plans, called through the C ABI in the step's
own form (device images from cddpm_op_pack_conv under the exponent rule of cddpm_op_absmax, cddpm_op_conv_packed, cddpm_op_conv_wgrad,
cddpm_op_gn_coef_rec, cddpm_op_gn_silu_backward) and compared element by element with float64 torch.

  A  precision 16 (cddpm_set_train_precision) checked by its definition: float64 sums of fp16(a) fp16(b), fp16 = torch's .half()
     (round to nearest even, gradual underflow); the weight operand of the forward / input-gradient images is fp16(w 2^e) 2^-e
  B  the precision-32 backward convolutions at the domain edges of the unscaled fp16 operand split (dy carries the loss scale)
  C  the per-call 256-cout plan of cddpm_op_conv_packed (>= 512 workgroups of the 128-cout form) and its GroupNorm statistics records
  D  cddpm_op_gn_silu_backward as the decoder calls it: two sources, records from the producing convolutions, add_dev
  E  cddpm_op_grad_check and cddpm_op_absmax at their tails

Accumulation bound of every MFMA family here: fp32 accumulation of exact fp32 products (a product of two fp16 values has at most 22
significant bits), 2^-20 sum |a||b| over the contraction -- the allowance of the forward family (test_gpu_kernels.py::conv_bound). The
float64 references cover three batch items (first, middle, last); the operators always run the whole batch, because the plan depends on it.
Measured on gfx950: the 16-bit MFMA inputs keep fp16 subnormals (gradual underflow), see test_precision16_keeps_fp16_subnormals."""
import ctypes as C
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg
from conv_p16_reference import (U20, U24, U25, f16, f16_ulp, folded_classes, folded_conv, fused_act, near_f16_midpoint,  # noqa: F401
                               p16_forward_ref, w16)

gpu = pytest.mark.gpu



@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=32, max_w=32)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def _p(t):
    return None if t is None else t.data_ptr()


def _ck(eng, rc, what):
    assert rc == 0, f"{what}: {eng.lib.cddpm_last_error(eng._h).decode()}"


@contextmanager
def precision(eng, bits):
    prev = eng.lib.cddpm_set_train_precision(bits)
    assert prev in (16, 32)
    try:
        yield
    finally:
        eng.lib.cddpm_set_train_precision(32)


# ---- float64 helpers: conv_p16_reference.py (shared with test_gpu_conv_planned.py) ---------------------------------------------------------
def weight_exp(eng, w, mult=1.0):
    """the pre-scale exponent of a weight tensor: max |w| from cddpm_op_absmax, then the largest e in [0, 24] with mult max|w| 2^e < 2^14
    (mult 4: the folded-upsample class sums reach 4 max|w|)"""
    out = torch.zeros(1, device="cuda")
    wd = w.float().cuda().contiguous()
    _ck(eng, eng.lib.cddpm_op_absmax(eng._h, wd.data_ptr(), wd.numel(), out.data_ptr(), None), "absmax")
    torch.cuda.synchronize()
    m = float(out.item()) * mult
    assert m == float(w.abs().max()) * mult
    e = 24
    while e > 0 and math.ldexp(m, e) >= 16384.0:
        e -= 1
    return e


def pack(eng, w, mode, e):
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    O, I = (Cin, Cout) if mode == 1 else (Cout, Cin)
    taps = 4 if mode == 2 else k * k
    nb = (4 if mode == 2 else 1) * eng.lib.cddpm_packed_conv_bytes(O, I, taps)
    dev = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    wd = w.float().cuda().contiguous()
    _ck(eng, eng.lib.cddpm_op_pack_conv(eng._h, wd.data_ptr(), Cout, Cin, k, mode, e, dev.data_ptr(), None), "pack_conv")
    return dev


def ratio_check(got, ref, lim, what):
    err = (got.double() - ref).abs()
    r = float((err / lim).max())
    assert r <= 1.0, f"{what}: max err/bound {r:.3f} (max err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e})"
    return r


def conv_packed(eng, x0, packed, e, Cout, k, B, H, W, x1=None, coef=None, silu=False, folded=False, bias=None, res=None, res_up=False,
                skip=None, skip1=None, skip_packed=None, stats=False):
    """cddpm_op_conv_packed on NHWC device tensors; -> (out NHWC, records or None)"""
    out = torch.empty(B, H, W, Cout, device="cuda")
    rec = torch.full((B, eng.lib.cddpm_stat_records(H, W, 1 if folded else 0), Cout, 2), float("nan"), device="cuda") if stats else None
    _ck(eng, eng.lib.cddpm_op_conv_packed(
        eng._h, _p(x0), x0.shape[-1], _p(x1), x1.shape[-1] if x1 is not None else 0, _p(coef), int(silu), int(folded), _p(packed), e, _p(bias),
        Cout, k, _p(res), int(res_up), _p(skip), skip.shape[-1] if skip is not None else 0, _p(skip1), skip1.shape[-1] if skip1 is not None else 0,
        _p(skip_packed), _p(out), _p(rec), B, H, W, None), "conv_packed")
    torch.cuda.synchronize()
    return out, rec


def conv_wgrad(eng, x0, dy, Cout, k, B, H, W, x1=None, coef=None, silu=False, up=False, bias=True):
    Cin = x0.shape[-1] + (x1.shape[-1] if x1 is not None else 0)
    dw = torch.full((Cout, Cin, k, k), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda") if bias else None
    _ck(eng, eng.lib.cddpm_op_conv_wgrad(eng._h, _p(x0), x0.shape[-1], _p(x1), x1.shape[-1] if x1 is not None else 0, _p(coef), int(silu),
                                         int(up), _p(dy), Cout, k, _p(dw), _p(db), B, H, W, None), "conv_wgrad")
    torch.cuda.synchronize()
    return dw.cpu(), (db.cpu() if bias else None)


def wgrad64(a, dy, k):
    """dL/dW of conv2d(a, W, padding k // 2) for the upstream gradient dy, float64"""
    w = torch.zeros(dy.shape[1], a.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(a, w, None, padding=k // 2).backward(dy)
    return w.grad


def items(B):
    return sorted({0, B // 2, B - 1})


# ---- CPU: the reference helper against the host packer ------------------------------------------------------------------------------------
def test_fp16_operand_helper_is_the_packers_hi_term():
    """w16(w, e) -- the weight operand of every precision-16 reference below -- is, bit for bit, the hi term of the host packer's image
    (cddpm_pack_conv_weights, format 2, the layout of include/cddpm.h) times 2^-e, with e the packer's exponent"""
    lib = load_pkg("_lib").load_library()
    rng = np.random.default_rng(3)
    for Cout, Cin, taps in ((256, 64, 9), (128, 96, 1)):
        k = 3 if taps == 9 else 1
        w = (rng.standard_normal((Cout, Cin, k, k)) * 0.03).astype(np.float32)
        w.flat[:6] = [0.0, 3.0e-9, -1.0e-7, 0.2, 2.0 ** -30, -0.21]        # exponent-limited and fp16-subnormal after the pre-scale
        n = lib.cddpm_packed_conv_bytes(Cout, Cin, taps)
        buf = np.zeros(n, dtype=np.uint8)
        e = C.c_int(-1)
        fmt = lib.cddpm_pack_conv_weights(w.ctypes.data_as(C.POINTER(C.c_float)), Cout, Cin, taps, buf.ctypes.data, C.byref(e))
        if fmt != 2:
            pytest.skip("not the fp16 split family")
        img = buf.view(np.uint16).reshape(Cout // 128, Cin // 32, taps, 128, 8, 8)
        hi = np.zeros((Cout, Cin, taps), np.float64)
        for j in range(128):
            for u in range(4):
                raw = img[:, :, :, j, u ^ ((j >> 1) & 7), :]                                      # [cout block][chunk][tap][8]
                hi.reshape(Cout // 128, 128, Cin // 32, 4, 8, taps)[:, j, :, u] = raw.view(np.float16).astype(np.float64).transpose(0, 1, 3, 2)
        assert 0 <= e.value <= 24 and float(np.abs(w).max()) * 2.0 ** e.value < 2.0 ** 14 <= float(np.abs(w).max()) * 2.0 ** (e.value + 1)
        want = w16(torch.from_numpy(w), e.value).numpy().reshape(Cout, Cin, taps)
        assert np.array_equal(hi * 2.0 ** -e.value, want)


def test_fp16_midpoint_helper():
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -12, 3 * 2.0 ** -25, 2.0 ** -25 * 1.5, 65504.0 + 16])
    assert near_f16_midpoint(v.double(), 2.0 ** -28).tolist() == [True, True, False, True, False, True]
    assert f16_ulp(torch.tensor([1.0, 1e-6, 2.0 ** -14, 65504.0]).double()).tolist() == [2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 32.0]


# ---- A: precision 16 by its definition ------------------------------------------------------------------------------------------------
P16_CONV = [
    # name, B, C0, C1, Cout, k, H, W, coef, silu, folded, skip S0, S1, res
    ("3x3_act", 2, 128, 0, 128, 3, 12, 40, True, True, False, 0, 0, "same"),
    ("1x1_qkv", 2, 256, 0, 384, 1, 8, 24, True, False, False, 0, 0, None),
    ("1x1_raw_res", 2, 128, 0, 128, 1, 6, 20, False, False, False, 0, 0, "same"),
    ("folded_up", 2, 128, 0, 128, 3, 16, 48, True, True, True, 0, 0, "up"),
    ("concat", 2, 128, 128, 128, 3, 8, 32, True, True, False, 0, 0, None),
    ("skip_segment", 2, 128, 0, 128, 3, 8, 40, True, True, False, 128, 64, None),
    ("3x3_nb2", 16, 64, 0, 256, 3, 64, 64, True, True, False, 0, 0, None),
    ("folded_up_nb2", 16, 64, 0, 256, 3, 64, 64, True, True, True, 0, 0, None),
]


@gpu
@pytest.mark.parametrize("case", P16_CONV, ids=[c[0] for c in P16_CONV])
def test_precision16_conv_packed_is_fp16_operands(eng, case):
    """cddpm_op_conv_packed under precision 16 against its definition (p16_forward_ref): 3x3, 1x1, folded upsample, a concatenated source,
    the fused 1x1 skip segment on two tensors, and the 128-cout (B = 2) and 256-cout (B = 16 at 64 x 64: 512 workgroups of the 128-cout form)
    plans -- the five hi-only kernel instantiations"""
    name, B, C0, C1, Cout, k, H, W, use_coef, silu, folded, S0, S1, resmode = case
    torch.manual_seed(len(name) + B + C0)
    Cin = C0 + C1
    h, w_ = (H // 2, W // 2) if folded else (H, W)
    x = torch.randn(B, Cin, h, w_) * 1.3 + 0.2
    coef = torch.stack([torch.randn(B, Cin) * 0.2, 1 + 0.3 * torch.randn(B, Cin), torch.randn(B, Cin) * 0.3]) if use_coef else None
    wt = torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    ws = torch.randn(Cout, S0 + S1, 1, 1) / (S0 + S1) ** 0.5 if S0 else None
    bias = torch.randn(Cout) * 0.1
    e = weight_exp(eng, wt if ws is None else torch.cat([wt.flatten(), ws.flatten()]), 4.0 if folded else 1.0)
    pk = pack(eng, wt, 2 if folded else 0, e)
    spk = pack(eng, ws, 0, e) if S0 else None
    sk = torch.randn(B, S0 + S1, H, W) * 2.0 if S0 else None
    res = torch.randn(B, Cout, H // 2, W // 2) if resmode == "up" else torch.randn(B, Cout, H, W) if resmode == "same" else None
    with precision(eng, 16):
        out, _ = conv_packed(eng, nhwc(x[:, :C0]), pk, e, Cout, k, B, H, W, x1=nhwc(x[:, C0:]) if C1 else None,
                             coef=coef.cuda().contiguous() if use_coef else None, silu=silu, folded=folded, bias=bias.cuda(),
                             res=nhwc(res) if res is not None else None, res_up=resmode == "up",
                             skip=nhwc(sk[:, :S0]) if S0 else None, skip1=nhwc(sk[:, S0:]) if S1 else None, skip_packed=spk)
    it = items(B)
    ref, lim = p16_forward_ref(x[it], coef[:, it] if use_coef else None, silu, wt, e, k, bias, folded=folded,
                               skip=sk[it] if S0 else None, ws=ws, res=res[it] if res is not None else None, res_up=resmode == "up")
    r = ratio_check(nchw(out)[it], ref, lim, name)
    print(name, f"err/bound {r:.3f}")


P16_WGRAD = [
    # name, B, C0, C1, Cout, k, H, W, coef, silu, up
    ("3x3_act", 3, 128, 0, 128, 3, 8, 24, True, True, False),
    ("3x3_concat", 2, 128, 64, 64, 3, 6, 16, True, True, False),
    ("1x1_cin64", 2, 256, 0, 128, 1, 8, 16, True, False, False),
    ("1x1_cin32_x", 2, 96, 0, 64, 1, 8, 16, False, False, False),
    ("1x1_cin32_concat_x", 2, 64, 96, 128, 1, 6, 12, True, False, False),
    ("3x3_up", 2, 128, 0, 128, 3, 12, 20, True, True, True),
    ("batch_11", 11, 64, 0, 64, 3, 6, 10, True, True, False),
]


def p16_wgrad_ref(x, coef, silu, up, dy, k):
    """dW = sum over (sample, pixel) fp16(act) fp16(dy): NO pre-scale on either operand; bound 2^-20 sum |.||.| + one fp16 ulp of the
    transform's output where it lies near an fp16 rounding midpoint"""
    v, tol = fused_act(x, coef, silu)
    slack = near_f16_midpoint(v, tol).double() * f16_ulp(v) if coef is not None else torch.zeros_like(v)
    fa = f16(v)
    if up:
        fa, slack = F.interpolate(fa, scale_factor=2, mode="nearest"), F.interpolate(slack, scale_factor=2, mode="nearest")
    fd = f16(dy)
    ref = wgrad64(fa, fd, k)
    lim = U20 * wgrad64(fa.abs(), fd.abs(), k) + wgrad64(slack, fd.abs(), k) + 1e-300
    return ref, lim


@gpu
@pytest.mark.parametrize("case", P16_WGRAD, ids=[c[0] for c in P16_WGRAD])
def test_precision16_conv_wgrad_is_fp16_operands(eng, case):
    """cddpm_op_conv_wgrad under precision 16 against its definition (p16_wgrad_ref): the image kernels <9, 1> and <1, 1> (3x3; 1x1 with
    Cin % 64 == 0), conv_wgrad_x_kernel<1> (1x1 with Cin % 64 == 32, with its bias_grad_run branch), an upsampled input and a batch that
    does not fill its last group of 8. db: the fp32 sums of the raw dy (bound 2^-20 sum |dy|)"""
    name, B, C0, C1, Cout, k, H, W, use_coef, silu, up = case
    torch.manual_seed(B + C0 + C1 + Cout + H)
    Cin = C0 + C1
    hs, ws = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(B, Cin, hs, ws) * 1.5
    coef = torch.stack([torch.randn(B, Cin) * 0.2, 1 + 0.3 * torch.randn(B, Cin), torch.randn(B, Cin) * 0.3]) if use_coef else None
    dy = torch.randn(B, Cout, H, W) * 3.0
    with precision(eng, 16):
        dw, db = conv_wgrad(eng, nhwc(x[:, :C0]), nhwc(dy), Cout, k, B, H, W, x1=nhwc(x[:, C0:]) if C1 else None,
                            coef=coef.cuda().contiguous() if use_coef else None, silu=silu, up=up)
    ref, lim = p16_wgrad_ref(x, coef, silu, up, dy, k)
    r = ratio_check(dw, ref, lim, name + " dW")
    rb = ratio_check(db, dy.double().sum((0, 2, 3)), U20 * dy.double().abs().sum((0, 2, 3)) + 1e-300, name + " db")
    print(name, f"dW err/bound {r:.3f}  db {rb:.3f}")


@gpu
def test_precision16_equals_precision32_on_fp16_exact_operands(eng):
    """operands that are fp16 values (activations, and weights after the 2^e pre-scale): the mid terms of the precision-32 split are zero,
    both precisions sum the same exact products in fp32 -- they agree within the accumulation bound (twice: each side's), for the forward /
    input-gradient image and for the weight gradient"""
    torch.manual_seed(21)
    B, Cin, Cout, H, W = 2, 128, 128, 8, 32
    x = torch.randn(B, Cin, H, W).half().float()
    wt = (torch.randn(Cout, Cin, 3, 3) * 8).half().float() / 512
    e = weight_exp(eng, wt)
    assert torch.equal(w16(wt, e), wt.double())
    pk, pkT = pack(eng, wt, 0, e), pack(eng, wt, 1, e)
    dy = torch.randn(B, Cout, H, W).half().float()
    got = {}
    for bits in (32, 16):
        with precision(eng, bits):
            out, _ = conv_packed(eng, nhwc(x), pk, e, Cout, 3, B, H, W)
            dx, _ = conv_packed(eng, nhwc(dy), pkT, e, Cin, 3, B, H, W)
            dw, _ = conv_wgrad(eng, nhwc(x), nhwc(dy), Cout, 3, B, H, W, bias=False)
        got[bits] = (nchw(out).double(), nchw(dx).double(), dw.double())
    x64, w64, d64 = x.double(), wt.double(), dy.double()
    wT = w64.transpose(0, 1).flip(2, 3)
    lims = (2 * U20 * F.conv2d(x64.abs(), w64.abs(), padding=1), 2 * U20 * F.conv2d(d64.abs(), wT.abs(), padding=1),
            2 * U20 * wgrad64(x64.abs(), d64.abs(), 3))
    for i, what in enumerate(("forward", "input gradient", "weight gradient")):
        r = ratio_check(got[16][i], got[32][i], lims[i] + 1e-300, what)
        print(what, f"|p16 - p32| / bound {r:.3f}")


@gpu
def test_precision16_keeps_fp16_subnormals(eng):
    """operands in the fp16 subnormal range (|x| ~ 1e-6 < 2^-14): torch's .half() keeps them to 2^-25 absolute (gradual underflow). MEASURED
    on gfx950: the precision-16 kernels keep them too -- the result meets the gradual-underflow reference within the accumulation bound, and
    a flush to zero would miss it by sum |a||w|, 2^20 bounds. Forward (activations subnormal), input gradient (dy subnormal: a tiny loss
    scale), weight gradient (either operand subnormal)"""
    torch.manual_seed(8)
    B, Cin, Cout, H, W = 2, 128, 128, 8, 32
    x = torch.randn(B, Cin, H, W) * 1e-6
    dy = torch.randn(B, Cout, H, W) * 1e-6
    assert float(x.abs().max()) < 2.0 ** -14
    wt = torch.randn(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5
    e = weight_exp(eng, wt)
    pk, pkT = pack(eng, wt, 0, e), pack(eng, wt, 1, e)
    xo, dyo = torch.randn(B, Cin, H, W), torch.randn(B, Cout, H, W)
    with precision(eng, 16):
        out, _ = conv_packed(eng, nhwc(x), pk, e, Cout, 3, B, H, W)
        dx, _ = conv_packed(eng, nhwc(dy), pkT, e, Cin, 3, B, H, W)
        dw_a, _ = conv_wgrad(eng, nhwc(x), nhwc(dyo), Cout, 3, B, H, W, bias=False)
        dw_d, _ = conv_wgrad(eng, nhwc(xo), nhwc(dy), Cout, 3, B, H, W, bias=False)
    fw = w16(wt, e)
    fwT = fw.transpose(0, 1).flip(2, 3)
    checks = [("forward", nchw(out), F.conv2d(f16(x), fw, padding=1), F.conv2d(f16(x).abs(), fw.abs(), padding=1)),
              ("input gradient", nchw(dx), F.conv2d(f16(dy), fwT, padding=1), F.conv2d(f16(dy).abs(), fwT.abs(), padding=1)),
              ("weight gradient, subnormal activations", dw_a, wgrad64(f16(x), f16(dyo), 3), wgrad64(f16(x).abs(), f16(dyo).abs(), 3)),
              ("weight gradient, subnormal dy", dw_d, wgrad64(f16(xo), f16(dy), 3), wgrad64(f16(xo).abs(), f16(dy).abs(), 3))]
    for what, got, ref, sabs in checks:
        assert float(got.abs().max()) > 0
        r = ratio_check(got, ref, U20 * sabs + 1e-300, what)
        print(what, f"err/bound {r:.3f}")


# ---- B: domain edges of the precision-32 backward convolutions -------------------------------------------------------------------------
def conv_bound(v64, w64, pad):
    """the forward family's bound (test_gpu_kernels.py): 2^-20 sum |v||w| + 2^-24 sum |w| (the absolute floor 2^-25 of the unscaled operand's
    two-term split, doubled)"""
    return U20 * F.conv2d(v64.abs(), w64.abs(), None, padding=pad) + U24 * F.conv2d(torch.ones_like(v64), w64.abs(), None, padding=pad) + 1e-300


def wgrad_bound(a64, d64, k):
    """both operands split unscaled, x = hi + mid + r: |r| <= 2^-23 |x| while mid is a normal fp16, else <= 2^-25 (absolute). A product
    hi hi + hi mid + mid hi misses r_a b + a r_b - r_a r_b + mid_a mid_b, |mid| <= 2^-11 |x|: <= 2^-21 |a||b| + 2^-25 (|a| + |b|);
    fp32 accumulation 2^-21 sum |a||b| more. Over the contraction: 2^-20 sum |a||dy| + 2^-25 (sum |a| + sum |dy|), where the sums run over
    the (sample, pixel) pairs that multiply (taps over the zero padding contribute exact zeros)"""
    ones_a, ones_d = torch.ones_like(a64), torch.ones_like(d64)
    return U20 * wgrad64(a64.abs(), d64.abs(), k) + U25 * (wgrad64(a64.abs(), ones_d, k) + wgrad64(ones_a, d64.abs(), k)) + 1e-300


DY_SCALES = [1e-6, 1e-3, 2.0 ** 10, 1e4]


@gpu
@pytest.mark.parametrize("s", DY_SCALES)
def test_dgrad_domain_scaled_dy(eng, s):
    """the input gradient as training.py::dgrad runs it (cddpm_op_conv_packed on the mode-1 image) with dy = loss scale x dL/d(out) over
    10^-6 .. 10^4; bound: the forward family's (conv_bound) with dy as the unscaled operand"""
    torch.manual_seed(40 + DY_SCALES.index(s))
    B, Cin, Cout, H, W = 2, 128, 256, 8, 32
    wt = torch.randn(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5
    e = weight_exp(eng, wt)
    pkT = pack(eng, wt, 1, e)
    dy = torch.randn(B, Cout, H, W) * s
    dx, _ = conv_packed(eng, nhwc(dy), pkT, e, Cin, 3, B, H, W)
    wT = wt.double().transpose(0, 1).flip(2, 3)
    r = ratio_check(nchw(dx), F.conv2d(dy.double(), wT, padding=1), conv_bound(dy.double(), wT, 1), f"dgrad dy x {s:g}")
    print(f"dgrad dy x {s:g}: err/bound {r:.3f}")


WG_SCALES = [("a_1e-6", 1e-6, 1.0), ("a_1e4", 1e4, 1.0), ("dy_1e-6", 1.0, 1e-6), ("dy_1e4", 1.0, 1e4), ("both_1e3", 1e3, 1e3),
             ("both_1e-4", 1e-4, 1e-4)]


@gpu
@pytest.mark.parametrize("name,sa,sd", WG_SCALES, ids=[c[0] for c in WG_SCALES])
def test_wgrad_domain_scaled_operands(eng, name, sa, sd):
    """cddpm_op_conv_wgrad (precision 32) with the activations and dy each scaled over 10^-6 .. 10^4: the unscaled two-term split's bound
    (wgrad_bound); 3x3 over the image kernels and 1x1 over conv_wgrad_x_kernel (Cin % 64 == 32); db against the fp32 sum's 2^-20 sum |dy|"""
    torch.manual_seed(sum(name.encode()))
    B, H, W = 3, 8, 16
    for Cin, Cout, k in ((128, 128, 3), (96, 64, 1)):
        a = torch.randn(B, Cin, H, W) * sa
        dy = torch.randn(B, Cout, H, W) * sd
        dw, db = conv_wgrad(eng, nhwc(a), nhwc(dy), Cout, k, B, H, W)
        a64, d64 = a.double(), dy.double()
        r = ratio_check(dw, wgrad64(a64, d64, k), wgrad_bound(a64, d64, k), f"{name} k{k} dW")
        rb = ratio_check(db, d64.sum((0, 2, 3)), U20 * d64.abs().sum((0, 2, 3)) + 1e-300, f"{name} k{k} db")
        print(name, k, f"dW err/bound {r:.3f}  db {rb:.3f}")


@gpu
def test_wgrad_domain_mixed_magnitudes_and_raw_residual_stream(eng):
    """log-uniform magnitudes 10^-6 .. 10^4 with random signs on both operands (3x3), and the fused skip_connection's weight gradient: a
    1x1 convolution of the RAW residual stream at 10^3 .. 10^4 (no GroupNorm in front, OpenAI_Unet.py:338) on both 1x1 kernels"""
    torch.manual_seed(13)
    B, H, W = 2, 8, 24

    def lu(*shape):
        return torch.sign(torch.randn(*shape)) * 10.0 ** (torch.rand(*shape) * 10 - 6)
    a, dy = lu(B, 128, H, W), lu(B, 128, H, W)
    dw, _ = conv_wgrad(eng, nhwc(a), nhwc(dy), 128, 3, B, H, W, bias=False)
    r = ratio_check(dw, wgrad64(a.double(), dy.double(), 3), wgrad_bound(a.double(), dy.double(), 3), "mixed magnitudes")
    print(f"mixed magnitudes: err/bound {r:.3f}")
    for Cin in (256, 160):
        sk = torch.randn(B, Cin, H, W) * 10.0 ** (3 + torch.rand(B, Cin, H, W))
        dy = torch.randn(B, 128, H, W)
        dw, _ = conv_wgrad(eng, nhwc(sk), nhwc(dy), 128, 1, B, H, W, bias=False)
        r = ratio_check(dw, wgrad64(sk.double(), dy.double(), 1), wgrad_bound(sk.double(), dy.double(), 1), f"raw stream Cin {Cin}")
        print(f"raw residual stream 1e3..1e4, Cin {Cin}: err/bound {r:.3f}")


@gpu
def test_backward_beyond_the_fp16_range_is_loud(eng):
    """|operand| >= 65520 overflows the unscaled fp16 split (hi = inf, mid = -inf): every output that reads it must be NON-FINITE, never a
    finite wrong number, and every other output finite and within its bound; 65000 (inside) meets the bound. dgrad: one dy element; wgrad: one
    activation element (-> the column dW[:, ci]) or one dy element (-> the row dW[co]); db is a plain fp32 sum of dy and stays exact"""
    torch.manual_seed(17)
    B, Cin, Cout, H, W = 1, 128, 128, 8, 32
    wt = torch.randn(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5
    e = weight_exp(eng, wt)
    pkT = pack(eng, wt, 1, e)
    wT = wt.double().transpose(0, 1).flip(2, 3)
    for v in (65000.0, 1.0e5):
        dy = torch.randn(B, Cout, H, W)
        dy[0, 5, 3, 7] = v
        dx = nchw(conv_packed(eng, nhwc(dy), pkT, e, Cin, 3, B, H, W)[0])
        reads = torch.zeros_like(dx, dtype=torch.bool)
        reads[0, :, 2:5, 6:9] = True
        if v < 65504:
            ratio_check(dx, F.conv2d(dy.double(), wT, padding=1), conv_bound(dy.double(), wT, 1), "dgrad at 65000")
        else:
            assert bool((~torch.isfinite(dx[reads])).all()), "every input gradient that reads the out-of-range dy must be non-finite"
            ref, lim = F.conv2d(dy.double(), wT, padding=1), conv_bound(dy.double(), wT, 1)
            ratio_check(dx[~reads], ref[~reads], lim[~reads], "dgrad away from the out-of-range dy")
    B, H, W = 2, 8, 16
    for which in ("act", "dy"):
        for v in (65000.0, 1.0e5):
            a, dy = torch.randn(B, Cin, H, W), torch.randn(B, Cout, H, W)
            (a if which == "act" else dy)[1, 9, 4, 5] = v
            dw, db = conv_wgrad(eng, nhwc(a), nhwc(dy), Cout, 3, B, H, W)
            ref, lim = wgrad64(a.double(), dy.double(), 3), wgrad_bound(a.double(), dy.double(), 3)
            ratio_check(db, dy.double().sum((0, 2, 3)), U20 * dy.double().abs().sum((0, 2, 3)) + 1e-300, f"db, {which} = {v:g}")
            if v < 65504:
                ratio_check(dw, ref, lim, f"dW, {which} = 65000")
                continue
            reads = torch.zeros_like(dw, dtype=torch.bool)
            if which == "act":
                reads[:, 9] = True
            else:
                reads[9] = True
            assert bool((~torch.isfinite(dw[reads])).all()), f"every weight gradient that reads the out-of-range {which} must be non-finite"
            ratio_check(dw[~reads], ref[~reads], lim[~reads], f"dW away from the out-of-range {which}")


# ---- C: the per-call plan, ragged tiles, statistics records ---------------------------------------------------------------------------
PLAN = [
    # name, B, H, W, folded, ratio, film
    ("b15_64x64", 15, 64, 64, False, 10.0, False),
    ("b16_64x64", 16, 64, 64, False, 0.0, True),
    ("b16_60x44_ragged", 16, 60, 44, False, 100.0, False),
    ("b16_folded_64x64", 16, 64, 64, True, 10.0, True),
]


@gpu
@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("case", PLAN, ids=[c[0] for c in PLAN])
def test_conv_packed_plan_edges_and_statistics_records(eng, case, bits):
    """Cout = 256 just below (B = 15: 480 workgroups of the 128-cout form) and at the 512-workgroup threshold of the per-call 256-cout plan,
    a geometry with H % 8 != 0 and W % 32 != 0, and a folded-upsample call, in both precisions: the output against float64 (precision 32:
    conv_bound; 16: p16_forward_ref) and its statistics records through cddpm_op_gn_coef_rec against float64 GroupNorm (+ FiLM) of the
    output AS STORED, |mean| / sigma = ratio set by the bias; bound on the normalised value 1e-5 (1 + ratio) as
    test_gpu_kernels.py::test_groupnorm_statistics_from_the_conv_epilogue_with_large_mean"""
    name, B, H, W, folded, ratio, film = case
    torch.manual_seed(B + H + W + bits)
    Cin, Cout = 64, 256
    h, w_ = (H // 2, W // 2) if folded else (H, W)
    x = torch.randn(B, Cin, h, w_)
    coef = torch.stack([torch.randn(B, Cin) * 0.2, 1 + 0.2 * torch.randn(B, Cin), torch.randn(B, Cin) * 0.2])
    wt = torch.randn(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5 * (0.5 if folded else 1.0)
    bias = ratio * (1 + 0.05 * torch.randn(Cout))
    e = weight_exp(eng, wt, 4.0 if folded else 1.0)
    pk = pack(eng, wt, 2 if folded else 0, e)
    with precision(eng, bits):
        out, rec = conv_packed(eng, nhwc(x), pk, e, Cout, 3, B, H, W, coef=coef.cuda().contiguous(), silu=True, folded=folded,
                               bias=bias.cuda(), stats=True)
    it = items(B)
    if bits == 16:
        ref, lim = p16_forward_ref(x[it], coef[:, it], True, wt, e, 3, bias, folded=folded)
    else:
        v, _ = fused_act(x[it], coef[:, it], True)
        if folded:
            cls = folded_classes(wt)
            ref = folded_conv(v, cls) + bias.double()[None, :, None, None]
            # the transform's fp32 evaluation (a few ulp of |v|) on top of the forward family's bound, as test_gpu_kernels.py does
            lim = (U20 + 2.0 ** -20) * folded_conv(v.abs(), {c: t.abs() for c, t in cls.items()}) + \
                U24 * folded_conv(torch.ones_like(v), {c: t.abs() for c, t in cls.items()}) + 2.0 ** -23 * ref.abs()
        else:
            ref = F.conv2d(v, wt.double(), bias.double(), padding=1)
            lim = conv_bound(v, wt.double(), 1) + 2.0 ** -20 * F.conv2d(v.abs(), wt.double().abs(), padding=1) + 2.0 ** -23 * ref.abs()
    r = ratio_check(nchw(out)[it], ref, lim, f"{name} p{bits} output")
    gamma, beta = 1 + 0.1 * torch.randn(Cout), 0.1 * torch.randn(Cout)
    fl = torch.randn(B, 2 * Cout) * 0.3 if film else None
    cf = torch.empty(3, B, Cout, device="cuda")
    gd, bd, fd = gamma.cuda(), beta.cuda(), (fl.cuda() if film else None)         # (kept alive across the call)
    _ck(eng, eng.lib.cddpm_op_gn_coef_rec(eng._h, _p(rec), rec.shape[1], Cout, None, 0, 0, _p(gd), _p(bd), _p(fd), _p(cf), B, H * W, None),
        "gn_coef_rec")
    torch.cuda.synchronize()
    rg = gn_check(nchw(out)[it].double(), cf.cpu().double()[:, it], gamma, beta, fl[it] if film else None, ratio)
    print(name, bits, f"output err/bound {r:.3f}  normalised err / 1e-5 (1 + ratio) {rg:.3f}")


def gn_check(o64, cf, gamma, beta, fl, ratio):
    C = o64.shape[1]
    ref = F.group_norm(o64, 32, gamma.double(), beta.double(), eps=1e-5)
    if fl is not None:
        ref = ref * (1 + fl.double()[:, :C, None, None]) + fl.double()[:, C:, None, None]
    got = (o64 - cf[0][:, :, None, None]) * cf[1][:, :, None, None] + cf[2][:, :, None, None]
    err = float((got - ref).abs().max())
    bound = 1e-5 * (1 + ratio) * (1 + (float(fl.abs().max()) if fl is not None else 0.0))
    assert err <= bound, (err, bound)
    return err / bound


@gpu
@pytest.mark.parametrize("ratio", [0.0, 100.0])
def test_gn_coef_rec_two_sources_of_different_record_kinds(eng, ratio):
    """cddpm_op_gn_coef_rec on cat[x0, x1] where x0 comes from a 3x3 convolution (records of kind 0) and x1 from a folded-upsample one
    (kind 1; cddpm_stat_records) -- the decoder's input GroupNorm after the skip concatenation -- with FiLM, against float64 GroupNorm of the
    two outputs as stored"""
    torch.manual_seed(int(ratio) + 5)
    B, H, W, Cin, C0, C1 = 2, 16, 32, 64, 256, 128
    assert eng.lib.cddpm_stat_records(H, W, 0) != eng.lib.cddpm_stat_records(H, W, 1)
    x = torch.randn(B, Cin, H, W)
    xs = torch.randn(B, Cin, H // 2, W // 2)
    w0 = torch.randn(C0, Cin, 3, 3) / (Cin * 9) ** 0.5
    w1 = torch.randn(C1, Cin, 3, 3) / (Cin * 9) ** 0.5 * 0.5
    e0, e1 = weight_exp(eng, w0), weight_exp(eng, w1, 4.0)
    b0, b1 = ratio * (1 + 0.05 * torch.randn(C0)), -ratio * (1 + 0.05 * torch.randn(C1))
    o0, r0 = conv_packed(eng, nhwc(x), pack(eng, w0, 0, e0), e0, C0, 3, B, H, W, bias=b0.cuda(), stats=True)
    o1, r1 = conv_packed(eng, nhwc(xs), pack(eng, w1, 2, e1), e1, C1, 3, B, H, W, folded=True, bias=b1.cuda(), stats=True)
    C = C0 + C1
    gamma, beta, fl = 1 + 0.1 * torch.randn(C), 0.1 * torch.randn(C), torch.randn(B, 2 * C) * 0.3
    cf = torch.empty(3, B, C, device="cuda")
    gd, bd, fd = gamma.cuda(), beta.cuda(), fl.cuda()
    _ck(eng, eng.lib.cddpm_op_gn_coef_rec(eng._h, _p(r0), r0.shape[1], C0, _p(r1), r1.shape[1], C1, _p(gd), _p(bd), _p(fd), _p(cf), B, H * W, None),
        "gn_coef_rec")
    torch.cuda.synchronize()
    o64 = torch.cat([nchw(o0), nchw(o1)], 1).double()
    rg = gn_check(o64, cf.cpu().double(), gamma, beta, fl, ratio)
    print(f"two record kinds, |mean|/sigma {ratio:g}: normalised err / bound {rg:.3f}")


# ---- D: the decoder's GroupNorm backward as the step calls it -------------------------------------------------------------------------
GNB = [
    # C0, C1, film, silu, ratio, add
    (256, 128, True, True, 0.0, True),
    (256, 256, True, True, 100.0, True),
    (128, 128, False, True, 10.0, False),
    (256, 256, False, False, 0.0, True),
    (256, 0, True, True, 100.0, True),
]


@gpu
@pytest.mark.parametrize("C0,C1,film,silu,ratio,add", GNB)
def test_gn_silu_backward_two_sources_records_and_add(eng, C0, C1, film, silu, ratio, add):
    """cddpm_op_gn_silu_backward with the arguments training.py::gn_bwd passes and the engine wrapper does not: a two-source input
    (x1_dev / dx1_dev), the statistics records of the producing convolutions (rec_dev / nrec; |mean| / sigma up to 100 through the bias) and
    add_dev, with / without FiLM and SiLU; against float64 autograd of the outputs as stored. Bound of
    test_gpu_train_ops.py::test_gn_film_silu_backward_vs_autograd: 2e-5 of each gradient's largest element"""
    torch.manual_seed(C0 + C1 + int(ratio) + 2 * int(film) + int(silu))
    B, H, W, Cin = 2, 8, 32, 64
    C = C0 + C1
    wts = [torch.randn(c, Cin, 3, 3) / (Cin * 9) ** 0.5 for c in (C0, C1) if c]
    srcs = []
    for i, wt in enumerate(wts):
        e = weight_exp(eng, wt)
        bias = ratio * (1 + 0.05 * torch.randn(wt.shape[0])) * (1 if i == 0 else -1)
        srcs.append(conv_packed(eng, nhwc(torch.randn(B, Cin, H, W)), pack(eng, wt, 0, e), e, wt.shape[0], 3, B, H, W, bias=bias.cuda(), stats=True))
    (x0, r0), (x1, r1) = srcs[0], (srcs[1] if C1 else (None, None))
    rec = torch.cat([r0, r1], dim=2).contiguous() if C1 else r0
    gamma, beta = 1 + 0.1 * torch.randn(C), 0.1 * torch.randn(C)
    fl = torch.randn(B, 2 * C) * 0.3 if film else None
    da = torch.randn(B, C, H, W)
    addt = torch.randn(B, C, H, W) if add else None
    dx0, dx1 = torch.empty_like(x0), (torch.empty_like(x1) if C1 else None)
    dg, dbt = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dfl = torch.empty(B, 2 * C, device="cuda") if film else None
    dad, gd, bd, fd, ad = nhwc(da), gamma.cuda(), beta.cuda(), (fl.cuda() if film else None), (nhwc(addt) if add else None)
    _ck(eng, eng.lib.cddpm_op_gn_silu_backward(eng._h, _p(x0), _p(x1), C1, _p(dad), _p(gd), _p(bd), _p(fd), int(silu), _p(dx0), _p(dx1), _p(dg),
                                               _p(dbt), _p(dfl), _p(rec), rec.shape[1], _p(ad), B, H * W, C, None), "gn_silu_backward")
    torch.cuda.synchronize()
    xin = torch.cat([nchw(x0)] + ([nchw(x1)] if C1 else []), 1).double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    f64 = fl.double().requires_grad_(True) if film else None
    u = F.group_norm(xin, 32, g64, b64, eps=1e-5)
    if film:
        u = u * (1 + f64[:, :C, None, None]) + f64[:, C:, None, None]
    (F.silu(u) if silu else u).backward(da.double())
    want_dx = xin.grad + (addt.double() if add else 0)
    got_dx = torch.cat([nchw(dx0)] + ([nchw(dx1)] if C1 else []), 1).double()

    def rel(g, r):
        return float((g.double().cpu() - r).abs().max() / (r.abs().max() + 1e-12))
    r = {"dx": rel(got_dx, want_dx), "dgamma": rel(dg, g64.grad), "dbeta": rel(dbt, b64.grad)}
    if film:
        r["dfilm"] = rel(dfl, f64.grad)
    print(C0, C1, film, silu, ratio, add, {k: f"{v / 2e-5:.3f}" for k, v in r.items()})
    assert max(r.values()) < 2e-5, r


# ---- E: small edges ------------------------------------------------------------------------------------------------------------------
@gpu
def test_grad_check_finds_every_non_finite_position(eng):
    """cddpm_op_grad_check ORs 1 into ctrl[0] for a single inf, -inf or NaN anywhere: first and last element, each tail position of a length
    n % 4 = 1, 2, 3, and beyond the first sweep of its 2048-block grid-stride loop (n > 2^21); the largest finite float and subnormals do not"""
    lib = eng.lib
    ctrl = torch.zeros(8, dtype=torch.int32, device="cuda")

    def flag(g):
        ctrl.zero_()
        _ck(eng, lib.cddpm_op_grad_check(eng._h, g.data_ptr(), g.numel(), ctrl.data_ptr(), None), "grad_check")
        torch.cuda.synchronize()
        return int(ctrl[0].item())

    big = 2 ** 22 + 3
    base = torch.randn(big, device="cuda")
    for n in (1, 2, 3, 4, 1001, 1002, 1003, 1028, 2 ** 21 + 1, big):
        g = base[:n].clone()
        assert flag(g) == 0, n
        finite = g.clone()
        finite[0], finite[n - 1] = 3.4028234e38, -1.0e-45
        if n > 2:
            finite[n // 2] = 1.0e-40
        assert flag(finite) == 0, ("finite values flagged", n)
        positions = {0, n - 1} | {(n & ~3) + t for t in range(n & 3)} | ({2 ** 21 + 5, n - 2} if n > 2 ** 21 + 5 else set())
        for pos in sorted(positions):
            for v in (float("inf"), float("-inf"), float("nan")):
                g2 = g.clone()
                g2[pos] = v
                assert flag(g2) == 1, (n, pos, v)


@gpu
def test_absmax_tail_negative_and_subnormal(eng):
    """cddpm_op_absmax = max |x| exactly: the maximum in the last (tail) element, a negative maximum, only subnormals, a length beyond one
    sweep of its 1024-block grid"""
    out = torch.zeros(1, device="cuda")

    def am(x):
        _ck(eng, eng.lib.cddpm_op_absmax(eng._h, x.data_ptr(), x.numel(), out.data_ptr(), None), "absmax")
        torch.cuda.synchronize()
        return float(out.item())

    torch.manual_seed(4)
    for n in (1, 3, 1027, 2 ** 18 + 1, 2 ** 20 + 7):
        x = torch.rand(n, device="cuda") - 0.5
        x[n - 1] = 7.25
        assert am(x) == 7.25, n
        x[n - 1] = -9.5
        assert am(x) == 9.5, n
        s = (torch.rand(n, device="cuda") * 1e-39).clone()
        s[n // 3] = -1.1e-38
        assert 0 < am(s) == float(s.abs().max().item()), n
    assert am(torch.zeros(5, device="cuda")) == 0.0
