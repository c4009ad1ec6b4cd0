"""GPU: the precision-16 convolution operators of the context encoder (csrc/encoder_train_p16.hip behind cddpm_op_enc_pack_w_p16 /
_conv_p16 / _conv_wgrad_p16), one call at a time. The yardstick is float64 arithmetic on the SAME rounded operands (t.half().double()):
an fp16 x fp16 product is exact in fp32, so what is left is fp32 accumulation, for which tests/test_gpu_encoder_ops.py's own limit of
5e-6 of the result's maximum holds; an end-to-end tolerance against an independent run means nothing here (training-mode BatchNorm
amplifies a single convolution's 3e-4 to several percent). Reference semantics: torch.nn.Conv2d(bias=False, padding=k//2) under fp16
autocast, what the reference's `precision: 16` (configs/trainer/default.yaml:7) makes of timm's ResNet
(src/models/modules/DDPM_encoder.py:21-23)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg

pytestmark = pytest.mark.gpu

LIMIT = 5e-6                 # fp32 accumulation of exact products, relative to the result's maximum (test_gpu_encoder_ops.py)
CASES = [(3, 64, 64, 3, 1, 7, 9), (3, 64, 128, 3, 2, 9, 7), (3, 128, 64, 1, 1, 5, 6), (3, 64, 128, 1, 2, 8, 5), (3, 256, 64, 3, 2, 4, 4),
         (3, 512, 2048, 1, 1, 2, 2), (3, 2048, 512, 1, 1, 2, 2),       # few rows, long contraction: the split path
         (3, 512, 512, 3, 2, 3, 3),                                    # odd size, stride 2: three parity classes of input pixels
         (1, 64, 64, 3, 1, 1, 1)]


@pytest.fixture(scope="module")
def ops():
    tr = load_pkg("training")
    o = tr.UNetTrainer({"w": torch.zeros(64)}, device=torch.device("cuda", 0))
    o._fit(4, 64, 64)
    return o


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu().double()


def rounded(t):
    """what the operator makes of an fp32 operand: torch's own round-to-nearest-even conversion, then exact"""
    return t.float().half().double()


def images(ops, w):
    """fp16 weight images (forward, input gradient) of the float64 weight w [Cout][Cin][K][K]"""
    Cout, Cin, K, _ = w.shape
    wd = w.float().cuda().contiguous()
    wf, wdt = (torch.empty(wd.numel(), dtype=torch.float16, device="cuda") for _ in range(2))
    assert ops.lib.cddpm_op_enc_pack_w_p16(ops.h, wd.data_ptr(), Cout, Cin, K, wf.data_ptr(), wdt.data_ptr(), None) == 0, ops.lib.cddpm_last_error(ops.h)
    return wf, wdt


def run(ops, x, w, dy, stride, roles="ydw"):
    """the three roles on the device from float64 NCHW x, w, dy -> (y, dx, dw) as float64 NCHW / PyTorch layout (None where not asked)"""
    lib, h = ops.lib, ops.h
    B, Cin, H, W = x.shape
    Cout, _, K, _ = w.shape
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    wf, wdt = images(ops, w)
    xg, dyg = nhwc(x), nhwc(dy)
    y = dx = dw = None
    if "y" in roles:
        yg = torch.empty(B, Ho, Wo, Cout, device="cuda")
        assert lib.cddpm_op_enc_conv_p16(h, xg.data_ptr(), wf.data_ptr(), yg.data_ptr(), B, H, W, Cin, Cout, K, stride, 0, None) == 0, lib.cddpm_last_error(h)
        y = nchw(yg)
    if "d" in roles:
        dxg = torch.empty(B, H, W, Cin, device="cuda")
        assert lib.cddpm_op_enc_conv_p16(h, dyg.data_ptr(), wdt.data_ptr(), dxg.data_ptr(), B, H, W, Cin, Cout, K, stride, 1, None) == 0, lib.cddpm_last_error(h)
        dx = nchw(dxg)
    if "w" in roles:
        dwg = torch.empty(Cout, Cin, K, K, device="cuda")
        assert lib.cddpm_op_enc_conv_wgrad_p16(h, xg.data_ptr(), dyg.data_ptr(), dwg.data_ptr(), B, H, W, Cin, Cout, K, stride, None) == 0, lib.cddpm_last_error(h)
        dw = dwg.cpu().double()
    torch.cuda.synchronize()
    return y, dx, dw


def reference(x, w, dy, stride):
    """float64 convolution, input gradient and weight gradient of the operands as given"""
    K = w.shape[2]
    y = F.conv2d(x, w, None, stride=stride, padding=K // 2)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=stride, padding=K // 2)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=stride, padding=K // 2)
    return y, dx, dw


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def make(B, Cin, Cout, K, stride, H, W):
    torch.manual_seed(Cin + Cout + K + stride + H)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64)
    w = torch.randn(Cout, Cin, K, K, dtype=torch.float64) / (Cin * K * K) ** 0.5
    dy = torch.randn(B, Cout, (H + stride - 1) // stride, (W + stride - 1) // stride, dtype=torch.float64)
    return x, w, dy


@pytest.mark.parametrize("B,Cin,Cout,K,stride,H,W", CASES)
def test_operators_against_float64_on_rounded_operands(ops, B, Cin, Cout, K, stride, H, W):
    x, w, dy = make(B, Cin, Cout, K, stride, H, W)
    got = run(ops, x, w, dy, stride)
    ref = reference(rounded(x), rounded(w), rounded(dy), stride)
    plain = reference(x, w, dy, stride)
    e = [rel(g, r) for g, r in zip(got, ref)]
    u = [rel(g, r) for g, r in zip(got, plain)]
    print((B, Cin, Cout, K, stride, H, W), "rounded operands: y %.1e dx %.1e dw %.1e" % tuple(e), "| unrounded: y %.1e dx %.1e dw %.1e" % tuple(u))
    assert max(e) < LIMIT
    assert min(u) > 2e-5            # the operands really are rounded to fp16


def crafted(n, seed):
    """n fp32 values: ties, the largest fp16, fp16 subnormals, signed zero, then random values over the normal and subnormal range"""
    special = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 2.0 ** -15, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, -0.0, 0.0,
               1 + 2.0 ** -10, 65519.0, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26, 1 - 2.0 ** -12]
    special = special + [-v for v in special]
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n - len(special), generator=g) * 10.0 ** (torch.rand(n - len(special), generator=g) * 10 - 8)
    r = r.clamp(-65000, 65000)
    return torch.cat([torch.tensor(special, dtype=torch.float32), r.float()])


def same_bits(got, want):
    """bit for bit, but for the sign of a zero: a sum that starts from +0 gives +0 where fp16(x) is -0 (IEEE 754: (+0) + (-0) = +0 to
    nearest), as the float64 yardstick of the test above does"""
    got, want = got.float().contiguous(), want.float().contiguous()
    nz = want != 0
    return bool(torch.equal(got.view(torch.int32)[nz], want.view(torch.int32)[nz])) and bool((got[~nz] == 0).all())


def test_rounding_bit_for_bit(ops):
    """identity weights pass the rounded operand through: forward and input gradient return v.half().float(); a one-hot x makes the weight
    gradient the rounded dz rows"""
    lib, h = ops.lib, ops.h
    B, H, W, Cc = 1, 8, 8, 64
    v = crafted(B * H * W * Cc, 1)
    v = v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(2))].reshape(B, H, W, Cc)
    want = v.half().float()
    assert float(want[v == 1 + 2.0 ** -11][0]) == 1.0 and float(want[v == 1 + 3 * 2.0 ** -11][0]) == 1 + 2.0 ** -9     # ties to even
    assert float(want[v == 2.0 ** -25][0]) == 0.0 and float(want[v == 3 * 2.0 ** -25][0]) == 2.0 ** -23 and float(want[v == 2.0 ** -24][0]) == 2.0 ** -24
    wf, wdt = images(ops, torch.eye(Cc, dtype=torch.float64).reshape(Cc, Cc, 1, 1))
    vg = v.cuda().contiguous()
    for transposed, img in ((0, wf), (1, wdt)):
        out = torch.full((B, H, W, Cc), 7.0, device="cuda")
        assert lib.cddpm_op_enc_conv_p16(h, vg.data_ptr(), img.data_ptr(), out.data_ptr(), B, H, W, Cc, Cc, 1, 1, transposed, None) == 0, lib.cddpm_last_error(h)
        torch.cuda.synchronize()
        assert same_bits(out.cpu(), want), ("input gradient" if transposed else "forward")
    onehot = torch.eye(Cc).reshape(B, H, W, Cc).cuda().contiguous()          # pixel p has channel p set
    dw = torch.full((Cc, Cc, 1, 1), 7.0, device="cuda")
    assert lib.cddpm_op_enc_conv_wgrad_p16(h, onehot.data_ptr(), vg.data_ptr(), dw.data_ptr(), B, H, W, Cc, Cc, 1, 1, None) == 0, lib.cddpm_last_error(h)
    torch.cuda.synchronize()
    assert same_bits(dw.cpu().reshape(Cc, Cc).t(), want.reshape(H * W, Cc))  # dw[co][ci] = dz[pixel ci][co]


def test_range(ops):
    """|v| > 65504 rounds to inf, as torch's .half(): what it reaches is non-finite and everything else is as good as before; most of a
    dz scaled into the fp16 subnormal range is still multiplied as .half() rounds it"""
    B, Cin, Cout, K, stride, H, W = 3, 64, 128, 3, 2, 9, 7
    x, w, dy = make(B, Cin, Cout, K, stride, H, W)
    xb = x.clone()
    xb[1, 5, 4, 3] = 7e4
    ind = torch.zeros_like(x)
    ind[1, 5, 4, 3] = 1
    reach = F.conv2d(ind, torch.ones_like(w), None, stride=stride, padding=K // 2) > 0
    assert 0 < int(reach.sum()) < reach.numel()
    y, _, _ = run(ops, xb, w, dy, stride, roles="y")
    ref = reference(rounded(x), rounded(w), rounded(dy), stride)
    assert not torch.isfinite(y[reach]).any()
    assert float((y[~reach] - ref[0][~reach]).abs().max() / ref[0].abs().max()) < LIMIT
    # a dz of that size: the weight gradients of its output channel are non-finite, and the gradient check sees them
    dyb = dy.clone()
    dyb[2, 17, 1, 2] = -7e4
    lib, h = ops.lib, ops.h
    dwg = torch.empty(Cout, Cin, K, K, device="cuda")
    xg, dyg = nhwc(x), nhwc(dyb)
    assert lib.cddpm_op_enc_conv_wgrad_p16(h, xg.data_ptr(), dyg.data_ptr(), dwg.data_ptr(), B, H, W, Cin, Cout, K, stride, None) == 0, lib.cddpm_last_error(h)
    ctrl = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.cddpm_op_grad_check(h, dwg.data_ptr(), dwg.numel(), ctrl.data_ptr(), None) == 0, lib.cddpm_last_error(h)
    torch.cuda.synchronize()
    dw = dwg.cpu().double()
    hit = torch.zeros(Cout, dtype=torch.bool)
    hit[17] = True
    assert not torch.isfinite(dw[hit]).any() and torch.isfinite(dw[~hit]).all()
    assert float((dw[~hit] - ref[2][~hit]).abs().max() / ref[2].abs().max()) < LIMIT
    assert int(ctrl[0].item()) == 1
    ctrl.zero_()
    clean = ref[2].float().cuda()
    assert lib.cddpm_op_grad_check(h, clean.data_ptr(), clean.numel(), ctrl.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(ctrl[0].item()) == 0
    # gradual underflow: dz 2^-18 puts most of it below 2^-14
    dys = dy * 2.0 ** -18
    assert float((dys.abs() < 2.0 ** -14).double().mean()) > 0.5
    _, dx, dw = run(ops, x, w, dys, stride, roles="dw")
    _, rdx, rdw = reference(rounded(x), rounded(w), rounded(dys), stride)
    e = (rel(dx, rdx), rel(dw, rdw))
    print("dz 2^-18: dx %.1e dw %.1e" % e)
    assert max(e) < LIMIT


def test_two_calls_return_identical_bits(ops):
    x, w, dy = make(3, 512, 2048, 1, 1, 2, 2)
    a, b = run(ops, x, w, dy, 1), run(ops, x, w, dy, 1)
    for u, v in zip(a, b):
        assert torch.equal(u.float().view(torch.int32), v.float().view(torch.int32))
