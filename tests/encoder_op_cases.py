"""What the operator tests of the context encoder's training step share (tests/test_encoder_op_cases_host.py, test_gpu_encoder_ops_edges.py,
test_gpu_encoder_training_calls.py): the case tables, the plans the library itself states for a case, seeded operands and the float64
references, each computed once per process and never modified. Nothing here needs a GPU.

The tables are data. Which plan a case reaches -- the contraction split Z of a convolution (enc_conv_split), the pixel ranges P of a weight
gradient (enc_wgrad_parts, enc_wgrad_p16_parts), the chunks of a BatchNorm reduction (enc_bn_chunks: the rule of the
cddpm_op_enc_bn_* entries in csrc/cddpm_ops.hip; the BatchNorm itself is csrc/batchnorm_train.hip) -- is read back from the library's own
size queries (cddpm_op_enc_*_scratch of include/cddpm.h: host code): a request is a whole number of planes, so the plane count is the
quotient. No plan formula is restated here; tests/test_encoder_op_cases_host.py asserts that the tables reach the plans they are there for.

Reference semantics: torch.nn.Conv2d(bias=False, padding=k//2), BatchNorm2d in training mode, MaxPool2d(3, 2, 1), as timm's ResNet uses them
(reference src/models/modules/DDPM_encoder.py:21-23)."""
import functools

import torch
import torch.nn.functional as F

from conftest import load_pkg

# ---------------------------------------------------------------------------------------------------------------- convolutions
# (B, Cin, Cout, K, stride, H, W) -> the roles the fp32 operators take it in: y forward, d input gradient, w weight gradient
CONV_CASES = {
    (3, 64, 64, 3, 1, 7, 9): "ydw", (3, 64, 128, 3, 2, 9, 7): "ydw", (3, 128, 64, 1, 1, 5, 6): "ydw", (3, 64, 128, 1, 2, 8, 5): "ydw",
    (3, 256, 64, 3, 2, 4, 4): "ydw",                                  # the five of tests/test_gpu_encoder_ops.py
    (3, 512, 2048, 1, 1, 2, 2): "ydw", (3, 2048, 512, 1, 1, 2, 2): "ydw",       # few rows, long contraction
    (3, 512, 512, 3, 2, 3, 3): "ydw",                                 # odd size, stride 2
    (1, 64, 64, 3, 1, 1, 1): "ydw",                                   # one pixel: eight of nine taps are padding
    (5, 64, 64, 3, 1, 19, 21): "ydw",                                 # 1995 rows: 32 row tiles, the last of 11 rows; P at its cap, ragged ranges
    (2, 64, 64, 1, 1, 23, 29): "ydw",                                 # 1334 rows, unsplit contraction, 1x1 weight gradient over many ranges
    (2, 128, 64, 3, 2, 33, 31): "ydw",                                # odd size at stride 2: every parity class of the input gradient
    (2, 192, 192, 3, 1, 21, 20): "ydw",                               # a P that is neither 1 nor the cap
    (3, 192, 64, 3, 2, 5, 5): "ydw",                                  # forward: 108 steps over 8 planes, an uneven split
    (2, 48, 64, 3, 1, 9, 11): "y",                                    # contraction 48: a multiple of 16, not of 64
    (2, 64, 80, 3, 2, 9, 11): "d",                                    # contraction 80 in the input gradient
    (2, 64, 64, 3, 2, 2, 3): "ydw",
}
ROLES = {"y": "forward", "d": "input gradient", "w": "weight gradient"}
STEP = {32: 16, 16: 64}          # contraction channels one step of the forward / input-gradient kernels multiplies (csrc/encoder_train*.hip)
SPLIT_CASES = [(3, 512, 2048, 1, 1, 2, 2), (3, 192, 64, 3, 2, 5, 5), (2, 192, 192, 3, 1, 21, 20)]     # determinism: split contraction, folded ranges


def conv_id(case):
    return "x".join(map(str, case))


def out_hw(case):
    _B, _ci, _co, _K, st, H, W = case
    return (H + st - 1) // st, (W + st - 1) // st


def p16_accepts(case):
    """the precision-16 operators take the cases whose Cin and Cout are multiples of 64 (include/cddpm.h)"""
    return case[1] % 64 == 0 and case[2] % 64 == 0


def _query(op, *args):
    return load_pkg("training").scratch_query(op, *args)


def _planes(nbytes, plane_bytes, what):
    assert nbytes % plane_bytes == 0, (what, nbytes, plane_bytes)     # every plane here is a multiple of the arena's 256-byte granule
    return nbytes // plane_bytes


def conv_plan(case, precision=32):
    """{role: planes} of `case` as the library plans it: Z for y and d (1: the kernel writes the result itself), P for w. Only the roles
    the operators of that precision take."""
    B, Cin, Cout, K, st, H, W = case
    Ho, Wo = out_hw(case)
    sfx = "_p16" if precision == 16 else ""
    roles = CONV_CASES[case] if precision == 32 else ("ydw" if p16_accepts(case) else "")
    plan = {}
    if "y" in roles:
        plan["y"] = max(1, _planes(_query("enc_conv" + sfx, B, H, W, Cin, Cout, K, st, 0), B * Ho * Wo * Cout * 4, (case, "y")))
    if "d" in roles:
        plan["d"] = max(1, _planes(_query("enc_conv" + sfx, B, H, W, Cin, Cout, K, st, 1), B * H * W * Cin * 4, (case, "d")))
    if "w" in roles:
        n = _query("enc_conv_wgrad" + sfx, B, H, W, Cin, Cout, K, st)
        # precision 16 asks for nothing when one range of a 1x1 writes dw itself; the fp32 operator always folds at least one plane
        assert n > 0 or (precision == 16 and K == 1), (case, "the weight gradient refuses the case")
        plan["w"] = max(1, _planes(n, K * K * Cin * Cout * 4, (case, "w")))
    return plan


def conv_rows(case, role):
    B, _ci, _co, _K, _st, H, W = case
    Ho, Wo = out_hw(case)
    return B * H * W if role == "d" else B * Ho * Wo


def conv_steps(case, role, precision=32):
    """steps of the forward / input-gradient contraction: taps x contraction channels / step width"""
    _B, Cin, Cout, K, _st, _H, _W = case
    return K * K * (Cout if role == "d" else Cin) // STEP[precision]


def rounded(t):
    """what a precision-16 operator makes of an fp32 operand: torch's own round-to-nearest-even conversion, then exact"""
    return t.float().half().double()


def identity(t):
    return t


@functools.lru_cache(maxsize=None)
def conv_operands(case, kind):
    """(x, w, dy) in float64 NCHW / PyTorch layout, every value an fp32 number. kind `random`: N(0,1), w scaled by the fan-in;
    `integer`: drawn from -2 .. 2, so every product and every partial sum in any order is an integer below 2^24, exact in fp32 -- and in
    fp16 operands."""
    B, Cin, Cout, K, st, H, W = case
    Ho, Wo = out_hw(case)
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + K + st + H + 7 * W + (kind == "integer"))
    shapes = ((B, Cin, H, W), (Cout, Cin, K, K), (B, Cout, Ho, Wo))
    if kind == "integer":
        return tuple(torch.randint(-2, 3, s, generator=g).double() for s in shapes)
    assert kind == "random", kind
    x, w, dy = (torch.randn(s, generator=g) for s in shapes)
    return x.double(), (w / (Cin * K * K) ** 0.5).double(), dy.double()


@functools.lru_cache(maxsize=None)
def conv_reference(case, kind, precision=32):
    """float64 (y, dx, dw) of conv_operands(case, kind), the operands rounded to fp16 first at precision 16"""
    r = rounded if precision == 16 else identity
    x, w, dy = (r(t) for t in conv_operands(case, kind))
    st, K = case[4], case[3]
    y = F.conv2d(x, w, None, stride=st, padding=K // 2)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, stride=st, padding=K // 2)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=st, padding=K // 2)
    return y, dx, dw


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
BN_CASES = [(4, 64, 6, 5),          # N = 120: one chunk
            (3, 64, 19, 9),         # N = 513: two chunks, 257 + 256
            (2, 128, 23, 29),       # N = 1334: five chunks, ragged
            (2, 64, 65, 65),        # N = 8450: the cap of 32 chunks, ragged; HW = 4225 puts the sample boundary inside a chunk
            (16, 2048, 1, 1)]       # N = 16: the widest channel count, the real last stage at a 32 x 32 input
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# relu / shortcut operand / per-sample scale (with a zero) / dres requested / running statistics (random start, or both NULL) /
# the backward's y (NULL is legal only without relu)
BN_OPTIONS = [dict(relu=True, res=False, drop=False, dres=True, run=True, y_null=False),
              dict(relu=True, res=True, drop=True, dres=True, run=True, y_null=False),
              dict(relu=False, res=False, drop=False, dres=False, run=False, y_null=True),
              dict(relu=False, res=True, drop=True, dres=True, run=True, y_null=False),
              dict(relu=True, res=True, drop=False, dres=False, run=False, y_null=False)]


def bn_option_id(o):
    return "-".join(k for k in ("relu", "res", "drop", "dres", "run", "y_null") if o[k]) or "plain"


def bn_chunks(case, backward=False):
    B, C_, H, W = case
    n = _query("enc_bn_backward" if backward else "enc_bn_forward", B * H * W, H * W, C_)
    if backward:
        n -= 256 * ((2 * C_ * 4 + 255) // 256)           # the two per-channel means of the elementwise pass, one request of its own
    return _planes(n, 2 * C_ * 8, (case, backward))


def sample_scale(B):
    """a stochastic-depth scale per sample: all different, sample 1 (and 7) dropped"""
    s = 1.0 + 0.125 * torch.arange(B, dtype=torch.float64)
    s[1::6] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def bn_operands(case, ratio=0.0):
    """float64 tensors of fp32 values: z [B,C,H,W] (sigma 1.5, mean 0.3, or |mean| / sigma = ratio with the sign alternating by channel),
    gamma, beta, res, dy, and a random start of the running statistics"""
    B, C_, H, W = case
    g = torch.Generator().manual_seed(C_ + 3 * H + 5 * W + int(ratio))
    f = lambda *s: torch.randn(*s, generator=g)
    z = f(B, C_, H, W) * 1.5
    if ratio:
        sign = 1.0 - 2.0 * (torch.arange(C_) % 2).float()
        z = z + (1.5 * ratio * sign).reshape(1, C_, 1, 1)
    else:
        z = z + 0.3
    d = dict(z=z, gamma=1 + 0.2 * f(C_), beta=0.2 * f(C_), res=f(B, C_, H, W), dy=f(B, C_, H, W), run_mean=0.5 * f(C_),
             run_var=0.5 + torch.rand(C_, generator=g))
    return {k: v.float().double() for k, v in d.items()}


def bn_reference(z, gamma, beta, dy, relu, mask=None, res=None, ss=None, run_mean=None, run_var=None, dtype=torch.float64):
    """training-mode BatchNorm (+ per-sample scale, shortcut, ReLU on the GIVEN mask: the branch of the network the implementation is on,
    see oracle/encoder_oracle.py) and its backward by autograd, in `dtype` on the CPU. NCHW. -> dict of y, mean, rstd, run_mean, run_var
    (updated copies, None without), dz, dres, dgamma, dbeta"""
    t = lambda v: None if v is None else v.detach().to(dtype).clone()
    z, gamma, beta, res = t(z).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True), t(res)
    if res is not None:
        res.requires_grad_(True)
    rm, rv = t(run_mean), t(run_var)
    u = F.batch_norm(z, rm, rv, gamma, beta, True, BN_MOMENTUM, BN_EPS)
    if ss is not None:
        u = u * t(ss).reshape(-1, 1, 1, 1)
    if res is not None:
        u = u + res
    y = u * mask.to(dtype) if relu else u
    out = dict(y=y.detach(), run_mean=rm, run_var=rv)
    if dy is not None:
        y.backward(t(dy))
        out.update(dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=(t(dy) * mask.to(dtype) if relu else t(dy)))
    zd = z.detach()
    out["mean"] = zd.mean(dim=(0, 2, 3))
    out["rstd"] = 1.0 / torch.sqrt(zd.var(dim=(0, 2, 3), unbiased=False) + BN_EPS)
    return out


# ---------------------------------------------------------------------------------------------------------------- pooling, stem
MAXPOOL_SHAPES = [(9, 11), (8, 6), (1, 1), (2, 5), (32, 32)]
MAXPOOL_CHANNELS = [4, 64]
AVGPOOL_CASES = [(3, 64, 1), (2, 2048, 4), (3, 68, 99)]          # (B, C, HW); B C = 192 and 204 are no multiples of the 256-thread block
STEM_CASES = [(3, 21, 18), (1, 7, 7), (2, 32, 32), (2, 33, 47)]  # (B, H, W); (1, 7, 7) has 16 output pixels for the 32 pixel ranges of the weight gradient


@functools.lru_cache(maxsize=None)
def maxpool_input(kind, B, C_, H, W):
    """(x, dy) float64 NCHW. `ties`: x drawn from {-1, 0, 1} -- most windows have a tied maximum; `random`: N(0,1) fp32 values, no ties.
    dy is drawn from the integers -3 .. 3: an input element collects up to four windows, and a sum of four such values is exact in fp32"""
    assert kind in ("ties", "random"), kind
    g = torch.Generator().manual_seed(31 * H + W + C_ + (kind == "ties"))
    x = torch.randint(-1, 2, (B, C_, H, W), generator=g).double() if kind == "ties" else torch.randn(B, C_, H, W, generator=g).double()
    dy = torch.randint(-3, 4, (B, C_, (H + 1) // 2, (W + 1) // 2), generator=g).double()
    return x, dy


def tie_share(x):
    """share of the 3x3 / 2 windows (padding 1) of x [B,C,H,W] whose maximum is taken more than once"""
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    u = xp.unfold(2, 3, 2).unfold(3, 3, 2).reshape(x.shape[0], x.shape[1], (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2, 9)
    return float(((u == u.amax(dim=-1, keepdim=True)).sum(-1) > 1).double().mean())


def maxpool_first(x, dy=None):
    """3x3 / 2 max pool, padding 1, by brute force: every window is scanned in row-major order and a later element replaces the maximum
    only when it is strictly larger, so dy goes to the FIRST maximum. -> (y, dx or None)"""
    B, C_, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y = torch.empty(B, C_, Ho, Wo, dtype=x.dtype)
    dx = None if dy is None else torch.zeros_like(x)
    bi, ci = torch.meshgrid(torch.arange(B), torch.arange(C_), indexing="ij")
    for yo in range(Ho):
        for xo in range(Wo):
            best = by = bx = None
            for ky in range(3):
                for kx in range(3):
                    yi, xi = 2 * yo + ky - 1, 2 * xo + kx - 1
                    if not (0 <= yi < H and 0 <= xi < W):
                        continue
                    v = x[:, :, yi, xi]
                    if best is None:
                        best, by, bx = v.clone(), torch.full((B, C_), yi), torch.full((B, C_), xi)
                    else:
                        m = v > best
                        best, by, bx = torch.where(m, v, best), torch.where(m, torch.full_like(by, yi), by), torch.where(m, torch.full_like(bx, xi), bx)
            y[:, :, yo, xo] = best
            if dx is not None:
                dx.index_put_((bi, ci, by, bx), dy[:, :, yo, xo], accumulate=True)
    return y, dx


def maxpool_torch(x, dy):
    """torch's float64 max_pool2d(3, 2, 1) and its backward"""
    x = x.detach().double().clone().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(dy.double())
    return y.detach(), x.grad


def maxpool_backward_fp32_order(x, dy):
    """torch's float64 max-pool backward of fp32 values with the at most four windows of an input element added in fp32, in the row-major
    order of the windows (what a gather over the windows of an element gives). The windows are split by the parity of (yo, xo): the
    windows of one class do not overlap, so each class's float64 backward holds single fp32 values and nothing rounds; the classes are
    then added in fp32, the lower window first. For a dy whose sums are exact in fp32 this is maxpool_torch's dx."""
    B, C_, H, W = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    cls = {}
    for py in (0, 1):
        for px in (0, 1):
            m = torch.zeros(Ho, Wo, dtype=torch.float64)
            m[py::2, px::2] = 1.0
            cls[py, px] = maxpool_torch(x, dy.double() * m)[1].float()
    fy = ((torch.arange(H) // 2) % 2).reshape(H, 1).expand(H, W)          # parity of the lower window row of input row yi, and of column xi
    fx = ((torch.arange(W) // 2) % 2).reshape(1, W).expand(H, W)
    pick = lambda ay, ax: sum(torch.where((ay == py) & (ax == px), cls[py, px], torch.zeros(())) for py in (0, 1) for px in (0, 1))
    return (((pick(fy, fx) + pick(fy, 1 - fx)) + pick(1 - fy, fx)) + pick(1 - fy, 1 - fx)).double()


@functools.lru_cache(maxsize=None)
def stem_operands(case, kind):
    """(x [B,1,H,W], w [64,1,7,7], dz [B,64,Ho,Wo]) float64 of fp32 values; `integer`: from -2 .. 2"""
    B, H, W = case
    g = torch.Generator().manual_seed(H + 3 * W + (kind == "integer"))
    shapes = ((B, 1, H, W), (64, 1, 7, 7), (B, 64, (H + 1) // 2, (W + 1) // 2))
    if kind == "integer":
        return tuple(torch.randint(-2, 3, s, generator=g).double() for s in shapes)
    assert kind == "random", kind
    return torch.rand(shapes[0], generator=g).double(), (torch.randn(shapes[1], generator=g) / 7).double(), torch.randn(shapes[2], generator=g).double()


@functools.lru_cache(maxsize=None)
def stem_reference(case, kind):
    x, w, dz = stem_operands(case, kind)
    return F.conv2d(x, w, None, stride=2, padding=3), torch.nn.grad.conv2d_weight(x, w.shape, dz, stride=2, padding=3)
