"""What the tests of the memory-bound operators share (tests/test_small_op_cases_host.py, tests/test_gpu_small_ops_edges.py): one table of
cases per operator, seeded operands, float64 references written from each operation's definition, the derived error bounds, and the
mutations a wrong kernel of that kind would produce. Nothing here needs a GPU; everything is computed once per process (lru_cache) and
never modified.

Operators: csrc/small_kernels.hip (conv_in1, head, pool_act, linear), the elementwise / reduction part of csrc/train_kernels.hip
(unpool2, sumpool2, add_inplace, bias_grad, chan_image_corr, head_dgrad, loss, adam, linear_backward) and the stand-alone GroupNorm
statistics sweep of csrc/norm_kernels.hip (gn_coef). Layouts are the kernels': activations NHWC [B,H,W,C], one-channel images [B,H,W],
coefficient planes coef[3][B][C] = (mean, a, d), the head's weight image w9[9][C], the input convolution's w[C][9].

Inputs: every operand is an fp32 number held in float64, |x| in [0.5, 2] with random signs unless a case says otherwise, so that no
contribution to any output is negligible and a dropped term is visible.

Bounds: |got - ref64| <= bound per element, u = 2^-24. bound = n u A 1.01, A = the operation's own expression evaluated in float64 with
every term replaced by its absolute value, n = the number of fp32 roundings on the longest dependency chain to one output as counted
from the kernel source (N_ROUNDINGS, one line of justification each), 1.01 for the second-order terms. Where the device accumulates in
fp64 only the final rounding and the fp32 input transform count. An activation act(x) = SiLU((x - mean) a + d) evaluated in fp32 is
allowed 2^-20 (|x - mean| |a| + |d|) per element (the allowance of tests/test_gpu_kernels.py::
test_conv_domain_mixed_magnitudes_and_weight_outliers), pushed through the absolute-value expression. No bound is fitted to what a
kernel delivers."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SECOND = 1.01            # second-order terms of the first-order bound
ACT = 2.0 ** -20         # the fused activation's own error, per unit of |x - mean| |a| + |d|

# n per operator: fp32 roundings on the longest chain to one output, read from the kernel
N_ROUNDINGS = {
    "conv_in1": "9: acc = bias, then one fma per tap (conv_in1_kernel)",
    "head": "C + 9: C fma from 0 per (pixel, tap) in head_dots_kernel, then bias + up to 9 adds in head_gather_kernel",
    "pool_act": "3: four adds from 0 (the first exact), times 0.25 exact",
    "linear": "4 ceil(K / 256) + 7: four fma per 256-step of a lane, 6 shuffle adds, the bias add",
    "unpool2 (accumulating)": "2: the product and the add (one if contracted to an fma)",
    "sumpool2 (accumulating)": "4: three adds of the 2x2 block from 0, the add of the old value",
    "bias_grad": "1: fp64 sums, rounded once",
    "chan_image_corr": "1: fp64 products and sums of fp32 operands, rounded once (+ the fp32 activation's allowance)",
    "head_dgrad": "9: nine product-adds from 0",
    "loss value": "L2 3, L1 2: d = out - target rounded once (twice in d^2), fp64 sum, the final rounding",
    "loss gradient": "L2 5, L1 4: scale * wb, B * HW, their quotient, d, the product (L1: without d)",
    "adam m": "4: g * unscale, 1 - beta1, the product, the add (beta1 * m: 2)",
    "adam v": "6: g * unscale twice, 1 - beta2, two products, the add",
    "adam p": "the relative errors of lr / bc1, m, the denominator, the quotient and the product, then the subtraction; 1 - beta^step "
              "counts 3 (powf: 1 ulp = 2 u, the subtraction) on 1 + beta^step",
    "gn_coef": "measure of test_groupnorm_statistics_from_the_conv_epilogue_with_large_mean: normalised value to 1e-5 (1 + ratio)",
    "linear_backward dW": "M + 1: one fp32 MFMA accumulation per row of the contraction, times alpha",
    "linear_backward db": "1: fp64 column sums, rounded once",
    "linear_backward dx": "skinny: ceil(N / 32) fma per range + 32 adds of the fold; else N + 1 (GEMM); + 1 for the SiLU' product",
}


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def mags(g, shape, lo=0.5, hi=2.0):
    """fp32 numbers with |x| in [lo, hi] and random signs, as float64"""
    v = lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (v * s).float().double()


def coef_planes(g, B, C):
    """(mean, a, d) per (sample, channel): mean and d of size 0.1, a in [0.75, 1.25]"""
    return torch.stack([mags(g, (B, C)) * 0.1, mags(g, (B, C), 0.75, 1.25).abs(), mags(g, (B, C)) * 0.1]).float().double()


def act64(x, coef):
    """SiLU((x - mean) a + d) on NHWC x with coef [3][B][C]"""
    m, a, d = (coef[i][:, None, None, :] for i in range(3))
    return F.silu((x - m) * a + d)


def affine64(x, coef):
    m, a, d = (coef[i][:, None, None, :] for i in range(3))
    return (x - m) * a + d


def act_allowance(x, coef):
    m, a, d = (coef[i][:, None, None, :] for i in range(3))
    return ACT * ((x - m).abs() * a.abs() + d.abs())


def taps(img, mode="pad", sign=1):
    """[B,H,W] -> [B,H,W,9]: tap t = the image at (y + sign (t / 3 - 1), x + sign (t % 3 - 1)).
    mode `pad`: zero outside the image (the definition). `slice`: the flat neighbour p + dy W + dx within the slice's H W pixels (a
    read that runs across a row end); `flat`: the flat neighbour within all B H W pixels (across a slice end too)."""
    B, H, W = img.shape
    out = []
    for t in range(9):
        dy, dx = sign * (t // 3 - 1), sign * (t % 3 - 1)
        if mode == "pad":
            p = F.pad(img, (1, 1, 1, 1))
            out.append(p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        else:
            flat = img.reshape(B, H * W) if mode == "slice" else img.reshape(1, B * H * W)
            n, o = flat.shape[1], dy * W + dx
            p = F.pad(flat, (W + 1, W + 1))
            out.append(p[:, W + 1 + o:W + 1 + o + n].reshape(B, H, W))
    return torch.stack(out, dim=-1)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def case_id(case):
    return "-".join(str(c).replace(" ", "") for c in case)


GEOMETRIES = {          # (B, H, W) of the one-channel convolutions, with the reason in the kernels' terms
    (3, 5, 7): "105 pixels: a tail block, blocks that straddle slices, odd W",
    (1, 1, 1): "one pixel: eight of nine taps are padding",
    (2, 1, 9): "one row: every vertical tap is padding, the flat neighbour p - W lies in the other slice",
    (2, 9, 1): "one column: every horizontal tap is padding, the flat neighbour p - 1 is the row above",
    (2, 16, 24): "768 pixels, the geometry of tests/arch_cases.py",
}

# ------------------------------------------------------------------------------------------------------------------ conv_in1
CONV_IN1_C = {64: "16 quads, 16 pixel lanes", 128: "32 quads, 8 pixel lanes", 192: "48 quads: 5 lanes, 16 surplus threads on lane 0's second trip",
              320: "80 quads: 3 lanes, 16 surplus threads", 512: "128 quads: 2 pixel lanes"}
CONV_IN1_CASES = {(C, g): f"{CONV_IN1_C[C]}; {GEOMETRIES[g]}" for C in CONV_IN1_C for g in GEOMETRIES}


def conv_in1_ppb(C):
    """pixels per block of conv_in1_kernel: 16 per pixel lane, 256 / (C / 4) lanes"""
    return 16 * (256 // (C // 4))


@functools.lru_cache(maxsize=None)
def conv_in1_operands(case):
    C, (B, H, W) = case
    g = _gen("conv_in1", case)
    return mags(g, (B, H, W)), mags(g, (C, 9)), mags(g, (C,))


def conv_in1_ref(case, mutation=None):
    C, (B, H, W) = case
    x, w, b = conv_in1_operands(case)
    if mutation in ("slice", "flat"):
        out = taps(x, mutation) @ w.t() + b
    else:
        out = nhwc(F.conv2d(x[:, None], w.reshape(C, 1, 3, 3), b, padding=1))
    return _drop(out, mutation)


def conv_in1_bound(case):
    C, _ = case
    x, w, b = conv_in1_operands(case)
    return 9 * U * SECOND * nhwc(F.conv2d(x.abs()[:, None], w.abs().reshape(C, 1, 3, 3), b.abs(), padding=1))


def _drop(out, mutation):
    """the mutations of an elementwise-output kernel: the last pixel of the flat range, or the last channel quad, not computed"""
    if mutation == "last_pixel":
        out = out.clone()
        out.reshape(-1, out.shape[-1])[-1] = 0
    elif mutation == "last_quad":
        out = out.clone()
        out[..., -4:] = 0
    return out


def neighbour_mutations(geom):
    """which wrong-neighbour mutations can show at a geometry: a row end needs a second row, a slice end a second slice"""
    B, H, W = geom
    return (["slice"] if H > 1 else []) + (["flat"] if B > 1 else [])


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_C = {32: "8 quads: the smallest C the entry takes", 128: "the flagship model", 256: "75 KB of LDS: above the 64 KB a launch gets by default",
          384: "96 quads", 512: "150.5 KB of LDS"}
HEAD_GEOMETRIES = dict(GEOMETRIES)
HEAD_GEOMETRIES[(2, 8, 8)] = "128 pixels: two full blocks of 64, no tail"
HEAD_CASES = {(C, g): f"{HEAD_C[C]}; {HEAD_GEOMETRIES[g]}" for C in HEAD_C for g in HEAD_GEOMETRIES}


@functools.lru_cache(maxsize=None)
def head_operands(case):
    C, (B, H, W) = case
    g = _gen("head", case)
    return mags(g, (B, H, W, C)), coef_planes(g, B, C), mags(g, (9, C)), float(mags(g, (1,))[0])


def head_ref(case, mutation=None):
    """out = bias + conv3x3(act(x), w), w[0][c][ky][kx] = w9[3 ky + kx][c]"""
    C, (B, H, W) = case
    x, coef, w9, bias = head_operands(case)
    a = act64(x, coef)
    if mutation is None:
        return F.conv2d(nchw(a), w9.t().reshape(1, C, 3, 3), torch.tensor([bias], dtype=torch.float64), padding=1)[:, 0]
    return head_by_gather(case, mutation)


def head_by_gather(case, mutation=None):
    """the same through the kernel pair's split: P[pixel][tap] = sum_c w9[tap][c] act(x)[pixel][c], out = bias + sum_tap P[neighbour][tap]"""
    C, (B, H, W) = case
    x, coef, w9, bias = head_operands(case)
    a = act64(x, coef)
    if mutation == "last_quad":
        a = a.clone()
        a[..., -4:] = 0
    P = a @ w9.t()                                              # [B,H,W,9]
    mode = mutation if mutation in ("slice", "flat") else "pad"
    out = bias + sum(taps(P[..., t], mode)[..., t] for t in range(9))
    if mutation == "last_pixel":
        out = out.clone()
        out.reshape(-1)[-1] = 0
    return out


def head_bound(case):
    C, (B, H, W) = case
    x, coef, w9, bias = head_operands(case)
    wk = w9.abs().t().reshape(1, C, 3, 3)
    A = abs(bias) + F.conv2d(nchw(act64(x, coef).abs()), wk, padding=1)[:, 0]
    return (C + 9) * U * SECOND * A + F.conv2d(nchw(act_allowance(x, coef)), wk, padding=1)[:, 0]


# ------------------------------------------------------------------------------------------------------------------ pool_act
POOL_ACT_CASES = {(C, g): why for C in (4, 128, 384) for g, why in {
    (3, 6, 10): "45 output pixels: a tail block at every C, slices of odd output width 5",
    (1, 2, 2): "one output pixel",
    (2, 2, 14): "one output row per slice",
}.items()}


@functools.lru_cache(maxsize=None)
def pool_act_operands(case):
    C, (B, H, W) = case
    g = _gen("pool_act", case)
    return mags(g, (B, H, W, C)), coef_planes(g, B, C)


def pool_act_ref(case, mutation=None):
    x, coef = pool_act_operands(case)
    hp, xp = nhwc(F.avg_pool2d(nchw(act64(x, coef)), 2)), nhwc(F.avg_pool2d(nchw(x), 2))
    return _drop(hp, mutation), _drop(xp, mutation)


def pool_act_bound(case):
    x, coef = pool_act_operands(case)
    pool = lambda t: nhwc(F.avg_pool2d(nchw(t), 2))
    return 3 * U * SECOND * pool(act64(x, coef).abs()) + pool(act_allowance(x, coef)), 3 * U * SECOND * pool(x.abs())


# ------------------------------------------------------------------------------------------------------------------ linear
LINEAR_CASES = {        # (M, N, K, silu, bias)
    (1, 1, 4, 0, True): "one output, one quad: lane 0 alone",
    (3, 5, 260, 1, True): "lane 0 takes a second trip; M N = 15 is no multiple of the 4 waves of a block",
    (2, 7, 256, 0, False): "exactly one trip of every lane, no bias",
    (5, 3, 252, 1, True): "the last lane idle",
    (16, 128, 1024, 1, True): "four trips: the emb_layers shape",
    (2, 128, 2048, 0, True): "eight trips: the encoder's fc",
}
LINEAR_REFUSED_K = (6, 255)


@functools.lru_cache(maxsize=None)
def linear_operands(case):
    M, N, K, silu, bias = case
    g = _gen("linear", case)
    return mags(g, (M, K)), mags(g, (N, K)), (mags(g, (N,)) if bias else None)


def linear_ref(case, mutation=None):
    M, N, K, silu, bias = case
    x, w, b = linear_operands(case)
    a = F.silu(x) if silu else x
    if mutation == "last_k4":
        a, w = a[:, :-4], w[:, :-4]
    y = F.linear(a, w, b)
    if mutation == "last_pixel":
        y = y.clone()
        y[-1, -1] = 0
    return y


def linear_bound(case):
    M, N, K, silu, bias = case
    x, w, b = linear_operands(case)
    a = F.silu(x) if silu else x
    A = a.abs() @ w.abs().t() + (b.abs() if bias else 0.0)
    n = 4 * math.ceil(K / 256) + 7
    return n * U * SECOND * A + (ACT * (x.abs() @ w.abs().t()) if silu else 0.0)


# ------------------------------------------------------------------------------------------------------------------ unpool2 / sumpool2 / add_inplace
RESAMPLE_CASES = {      # (B, H, W, C) of the full-resolution tensor
    (3, 6, 10, 4): "one quad per pixel: 180 / 45 threads, slices of odd half width",
    (1, 2, 2, 128): "one half-resolution pixel",
    (2, 4, 14, 192): "48 quads: 5376 threads at full resolution (21 full blocks), 1344 at half (a tail block)",
}
UNPOOL_SCALES = (0.25, 3.0)
ADD_INPLACE_N = {4: "one thread", 1020: "255 threads: a tail block", 1024: "one full block", 1028: "one thread of a second block"}


@functools.lru_cache(maxsize=None)
def resample_operands(case):
    """(half-resolution tensor, full-resolution tensor): each serves as the source of one operator and the old value of the other"""
    B, H, W, C = case
    g = _gen("resample", case)
    return mags(g, (B, H // 2, W // 2, C)), mags(g, (B, H, W, C))


def unpool2_ref(case, scale, accumulate, mutation=None):
    """dx (+)= scale * dyp at (y / 2, x / 2): scale times the nearest x2 upsampling"""
    half, full = resample_operands(case)
    out = nhwc(F.interpolate(nchw(half), scale_factor=2, mode="nearest")) * float(torch.tensor(scale, dtype=torch.float32))
    return _drop(out + full if accumulate else out, mutation)


def unpool2_f32(case, scale):
    """the non-accumulating result as fp32 arithmetic states it: one rounded product"""
    half, _ = resample_operands(case)
    return nhwc(F.interpolate(nchw(half.float()), scale_factor=2, mode="nearest")) * torch.tensor(scale, dtype=torch.float32)


def unpool2_bound(case, scale):
    half, full = resample_operands(case)
    return 2 * U * SECOND * (unpool2_ref(case, scale, False).abs() + full.abs())


def sumpool2_ref(case, accumulate, mutation=None):
    """dxp (+)= the sum of the 2x2 block"""
    half, full = resample_operands(case)
    out = 4 * nhwc(F.avg_pool2d(nchw(full), 2))
    return _drop(out + half if accumulate else out, mutation)


def sumpool2_f32(case):
    """the non-accumulating result as fp32 arithmetic states it: (0,0), (0,1), (1,0), (1,1) added in that order from 0"""
    _, full = resample_operands(case)
    f = full.float()
    r = torch.zeros_like(f[:, 0::2, 0::2])
    for dy in (0, 1):
        for dx in (0, 1):
            r = r + f[:, dy::2, dx::2]
    return r


def sumpool2_bound(case):
    half, full = resample_operands(case)
    return 4 * U * SECOND * (4 * nhwc(F.avg_pool2d(nchw(full.abs()), 2)) + half.abs())


@functools.lru_cache(maxsize=None)
def add_inplace_operands(n):
    g = _gen("add_inplace", n)
    return mags(g, (n,)), mags(g, (n,))


# ------------------------------------------------------------------------------------------------------------------ bias_grad
BIAS_GRAD_NPIX = {1: "one chunk of one pixel", 511: "511 chunks of one pixel", 513: "per = 2: 257 chunks, the last of one pixel, 255 empty ones",
                  1025: "per = 3: 342 chunks, the last of two pixels, 170 empty ones"}
BIAS_GRAD_C = {4: "rows = 256: one quad", 12: "rows = 85: one idle thread", 128: "rows = 8", 1024: "rows = 1: the widest C the entry takes"}
BIAS_GRAD_CASES = {(npix, C): f"{BIAS_GRAD_NPIX[npix]}; {BIAS_GRAD_C[C]}" for npix in BIAS_GRAD_NPIX for C in BIAS_GRAD_C}
BIAS_GRAD_REFUSED_C = (6, 1028)


def bias_grad_plan(npix):
    """(nchunk, per, chunks that hold a pixel, pixels of the last of them) of bias_grad_partial_kernel under launch_bias_grad"""
    nchunk = min(512, npix)
    per = -(-npix // nchunk)
    used = -(-npix // per)
    return nchunk, per, used, npix - (used - 1) * per


@functools.lru_cache(maxsize=None)
def bias_grad_operands(case):
    npix, C = case
    return mags(_gen("bias_grad", case), (npix, C))


def bias_grad_ref(case, mutation=None):
    npix, C = case
    dy = bias_grad_operands(case)
    if mutation == "last_pixel":
        dy = dy[:-1]
    elif mutation == "last_chunk":
        dy = dy[:npix - bias_grad_plan(npix)[3]]
    out = dy.sum(0)
    if mutation == "last_quad":
        out[-4:] = 0
    return out


def bias_grad_bound(case):
    return U * SECOND * bias_grad_operands(case).abs().sum(0)


# ------------------------------------------------------------------------------------------------------------------ chan_image_corr
CORR_GEOMETRIES = {
    (3, 5, 7): "105 pixels in 256 splits: per = 1, 151 empty splits",
    (1, 1, 1): "one pixel: 255 empty splits, eight padded taps",
    (2, 9, 1): "18 pixels, one column",
    (2, 16, 17): "544 pixels: per = 3, 182 splits, the last of one pixel",
}
CORR_CASES = {(sign, act, C, g): why for sign in (1, -1) for act in (0, 1) for C in (64, 192) for g, why in CORR_GEOMETRIES.items()}


def corr_plan(npix):
    """(per, splits that hold a pixel, pixels of the last of them) of chan_image_corr_kernel's 256 splits"""
    per = -(-npix // 256)
    used = -(-npix // per)
    return per, used, npix - (used - 1) * per


@functools.lru_cache(maxsize=None)
def corr_operands(case):
    sign, act, C, (B, H, W) = case
    g = _gen("corr", case)
    return mags(g, (B, H, W, C)), (coef_planes(g, B, C) if act else None), mags(g, (B, H, W))


def corr_ref(case, mutation=None):
    """dw[c][tap] = sum_{b,q} act(T)[b,q,c] s[b, q + sign tap]"""
    sign, act, C, (B, H, W) = case
    T, coef, s = corr_operands(case)
    Ta = act64(T, coef) if act else T
    npix = B * H * W
    if mutation in ("last_pixel", "last_chunk"):
        Ta = Ta.clone()
        Ta.reshape(npix, C)[npix - (1 if mutation == "last_pixel" else corr_plan(npix)[2]):] = 0
    st = taps(s, mutation if mutation in ("slice", "flat") else "pad", sign)
    dw = torch.einsum("bhwc,bhwt->ct", Ta, st)
    if mutation == "last_quad":
        dw[-4:] = 0
    return dw


def corr_bound(case):
    sign, act, C, (B, H, W) = case
    T, coef, s = corr_operands(case)
    st = taps(s, "pad", sign).abs()
    b = U * SECOND * torch.einsum("bhwc,bhwt->ct", (act64(T, coef) if act else T).abs(), st)
    return b + (torch.einsum("bhwc,bhwt->ct", act_allowance(T, coef), st) if act else 0.0)


# ------------------------------------------------------------------------------------------------------------------ head_dgrad
HEAD_DGRAD_CASES = {(C, g): why for C in (4, 128) for g, why in GEOMETRIES.items()}


@functools.lru_cache(maxsize=None)
def head_dgrad_operands(case):
    C, (B, H, W) = case
    g = _gen("head_dgrad", case)
    return mags(g, (B, H, W)), mags(g, (9, C))


def head_dgrad_ref(case, mutation=None):
    """dact[b,q,c] = sum_tap w9[tap][c] dout[b, q - tap]"""
    dout, w9 = head_dgrad_operands(case)
    return _drop(taps(dout, mutation if mutation in ("slice", "flat") else "pad", -1) @ w9, mutation)


def head_dgrad_bound(case):
    dout, w9 = head_dgrad_operands(case)
    return 9 * U * SECOND * (taps(dout, "pad", -1).abs() @ w9.abs())


# ------------------------------------------------------------------------------------------------------------------ loss
LOSS_HW = {1: "one thread works", 255: "one idle thread", 257: "thread 0 takes a second trip", 1000: "four trips, a partial last one"}
LOSS_CASES = {(l2, wb, HW, B, scale): LOSS_HW[HW] for l2 in (0, 1) for wb in (False, True) for HW in LOSS_HW for B in (1, 3) for scale in (1.0, 256.0)}


@functools.lru_cache(maxsize=None)
def loss_operands(case):
    """(out, target, w_b or None): every fourth position (1, 5, ...; never the last one at these HW) has out == target exactly"""
    l2, wb, HW, B, scale = case
    g = _gen("loss", case)
    target = mags(g, (B, HW))
    out = (target + mags(g, (B, HW), 0.25, 1.0)).float().double()
    out[:, 1::4] = target[:, 1::4]
    return out, target, (mags(g, (B,)).abs() if wb else None)


def loss_ref(case, mutation=None):
    """p_losses: loss_b = w_b mean_p |out - target|^(1|2); dout = scale dL/d(out) with L = mean_b loss_b"""
    l2, wb, HW, B, scale = case
    out, target, w = loss_operands(case)
    w = w if wb else torch.ones(B, dtype=torch.float64)
    d = out - target
    sgn = torch.sign(d) if mutation != "sign0" else torch.where(d >= 0, 1.0, -1.0).double()
    dout = scale * w[:, None] / (B * HW) * (2 * d if l2 else sgn)
    e = d * d if l2 else d.abs()
    if mutation == "last_pixel":
        dout, e = dout.clone(), e.clone()
        dout[:, -1], e[:, -1] = 0, 0                          # the last position of every slice not visited
    return dout, e.mean(1) * w


def loss_bound(case):
    l2 = case[0]
    dout, lb = loss_ref(case)
    return (5 if l2 else 4) * U * SECOND * dout.abs(), (3 if l2 else 2) * U * SECOND * lb.abs()


# ------------------------------------------------------------------------------------------------------------------ adam
ADAM_HYPER = (1e-4, 0.9, 0.999, 1e-8)          # lr, beta1, beta2, eps of DDPM_2D.configure_optimizers (torch.optim.Adam defaults)
ADAM_N = {1: "one thread", 255: "a tail block", 257: "one thread of a second block", 4099: "17 blocks, the last of 3 threads"}
ADAM_CASES = {(n, step, unscale): ADAM_N[n] for n in ADAM_N for step in (1, 2, 1000, 100000) for unscale in (1.0, 2.0 ** -10)}
ADAM_GRADS = (0.0, 1e-12, 1e10)                # next to the [0.5, 2] ones: exact zeros, sqrt(v) below eps, large


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adam_hyper_abi():
    """the hyper-parameters as the C ABI carries them: fp32 values, widened"""
    return tuple(f32(v) for v in ADAM_HYPER)


@functools.lru_cache(maxsize=None)
def adam_operands(case):
    """(p, g, m, v): |p| in [0.5, 2] 2^-10 (a weight whose ulp does not swallow an update of size lr); the gradient cycles through
    [0.5, 2], 0, 1e-12, 1e10 (times 1 / unscale, so that the unscaled gradient does); m and v are a plausible state for that gradient --
    m of its size, v of its square (1e-3 and 1e-6 where it is 0), every fifth v exactly 0"""
    n, step, unscale = case
    g_ = _gen("adam", case)
    p = (mags(g_, (n,)) * 2.0 ** -10).float().double()
    kind = torch.arange(n) % 4
    base = mags(g_, (n,))
    gr = torch.where(kind == 0, base, torch.where(kind == 1, torch.zeros(n, dtype=torch.float64), torch.where(kind == 2, base.sign() * 1e-12, base.sign() * 1e10)))
    size = torch.where(gr == 0, torch.full((n,), 1e-3, dtype=torch.float64), gr.abs())
    m = (mags(g_, (n,)) * size).float().double()
    v = (mags(g_, (n,)).abs() * size * size).float().double()
    v[4::5] = 0
    return p, (gr / unscale).float().double(), m, v


def adam_ref(case, mutation=None, hyper=None):
    """one step of torch.optim.Adam (no weight decay, no amsgrad) in float64 -> (p, m, v)"""
    n, step, unscale = case
    lr, b1, b2, eps = hyper or adam_hyper_abi()
    p, g, m, v = adam_operands(case)
    g = g * unscale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    k = step - 1 if mutation == "bias_step" else step
    bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)) if bc1 > 0 else torch.full_like(p, math.inf)
    return _drop1(p, mutation), _drop1(m, mutation), _drop1(v, mutation)


def _drop1(t, mutation):
    if mutation == "last_pixel":
        t = t.clone()
        t[-1] = 0
    return t


def adam_bound(case):
    """first-order bounds of (p, m, v), see N_ROUNDINGS"""
    n, step, unscale = case
    lr, b1, b2, eps = adam_hyper_abi()
    p, g, m, v = adam_operands(case)
    g = (g * unscale).abs()
    pn, mn, vn = adam_ref(case)
    Am = b1 * m.abs() + (1 - b1) * g
    bm, bv = 4 * U * SECOND * Am, 6 * U * SECOND * vn
    r1, r2 = b1 ** step, b2 ** step
    rel_bc1, rel_bc2 = 3 * U * (1 + r1) / (1 - r1), 3 * U * (1 + r2) / (1 - r2)
    A = vn.sqrt() / math.sqrt(1 - r2)                          # sqrt(v) / sqrt(bc2): v 6 u -> 3 u, its root u; bc2's root; the quotient
    denom = A + eps
    err_denom = A * (3 * U + U + rel_bc2 / 2 + U + U) + U * denom
    upd = (lr / (1 - r1)) * (mn.abs() / denom)
    err_upd = upd * (rel_bc1 + U + err_denom / denom + 2 * U) + (lr / (1 - r1)) * bm / denom
    return SECOND * (err_upd + U * (p.abs() + upd)), bm, bv


# ------------------------------------------------------------------------------------------------------------------ gn_coef
GN_HW = {(1, 1): "HW = 1: one record of one pixel", (7, 9): "HW = 63: one record, a pixel short of the 64", (5, 13): "HW = 65: two records, the second of one pixel",
         (63, 65): "HW = 4095: 64 records of 64 pixels, the last split before gn_nsplit changes", (64, 64): "HW = 4096: 16 records of 256 pixels",
         (50, 82): "HW = 4100: 17 records of 242 pixels, the last of 228"}
GN_CHANNELS = {(128, 0): "32 quads, 8 pixel lanes; groups of 4", (384, 0): "96 quads: 2 pixel lanes, 64 idle threads; groups of 12",
               (36, 92): "two sources, C0 % 32 != 0: 9 and 23 quads (4 and 3 idle threads)", (32, 352): "two sources: the third group of 12 straddles them"}
# The last pixel of every slice lies at 5 sigma, so that a sweep that drops it shows even among 4100 pixels (the group's variance moves by
# 25 / HW, the pixel's own normalised value by 125 / (2 HW)). No further out: the measure bounds the NORMALISED value, whose error is the
# relative error of rstd times |z|, and 5 is the largest |z| the N(0,1) tensors of the tests this measure comes from hold anyway.
GN_OUTLIER = 5.0


def _gn_cases():
    cases = {}
    for ch, why in GN_CHANNELS.items():
        for hw, why2 in GN_HW.items():
            for ratio in (0.0, 100.0):
                cases[ch + hw + (True, ratio)] = f"{why}; {why2}"
                if hw in ((5, 13), (64, 64)):
                    cases[ch + hw + (False, ratio)] = f"{why}; {why2}; no FiLM"
    for hw in ((1, 1), (7, 9), (5, 13)):
        for ratio in (0.0, 100.0):
            cases[(1024, 0) + hw + (True, ratio)] = f"256 quads: one pixel lane; groups of 32; {GN_HW[hw]}"
    cases[(1024, 0, 5, 13, False, 0.0)] = "256 quads: one pixel lane; no FiLM"
    return cases


GN_CASES = _gn_cases()          # (C0, C1, H, W, film, |mean| / sigma)
GN_B = 2


def gn_nsplit(HW):
    """records per slice of the stand-alone sweep (norm_kernels.hip::gn_nsplit)"""
    ppb = 256 if HW >= 4096 else 64
    return -(-HW // ppb)


@functools.lru_cache(maxsize=None)
def gn_operands(case):
    """(x [B,H,W,C0+C1], gamma, beta, film [B][2C] or None): x = ratio + N(0,1) with the last pixel of every slice at ratio +- GN_OUTLIER"""
    C0, C1, H, W, film, ratio = case
    C = C0 + C1
    g = _gen("gn", case)
    x = torch.randn((GN_B, H, W, C), generator=g, dtype=torch.float64) + ratio
    x[:, -1, -1, :] = ratio + GN_OUTLIER * (torch.randint(0, 2, (GN_B, C), generator=g).double() * 2 - 1)
    x = x.float().double()
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).double(), (0.1 * torch.randn(C, generator=g)).double()
    fl = (0.3 * torch.randn((GN_B, 2 * C), generator=g)).double() if film else None
    return x, gamma, beta, fl


def gn_normalised(case, mutation=None):
    """GroupNorm32(x) (1 + scale) + shift, NCHW; mutations state the statistics a wrong sweep would deliver"""
    C0, C1, H, W, film, ratio = case
    C = C0 + C1
    x, gamma, beta, fl = gn_operands(case)
    xc = nchw(x)
    if mutation is None:
        ref = F.group_norm(xc, 32, gamma, beta, eps=1e-5)
    else:
        ref = _gn_by_sums(case, mutation)
    if fl is not None:
        ref = ref * (1 + fl[:, :C, None, None]) + fl[:, C:, None, None]
    return ref


def _gn_by_sums(case, mutation=None):
    """GroupNorm from per-channel sums (the sweep's form): biased variance E[x^2] - mean^2 over a group's C / 32 channels x HW pixels"""
    C0, C1, H, W, film, ratio = case
    C = C0 + C1
    x, gamma, beta, fl = gn_operands(case)
    xs = x.reshape(GN_B, H * W, C)
    if mutation == "last_pixel":
        xs = xs[:, :-1]
    s, q = xs.sum(1), (xs * xs).sum(1)                          # [B][C]
    if mutation == "last_quad":
        for end in ((C0, C) if C1 else (C,)):                   # the last quad of each source's sweep
            s[:, end - 4:end], q[:, end - 4:end] = 0, 0
    n = (C // 32) * H * W
    mean = s.reshape(GN_B, 32, -1).sum(2) / n
    var = (q.reshape(GN_B, 32, -1).sum(2) / n - mean * mean).clamp_min(0)
    mean, rstd = mean.repeat_interleave(C // 32, 1), (var + 1e-5).rsqrt().repeat_interleave(C // 32, 1)
    return ((nchw(x) - mean[:, :, None, None]) * rstd[:, :, None, None]) * gamma[None, :, None, None] + beta[None, :, None, None]


def gn_bound(case):
    C0, C1, H, W, film, ratio = case
    fl = gn_operands(case)[3]
    return 1e-5 * (1 + ratio) * (1 + (float(fl.abs().max()) if fl is not None else 0.0))


def gn_apply(case, coef):
    """the normalised value the device's coefficients coef[3][B][C] give, NCHW float64"""
    x = nchw(gn_operands(case)[0])
    return (x - coef[0][:, :, None, None]) * coef[1][:, :, None, None] + coef[2][:, :, None, None]


# ------------------------------------------------------------------------------------------------------------------ linear_backward
LINBWD_CASES = {        # (M, N, K, silu)
    (64, 1024, 100, 1): "skinny, its largest M: 16 rows per thread; K = 100 is no multiple of the 64 columns of a block; ranges of 32 in a 64-step",
    (65, 1024, 64, 0): "M one above the skinny path: the GEMM",
    (3, 1023, 64, 1): "N one below the skinny path: the GEMM",
    (7, 1500, 200, 1): "skinny: M % 4 != 0 (the last row group holds one row), ranges of 47",
    (1, 1024, 4, 0): "skinny: one row, three of the four row groups idle; 4 of 64 columns",
}
LIN_NSPLIT = 32


def linbwd_skinny(case):
    M, N, K, silu = case
    return M <= 64 and N >= 1024


@functools.lru_cache(maxsize=None)
def linbwd_operands(case):
    M, N, K, silu = case
    g = _gen("linbwd", case)
    return mags(g, (M, K)), mags(g, (N, K)), mags(g, (M, N))


def silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def linbwd_ref(case, mutation=None):
    """y = [SiLU](x) W^T + b, given dy: dW = dy^T act(x), db = column sums of dy, dx = (dy W) o act'(x)"""
    M, N, K, silu = case
    x, w, dy = linbwd_operands(case)
    a = F.silu(x) if silu else x
    dyw, dya = dy, dy
    if mutation == "last_pixel":            # the last row of the contraction over M (dW, db), the last column of the one over N (dx)
        dya, a = dy[:-1], a[:-1]
        dyw, w = dy[:, :-1], w[:-1]
    dw, db, dx = dya.t() @ a, dya.sum(0), dyw @ w
    if mutation == "last_k4":               # the last four columns of K not produced
        dw, dx = dw.clone(), dx.clone()
        dw[:, -4:], dx[:, -4:] = 0, 0
    return dw, db, dx * silu_grad64(x) if silu else dx


def linbwd_bound(case):
    M, N, K, silu = case
    x, w, dy = linbwd_operands(case)
    a = F.silu(x) if silu else x
    bw = (M + 1) * U * SECOND * (dy.abs().t() @ a.abs()) + (ACT * (dy.abs().t() @ x.abs()) if silu else 0.0)
    bb = U * SECOND * dy.abs().sum(0)
    n = (math.ceil(N / LIN_NSPLIT) + LIN_NSPLIT) if linbwd_skinny(case) else N + 1
    pre = dy.abs() @ w.abs()
    if not silu:
        return bw, bb, n * U * SECOND * pre
    # SiLU'(x) = s (1 + x (1 - s)) in fp32: s to (|x| + 5) u (the rounded argument, v_exp, 1 + e, v_rcp), the rest four roundings:
    # below 2^-20 s (1 + |x|) for |x| <= 2, which the operands are
    assert float(x.abs().max()) <= 2.0
    s = torch.sigmoid(x)
    return bw, bb, (n + 1) * U * SECOND * pre * silu_grad64(x).abs() + ACT * s * (1 + x.abs()) * pre
