"""What the tests of the chain's step kernels share (tests/test_step_op_cases_host.py, tests/test_gpu_step_ops_edges.py): case tables,
seeded operands, float64 references written from each operation's definition, the derived error bounds, numpy float32 restatements where
the kernel's text pins every rounding, and the results a wrong kernel of a named kind would give. Nothing here needs a GPU; tables and
operands are computed once per process (lru_cache) and never modified.

Operators: the second half of csrc/small_kernels.hip -- step_kernel (cddpm_p_sample, cddpm_reverse_range, cddpm_reverse),
ddim_step_kernel (cddpm_ddim_step), noise_fill_kernel with normal4 / Philox4x32-10 (cddpm_noise_fill, and the z = NULL draws of both
steps), q_sample_kernel (cddpm_q_sample), slice_status_kernel (cddpm_slice_status). Images are [B][HW] fp32, one thread per quad of 4.

The steps sit behind the UNet. They are isolated through the bits of cddpm_unet_forward on the same handle: the device test downloads
model_out and every reference here takes it (and the fp32 schedule tables the test installed) as an operand, so what is compared is
the step's own arithmetic. The host tests use a seeded stand-in for model_out.

Bounds: |got - ref64| <= bound per element, u = 2^-24: bound = 1.01 (n u A + the math functions' allowances), A = the operation's own
expression in float64 with every term replaced by its absolute value, n = the number of fp32 roundings on the longest chain to one output
as counted from the kernel (N_ROUNDINGS). The clamp is 1-Lipschitz: the bound on x0 passes through it. expf, logf, sqrtf, sinf and cosf
are allowed TWICE their worst deviation from float64 measured on the device over the arguments these kernels can form
(tools/step_math_ulp.hip: ROCm ships no accuracy table; MATH_ULP_MEASURED); an allowance of k ulp is a relative error of 2 k u of the
function's value. No bound is fitted to what a kernel under test delivers."""
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

import cddpm_oracle
from conftest import load_pkg

synth = load_pkg("synth")
schedule = load_pkg("schedule")

U = 2.0 ** -24
SECOND = 1.01
T = 1000
MAX_B, MAX_H, MAX_W = 5, 32, 32
F32 = np.float32

# worst |fp32 - float64| / ulp(float64 result) of the device's functions: tools/step_math_ulp.hip on an MI355X (ROCm 7, -O3), logf / sqrtf /
# sinf / cosf over all 2^23 values u01() returns (the arguments of normal4), expf over 0.5 posterior_log_variance_clipped[t] of the cosine and
# the linear schedule at T = 1000 (0.7148) and over 2^22 points of the clipped range [-23.05, 0] (0.8344: the larger is taken)
MATH_ULP_MEASURED = {"logf": 2.1386, "sqrtf": 0.5000, "sinf": 1.4519, "cosf": 1.5392, "expf": 0.8344}
MATH_ULP = {k: 2.0 * v for k, v in MATH_ULP_MEASURED.items()}
# Box-Muller r cos(theta): relative error in units of u. logf's 2 k u on ln u is halved by the square root; sqrtf, the trigonometric function
# (the larger of the two allowances); the product's own rounding. theta = 6.2831855f * u01 is one fp32 product, restated exactly.
K_NORMAL = MATH_ULP["logf"] + 2 * MATH_ULP["sqrtf"] + 2 * max(MATH_ULP["sinf"], MATH_ULP["cosf"]) + 1
K_EXP = 2 * MATH_ULP["expf"]

N_ROUNDINGS = {
    "p_sample pred_x0": "2 + [t > 0] + [finalize]: c1 x0 | c2 x, their sum; sigma z and its addition (sigma z itself: 1, shorter); r + 1 (x 0.5 exact)",
    "p_sample pred_noise": "4 + [t > 0] + [finalize]: sr x | srm1 eps, their difference, then as pred_x0 (a fused product only removes a rounding)",
    "ddim pred_x0": "6 + [finalize]: sr x, - x0, / srm1, coef_eps eps, the sum with x0 coef_x0, + sigma z (always executed; sigma z itself: 1, shorter)",
    "ddim pred_noise": "5 + [finalize]: sr x | srm1 eps, their difference, x0 coef_x0, the sum, + sigma z",
    "noise_fill": f"K_NORMAL = {K_NORMAL:.2f} u relative: logf halved by sqrtf, sqrtf, sinf / cosf, one product (u01 and -2 x are exact)",
    "q_sample": "2: 2 x - 1 (2 x exact) | cb n, then one fused multiply-add",
    "slice_status": "integer logic: exact",
}

GEOMETRIES = {      # (B, H, W): quads B H W / 4 against the 256-thread blocks of the step kernels
    (1, 4, 4): "4 quads: a single partial wave",
    (3, 12, 20): "180 quads: one partial block",
    (3, 20, 28): "420 quads: a ragged second block",
    (2, 32, 32): "512 quads: exact blocks",
    (5, 4, 8): "40 quads: b = e / nq with nq = 8, far below a wave: five slices in one",
}
SCHEDULES = ("cosine", "linear")
OBJECTIVES = ("pred_x0", "pred_noise")
P_SAMPLE_T = (0, 1, 2, 500, 998, 999)
STREAM_XT, STREAM_Z = synth.STREAM_XT, synth.STREAM_Z
SEED_HI = (1 << 32) + 7          # the seed of the steps' Philox cases: a key whose high word is not zero
SLICE0 = 5


def case_id(case):
    return "-".join(str(c).replace(" ", "") for c in case)


def quads(geom):
    B, H, W = geom
    return B * H * W // 4


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------ schedule tables
# rows of the clamp schedule whose pred_noise x0 = sr x - srm1 beta is exact in every evaluation order, so that x places x0 on a chosen fp32
# value: CLAMP_T_SHIFT has x0 = 2 x - 0.125 (beta = 0.25), CLAMP_T_PURE x0 = 2 x (every neighbour of +-1 has an exact pre-image)
BETA = 0.25
CLAMP_T_SHIFT, CLAMP_T_PURE = 7, 8


@functools.lru_cache(maxsize=None)
def buffers(kind):
    """the schedule buffers a test installs (torch fp32, schedule.schedule_buffers); kind `clamp`: the linear schedule with two rows of
    sqrt_recip / sqrt_recipm1 replaced (see CLAMP_T_SHIFT)"""
    buf = {k: v.clone() for k, v in schedule.schedule_buffers(T, "linear" if kind == "clamp" else kind).items()}
    if kind == "clamp":
        buf["sqrt_recip_alphas_cumprod"][CLAMP_T_SHIFT] = 2.0
        buf["sqrt_recipm1_alphas_cumprod"][CLAMP_T_SHIFT] = 0.5
        buf["sqrt_recip_alphas_cumprod"][CLAMP_T_PURE] = 2.0
        buf["sqrt_recipm1_alphas_cumprod"][CLAMP_T_PURE] = 0.0
    return buf


class Tables:
    """the fp32 tables as numpy arrays, as stored"""

    def __init__(self, kind):
        b = buffers(kind)
        g = lambda k: b[k].numpy().astype(F32)
        self.c1, self.c2, self.logvar = g("posterior_mean_coef1"), g("posterior_mean_coef2"), g("posterior_log_variance_clipped")
        self.sr, self.srm1 = g("sqrt_recip_alphas_cumprod"), g("sqrt_recipm1_alphas_cumprod")
        self.sa, self.s1 = g("sqrt_alphas_cumprod"), g("sqrt_one_minus_alphas_cumprod")
        self.acp_prev = g("alphas_cumprod_prev")


@functools.lru_cache(maxsize=None)
def tables(kind):
    return Tables(kind)


def zero_head_state_dict(sd):
    """a copy of the state dict whose output convolution has weight 0 and bias BETA: model_out is BETA for every finite input"""
    sd = dict(sd)
    sd["out.2.weight"] = np.zeros_like(sd["out.2.weight"])
    sd["out.2.bias"] = np.full_like(sd["out.2.bias"], BETA)
    return sd


# ------------------------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def image(geom, tag="x"):
    """N(0,1) fp32 [B, HW]"""
    B, H, W = geom
    return rng("image", geom, tag).standard_normal((B, H * W)).astype(F32)


@functools.lru_cache(maxsize=None)
def cond(B):
    return rng("cond", B).standard_normal((B, 128)).astype(F32)


@functools.lru_cache(maxsize=None)
def noise_explicit(geom, tag="z"):
    """an injected draw: N(0,1) with exact zeros (every 7th element) and |z| = 6 at both ends"""
    z = image(geom, tag).copy()
    z.reshape(-1)[::7] = 0.0
    z.reshape(-1)[3], z.reshape(-1)[-1] = 6.0, -6.0
    return z


@functools.lru_cache(maxsize=None)
def model_out_standin(geom, tag="mo"):
    """what the host tests use for model_out: uniform in [-1.6, 1.6] (so that the clamp acts on a part), some elements exactly +-1"""
    B, H, W = geom
    mo = rng("model_out", geom, tag).uniform(-1.6, 1.6, (B, H * W)).astype(F32)
    mo.reshape(-1)[1::11] = 1.0
    mo.reshape(-1)[2::13] = -1.0
    return mo


ONE_UP, ONE_DOWN = float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(1), F32(0)))
# 16 targets of x0: 4 clamped high, 4 clamped low, 8 left as they are (+-1 exactly, their inner neighbours, two below 1e-3, two general)
CLAMP_TARGETS = {
    CLAMP_T_PURE: (ONE_UP, 3.0, 1.5, 2.25, -ONE_UP, -3.0, -1.5, -2.25, 1.0, -1.0, ONE_DOWN, -ONE_DOWN, 5e-4, -2.5e-4, 0.375, -0.625),
    # x = (x0 + 0.125) / 2 has no fp32 value for 1 - 2^-24: two ulps below 1 instead
    CLAMP_T_SHIFT: (ONE_UP, 3.0, 1.5, 2.25, -ONE_UP, -3.0, -1.5, -2.25, 1.0, -1.0, 1.0 - 2.0 ** -23, -ONE_DOWN, 5e-4, -2.5e-4, 0.375, -0.625),
}


@functools.lru_cache(maxsize=None)
def clamp_image(geom, t):
    """x [B, HW] that puts the pred_noise x0 = sr x - srm1 BETA of the clamp schedule's row t on CLAMP_TARGETS, each block of 16 elements a
    permutation of the 16 targets"""
    tab = tables("clamp")
    n = quads(geom) * 4
    i = np.arange(n)
    target = np.array(CLAMP_TARGETS[t], dtype=np.float64)[(5 * i + i // 16) % 16]
    x = ((target + float(tab.srm1[t]) * BETA) / float(tab.sr[t])).astype(F32)
    return x.reshape(geom[0], -1)


# ------------------------------------------------------------------------------------------------------------------ clamp, Philox
def clamp64(v, mutation=None):
    """torch.clamp(v, -1, 1): a NaN stays a NaN. Mutation `nan_to_-1`: fminf(fmaxf(v, -1), 1) alone, which turns a NaN into -1"""
    if mutation == "nan_to_-1":
        return np.fmin(np.fmax(v, -1.0), 1.0)
    return np.clip(v, -1.0, 1.0)


def normal64(nq, t, slice_, stream, seed, mutation=None):
    """float64 [4 nq]: normal4 of quads 0 .. nq - 1 from its definition. Philox4x32-10 (synth.philox4x32) with key = the two halves of
    seed, counter = (quad, t, slice, stream), each taken modulo 2^32; u01 exact; theta = the fp32 product 6.2831855f u; r = sqrt(-2 ln u);
    (ra cos ta, ra sin ta, rb cos tb, rb sin tb)."""
    m = 0xFFFFFFFF
    k0, k1 = seed & m, 0 if mutation == "key_hi_dropped" else (seed >> 32) & m
    c1 = 0 if mutation == "t_missing" else t & m
    c3 = STREAM_XT if mutation == "stream_fixed" else stream & m
    xs = synth.philox4x32(np.arange(nq, dtype=np.uint32), np.uint32(c1), np.uint32(slice_ & m), np.uint32(c3), k0, k1)
    u = [synth._u01(x) for x in xs]
    assert all(v.dtype == F32 for v in u)
    ra, rb = (np.sqrt(-2.0 * np.log(v.astype(np.float64))) for v in (u[0], u[2]))
    ta, tb = ((F32(6.28318530717958647692) * v).astype(np.float64) for v in (u[1], u[3]))
    if mutation == "sincos_swapped":
        out = (ra * np.sin(ta), ra * np.cos(ta), rb * np.sin(tb), rb * np.cos(tb))
    else:
        out = (ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb))
    return np.stack(out, axis=-1).reshape(-1)


def noise_ref(B, HW, t, slice0, stream, seed, mutation=None):
    """float64 [B, HW]: noise_fill_kernel; slice b is keyed by (slice0 + b) mod 2^32"""
    nq = HW // 4
    if mutation == "wrong_nq":       # b = e / (nq + 1): the flat quad e of slice b draws with a wrong slice index (and its own q)
        e = np.arange(B * nq)
        rows = [normal64(nq, t, slice0 + int(b), stream, seed) for b in range(B)]
        out = np.stack(rows).reshape(B * nq, 4)
        bad = e // (nq + 1)
        for i in np.nonzero(bad != e // nq)[0]:
            out[i] = rows[bad[i]].reshape(nq, 4)[i % nq]
        return out.reshape(B, HW)
    out = np.stack([normal64(nq, t, (0 if mutation == "slice0_not_added" else slice0) + b, stream, seed, mutation) for b in range(B)])
    if mutation == "last_quad":      # never written: the output's sentinel, a NaN, stays
        out[:, -4:] = np.nan
    return out


def noise_bound(ref):
    return SECOND * K_NORMAL * U * np.abs(ref)


# ------------------------------------------------------------------------------------------------------------------ posterior step
def step_ref(x, mo, t, tab, objective, clip, z, finalize, mutation=None):
    """float64: p_sample -> p_mean_variance -> model_predictions -> q_posterior on the fp32 operands as stored. z [B, HW] is read for
    t > 0 only (mutation `noise_at_0`: always)."""
    x, mo = x.astype(np.float64), mo.astype(np.float64)
    f = lambda a: float(a[t])
    x0 = mo if objective == "pred_x0" else f(tab.sr) * x - f(tab.srm1) * mo
    if clip or mutation == "clip_always":
        x0 = clamp64(x0, mutation)
    c1, c2 = (f(tab.c2), f(tab.c1)) if mutation == "coef_swapped" else (f(tab.c1), f(tab.c2))
    r = c1 * x0 + c2 * x
    if t > 0 or mutation == "noise_at_0":
        sigma = math.exp((1.0 if mutation == "sigma_full" else 0.5) * f(tab.logvar))
        r = r + sigma * z.astype(np.float64)
    if finalize or mutation == "map_always":
        r = (r + 1.0) * 0.5
    return r


def step_bound(x, mo, t, tab, objective, z, finalize, philox):
    """1.01 u (n A + the allowances on sigma |z|: expf, and the draw's own K_NORMAL when the kernel draws z itself)"""
    ax, amo = np.abs(x.astype(np.float64)), np.abs(mo.astype(np.float64))
    f = lambda a: abs(float(a[t]))
    n = (2 if objective == "pred_x0" else 4) + (1 if t > 0 else 0) + (1 if finalize else 0)
    ax0 = amo if objective == "pred_x0" else f(tab.sr) * ax + f(tab.srm1) * amo
    A = f(tab.c1) * ax0 + f(tab.c2) * ax
    extra = 0.0
    if t > 0:
        sz = math.exp(0.5 * float(tab.logvar[t])) * np.abs(z.astype(np.float64))
        A = A + sz
        extra = (K_EXP + (K_NORMAL if philox else 0.0)) * sz
    if finalize:
        A, extra = (A + 1.0) * 0.5, extra * 0.5
    return SECOND * U * (n * A + extra)


def sigma_candidates(t, tab):
    """the three fp32 neighbours of fp32(exp(0.5 logvar[t])): the device's expf is the one rounding step_kernel does not pin"""
    s = F32(math.exp(float(F32(0.5) * tab.logvar[t])))
    return [np.nextafter(s, F32(-np.inf)), s, np.nextafter(s, F32(np.inf))]


def step_f32(x, mo, t, tab, clip, z, finalize, sigma):
    """step_kernel under pred_x0 in numpy float32, one rounding per operation: the kernel's body is compiled with contraction off"""
    with np.errstate(invalid="ignore"):
        x0 = np.clip(mo, F32(-1), F32(1)) if clip else mo
        r = tab.c1[t] * x0 + tab.c2[t] * x
        if t > 0:
            r = r + F32(sigma) * z
        if finalize:
            r = (r + F32(1)) * F32(0.5)
    assert r.dtype == F32
    return r


def unit_map_f32(r):
    return (r + F32(1)) * F32(0.5)


# ------------------------------------------------------------------------------------------------------------------ DDIM
DDIM_SAMPLING_STEPS = 50


@functools.lru_cache(maxsize=None)
def ddim_pairs():
    """an early, a middle and the last (time, time_next) pair of ddim_sample with 50 sampling steps"""
    pairs = cddpm_oracle.ddim_time_pairs(T, DDIM_SAMPLING_STEPS)
    return (pairs[0], pairs[len(pairs) // 2], pairs[-1])


@functools.lru_cache(maxsize=None)
def ddim_coefficients(kind, pair, eta):
    """(coef_x0, coef_eps, sigma) as cond_DDPM.ddim_coefficients forms them in fp32 from alphas_cumprod_prev"""
    class Holder:
        ddim_sampling_eta = eta
        alphas_cumprod_prev = buffers(kind)["alphas_cumprod_prev"]
    return load_pkg("cond_DDPM").GaussianDiffusion.ddim_coefficients(Holder, pair[0], pair[1], eta)


def ddim_ref(x, mo, t, tab, objective, clip, coefs, z, add_noise, finalize, mutation=None):
    """float64: one iteration of ddim_sample's loop, eps from the UNCLIPPED x0, the coefficients as given (the device test hands the
    fp32 values of cond_DDPM.ddim_coefficients to both sides)"""
    x, mo = x.astype(np.float64), mo.astype(np.float64)
    sr, srm1 = float(tab.sr[t]), float(tab.srm1[t])
    cx0, ceps, sigma = (float(c) for c in coefs)
    with np.errstate(invalid="ignore", divide="ignore"):
        if objective == "pred_x0":
            x0, eps = mo, (sr * x - mo) / srm1
        else:
            eps = mo
            x0 = sr * x - srm1 * eps
        if clip or mutation == "clip_always":
            x0 = clamp64(x0, mutation)
            if mutation == "eps_from_clamped":
                eps = (sr * x - x0) / srm1
        if mutation == "coef_swapped":
            cx0, ceps = ceps, cx0
        r = x0 * cx0 + ceps * eps
        r = r + sigma * (z.astype(np.float64) if add_noise else 0.0)
    if finalize:
        r = (r + 1.0) * 0.5
    return r


def ddim_bound(x, mo, t, tab, objective, coefs, z, add_noise, finalize, philox=False):
    ax, amo = np.abs(x.astype(np.float64)), np.abs(mo.astype(np.float64))
    sr, srm1 = abs(float(tab.sr[t])), abs(float(tab.srm1[t]))
    cx0, ceps, sigma = (abs(float(c)) for c in coefs)
    if objective == "pred_x0":
        n, ax0, aeps = 6, amo, (sr * ax + amo) / srm1
    else:
        n, ax0, aeps = 5, sr * ax + srm1 * amo, amo
    sz = sigma * np.abs(z.astype(np.float64)) if add_noise else 0.0
    A = ax0 * cx0 + ceps * aeps + sz
    extra = K_NORMAL * sz if philox else 0.0
    if finalize:
        n, A, extra = n + 1, (A + 1.0) * 0.5, extra * 0.5
    return SECOND * U * (n * A + extra)


def ddim_f32(x, mo, t, tab, objective, clip, coefs, z, add_noise, finalize):
    """ddim_step_kernel in numpy float32: every product, sum and difference of it is rounded on its own (contraction is off in its
    body), the division is correctly rounded"""
    sr, srm1 = tab.sr[t], tab.srm1[t]
    cx0, ceps, sigma = (F32(c) for c in coefs)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if objective == "pred_x0":
            x0 = mo
            eps = (sr * x - x0) / srm1
        else:
            eps = mo
            x0 = sr * x - srm1 * eps
        if clip:
            x0 = np.clip(x0, F32(-1), F32(1))
        r = x0 * cx0 + ceps * eps
        r = r + sigma * (z if add_noise else np.zeros_like(x))
        if finalize:
            r = (r + F32(1)) * F32(0.5)
    assert r.dtype == F32
    return r


# the flag combinations of one DDIM call: (add_noise, finalize, z) with z `explicit`, `null` (the device Philox) or `nan` (an injected
# draw of NaN that add_noise = 0 must not read)
DDIM_VARIANTS = ((1, 0, "explicit"), (1, 0, "null"), (0, 0, "nan"), (1, 1, "explicit"), (0, 1, "null"))
DDIM_ETAS = (1.0, 0.0)       # eta 0: sigma = 0


# ------------------------------------------------------------------------------------------------------------------ noise_fill
NOISE_SEEDS = (7, 1 << 32, (1 << 32) + 7, (1 << 64) - 1, 0x9E3779B97F4A7C15)
NOISE_SLICE0 = (0, 5, (1 << 32) - 2, (1 << 40) + 3)
NOISE_T = (0, 1, 999, (1 << 31) - 1)
WRAP_GEOM = (4, 4, 8)        # slice0 = 2^32 - 2 with B = 4: slices 2^32 - 2, 2^32 - 1, 0, 1


def _noise_cases():
    """(seed, slice0, t, stream, geom): every listed value of every axis, one axis at a time from a base case, then the combinations
    that name an edge"""
    base = dict(seed=NOISE_SEEDS[2], slice0=5, t=999, stream=STREAM_Z, geom=(3, 20, 28))
    cases = []
    def add(**kw):
        c = dict(base, **kw)
        if c["slice0"] == (1 << 32) - 2:
            c["geom"] = WRAP_GEOM
        tup = (c["seed"], c["slice0"], c["t"], c["stream"], c["geom"])
        if tup not in cases:
            cases.append(tup)
    add()
    for s in NOISE_SEEDS:
        add(seed=s)
    for s0 in NOISE_SLICE0:
        add(slice0=s0)
    for t in NOISE_T:
        add(t=t)
    add(stream=STREAM_XT, t=0)
    for g in GEOMETRIES:
        add(geom=g)
        add(geom=g, seed=7, stream=STREAM_XT, t=0, slice0=0)
    add(seed=(1 << 64) - 1, slice0=(1 << 32) - 2, t=(1 << 31) - 1)
    return tuple(cases)


NOISE_CASES = _noise_cases()


# ------------------------------------------------------------------------------------------------------------------ q_sample
Q_T_MODES = ("per_sample", "uniform")
Q_T_PER_SAMPLE = (0, 999, 500)
Q_T_UNIFORM = 500
Q_CASES = tuple((kind, mode, geom) for kind in SCHEDULES for mode in Q_T_MODES for geom in GEOMETRIES)


def q_t(mode, B):
    return [Q_T_PER_SAMPLE[b % 3] for b in range(B)] if mode == "per_sample" else [Q_T_UNIFORM] * B


@functools.lru_cache(maxsize=None)
def q_operands(geom):
    """x01 [B, HW] in [0, 1] with 0, 0.5 and 1 exactly; noise with exact zeros and |n| up to 6"""
    B, H, W = geom
    x = rng("q x", geom).uniform(0.0, 1.0, (B, H * W)).astype(F32)
    f = x.reshape(-1)
    f[0::5], f[1::5], f[2::5] = 0.0, 0.5, 1.0
    return x, noise_explicit(geom, "q noise")


def q_sample_ref(x01, noise, ts, tab, mutation=None):
    if mutation == "t_from_slice0":
        ts = [ts[0]] * len(ts)
    ca = np.array([float(tab.sa[t]) for t in ts])[:, None]
    cb = np.array([float(tab.s1[t]) for t in ts])[:, None]
    return ca * (2.0 * x01.astype(np.float64) - 1.0) + cb * noise.astype(np.float64)


def q_sample_bound(x01, noise, ts, tab):
    ca = np.array([abs(float(tab.sa[t])) for t in ts])[:, None]
    cb = np.array([abs(float(tab.s1[t])) for t in ts])[:, None]
    return SECOND * 2 * U * (ca * (2.0 * np.abs(x01.astype(np.float64)) + 1.0) + cb * np.abs(noise.astype(np.float64)))


def round_f32(q):
    """a Fraction rounded once to fp32, to nearest, ties to even"""
    c = F32(float(q))
    cands = (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf)))
    key = lambda v: (abs(Fraction(float(v)) - q), int(np.array(v, dtype=F32).view(np.uint32)) & 1)
    return min(cands, key=key)


def q_sample_exact_f32(x01, noise, ts, tab):
    """q_sample_value to the bit: fma(ca, fl(2 x - 1), fl(cb n)), the fused sum formed exactly (Fraction) and rounded once"""
    out = np.empty_like(x01)
    for b, t in enumerate(ts):
        ca, cb = tab.sa[t], tab.s1[t]
        y = x01[b] * F32(2) - F32(1)
        p = cb * noise[b]
        fca = Fraction(float(ca))
        out[b] = [round_f32(fca * Fraction(float(yy)) + Fraction(float(pp))) for yy, pp in zip(y, p)]
    return out


# ------------------------------------------------------------------------------------------------------------------ slice_status
STATUS_THREADS = 1024
STATUS_NQ = (1, 63, 1023, 1024, 1025, 1537)
STATUS_B = (1, 5)
STATUS_PLANTS = {"+inf": 0x7F800000, "-inf": 0xFF800000, "quiet NaN": 0x7FC00000, "signalling NaN": 0x7F800001, "negative NaN": 0xFFC00001}
STATUS_CASES = tuple((nq, B) for nq in STATUS_NQ for B in STATUS_B)


def status_clean(nq, kind):
    """a slice without inf or NaN (uint32 bits [4 nq]): the largest finite magnitudes, subnormals, -0.0"""
    vals = {"huge": [3.4e38, -3.4e38], "tiny": [1e-45, -1e-40, 1.1754942e-38], "zero": [-0.0, 0.0]}[kind]
    return np.resize(np.array(vals, dtype=F32), 4 * nq).view(np.uint32).copy()


def status_calls(nq, B):
    """-> (bits uint32 [calls, B, 4 nq], flags int32 [calls, B]): every plant alone in each lane of the first and of the last quad, in
    slice (call index mod B) of a batch whose other slices are clean; then three calls of clean slices only (each kind in each slice)"""
    slices, flags = [], []
    kinds = ("huge", "tiny", "zero")
    n = 0
    for bits in STATUS_PLANTS.values():
        for quad in sorted({0, nq - 1}):
            for lane in range(4):
                batch = [status_clean(nq, kinds[(n + b) % 3]) for b in range(B)]
                batch[n % B][4 * quad + lane] = bits
                slices.append(np.stack(batch))
                flags.append([1 if b == n % B else 0 for b in range(B)])
                n += 1
    for k in range(3):
        slices.append(np.stack([status_clean(nq, kinds[(k + b) % 3]) for b in range(B)]))
        flags.append([0] * B)
    return np.stack(slices), np.array(flags, dtype=np.int32)


def status_ref(bits, mutation=None):
    """[..., 4 nq] uint32 -> 1 where a slice holds an exponent field of all ones. Mutation `first_1024_quads`: one trip of the loop only"""
    if mutation == "first_1024_quads":
        bits = bits[..., :4 * STATUS_THREADS]
    return ((bits & 0x7F800000) == 0x7F800000).any(axis=-1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ simplex
SIMPLEX_CASES = ((3, 16, 1, 0.5, 16.0), (-9876543210, 16, 2, 0.5, 16.0), (1234567, 20, 2, 0.5, 16.0), (3, 20, 6, 0.8, 64.0))     # seed, n, octaves, persistence, frequency


def differs(ref, mut, bound=None):
    """does a wrong result show? Bitwise cases (bound None): any differing element. Bounded cases: more than 4 bounds somewhere. A NaN on
    one side only always shows."""
    ref, mut = np.asarray(ref, dtype=np.float64), np.asarray(mut, dtype=np.float64)
    nan = np.isnan(ref) != np.isnan(mut)
    if nan.any():
        return True
    ok = ~np.isnan(ref)
    d = np.abs(ref[ok] - mut[ok])
    if bound is None:
        return bool((d > 0).any())
    return bool((d > 4 * np.broadcast_to(bound, ref.shape)[ok]).any())
