"""GPU: the chain's step kernels one call at a time (the second half of csrc/small_kernels.hip: step_kernel, ddim_step_kernel,
noise_fill_kernel with normal4, q_sample_kernel, slice_status_kernel), at block tails, schedule ends, clamp edges and 64-bit seeds, against
the float64 references of tests/step_op_cases.py and to its derived bounds -- and bit for bit against its numpy float32 restatements
wherever the kernel's text pins every rounding. tests/test_step_op_cases_host.py checks the references, the edges and that every case
would show a kernel that is wrong in the ways such kernels go wrong.

The steps run behind the UNet. cddpm_unet_forward and the step entries of one handle run the same forward, so the test downloads
model_out = unet_forward(x, t) and hands those bits to the reference: what is compared is the step's own arithmetic, not the UNet's.

Every operand and result is a 16-byte-aligned view inside a larger device tensor with 64 floats of guard on both sides (the arena of
tests/test_gpu_small_ops_edges.py): NaN around the inputs, a sentinel NaN pattern around (and, where the operator does not work in
place, in) the outputs. Refused calls return non-zero, leave a message and the output untouched."""
import numpy as np
import pytest
import torch

import step_op_cases as S
from conftest import load_pkg
from test_gpu_small_ops_edges import GUARD, SENTINEL, Out, inp, p

pytestmark = pytest.mark.gpu

gid = lambda g: "x".join(map(str, g))
GEOMS = list(S.GEOMETRIES)
SEED, SLICE0 = S.SEED_HI, S.SLICE0


@pytest.fixture(scope="module")
def engines(engine_factory, sd_np):
    """engines of T = 1000, 5 slices of 32x32, one per (schedule, objective, head, precision), made on first use"""
    made, own = {}, []

    def get(kind, objective, head="real", precision=32):
        key = (kind, objective, head, precision)
        if key not in made:
            if head == "real" and kind in S.SCHEDULES:
                e = engine_factory(timesteps=S.T, max_batch=S.MAX_B, max_h=S.MAX_H, max_w=S.MAX_W, objective=objective, beta_schedule=kind)
            else:
                e = load_pkg("engine").CddpmEngine(timesteps=S.T, max_batch=S.MAX_B, max_h=S.MAX_H, max_w=S.MAX_W)
                own.append(e)
                e.load_weights(S.zero_head_state_dict(sd_np) if head == "zero" else sd_np)
                e.set_schedule(S.buffers(kind), objective)
            if precision == 16:
                e.set_precision(16)
            made[key] = e
        return made[key]

    yield get
    for e in own:
        e.close()


def dev(a, shape=None):
    """a numpy fp32 array as a guarded device input"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return inp(t if shape is None else t.view(shape))


def take(out, nan_ok=False):
    """the result as numpy fp32 [B, HW] after the guard checks"""
    torch.cuda.synchronize()
    assert bool((out.bits[:GUARD] == SENTINEL).all()) and bool((out.bits[GUARD + out.n:] == SENTINEL).all()), "a write outside the output"
    got = out.t.cpu().numpy().reshape(out.t.shape[0], -1)
    assert nan_ok or not np.isnan(got).any(), "a NaN in the result: an element never written, or a read outside an input"
    return got


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def ratio(got, ref, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err = np.abs(got.astype(np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def call(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *args, None)
    assert rc == 0, (name, eng.lib.cddpm_last_error(eng._h))


def refused(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *args, None)
    msg = eng.lib.cddpm_last_error(eng._h)
    assert rc != 0 and msg, (name, rc, msg)
    return msg.decode()


_cond = {}


def forward(eng, x_dev, t):
    """model_out of the handle for x_dev [B,1,H,W] at step t, as the step entries compute it: numpy [B, HW]. Leaves the context prepared."""
    B = x_dev.shape[0]
    if B not in _cond:
        _cond[B] = torch.from_numpy(S.cond(B)).cuda()
    return eng.unet_forward(x_dev, int(t), _cond[B]).cpu().numpy().reshape(B, -1)


def image_out(geom, x):
    B, H, W = geom
    return Out((B, 1, H, W), init=torch.from_numpy(x).view(B, 1, H, W))


def p_sample(eng, geom, x, z_dev, t, seed=SEED, slice0=SLICE0, nan_ok=False):
    img = image_out(geom, x)
    call(eng, "cddpm_p_sample", img.ptr(), p(z_dev), seed, slice0, t, *geom)
    return take(img, nan_ok)


def noise_fill(eng, B, HW, t, slice0, stream, seed):
    out = Out((B, HW))
    call(eng, "cddpm_noise_fill", out.ptr(), seed, stream, t, slice0, B, HW // 4, 4)
    return take(out)


def bitwise_step(got, x, mo, t, tab, clip, z, finalize):
    """step_kernel under pred_x0 pins every rounding but expf's: one of the three fp32 neighbours of fp32(exp(0.5 logvar[t])) reproduces
    every element of the call"""
    cands = S.sigma_candidates(t, tab) if t > 0 else [np.float32(0)]
    return any(same_bits(got, S.step_f32(x, mo, t, tab, clip, z, finalize, s)) for s in cands)


# ---------------------------------------------------------------------------------------------------------------- 1. p_sample
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_p_sample(engines, kind, objective, geom):
    eng, tab = engines(kind, objective), S.tables(kind)
    B, H, W = geom
    x, z = S.image(geom), S.noise_explicit(geom)
    x_dev, z_dev, nan_dev = dev(x, (B, 1, H, W)), dev(z), dev(np.full_like(z, np.nan))
    worst = 0.0
    try:
        for t in S.P_SAMPLE_T:
            mo = forward(eng, x_dev, t)
            assert same_bits(mo, forward(eng, x_dev, t)), "two forwards of one handle on one input differ"
            assert not np.isnan(mo).any()
            z_philox = S.noise_ref(B, H * W, t, SLICE0, S.STREAM_Z, SEED)
            for clip in (True, False):
                eng.set_clip_denoised(clip)
                got_z = p_sample(eng, geom, x, z_dev, t)
                got_p = p_sample(eng, geom, x, None, t)
                for got, zz, philox in ((got_z, z, False), (got_p, z_philox, True)):
                    ref = S.step_ref(x, mo, t, tab, objective, clip, zz, False)
                    worst = max(worst, ratio(got, ref, S.step_bound(x, mo, t, tab, objective, zz, False, philox)))
                if t == 0:      # no noise at t = 0: a draw of NaN is not read, and the Philox call gives the same bits
                    assert same_bits(got_z, got_p) and same_bits(got_z, p_sample(eng, geom, x, nan_dev, t))
                else:           # the step that draws z itself is the explicit step fed the generator's field
                    field = noise_fill(eng, B, H * W, t, SLICE0, S.STREAM_Z, SEED)
                    assert same_bits(got_p, p_sample(eng, geom, x, dev(field), t, seed=0, slice0=0))
                    assert not same_bits(got_p, p_sample(eng, geom, x, None, t, seed=SEED & 0xFFFFFFFF))
                if objective == "pred_x0":
                    assert bitwise_step(got_z, x, mo, t, tab, clip, z, False), (t, clip)
                # p_sample never maps to [0,1]; a one-step reverse_range does exactly when its step is 0
                img = image_out(geom, x)
                call(eng, "cddpm_reverse_range", img.ptr(), None, SEED, SLICE0, t, t, *geom)
                assert same_bits(take(img), S.unit_map_f32(got_p) if t == 0 else got_p), (t, clip)
    finally:
        eng.set_clip_denoised(True)
    print(f"p_sample {kind} {objective} {gid(geom)}: err / bound {worst:.3f}" + ("  (explicit z: bit for bit)" if objective == "pred_x0" else ""))
    assert worst <= 1.0


def test_p_sample_precision16(engines):
    """only the forward changes at precision 16: the step stays fp32, to the bit"""
    eng, tab, geom, t = engines("cosine", "pred_x0", precision=16), S.tables("cosine"), (3, 20, 28), 500
    B, H, W = geom
    x, z = S.image(geom), S.noise_explicit(geom)
    x_dev = dev(x, (B, 1, H, W))
    mo = forward(eng, x_dev, t)
    assert same_bits(mo, forward(eng, x_dev, t)) and not np.isnan(mo).any()
    mo32 = forward(engines("cosine", "pred_x0"), x_dev, t)
    assert not same_bits(mo, mo32) and float(np.abs(mo - mo32).max()) < 0.05 * float(np.abs(mo32).max())       # the fp16-operand forward of the same model
    got = p_sample(eng, geom, x, dev(z), t)
    assert bitwise_step(got, x, mo, t, tab, True, z, False)
    r = ratio(got, S.step_ref(x, mo, t, tab, "pred_x0", True, z, False), S.step_bound(x, mo, t, tab, "pred_x0", z, False, False))
    print(f"p_sample precision 16: bit for bit, err / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("kind,objective,geom", [("cosine", "pred_x0", (3, 12, 20)), ("linear", "pred_noise", (5, 4, 8))], ids=["cosine-x0", "linear-noise"])
def test_reverse_range_is_its_p_sample_calls(engines, kind, objective, geom):
    eng = engines(kind, objective)
    B, H, W = geom
    x = S.image(geom)
    forward(eng, dev(x, (B, 1, H, W)), 0)          # prepares the context for B
    for t_hi in (2, 500):
        t_lo = t_hi - 2
        noise = S.rng("range noise", geom, t_hi).standard_normal((t_hi + 1, B, H * W)).astype(np.float32)
        noise[:t_lo] = np.nan                      # indexed by absolute t: nothing below t_lo is read (nor z_0)
        noise[0] = np.nan
        noise_dev = dev(noise)
        for explicit in (True, False):
            cur = x
            for t in range(t_hi, t_lo - 1, -1):
                cur = p_sample(eng, geom, cur, noise_dev[t] if explicit else None, t)
            want = S.unit_map_f32(cur) if t_lo == 0 else cur
            img = image_out(geom, x)
            call(eng, "cddpm_reverse_range", img.ptr(), p(noise_dev) if explicit else None, SEED, SLICE0, t_hi, t_lo, *geom)
            got = take(img)
            assert same_bits(got, want), (t_hi, explicit)
            if t_lo == 0:
                img = image_out(geom, x)
                call(eng, "cddpm_reverse", img.ptr(), p(noise_dev) if explicit else None, SEED, SLICE0, t_hi + 1, *geom)
                assert same_bits(take(img), got)
                assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0 and not same_bits(got, cur)      # clamped x0 at t = 0, mapped to [0,1]


# ---------------------------------------------------------------------------------------------------------------- 2. ddim_step
def ddim_step(eng, geom, x, z_dev, t, coefs, add_noise, finalize, seed=SEED, slice0=SLICE0, nan_ok=False):
    img = image_out(geom, x)
    call(eng, "cddpm_ddim_step", img.ptr(), p(z_dev), seed, slice0, t, *coefs, add_noise, finalize, *geom)
    return take(img, nan_ok)


def ddim_calls(eng, kind, objective, geom, pairs, tab, x=None):
    """every flag combination on the given pairs: bit for bit where the draw is injected or not read, the Philox call bit for bit against
    the explicit call fed the generator's field and inside the float64 bound; -> worst err / bound"""
    B, H, W = geom
    x = S.image(geom) if x is None else x
    z = S.noise_explicit(geom)
    x_dev = dev(x, (B, 1, H, W))
    z_dev = {"explicit": dev(z), "nan": dev(np.full_like(z, np.nan)), "null": None}
    worst = 0.0
    try:
        for t, coef_kind, pair in pairs:
            mo = forward(eng, x_dev, t)
            assert not np.isnan(mo).any()
            field = noise_fill(eng, B, H * W, t, SLICE0, S.STREAM_Z, SEED)
            z_philox = S.noise_ref(B, H * W, t, SLICE0, S.STREAM_Z, SEED)
            for eta in S.DDIM_ETAS:
                coefs = S.ddim_coefficients(coef_kind, pair, eta)
                assert (coefs[2] == 0.0) == (eta == 0.0 or pair[1] == 0)
                for clip in (True, False):
                    eng.set_clip_denoised(clip)
                    for add, fin, zmode in S.DDIM_VARIANTS:
                        got = ddim_step(eng, geom, x, z_dev[zmode], t, coefs, add, fin)
                        what = (kind, objective, geom, t, eta, clip, add, fin, zmode)
                        if zmode == "null" and add:
                            assert same_bits(got, ddim_step(eng, geom, x, dev(field), t, coefs, add, fin, seed=0, slice0=0)), what
                            assert same_bits(got, S.ddim_f32(x, mo, t, tab, objective, clip, coefs, field, add, fin)), what
                            zz, philox = z_philox, True
                        else:
                            assert same_bits(got, S.ddim_f32(x, mo, t, tab, objective, clip, coefs, z, add, fin)), what
                            zz, philox = z, False
                        ref = S.ddim_ref(x, mo, t, tab, objective, clip, coefs, zz, add, fin)
                        worst = max(worst, ratio(got, ref, S.ddim_bound(x, mo, t, tab, objective, coefs, zz, add, fin, philox)))
    finally:
        eng.set_clip_denoised(True)
    return worst


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_ddim_step(engines, kind, objective, geom):
    pairs = [(pair[0], kind, pair) for pair in S.ddim_pairs()]
    worst = ddim_calls(engines(kind, objective), kind, objective, geom, pairs, S.tables(kind))
    print(f"ddim_step {kind} {objective} {gid(geom)}: bit for bit, err / bound {worst:.3f}")
    assert worst <= 1.0


def test_ddim_step_precision16(engines):
    geom = (3, 20, 28)
    pair = S.ddim_pairs()[1]
    worst = ddim_calls(engines("cosine", "pred_x0", precision=16), "cosine", "pred_x0", geom, [(pair[0], "cosine", pair)], S.tables("cosine"))
    print(f"ddim_step precision 16: bit for bit, err / bound {worst:.3f}")
    assert worst <= 1.0


def test_ddim_step_refuses_a_nan_coefficient(engines):
    eng, geom = engines("cosine", "pred_x0"), (3, 12, 20)
    B, H, W = geom
    x = S.image(geom)
    forward(eng, dev(x, (B, 1, H, W)), 500)
    for bad in ((np.nan, 0.5, 0.1), (0.5, np.nan, 0.1), (0.5, 0.5, np.nan)):
        img = image_out(geom, x)
        assert "NaN coefficient" in refused(eng, "cddpm_ddim_step", img.ptr(), None, SEED, SLICE0, 500, *bad, 1, 0, *geom)
        assert img.untouched()


# ---------------------------------------------------------------------------------------------------------------- the clamp
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_clamp_edges_through_the_zero_head(engines, geom):
    """out.2.weight = 0, out.2.bias = BETA: model_out is BETA whatever the (finite) input, and under pred_noise x places x0 = sr x - srm1
    BETA on +-1, their fp32 neighbours, +-3 and values below 1e-3 -- exactly, on the two rows of the clamp schedule whose products are
    exact. Then every evaluation order of x0 gives the target, and the rest of the step is pinned: bit for bit, posterior and DDIM."""
    eng, tab = engines("clamp", "pred_noise", head="zero"), S.tables("clamp")
    B, H, W = geom
    z = S.noise_explicit(geom)
    z_dev = dev(z)
    beta = np.full((B, H * W), S.BETA, dtype=np.float32)
    assert same_bits(forward(eng, dev(S.image(geom), (B, 1, H, W)), 500), beta)
    coefs = S.ddim_coefficients("linear", S.ddim_pairs()[0], 1.0)
    worst = 0.0
    try:
        for t in (S.CLAMP_T_PURE, S.CLAMP_T_SHIFT):
            x = S.clamp_image(geom, t)
            mo = forward(eng, dev(x, (B, 1, H, W)), t)
            assert same_bits(mo, beta)
            x0 = (float(tab.sr[t]) * x.astype(np.float64) - float(tab.srm1[t]) * S.BETA).astype(np.float32)      # exact (host test)
            for clip in (True, False):
                eng.set_clip_denoised(clip)
                got = p_sample(eng, geom, x, z_dev, t)
                assert bitwise_step(got, x, x0, t, tab, clip, z, False), (t, clip)
                worst = max(worst, ratio(got, S.step_ref(x, mo, t, tab, "pred_noise", clip, z, False), S.step_bound(x, mo, t, tab, "pred_noise", z, False, False)))
                for fin in (0, 1):
                    got = ddim_step(eng, geom, x, z_dev, t, coefs, 1, fin)
                    assert same_bits(got, S.ddim_f32(x, mo, t, tab, "pred_noise", clip, coefs, z, 1, fin)), (t, clip, fin)
                    worst = max(worst, ratio(got, S.ddim_ref(x, mo, t, tab, "pred_noise", clip, coefs, z, 1, fin),
                                             S.ddim_bound(x, mo, t, tab, "pred_noise", coefs, z, 1, fin)))
    finally:
        eng.set_clip_denoised(True)
    print(f"clamp edges {gid(geom)}: bit for bit, err / bound {worst:.3f}")
    assert worst <= 1.0


def test_a_nan_stays_a_nan_through_the_clamp(engines):
    """one NaN in x of slice 0 of a batch of 2: that slice's model_out is NaN, so its x0 is NaN at every element and the clamp must hand it
    on (fminf / fmaxf alone would give -1 and a finite result); slice 1 keeps the bits of the clean call"""
    eng, tab, geom, t = engines("clamp", "pred_noise", head="zero"), S.tables("clamp"), (2, 32, 32), S.CLAMP_T_PURE
    B, H, W = geom
    clean = S.clamp_image(geom, t)
    x = clean.copy()
    x[0, 5] = np.nan
    z = S.noise_explicit(geom)
    z_dev = dev(z)
    coefs = S.ddim_coefficients("linear", S.ddim_pairs()[0], 1.0)
    forward(eng, dev(clean, (B, 1, H, W)), t)
    want_p, want_d = p_sample(eng, geom, clean, z_dev, t), ddim_step(eng, geom, clean, z_dev, t, coefs, 1, 0)
    mo = forward(eng, dev(x, (B, 1, H, W)), t)
    assert np.isnan(mo[0]).all() and same_bits(mo[1], np.full(H * W, S.BETA, dtype=np.float32))
    for got, want, ref in ((p_sample(eng, geom, x, z_dev, t, nan_ok=True), want_p, S.step_ref(x, mo, t, tab, "pred_noise", True, z, False)),
                           (ddim_step(eng, geom, x, z_dev, t, coefs, 1, 0, nan_ok=True), want_d, S.ddim_ref(x, mo, t, tab, "pred_noise", True, coefs, z, 1, 0))):
        assert np.isnan(ref[0]).all() and np.isnan(got[0]).all(), int(np.isnan(got[0]).sum())
        assert same_bits(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------- 3. noise_fill
@pytest.mark.parametrize("case", S.NOISE_CASES, ids=S.case_id)
def test_noise_fill(engines, case):
    seed, slice0, t, stream, (B, H, W) = case
    eng = engines("cosine", "pred_x0")
    got = noise_fill(eng, B, H * W, t, slice0, stream, seed)
    ref = S.noise_ref(B, H * W, t, slice0, stream, seed)
    r = ratio(got, ref, S.noise_bound(ref))
    assert same_bits(got, noise_fill(eng, B, H * W, t, slice0, stream, seed))
    for b in range(B):      # a slice's field depends on its global index only
        assert same_bits(got[b:b + 1], noise_fill(eng, 1, H * W, t, (slice0 + b) % 2 ** 64, stream, seed)), b
    print(f"noise_fill {S.case_id(case)}: err / bound {r:.3f}, worst |err| {float(np.abs(got - ref).max()):.2e}")
    assert r <= 1.0


def test_noise_fill_reads_both_key_words_and_identifies_slices_modulo_2_32(engines):
    eng = engines("cosine", "pred_x0")
    f = lambda seed, slice0=0: noise_fill(eng, 2, 32, 1, slice0, S.STREAM_Z, seed)
    assert not same_bits(f(7), f(2 ** 32 + 7)) and not same_bits(f(7), f(7 << 32))
    assert same_bits(f(7, 2 ** 40 + 3), f(7, 3)) and not same_bits(f(7, 3), f(7, 4))


def test_noise_fill_and_q_sample_refuse_what_their_kernels_cannot_compute(engines):
    eng = engines("cosine", "pred_x0")
    tab = S.tables("cosine")
    out, a = Out((4096,)), dev(np.ones(4096, dtype=np.float32))
    assert "aligned" in refused(eng, "cddpm_noise_fill", out.ptr() + 4, 7, S.STREAM_Z, 1, 0, 1, 4, 4)
    assert "aligned" in refused(eng, "cddpm_noise_fill", out.ptr() + 8, 7, S.STREAM_Z, 1, 0, 1, 4, 4)
    assert "2^31" in refused(eng, "cddpm_noise_fill", out.ptr(), 7, S.STREAM_Z, 1, 0, 1 << 15, 256, 256)
    for B, H, W in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 3, 3)):
        refused(eng, "cddpm_noise_fill", out.ptr(), 7, S.STREAM_Z, 1, 0, B, H, W)
    refused(eng, "cddpm_noise_fill", None, 7, S.STREAM_Z, 1, 0, 1, 4, 4)
    q = lambda x, n, o, tu, B, H, W: refused(eng, "cddpm_q_sample", x, n, None, tu, tab.sa.ctypes.data, tab.s1.ctypes.data, S.T, o, B, H, W)
    assert "aligned" in q(p(a) + 4, p(a), out.ptr(), 5, 1, 4, 4)
    assert "aligned" in q(p(a), p(a) + 8, out.ptr(), 5, 1, 4, 4)
    assert "aligned" in q(p(a), p(a), out.ptr() + 4, 5, 1, 4, 4)
    for B, H, W in ((0, 4, 4), (-1, 4, 4), (S.MAX_B + 1, 4, 4), (1, 0, 4), (1, 3, 3)):
        q(p(a), p(a), out.ptr(), 5, B, H, W)
    for tu in (-1, S.T):        # refused before anything is enqueued
        assert "outside" in q(p(a), p(a), out.ptr(), tu, 1, 4, 4)
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- 4. q_sample
@pytest.mark.parametrize("case", S.Q_CASES, ids=S.case_id)
def test_q_sample(engines, case):
    kind, mode, geom = case
    eng, tab = engines(kind, "pred_x0"), S.tables(kind)
    B, H, W = geom
    x01, noise = S.q_operands(geom)
    ts = S.q_t(mode, B)
    t_dev = torch.tensor(ts, dtype=torch.int32, device="cuda") if mode == "per_sample" else None
    out, x_dev, n_dev = Out((B, H * W)), dev(x01), dev(noise)
    call(eng, "cddpm_q_sample", p(x_dev), p(n_dev), p(t_dev), S.Q_T_UNIFORM if t_dev is None else -1, tab.sa.ctypes.data, tab.s1.ctypes.data,
         S.T, out.ptr(), B, H, W)
    got = take(out)
    r = ratio(got, S.q_sample_ref(x01, noise, ts, tab), S.q_sample_bound(x01, noise, ts, tab))
    print(f"q_sample {S.case_id(case)}: err / bound {r:.3f}")
    assert r <= 1.0
    assert same_bits(got, S.q_sample_exact_f32(x01, noise, ts, tab)), "q_sample_value is one fused multiply-add over the rounded second product"


# ---------------------------------------------------------------------------------------------------------------- 5. slice_status
@pytest.mark.parametrize("case", S.STATUS_CASES, ids=S.case_id)
def test_slice_status(engines, case):
    nq, B = case
    eng = engines("cosine", "pred_x0")
    bits, flags = S.status_calls(nq, B)
    ncalls, n = bits.shape[0], B * 4 * nq
    stride = n + 2 * GUARD
    arena = torch.full((ncalls, stride), float("nan"), dtype=torch.float32, device="cuda")
    arena[:, GUARD:GUARD + n] = torch.from_numpy(bits.reshape(ncalls, n).view(np.float32)).cuda()
    assert torch.equal(arena[:, GUARD:GUARD + n].cpu().view(torch.int32), torch.from_numpy(bits.reshape(ncalls, n).view(np.int32))), "the plants' payloads"
    status = torch.full((ncalls, B + 2 * GUARD), SENTINEL, dtype=torch.int32, device="cuda")
    for i in range(ncalls):
        x_ptr = arena[i, GUARD:].data_ptr()
        assert x_ptr % 16 == 0
        call(eng, "cddpm_slice_status", x_ptr, B, 4, nq, status[i, GUARD:].data_ptr())
    torch.cuda.synchronize()
    got = status.cpu().numpy()
    assert (got[:, :GUARD] == SENTINEL).all() and (got[:, GUARD + B:] == SENTINEL).all(), "a write outside the flags"
    wrong = np.nonzero((got[:, GUARD:GUARD + B] != flags).any(axis=1))[0]
    assert wrong.size == 0, (case, wrong[:8], got[wrong[:8], GUARD:GUARD + B], flags[wrong[:8]])


# ---------------------------------------------------------------------------------------------------------------- 6. simplex_fill
@pytest.mark.parametrize("case", S.SIMPLEX_CASES, ids=S.case_id)
def test_simplex_fill_with_other_octaves_persistence_and_frequency(engines, case):
    import simplex_oracle as SO
    seed, n, octaves, persistence, frequency = case
    eng, B = engines("cosine", "pred_x0"), 2
    sentinel = 0x7E55
    buf = torch.full((B * n * n + 2 * GUARD,), sentinel, dtype=torch.int16, device="cuda")
    call(eng, "cddpm_simplex_fill", buf[GUARD:].data_ptr(), seed, B, n, n, octaves, persistence, frequency)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == sentinel).all() and (got[GUARD + B * n * n:] == sentinel).all()
    field = SO.rand_2d_octaves(SO.init_perm(seed), n, n, octaves, persistence, frequency)
    want = torch.from_numpy(field).half().numpy().view(np.int16).reshape(-1)      # float64 -> float32 -> float16, as torch's .half()
    for b in range(B):
        assert np.array_equal(got[GUARD + b * n * n:GUARD + (b + 1) * n * n], want), (case, b)
