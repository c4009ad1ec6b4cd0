"""Host: the case tables, references, bounds and restatements of tests/step_op_cases.py are themselves checked here, with no GPU.
1. every float64 reference agrees to 1e-12 with an independent formulation: the project's CPU restatements of p_sample, ddim_sample and
   q_sample (oracle/cddpm_oracle.py) run in float64 on a given model_out, the draws with synth.noise_z / noise_xT / normal_quads (these
   are fp32 Box-Muller: compared at the 4e-6 the suite has always held them to);
2. every case reaches the edge it is there for: quad counts against the 256-thread blocks and the 1024-thread status workgroup, the slice
   index across 2^32, the clamp's shares and its exact targets;
3. every numpy float32 restatement lies inside the float64 bound of the same case;
4. sensitivity: the result a wrong kernel of each named kind would give differs from the reference by MORE than 4 bounds at one element or
   more (any bit, where the device test compares bits), for every case the mutation applies to."""
import math

import numpy as np
import pytest
import torch

import step_op_cases as S

synth = S.synth
GEOMS = list(S.GEOMETRIES)
gid = lambda g: "x".join(map(str, g))
SEED, SLICE0 = S.SEED_HI, S.SLICE0


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(np.abs(a - b).max()) <= rel * (1.0 + float(np.abs(b).max())), float(np.abs(a - b).max())


def buf64(kind):
    return {k: v.double() for k, v in S.buffers(kind).items()}


def philox_z(geom, t):
    B, H, W = geom
    return S.noise_ref(B, H * W, t, SLICE0, S.STREAM_Z, SEED)


# ---------------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_posterior_reference_is_the_oracles_p_sample_in_float64(oracle, monkeypatch, kind, objective, geom):
    B, H, W = geom
    x, mo, tab = S.image(geom), S.model_out_standin(geom), S.tables(kind)
    monkeypatch.setattr(oracle, "unet_forward", lambda *a, **k: torch.from_numpy(mo.astype(np.float64)))
    for t in S.P_SAMPLE_T:
        z = synth.noise_z(SEED, t, SLICE0, B, H, W).reshape(B, H * W)
        for clip in (True, False):
            want = oracle.p_sample(torch.from_numpy(x.astype(np.float64)), t, None, None, buf64(kind), torch.from_numpy(z.astype(np.float64)),
                                   objective, clip_denoised=clip).numpy()
            close(S.step_ref(x, mo, t, tab, objective, clip, z, False), want)
            close(S.step_ref(x, mo, t, tab, objective, clip, z, True), (want + 1) * 0.5)


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_ddim_reference_is_the_oracles_ddim_sample_in_float64(oracle, monkeypatch, kind, objective, geom):
    """one pair at a time: ddim_sample's own float64 coefficients from the fp32 alphas_cumprod_prev, handed to the reference as given"""
    x, mo, tab, z = S.image(geom), S.model_out_standin(geom), S.tables(kind), S.noise_explicit(geom)
    monkeypatch.setattr(oracle, "unet_forward", lambda *a, **k: torch.from_numpy(mo.astype(np.float64)))
    acp = S.buffers(kind)["alphas_cumprod_prev"].double().numpy()
    for pair in S.ddim_pairs():
        monkeypatch.setattr(oracle, "ddim_time_pairs", lambda *a, **k: [pair])
        time, time_next = pair
        for eta in S.DDIM_ETAS:
            a, an = float(acp[time]), float(acp[time_next])
            sigma = eta * math.sqrt((1 - a / an) * (1 - an) / (1 - a))
            coefs = (math.sqrt(an), math.sqrt((1 - an) - sigma ** 2), sigma)
            for clip in (True, False):
                want = oracle.ddim_sample(torch.from_numpy(x.astype(np.float64)), None, None, buf64(kind), lambda _t: torch.from_numpy(z.astype(np.float64)),
                                          1, eta=eta, objective=objective, clip_denoised=clip).numpy()
                close(S.ddim_ref(x, mo, time, tab, objective, clip, coefs, z, time_next > 0, False), want * 2 - 1)


def test_ddim_reference_maps_to_the_unit_interval_under_finalize_only():
    geom, tab = GEOMS[1], S.tables("cosine")
    x, mo, z = S.image(geom), S.model_out_standin(geom), S.noise_explicit(geom)
    pair = S.ddim_pairs()[0]
    coefs = S.ddim_coefficients("cosine", pair, 1.0)
    a = S.ddim_ref(x, mo, pair[0], tab, "pred_x0", True, coefs, z, True, False)
    close(S.ddim_ref(x, mo, pair[0], tab, "pred_x0", True, coefs, z, True, True), (a + 1) * 0.5)
    # add_noise = 0: the draw is not read
    close(S.ddim_ref(x, mo, pair[0], tab, "pred_x0", True, coefs, z * np.nan, False, False), S.ddim_ref(x, mo, pair[0], tab, "pred_x0", True, coefs, 0 * z, True, False))


def test_ddim_pairs_and_coefficients_are_the_mirrors():
    early, middle, last = S.ddim_pairs()
    assert early[0] > middle[0] > last[0] > last[1] == 0 and early[0] < S.T
    for kind in S.SCHEDULES:
        for pair in S.ddim_pairs():
            cx0, ceps, sigma = S.ddim_coefficients(kind, pair, 1.0)
            assert all(math.isfinite(c) for c in (cx0, ceps, sigma)) and 0 < cx0 <= 1
            assert S.ddim_coefficients(kind, pair, 0.0)[2] == 0.0
            assert (sigma == 0.0) == (pair[1] == 0)


@pytest.mark.parametrize("case", S.NOISE_CASES, ids=S.case_id)
def test_noise_reference_is_synths_draw_and_its_bound_stays_inside_the_old_limit(case):
    seed, slice0, t, stream, (B, H, W) = case
    ref = S.noise_ref(B, H * W, t, slice0, stream, seed)
    for b in range(B):
        got = synth.normal_quads(H * W // 4, t, slice0 + b, stream, seed)
        assert float(np.abs(got - ref[b]).max()) < 4e-6
    if stream == S.STREAM_Z:
        assert float(np.abs(synth.noise_z(seed, t, slice0, B, H, W).reshape(B, -1) - ref).max()) < 4e-6
    elif t == 0:
        assert float(np.abs(synth.noise_xT(seed, slice0, B, H, W).reshape(B, -1) - ref).max()) < 4e-6
    assert float(S.noise_bound(ref).max()) <= 4e-6 < 2e-5
    assert float(np.abs(ref).max()) > 2.5 and abs(float(ref.mean())) < 0.5


@pytest.mark.parametrize("case", S.Q_CASES, ids=S.case_id)
def test_q_sample_reference_is_the_oracles_q_sample_in_float64(oracle, case):
    kind, mode, geom = case
    x01, noise = S.q_operands(geom)
    ts = S.q_t(mode, geom[0])
    want = oracle.q_sample(torch.from_numpy(x01.astype(np.float64)) * 2 - 1, torch.tensor(ts), torch.from_numpy(noise.astype(np.float64)), buf64(kind)).numpy()
    close(S.q_sample_ref(x01, noise, ts, S.tables(kind)), want)


def test_status_reference_is_torchs_isfinite():
    for nq, B in S.STATUS_CASES:
        bits, flags = S.status_calls(nq, B)
        want = (~torch.isfinite(torch.from_numpy(bits.view(np.float32)))).any(dim=-1).int().numpy()
        assert np.array_equal(S.status_ref(bits), want) and np.array_equal(flags, want)


# ---------------------------------------------------------------------------------------------------------------- 2. edges
def test_geometries_reach_the_block_edges():
    q = {g: S.quads(g) for g in S.GEOMETRIES}
    assert sorted(q.values()) == [4, 40, 180, 420, 512]
    assert q[(1, 4, 4)] < 64                                              # a partial wave
    assert 64 < q[(3, 12, 20)] < 256                                      # one partial block
    assert 256 < q[(3, 20, 28)] < 512 and q[(3, 20, 28)] % 256 % 64       # a second block whose last wave is partial
    assert q[(2, 32, 32)] == 2 * 256
    assert q[(5, 4, 8)] == 5 * 8 < 64                                     # nq = 8: five slices inside one wave
    for B, H, W in S.GEOMETRIES:
        assert H % 4 == 0 and W % 4 == 0 and B <= S.MAX_B and H <= S.MAX_H and W <= S.MAX_W
    # slices end inside a block: a thread's b = e / nq changes within a wave
    assert (3 * 12 * 20 // 4) // 3 == 60 and 60 % 64


def test_noise_cases_cover_every_listed_value_and_the_slice_wrap():
    seeds, slices, ts, streams, geoms = (set(c[i] for c in S.NOISE_CASES) for i in range(5))
    assert seeds == set(S.NOISE_SEEDS) and slices == set(S.NOISE_SLICE0) and ts == set(S.NOISE_T)
    assert streams == {S.STREAM_XT, S.STREAM_Z} == {0x1001, 0x1002} and set(S.GEOMETRIES) <= geoms
    assert sum(1 for s in S.NOISE_SEEDS if s >> 32) == 4 and max(S.NOISE_SEEDS) == 2 ** 64 - 1
    wrap = [c for c in S.NOISE_CASES if c[1] == 2 ** 32 - 2]
    assert wrap and all(c[4][0] == 4 for c in wrap)                       # slices 2^32 - 2, 2^32 - 1, 0, 1
    B, H, W = S.WRAP_GEOM
    seed, t = wrap[0][0], wrap[0][2]
    ref = S.noise_ref(B, H * W, t, 2 ** 32 - 2, S.STREAM_Z, seed)
    assert np.array_equal(ref[2:], S.noise_ref(2, H * W, t, 0, S.STREAM_Z, seed))
    assert not np.array_equal(ref[:2], ref[2:])
    # slices are identified modulo 2^32, as synth masks them
    assert np.array_equal(S.noise_ref(1, 32, 1, 2 ** 40 + 3, S.STREAM_Z, 7), S.noise_ref(1, 32, 1, 3, S.STREAM_Z, 7))
    assert np.array_equal(synth.normal_quads(8, 1, 2 ** 40 + 3, S.STREAM_Z, 7), synth.normal_quads(8, 1, 3, S.STREAM_Z, 7))
    # seeds 7 and 2^32 + 7 share the low key word only
    assert not np.array_equal(S.normal64(8, 1, 0, S.STREAM_Z, 7), S.normal64(8, 1, 0, S.STREAM_Z, 2 ** 32 + 7))


def test_status_cases_straddle_the_workgroup_and_its_unroll():
    trips = lambda nq, thread: len(range(thread, nq, S.STATUS_THREADS))        # slice_status_kernel: q = thread, + 1024 while q < nq
    assert S.STATUS_THREADS == 1024
    assert trips(1, 0) == 1 and trips(1, 1) == 0
    assert trips(63, 62) == 1 and trips(63, 63) == 0                           # one wave, its last lane idle
    assert trips(1023, 1022) == 1 and trips(1023, 1023) == 0
    assert all(trips(1024, th) == 1 for th in (0, 1023))
    assert trips(1025, 0) == 2 and trips(1025, 1) == 1                         # the second trip has one thread
    assert trips(1537, 512) == 2 and trips(1537, 513) == 1                     # ... half a workgroup and one more
    for nq, B in S.STATUS_CASES:
        bits, flags = S.status_calls(nq, B)
        per_plant = 4 * len({0, nq - 1})
        n = len(S.STATUS_PLANTS) * per_plant
        assert bits.shape == (n + 3, B, 4 * nq)
        assert flags[:n].sum(axis=1).tolist() == [1] * n and flags[n:].sum() == 0
        planted = ((bits & 0x7F800000) == 0x7F800000)
        assert planted.sum(axis=(1, 2)).tolist() == [1] * n + [0] * 3                     # each plant alone
        where = {int(np.nonzero(p.reshape(-1))[0][0]) % (4 * nq) for p in planted[:n]}
        assert where == set(range(4)) | set(range(4 * nq - 4, 4 * nq))                    # every lane of the first and the last quad
        assert {int(np.nonzero(p.reshape(B, -1).any(axis=1))[0][0]) for p in planted[:n]} == set(range(B))      # in every slice of the batch
        f = np.abs(bits[n:].view(np.float32))
        assert f.max() > 3.3e38 and (f == 0).any() and ((f > 0) & (f < 1.17e-38)).any()
        assert (bits[n:] == 0x80000000).any()                                              # -0.0
    assert {bin(v >> 31) for v in S.STATUS_PLANTS.values()} == {"0b0", "0b1"}
    assert S.STATUS_PLANTS["signalling NaN"] & 0x00400000 == 0 and S.STATUS_PLANTS["quiet NaN"] & 0x00400000


@pytest.mark.parametrize("t", [S.CLAMP_T_PURE, S.CLAMP_T_SHIFT])
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_clamp_cases_place_x0_exactly_and_hold_their_shares(geom, t):
    tab = S.tables("clamp")
    x = S.clamp_image(geom, t)
    mo = np.full_like(x, S.BETA)
    x0 = float(tab.sr[t]) * x.astype(np.float64) - float(tab.srm1[t]) * mo.astype(np.float64)
    targets = np.array(S.CLAMP_TARGETS[t])
    # exact in every evaluation order: both products and the difference are fp32 numbers
    exact = targets[np.abs(targets) >= 0.3]
    assert set(exact.tolist()) <= set(np.unique(x0).tolist())
    assert np.array_equal(x0.astype(np.float32).astype(np.float64), x0)
    assert np.array_equal((tab.sr[t] * x).astype(np.float64), float(tab.sr[t]) * x.astype(np.float64))
    for v in (1.0, -1.0, S.ONE_UP, -S.ONE_UP, -S.ONE_DOWN, 3.0, -3.0) + ((S.ONE_DOWN,) if t == S.CLAMP_T_PURE else ()):
        assert (x0 == v).any(), v
    assert ((np.abs(x0) < 1e-3) & (x0 != 0)).any()
    n = x0.size
    assert n % 16 == 0
    assert (x0 > 1).sum() * 4 >= n and (x0 < -1).sum() * 4 >= n and (np.abs(x0) <= 1).sum() * 4 >= n
    # the shares on the float64 reference of the step itself: clip on and off differ exactly on the clamped elements
    z = S.noise_explicit(geom)
    on = S.step_ref(x, mo, t, tab, "pred_noise", True, z, False)
    off = S.step_ref(x, mo, t, tab, "pred_noise", False, z, False)
    assert np.array_equal(on != off, np.abs(x0) > 1)


def test_the_ill_conditioned_row_is_among_the_cases():
    tab = S.tables("linear")
    assert 999 in S.P_SAMPLE_T and 150 < float(tab.srm1[999]) < 165 and "pred_noise" in S.OBJECTIVES
    assert float(S.tables("cosine").logvar[0]) == float(np.float32(math.log(1e-20)))       # sigma(0) = 1e-10: only a NaN draw shows at t = 0


# ---------------------------------------------------------------------------------------------------------------- 3. restatements
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_float32_restatements_lie_inside_their_float64_bounds(kind, geom):
    x, mo, tab, z = S.image(geom), S.model_out_standin(geom), S.tables(kind), S.noise_explicit(geom)
    inside = lambda got, ref, bound: bool((np.abs(got.astype(np.float64) - ref) <= bound).all())
    for t in S.P_SAMPLE_T:
        for clip in (True, False):
            for fin in (False, True):
                for sigma in S.sigma_candidates(t, tab)[1:2]:
                    assert inside(S.step_f32(x, mo, t, tab, clip, z, fin, sigma), S.step_ref(x, mo, t, tab, "pred_x0", clip, z, fin),
                                  S.step_bound(x, mo, t, tab, "pred_x0", z, fin, False)), (t, clip, fin)
    for pair in S.ddim_pairs():
        for eta in S.DDIM_ETAS:
            coefs = S.ddim_coefficients(kind, pair, eta)
            for objective in S.OBJECTIVES:
                for clip in (True, False):
                    for add, fin, _z in S.DDIM_VARIANTS:
                        got = S.ddim_f32(x, mo, pair[0], tab, objective, clip, coefs, z, add, fin)
                        assert inside(got, S.ddim_ref(x, mo, pair[0], tab, objective, clip, coefs, z, add, fin),
                                      S.ddim_bound(x, mo, pair[0], tab, objective, coefs, z, add, fin)), (pair, eta, objective, clip, add, fin)
    for mode in S.Q_T_MODES:
        x01, noise = S.q_operands(geom)
        ts = S.q_t(mode, geom[0])
        if S.quads(geom) <= 180:       # Fractions: the small geometries
            assert inside(S.q_sample_exact_f32(x01, noise, ts, tab), S.q_sample_ref(x01, noise, ts, tab), S.q_sample_bound(x01, noise, ts, tab))


def test_round_f32_rounds_once_to_nearest_even():
    from fractions import Fraction as Fr
    one, up = Fr(1), Fr(float(np.nextafter(np.float32(1), np.float32(2))))
    assert S.round_f32((one + up) / 2) == np.float32(1)                          # a tie: the even mantissa
    assert S.round_f32((one + up) / 2 + Fr(1, 2 ** 80)) == np.float32(float(up))   # just above it: float64 would have rounded to the tie first
    assert S.round_f32(Fr(1, 3)) == np.float32(1 / 3)


# ---------------------------------------------------------------------------------------------------------------- 4. sensitivity
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_a_wrong_posterior_step_shows(kind, objective, geom):
    x, mo, tab = S.image(geom), S.model_out_standin(geom), S.tables(kind)
    bitwise = objective == "pred_x0"
    for t in S.P_SAMPLE_T:
        for z in (S.noise_explicit(geom), philox_z(geom, t)):
            for clip in (True, False):
                for fin in (False, True):
                    ref = S.step_ref(x, mo, t, tab, objective, clip, z, fin)
                    bound = S.step_bound(x, mo, t, tab, objective, z, fin, True)
                    muts = ["coef_swapped"] + (["sigma_full"] if t > 0 else []) + (["map_always"] if not fin else []) + (["clip_always"] if not clip else [])
                    for m in muts:
                        assert S.differs(ref, S.step_ref(x, mo, t, tab, objective, clip, z, fin, m), bound), (t, clip, fin, m)
        if bitwise and t > 0 and S.quads(geom) >= 180:      # a sigma one ulp off moves a bit somewhere: the three candidates are told apart
            r = [S.step_f32(x, mo, t, tab, True, S.noise_explicit(geom), False, s) for s in S.sigma_candidates(t, tab)]
            assert S.differs(r[0], r[1]) and S.differs(r[1], r[2])
    # noise at t = 0: sigma(0) = 1e-10 hides a finite draw, so the device test injects a draw of NaN
    nan_z = np.full_like(x, np.nan)
    ref = S.step_ref(x, mo, 0, tab, objective, True, nan_z, False)
    assert not np.isnan(ref).any() and S.differs(ref, S.step_ref(x, mo, 0, tab, objective, True, nan_z, False, "noise_at_0"))
    # the clamp turning a NaN into -1, under pred_x0: a NaN in model_out is x0 itself (pred_noise: the zero-head case below)
    if objective == "pred_x0":
        bad = mo.copy()
        bad[0, 1] = np.nan
        ref = S.step_ref(x, bad, 500, tab, objective, True, S.noise_explicit(geom), False)
        assert np.isnan(ref[0, 1]) and S.differs(ref, S.step_ref(x, bad, 500, tab, objective, True, S.noise_explicit(geom), False, "nan_to_-1"))


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
@pytest.mark.parametrize("objective", S.OBJECTIVES)
@pytest.mark.parametrize("kind", S.SCHEDULES)
def test_a_wrong_ddim_step_shows(kind, objective, geom):
    """bitwise cases: any bit of the fp32 restatement's neighbourhood, i.e. any difference of the float64 results beyond 4 bounds is more
    than enough; asserted at 4 bounds throughout"""
    x, mo, tab, z = S.image(geom), S.model_out_standin(geom), S.tables(kind), S.noise_explicit(geom)
    for pair in S.ddim_pairs():
        for eta in S.DDIM_ETAS:
            coefs = S.ddim_coefficients(kind, pair, eta)
            for add, fin, _z in S.DDIM_VARIANTS:
                bound = S.ddim_bound(x, mo, pair[0], tab, objective, coefs, z, add, fin, True)
                for clip in (True, False):
                    ref = S.ddim_ref(x, mo, pair[0], tab, objective, clip, coefs, z, add, fin)
                    muts = ["coef_swapped"] + (["eps_from_clamped"] if clip and pair[1] > 0 else []) + ([] if clip else ["clip_always"])
                    for m in muts:
                        assert S.differs(ref, S.ddim_ref(x, mo, pair[0], tab, objective, clip, coefs, z, add, fin, m), bound), (pair, eta, clip, add, fin, m)
    # the last pair has coef_eps = 0: eps does not enter and its source cannot show there -- it shows on the two others (above)
    assert S.ddim_coefficients(kind, S.ddim_pairs()[-1], 1.0)[1] == 0.0


def test_the_clamps_nan_shows_in_the_zero_head_case():
    """the device's NaN case: pred_noise on the clamp schedule, a NaN planted in x. Through the UNet the whole slice's model_out becomes
    NaN; x0 = sr x - srm1 eps is then NaN at EVERY element while c2 x is NaN at the planted one only: a clamp that returned -1 for a NaN
    would leave finite results everywhere else in the slice"""
    geom, t, tab = (2, 32, 32), S.CLAMP_T_PURE, S.tables("clamp")
    x = S.clamp_image(geom, t).copy()
    x[0, 5] = np.nan
    mo = np.full_like(x, S.BETA)
    mo[0] = np.nan
    z = S.noise_explicit(geom)
    ref = S.step_ref(x, mo, t, tab, "pred_noise", True, z, False)
    mut = S.step_ref(x, mo, t, tab, "pred_noise", True, z, False, "nan_to_-1")
    assert np.isnan(ref[0]).all() and not np.isnan(ref[1]).any()
    assert np.isnan(mut[0]).sum() == 1 and S.differs(ref, mut)
    coefs = S.ddim_coefficients("linear", S.ddim_pairs()[0], 1.0)
    ref = S.ddim_ref(x, mo, t, tab, "pred_noise", True, coefs, z, 1, 0)
    assert np.isnan(ref[0]).all() and not np.isnan(ref[1]).any()


@pytest.mark.parametrize("case", S.NOISE_CASES, ids=S.case_id)
def test_a_wrong_draw_shows(case):
    seed, slice0, t, stream, (B, H, W) = case
    ref = S.noise_ref(B, H * W, t, slice0, stream, seed)
    bound = S.noise_bound(ref)
    muts = ["sincos_swapped", "last_quad"]
    muts += ["key_hi_dropped"] if seed >> 32 else []
    muts += ["slice0_not_added"] if slice0 % 2 ** 32 else []
    muts += ["t_missing"] if t else []
    muts += ["stream_fixed"] if stream != S.STREAM_XT else []
    muts += ["wrong_nq"] if (B, H, W) == (5, 4, 8) else []
    for m in muts:
        assert S.differs(ref, S.noise_ref(B, H * W, t, slice0, stream, seed, m), bound), m


def test_every_draw_mutation_has_a_case():
    applies = {"key_hi_dropped": lambda c: c[0] >> 32, "slice0_not_added": lambda c: c[1] % 2 ** 32, "t_missing": lambda c: c[2],
               "stream_fixed": lambda c: c[3] != S.STREAM_XT, "wrong_nq": lambda c: c[4] == (5, 4, 8)}
    for name, f in applies.items():
        assert any(f(c) for c in S.NOISE_CASES), name


@pytest.mark.parametrize("case", S.Q_CASES, ids=S.case_id)
def test_a_wrong_q_sample_shows(case):
    kind, mode, geom = case
    x01, noise = S.q_operands(geom)
    ts, tab = S.q_t(mode, geom[0]), S.tables(kind)
    ref, bound = S.q_sample_ref(x01, noise, ts, tab), S.q_sample_bound(x01, noise, ts, tab)
    assert float((x01 == 0).sum()) and float((x01 == 0.5).sum()) and float((x01 == 1).sum()) and float((noise == 0).sum()) and float(np.abs(noise).max()) == 6.0
    if mode == "per_sample" and geom[0] > 1:
        assert S.differs(ref, S.q_sample_ref(x01, noise, ts, tab, "t_from_slice0"), bound)
    dropped = ref.copy()
    dropped[:, -4:] = np.nan          # the last quad of a slice not written: the sentinel stays
    assert S.differs(ref, dropped, bound)


def test_a_status_flag_from_the_first_trip_only_shows():
    for nq, B in S.STATUS_CASES:
        bits, flags = S.status_calls(nq, B)
        wrong = S.status_ref(bits, "first_1024_quads")
        assert (nq > S.STATUS_THREADS) == (not np.array_equal(wrong, flags)), nq
