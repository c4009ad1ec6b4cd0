"""Host: the case tables, references and bounds of tests/small_op_cases.py are themselves checked here, with no GPU.
1. every float64 reference agrees with an independent torch formulation of the same operation (autograd, torch.optim.Adam, the gather
   split of the head, sums instead of F.group_norm);
2. every case reaches the edge it is there for, recomputed from the constants of the kernels (and, where the library states a plan
   itself, from its own size queries);
3. sensitivity: the results a wrong kernel of that kind would give -- the last pixel of the flat range or the last channel quad dropped,
   the final partial chunk of a reduction dropped, zero padding replaced by the flat neighbour across a row end / a slice end, the last 4
   of K dropped, Adam's bias correction at step - 1, sign(0) = 1 -- differ from the reference by MORE than 4 bounds at one element or
   more, for every case the mutation applies to. A case that cannot show them would test nothing."""
import math

import pytest
import torch
import torch.nn.functional as F

import small_op_cases as S
from conftest import load_pkg

ids = lambda table: [S.case_id(c) for c in table]


def close(a, b, rel=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= rel * (1.0 + float(b.abs().max())), float((a - b).abs().max())


def visible(ref, mut, bound, what):
    """the mutated result differs by more than 4 bounds somewhere (tuples: in one output or more)"""
    if not isinstance(ref, tuple):
        ref, mut, bound = (ref,), (mut,), (bound,)
    worst = max(float(((r - m).abs() - 4 * b).max()) for r, m, b in zip(ref, mut, bound))
    assert worst > 0, (what, worst)


# ---------------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("case", S.CONV_IN1_CASES, ids=ids(S.CONV_IN1_CASES))
def test_conv_in1_reference_and_sensitivity(case):
    C, geom = case
    x, w, b = S.conv_in1_operands(case)
    ref, bound = S.conv_in1_ref(case), S.conv_in1_bound(case)
    close(ref, S.taps(x) @ w.t() + b)
    for mut in ["last_pixel", "last_quad"] + S.neighbour_mutations(geom):
        visible(ref, S.conv_in1_ref(case, mut), bound, (case, mut))


@pytest.mark.parametrize("case", S.HEAD_CASES, ids=ids(S.HEAD_CASES))
def test_head_reference_and_sensitivity(case):
    C, geom = case
    ref, bound = S.head_ref(case), S.head_bound(case)
    close(ref, S.head_by_gather(case))
    for mut in ["last_pixel", "last_quad"] + S.neighbour_mutations(geom):
        visible(ref, S.head_ref(case, mut), bound, (case, mut))
    if geom[0] >= 2:        # the slices differ, so a neighbour read across a slice end shows
        x = S.head_operands(case)[0]
        assert not torch.equal(x[0], x[1])


@pytest.mark.parametrize("case", S.POOL_ACT_CASES, ids=ids(S.POOL_ACT_CASES))
def test_pool_act_reference_and_sensitivity(case):
    C, (B, H, W) = case
    x, coef = S.pool_act_operands(case)
    ref, bound = S.pool_act_ref(case), S.pool_act_bound(case)
    blocks = lambda t: t.reshape(B, H // 2, 2, W // 2, 2, C).mean(dim=(2, 4))
    close(ref[0], blocks(S.act64(x, coef)))
    close(ref[1], blocks(x))
    for mut in ("last_pixel", "last_quad"):
        for o in (0, 1):
            visible(ref[o], S.pool_act_ref(case, mut)[o], bound[o], (case, mut, o))


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=ids(S.LINEAR_CASES))
def test_linear_reference_edges_and_sensitivity(case):
    M, N, K, silu, bias = case
    x, w, b = S.linear_operands(case)
    ref, bound = S.linear_ref(case), S.linear_bound(case)
    a = x * torch.sigmoid(x) if silu else x
    close(ref, (a[:, None, :] * w[None]).sum(-1) + (b if bias else 0.0))
    assert K % 4 == 0
    for mut in ("last_k4", "last_pixel"):
        visible(ref, S.linear_ref(case, mut), bound, (case, mut))


def test_linear_cases_reach_their_edges():
    trips = lambda K, lane: len(range(4 * lane, K, 256))         # linear_kernel: k = 4 lane, + 256 while k < K
    assert trips(4, 0) == 1 and trips(4, 1) == 0
    assert trips(260, 0) == 2 and trips(260, 1) == 1 and (3 * 5) % 4 != 0
    assert all(trips(256, l) == 1 for l in range(64))
    assert trips(252, 62) == 1 and trips(252, 63) == 0
    assert trips(1024, 63) == 4 and trips(2048, 63) == 8
    assert all(K % 4 for K in S.LINEAR_REFUSED_K)


@pytest.mark.parametrize("case", S.RESAMPLE_CASES, ids=ids(S.RESAMPLE_CASES))
def test_resampling_references_and_sensitivity(case):
    B, H, W, C = case
    half, full = S.resample_operands(case)
    # AvgPool2d(2) backward is 1/4 of the upsampled gradient; nearest x2 upsample backward is the 2x2 block sum
    xs = S.nchw(full).clone().requires_grad_(True)
    F.avg_pool2d(xs, 2).backward(S.nchw(half))
    hs = S.nchw(half).clone().requires_grad_(True)
    F.interpolate(hs, scale_factor=2, mode="nearest").backward(S.nchw(full))
    close(S.sumpool2_ref(case, False), S.nhwc(hs.grad))
    close(S.sumpool2_f32(case).double(), S.sumpool2_ref(case, False), 4 * S.U)
    zero = torch.zeros((), dtype=torch.float64)
    for scale in S.UNPOOL_SCALES:
        close(S.unpool2_ref(case, scale, False), S.nhwc(xs.grad) * 4 * scale)
        close(S.unpool2_f32(case, scale).double(), S.unpool2_ref(case, scale, False), S.U)
        for mut in ("last_pixel", "last_quad"):
            visible(S.unpool2_ref(case, scale, False), S.unpool2_ref(case, scale, False, mut), zero, (case, scale, mut))
            visible(S.unpool2_ref(case, scale, True), S.unpool2_ref(case, scale, True, mut), S.unpool2_bound(case, scale), (case, scale, mut, "acc"))
    for mut in ("last_pixel", "last_quad"):
        visible(S.sumpool2_ref(case, False), S.sumpool2_ref(case, False, mut), zero, (case, mut))
        visible(S.sumpool2_ref(case, True), S.sumpool2_ref(case, True, mut), S.sumpool2_bound(case), (case, mut, "acc"))
    # threads of the full- and the half-resolution kernel: tail blocks, and one case whose full-resolution grid has none
    full_n, half_n = B * H * W * C // 4, B * (H // 2) * (W // 2) * C // 4
    assert half_n % 256 != 0 and (full_n % 256 == 0) == (case == (2, 4, 14, 192))


def test_add_inplace_cases():
    for n in S.ADD_INPLACE_N:
        a, b = S.add_inplace_operands(n)
        assert n % 4 == 0 and float(b.abs().min()) >= 0.5        # an element not added is off by 0.5 or more: the comparison is exact
    assert [(-(-(n // 4) // 256), (n // 4) % 256) for n in S.ADD_INPLACE_N] == [(1, 1), (1, 255), (1, 0), (2, 1)]


@pytest.mark.parametrize("case", S.BIAS_GRAD_CASES, ids=ids(S.BIAS_GRAD_CASES))
def test_bias_grad_reference_edges_and_sensitivity(case):
    npix, C = case
    dy = S.bias_grad_operands(case)
    ref, bound = S.bias_grad_ref(case), S.bias_grad_bound(case)
    close(ref, torch.ones(npix, dtype=torch.float64) @ dy)
    nchunk, per, used, last = S.bias_grad_plan(npix)
    muts = ["last_pixel", "last_quad"] + (["last_chunk"] if last < per or used > 1 else [])
    for mut in muts:
        visible(ref, S.bias_grad_ref(case, mut), bound, (case, mut))
    assert C % 4 == 0 and C <= 1024 and all(c % 4 or c > 1024 for c in S.BIAS_GRAD_REFUSED_C)


def test_bias_grad_cases_reach_their_edges():
    plan = S.bias_grad_plan
    assert plan(1) == (1, 1, 1, 1) and plan(511) == (511, 1, 511, 1)
    assert plan(513) == (512, 2, 257, 1) and 512 - 257 == 255            # 255 empty chunks, the last used one partial
    assert plan(1025) == (512, 3, 342, 2)
    rows = lambda C: 256 // (C // 4)
    assert rows(4) == 256 and rows(12) == 85 and 256 - 85 * 3 == 1 and rows(128) == 8 and rows(1024) == 1


@pytest.mark.parametrize("case", S.CORR_CASES, ids=ids(S.CORR_CASES))
def test_chan_image_corr_reference_and_sensitivity(case):
    sign, act, C, geom = case
    B, H, W = geom
    T, coef, s = S.corr_operands(case)
    ref, bound = S.corr_ref(case), S.corr_bound(case)
    Ta = S.nchw(S.act64(T, coef) if act else T)
    if sign == 1:       # the input convolution's weight gradient: T is dL/d(output), s the image
        w = torch.zeros(C, 1, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(s[:, None], w, None, padding=1).backward(Ta)
    else:               # the head's: T is its input, s is dL/d(out)
        w = torch.zeros(1, C, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(Ta, w, None, padding=1).backward(s[:, None])
    close(ref, w.grad.reshape(C, 9))
    per, used, last = S.corr_plan(B * H * W)
    muts = ["last_pixel", "last_quad"] + (["last_chunk"] if used > 1 else []) + S.neighbour_mutations(geom)
    for mut in muts:
        visible(ref, S.corr_ref(case, mut), bound, (case, mut))


def test_chan_image_corr_cases_reach_their_edges():
    assert S.corr_plan(105) == (1, 105, 1) and 256 - 105 == 151
    assert S.corr_plan(1) == (1, 1, 1) and S.corr_plan(18) == (1, 18, 1)
    assert S.corr_plan(544) == (3, 182, 1)


@pytest.mark.parametrize("case", S.HEAD_DGRAD_CASES, ids=ids(S.HEAD_DGRAD_CASES))
def test_head_dgrad_reference_and_sensitivity(case):
    C, geom = case
    B, H, W = geom
    dout, w9 = S.head_dgrad_operands(case)
    ref, bound = S.head_dgrad_ref(case), S.head_dgrad_bound(case)
    a = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(a, w9.t().reshape(1, C, 3, 3), None, padding=1).backward(dout[:, None])
    close(ref, S.nhwc(a.grad))
    for mut in ["last_pixel", "last_quad"] + S.neighbour_mutations(geom):
        visible(ref, S.head_dgrad_ref(case, mut), bound, (case, mut))


def test_one_channel_geometries_reach_their_edges():
    for C in S.CONV_IN1_C:
        ncq = C // 4
        npl, ppb = 256 // ncq, S.conv_in1_ppb(C)
        assert (256 - npl * ncq == 16) == (C in (192, 320)) and (256 - npl * ncq == 0) == (C not in (192, 320))
        assert 105 % ppb != 0                                        # (3, 5, 7): a tail block at every C
        assert any((b * 35) % ppb for b in (1, 2)) or ppb > 105      # block ends that are no slice ends
    assert 256 // (512 // 4) == 2
    lds = lambda C: (64 * (C + 4) + 9 * C) * 4                       # head_dots_kernel's dynamic LDS
    assert lds(512) == 150528 and lds(128) < 65536 < lds(256)
    assert (2 * 8 * 8) % 64 == 0 and all((b * h * w) % 64 for b, h, w in S.GEOMETRIES if (b, h, w) != (2, 16, 24))


@pytest.mark.parametrize("case", S.LOSS_CASES, ids=ids(S.LOSS_CASES))
def test_loss_reference_and_sensitivity(case):
    l2, wb, HW, B, scale = case
    out, target, w = S.loss_operands(case)
    (dout, lb), bound = S.loss_ref(case), S.loss_bound(case)
    o = out.clone().requires_grad_(True)                             # p_losses: reduce over the pixels, weight, mean over the batch
    d = o - target
    per = ((d ** 2) if l2 else d.abs()).reshape(B, -1).mean(dim=1) * (w if wb else 1.0)
    per.mean().backward()
    close(lb, per.detach())
    close(dout, o.grad * scale)
    zeros = (out == target)
    assert bool(zeros.any()) == (HW >= 2) and not bool(zeros[:, -1].any())
    assert bool((dout[zeros] == 0).all())                            # torch.sign(0) = 0
    visible((dout, lb), S.loss_ref(case, "last_pixel"), bound, (case, "last_pixel"))
    if not l2 and HW >= 2:
        visible(dout, S.loss_ref(case, "sign0")[0], bound[0], (case, "sign0"))


@pytest.mark.parametrize("case", S.ADAM_CASES, ids=ids(S.ADAM_CASES))
def test_adam_reference_and_sensitivity(case):
    n, step, unscale = case
    lr, b1, b2, eps = S.adam_hyper_abi()
    p, g, m, v = S.adam_operands(case)
    ref, bound = S.adam_ref(case), S.adam_bound(case)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g * unscale
    opt.step()
    close(ref[0], q.detach(), 1e-11)
    close(ref[1], opt.state[q]["exp_avg"])
    close(ref[2], opt.state[q]["exp_avg_sq"])
    assert bool((v >= 0).all()) and bool((m != 0).all())
    if n >= 4:
        gu = (g * unscale).abs()
        assert bool((gu == 0).any()) and bool(((gu > 0) & (gu < 2e-12)).any()) and bool((gu > 1e9).any())
        small = (gu > 0) & (gu < 2e-12)
        assert bool((ref[2][small].sqrt() < eps).all())              # sqrt(v) below eps there
    visible(ref, S.adam_ref(case, "last_pixel"), bound, (case, "last_pixel"))
    if step <= 1000:        # at step 100000 both corrections are 1 to the last bit at either step count
        visible(ref[0], S.adam_ref(case, "bias_step")[0], bound[0], (case, "bias_step"))


@pytest.mark.parametrize("case", S.GN_CASES, ids=ids(S.GN_CASES))
def test_gn_reference_edges_and_sensitivity(case):
    C0, C1, H, W, film, ratio = case
    C = C0 + C1
    ref, bound = S.gn_normalised(case), S.gn_bound(case)
    fl = S.gn_operands(case)[3]
    by_sums = S._gn_by_sums(case)
    if fl is not None:
        by_sums = by_sums * (1 + fl[:, :C, None, None]) + fl[:, C:, None, None]
    # E[x^2] - mean^2 in float64 loses (mean / sigma)^2 2^-53 of the variance: 1e-12 relative at 100 sigma
    close(ref, by_sums, 1e-9)
    assert C0 % 4 == 0 and C1 % 4 == 0 and C % 32 == 0
    for mut in ("last_pixel", "last_quad"):
        worst = float((S.gn_normalised(case, mut) - ref).abs().max())
        assert worst > 4 * bound, (case, mut, worst, bound)


def test_gn_cases_reach_their_edges():
    lib = load_pkg("_lib").load_library()
    for (H, W) in S.GN_HW:
        assert lib.cddpm_stat_records(H, W, 2) == S.gn_nsplit(H * W), (H, W)       # the library's own count of the sweep's records
    assert [S.gn_nsplit(h * w) for h, w in S.GN_HW] == [1, 1, 2, 64, 16, 17]
    idle = lambda C: 256 - (256 // (C // 4)) * (C // 4)
    assert idle(128) == 0 and idle(384) == 64 and idle(1024) == 0 and 256 // (1024 // 4) == 1 and idle(36) == 4 and idle(92) == 3
    assert 32 % (384 // 32) != 0                                     # (32, 352): a group of 12 straddles the two sources
    assert {c[:2] for c in S.GN_CASES} == set(S.GN_CHANNELS) | {(1024, 0)}
    for ch in S.GN_CHANNELS:
        assert {c[2:4] for c in S.GN_CASES if c[:2] == ch} == set(S.GN_HW)
    assert {c[4] for c in S.GN_CASES} == {True, False} and {c[5] for c in S.GN_CASES} == {0.0, 100.0}


@pytest.mark.parametrize("case", S.LINBWD_CASES, ids=ids(S.LINBWD_CASES))
def test_linear_backward_reference_edges_and_sensitivity(case):
    M, N, K, silu = case
    x, w, dy = S.linbwd_operands(case)
    ref, bound = S.linbwd_ref(case), S.linbwd_bound(case)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), torch.zeros(N, dtype=torch.float64, requires_grad=True)
    F.linear(F.silu(xr) if silu else xr, wr, br).backward(dy)
    for got, want in zip(ref, (wr.grad, br.grad, xr.grad)):
        close(got, want)
    # the skinny path by the library's own rule: its scratch request holds LIN_NSPLIT partial planes of dx exactly when it is taken
    nbytes = load_pkg("training").scratch_query("linear_backward", M, N, K, silu)
    assert (nbytes >= S.LIN_NSPLIT * M * K * 4) == S.linbwd_skinny(case), (case, nbytes)
    for mut in ("last_pixel", "last_k4"):
        got = S.linbwd_ref(case, mut)
        for o in ((0, 1, 2) if mut == "last_pixel" else (0, 2)):
            visible(ref[o], got[o], bound[o], (case, mut, o))


def test_linear_backward_cases_reach_their_edges():
    per = lambda N: math.ceil(N / S.LIN_NSPLIT)
    assert per(1024) == 32 and per(1500) == 47 and (64 + 3) // 4 == 16 and 100 % 64 != 0
    assert (7 + 3) // 4 == 2 and 7 - 3 * 2 == 1                     # M = 7: row groups of 2, the last holds one row
    assert [S.linbwd_skinny(c) for c in S.LINBWD_CASES] == [True, False, False, True, True]


def test_every_operator_states_its_count():
    assert all(isinstance(v, str) and v for v in S.N_ROUNDINGS.values()) and len(S.N_ROUNDINGS) >= 15
