"""GPU: the memory-bound operators one call at a time, at loop and shape edges (csrc/small_kernels.hip, the elementwise / reduction part
of csrc/train_kernels.hip, the stand-alone GroupNorm sweep of csrc/norm_kernels.hip), against the float64 references of
tests/small_op_cases.py and to its derived bounds: |got - ref64| <= n u A 1.01 per element, bit for bit where the result is one rounding
or a fixed order of additions. tests/test_small_op_cases_host.py checks the references, the edges each case names and that every case
would show a kernel that is wrong in the ways such kernels go wrong.

Every operand and result is a 16-byte-aligned view inside a larger device tensor with 64 floats of guard on both sides: the inputs'
guards hold NaN, the outputs' guards (and the outputs, before the call) a sentinel bit pattern that is a NaN too. After the call the
outputs' guards must be unchanged to the bit and the result must hold no NaN: a read or a write a few elements past an end, or an element
never written, fails an assertion -- all of it inside one allocation. Refused calls return non-zero, leave a message and the output
untouched; nothing of them reaches a kernel."""
import math

import pytest
import torch

import small_op_cases as S

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FC5A5A5          # a quiet NaN: an output element that was never written shows up as one
ids = lambda table: [S.case_id(c) for c in table]


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=32, max_w=32)


class Out:
    """an output of `shape` between sentinel guards; init: the old value of an accumulating / in-place operator"""

    def __init__(self, shape, init=None):
        self.n = math.prod(shape)
        self.bits = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.bits.view(torch.float32)[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init.float())
        assert self.t.data_ptr() % 16 == 0
        self.before = self.bits.clone()

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """the result in float64 on the host, after the guard and NaN checks"""
        torch.cuda.synchronize()
        assert bool((self.bits[:GUARD] == SENTINEL).all()) and bool((self.bits[GUARD + self.n:] == SENTINEL).all()), "a write outside the output"
        assert not bool(torch.isnan(self.t).any()), "a NaN in the result: an element never written, or a read outside an input"
        return self.t.cpu().double()

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.bits, self.before)


def inp(t):
    """a device copy of `t` (fp32) between NaN guards; None stays None"""
    if t is None:
        return None
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    v = buf[GUARD:GUARD + n].view(t.shape)
    v.copy_(t.float())
    assert v.data_ptr() % 16 == 0
    return v


def p(t):
    return None if t is None else t.data_ptr()


def run(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *args, None)
    assert rc == 0, (name, eng.lib.cddpm_last_error(eng._h))


def refused(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *args, None)
    msg = eng.lib.cddpm_last_error(eng._h)
    assert rc != 0 and msg, (name, rc, msg)
    return msg.decode()


def ratio(got, ref, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return float(r.max())


def report(op, case, **ratios):
    print(f"{op} {S.case_id(case) if isinstance(case, tuple) else case}: " + "  ".join(f"{k} err / bound {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (op, case, ratios)


# ---------------------------------------------------------------------------------------------------------------- small_kernels.hip
@pytest.mark.parametrize("case", S.CONV_IN1_CASES, ids=ids(S.CONV_IN1_CASES))
def test_conv_in1(eng, case):
    C, (B, H, W) = case
    x, w, b = (inp(t) for t in S.conv_in1_operands(case))
    out = Out((B, H, W, C))
    run(eng, "cddpm_op_conv_in1", p(x), p(w), p(b), out.ptr(), B, H, W, C)
    report("conv_in1", case, out=ratio(out.get(), S.conv_in1_ref(case), S.conv_in1_bound(case)))


@pytest.mark.parametrize("by_pointer", [False, True], ids=["bias", "bias_dev"])
@pytest.mark.parametrize("case", S.HEAD_CASES, ids=ids(S.HEAD_CASES))
def test_head(eng, case, by_pointer):
    C, (B, H, W) = case
    x64, coef64, w964, bias = S.head_operands(case)
    x, coef, w9 = inp(x64), inp(coef64), inp(w964)
    bias_dev = inp(torch.tensor([bias])) if by_pointer else None
    out = Out((B, H, W))
    # the value argument is ignored when the pointer is given: pass one that would show
    run(eng, "cddpm_op_head", p(x), p(coef), p(w9), 1000.0 if by_pointer else bias, p(bias_dev), out.ptr(), B, H, W, C)
    report("head", case, out=ratio(out.get(), S.head_ref(case), S.head_bound(case)))


@pytest.mark.parametrize("case", S.POOL_ACT_CASES, ids=ids(S.POOL_ACT_CASES))
def test_pool_act(eng, case):
    C, (B, H, W) = case
    x, coef = (inp(t) for t in S.pool_act_operands(case))
    hp, xp = Out((B, H // 2, W // 2, C)), Out((B, H // 2, W // 2, C))
    run(eng, "cddpm_op_pool_act", p(x), p(coef), hp.ptr(), xp.ptr(), B, H, W, C)
    ref, bound = S.pool_act_ref(case), S.pool_act_bound(case)
    report("pool_act", case, hp=ratio(hp.get(), ref[0], bound[0]), xp=ratio(xp.get(), ref[1], bound[1]))


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=ids(S.LINEAR_CASES))
def test_linear(eng, case):
    M, N, K, silu, bias = case
    x, w, b = (inp(t) for t in S.linear_operands(case))
    y = Out((M, N))
    run(eng, "cddpm_op_linear", p(x), p(w), p(b), M, N, K, silu, y.ptr())
    report("linear", case, y=ratio(y.get(), S.linear_ref(case), S.linear_bound(case)))


@pytest.mark.parametrize("K", S.LINEAR_REFUSED_K)
def test_linear_refuses_a_k_that_is_no_multiple_of_four(eng, K):
    M, N = 3, 5
    x, w, b = inp(torch.ones(M, K)), inp(torch.ones(N, K)), inp(torch.ones(N))
    y = Out((M, N))
    msg = refused(eng, "cddpm_op_linear", p(x), p(w), p(b), M, N, K, 0, y.ptr())
    assert "multiple of 4" in msg and y.untouched()


def test_small_forward_entries_refuse_what_their_kernels_cannot_compute(eng):
    """non-positive extents, a flat pixel range of 2^31, a head wider than a workgroup's LDS, unaligned rows: a message, no launch"""
    a, o = inp(torch.ones(4096)), Out((4096,))
    lib = eng.lib
    for B, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4)):
        refused(eng, "cddpm_op_conv_in1", p(a), p(a), p(a), o.ptr(), B, H, W, 64)
        refused(eng, "cddpm_op_head", p(a), p(a), p(a), 0.0, None, o.ptr(), B, H, W, 32)
        refused(eng, "cddpm_op_pool_act", p(a), p(a), o.ptr(), o.ptr(), B, H, W, 4)
        refused(eng, "cddpm_op_unpool2", p(a), o.ptr(), B, H, W, 4, 0.25, 0)
        refused(eng, "cddpm_op_sumpool2", p(a), o.ptr(), B, H, W, 4, 0)
        refused(eng, "cddpm_op_head_dgrad", p(a), p(a), o.ptr(), B, H, W, 4)
        refused(eng, "cddpm_op_chan_image_corr", p(a), None, 0, p(a), 1, o.ptr(), B, H, W, 64)
    assert "2^31" in refused(eng, "cddpm_op_conv_in1", p(a), p(a), p(a), o.ptr(), 2048, 1024, 1024, 64)
    refused(eng, "cddpm_op_conv_in1", p(a), p(a), p(a), o.ptr(), 1, 2, 2, 96)
    refused(eng, "cddpm_op_conv_in1", p(a), p(a), p(a), o.ptr(), 1, 2, 2, 576)
    # (64 (C + 4) + 9 C) 4 bytes of LDS: 544 channels fit the 160 KB of a gfx950 workgroup, 576 do not
    assert (64 * (544 + 4) + 9 * 544) * 4 <= 160 * 1024 < (64 * (576 + 4) + 9 * 576) * 4
    assert "544" in refused(eng, "cddpm_op_head", p(a), p(a), p(a), 0.0, None, o.ptr(), 1, 2, 2, 576)
    refused(eng, "cddpm_op_head", p(a), p(a), p(a), 0.0, None, o.ptr(), 1, 2, 2, 48)
    for M, N, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        refused(eng, "cddpm_op_linear", p(a), p(a), None, M, N, K, 0, o.ptr())
    assert "aligned" in refused(eng, "cddpm_op_linear", p(a) + 4, p(a), None, 2, 2, 8, 0, o.ptr())
    assert "aligned" in refused(eng, "cddpm_op_linear", p(a), p(a) + 8, None, 2, 2, 8, 0, o.ptr())
    assert o.untouched()


# ---------------------------------------------------------------------------------------------------------------- resampling, add
@pytest.mark.parametrize("case", S.RESAMPLE_CASES, ids=ids(S.RESAMPLE_CASES))
def test_unpool2_and_sumpool2(eng, case):
    B, H, W, C = case
    half64, full64 = S.resample_operands(case)
    half, full = inp(half64), inp(full64)
    r = {}
    for scale in S.UNPOOL_SCALES:
        out = Out((B, H, W, C))
        run(eng, "cddpm_op_unpool2", p(half), out.ptr(), B, H, W, C, scale, 0)
        assert torch.equal(out.get().float(), S.unpool2_f32(case, scale)), ("unpool2 is one rounded product", case, scale)
        acc = Out((B, H, W, C), init=full64)
        run(eng, "cddpm_op_unpool2", p(half), acc.ptr(), B, H, W, C, scale, 1)
        r[f"unpool2+={scale}"] = ratio(acc.get(), S.unpool2_ref(case, scale, True), S.unpool2_bound(case, scale))
    out = Out((B, H // 2, W // 2, C))
    run(eng, "cddpm_op_sumpool2", p(full), out.ptr(), B, H, W, C, 0)
    assert torch.equal(out.get().float(), S.sumpool2_f32(case)), ("sumpool2 adds (0,0), (0,1), (1,0), (1,1) in order from 0", case)
    acc = Out((B, H // 2, W // 2, C), init=half64)
    run(eng, "cddpm_op_sumpool2", p(full), acc.ptr(), B, H, W, C, 1)
    r["sumpool2+="] = ratio(acc.get(), S.sumpool2_ref(case, True), S.sumpool2_bound(case))
    report("resampling (plain forms: bit for bit)", case, **r)


@pytest.mark.parametrize("n", S.ADD_INPLACE_N)
def test_add_inplace(eng, n):
    a64, b64 = S.add_inplace_operands(n)
    a, b = Out((n,), init=a64), inp(b64)
    run(eng, "cddpm_op_add_inplace", a.ptr(), p(b), n)
    assert torch.equal(a.get().float(), a64.float() + b64.float()), n
    print(f"add_inplace {n}: bit for bit")


def test_add_inplace_refuses_a_length_that_is_no_multiple_of_four(eng):
    a, b = Out((6,), init=torch.ones(6)), inp(torch.ones(6))
    refused(eng, "cddpm_op_add_inplace", a.ptr(), p(b), 6)
    assert a.untouched()


# ---------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("case", S.BIAS_GRAD_CASES, ids=ids(S.BIAS_GRAD_CASES))
def test_bias_grad(eng, case):
    npix, C = case
    dy = inp(S.bias_grad_operands(case))
    db = Out((C,))
    run(eng, "cddpm_op_bias_grad", p(dy), npix, C, db.ptr())
    report("bias_grad", case, db=ratio(db.get(), S.bias_grad_ref(case), S.bias_grad_bound(case)))


@pytest.mark.parametrize("C", S.BIAS_GRAD_REFUSED_C)
def test_bias_grad_refuses_unsupported_channels(eng, C):
    dy, db = inp(torch.ones(8, C)), Out((C,))
    refused(eng, "cddpm_op_bias_grad", p(dy), 8, C, db.ptr())
    assert db.untouched()


@pytest.mark.parametrize("case", S.CORR_CASES, ids=ids(S.CORR_CASES))
def test_chan_image_corr(eng, case):
    sign, act, C, (B, H, W) = case
    T, coef, s = (inp(t) for t in S.corr_operands(case))
    dw = Out((C, 9))
    run(eng, "cddpm_op_chan_image_corr", p(T), p(coef), act, p(s), sign, dw.ptr(), B, H, W, C)
    report("chan_image_corr", case, dw=ratio(dw.get(), S.corr_ref(case), S.corr_bound(case)))


@pytest.mark.parametrize("case", S.HEAD_DGRAD_CASES, ids=ids(S.HEAD_DGRAD_CASES))
def test_head_dgrad(eng, case):
    C, (B, H, W) = case
    dout, w9 = (inp(t) for t in S.head_dgrad_operands(case))
    dact = Out((B, H, W, C))
    run(eng, "cddpm_op_head_dgrad", p(dout), p(w9), dact.ptr(), B, H, W, C)
    report("head_dgrad", case, dact=ratio(dact.get(), S.head_dgrad_ref(case), S.head_dgrad_bound(case)))


@pytest.mark.parametrize("case", S.LOSS_CASES, ids=ids(S.LOSS_CASES))
def test_loss(eng, case):
    l2, wb, HW, B, scale = case
    out, target, w = (inp(t) for t in S.loss_operands(case))
    dout, lb = Out((B, HW)), Out((B,))
    run(eng, "cddpm_op_loss", p(out), p(target), p(w), l2, B, HW, scale, dout.ptr(), lb.ptr())
    ref, bound = S.loss_ref(case), S.loss_bound(case)
    got = dout.get()
    zeros = S.loss_operands(case)[0] == S.loss_operands(case)[1]
    assert bool((got[zeros] == 0).all()), "the gradient where out == target is 0, as torch.sign gives"
    report("loss", case, dout=ratio(got, ref[0], bound[0]), loss_b=ratio(lb.get(), ref[1], bound[1]))


# ---------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("case", S.ADAM_CASES, ids=ids(S.ADAM_CASES))
def test_adam(eng, case):
    n, step, unscale = case
    p64, g64, m64, v64 = S.adam_operands(case)
    pp, m, v, g = Out((n,), init=p64), Out((n,), init=m64), Out((n,), init=v64), inp(g64)
    run(eng, "cddpm_op_adam", pp.ptr(), p(g), m.ptr(), v.ptr(), n, *S.ADAM_HYPER, step, unscale)
    ref, bound = S.adam_ref(case), S.adam_bound(case)
    report("adam", case, p=ratio(pp.get(), ref[0], bound[0]), m=ratio(m.get(), ref[1], bound[1]), v=ratio(v.get(), ref[2], bound[2]))


@pytest.mark.parametrize("step", [1, 1000, 100000])
def test_adam_update_next_to_double_hyperparameters_is_measured(eng, step):
    """Not asserted, reported: launch_adam forms 1 - beta^step in fp32 from fp32 betas, torch.optim.Adam from Python doubles
    (0.999, not fp32(0.999)). The update of a zero weight (so that it is read back to one rounding) on the [0.5, 2] gradients of the
    4099-vector, next to the float64 recurrence with the double hyper-parameters."""
    case = (4099, step, 1.0)
    p64, g64, m64, v64 = S.adam_operands(case)
    keep = (g64.abs() >= 0.5) & (g64.abs() <= 2.0)
    pp, m, v, g = Out((4099,), init=torch.zeros(4099)), Out((4099,), init=m64), Out((4099,), init=v64), inp(g64)
    run(eng, "cddpm_op_adam", pp.ptr(), p(g), m.ptr(), v.ptr(), 4099, *S.ADAM_HYPER, step, 1.0)
    got = pp.get()[keep]
    dev = {}
    for name, hyper in (("double", S.ADAM_HYPER), ("fp32", S.adam_hyper_abi())):
        upd = (S.adam_ref(case, hyper=hyper)[0] - p64)[keep]
        dev[name] = float(((got - upd) / upd).abs().max())
    print(f"adam step {step}: update next to float64 Adam with double hyper-parameters: max relative deviation {dev['double']:.3e} "
          f"(with the fp32 ones widened: {dev['fp32']:.3e})")


# ---------------------------------------------------------------------------------------------------------------- GroupNorm sweep
@pytest.mark.parametrize("case", S.GN_CASES, ids=ids(S.GN_CASES))
def test_gn_coef(eng, case):
    C0, C1, H, W, film, ratio_ = case
    x, gamma, beta, fl = S.gn_operands(case)
    src0 = inp(x[..., :C0].contiguous())
    src1 = inp(x[..., C0:].contiguous()) if C1 else None
    coef = eng.op_gn_coef(src0, src1, gamma.float(), beta.float(), inp(fl))
    torch.cuda.synchronize()
    coef = coef.cpu().double()
    assert not bool(torch.isnan(coef).any()), "a NaN in the coefficients: a read outside a source"
    err = float((S.gn_apply(case, coef) - S.gn_normalised(case)).abs().max())
    report("gn_coef", case, normalised=err / S.gn_bound(case))


# ---------------------------------------------------------------------------------------------------------------- linear backward
@pytest.mark.parametrize("with_db_dx", [True, False], ids=["db+dx", "dw-only"])
@pytest.mark.parametrize("case", S.LINBWD_CASES, ids=ids(S.LINBWD_CASES))
def test_linear_backward(eng, case, with_db_dx):
    M, N, K, silu = case
    x, w, dy = (inp(t) for t in S.linbwd_operands(case))
    dw, db, dx = Out((N, K)), Out((N,)), Out((M, K))
    run(eng, "cddpm_op_linear_backward", p(x), p(w), p(dy), M, N, K, silu, dw.ptr(), db.ptr() if with_db_dx else None,
        dx.ptr() if with_db_dx else None)
    ref, bound = S.linbwd_ref(case), S.linbwd_bound(case)
    r = {"dW": ratio(dw.get(), ref[0], bound[0])}
    if with_db_dx:
        r["db"], r["dx"] = ratio(db.get(), ref[1], bound[1]), ratio(dx.get(), ref[2], bound[2])
    else:
        assert db.untouched() and dx.untouched()
    report("linear_backward", case, **r)
