"""GPU: the operators of SparK masked pre-training (csrc/spark_train.hip behind cddpm_op_spark_* and cddpm_op_adamw_guarded) one call at a
time at the edges of their plans: the second trip of the cell count, chunked reductions with ragged, empty and capped chunks, channel counts
that leave the vector path and the 64-channel tile, uneven contraction splits, weight-gradient pixel ranges up to the cap, non-square masks,
NULL for every optional pointer. The cases are tests/spark_op_cases.py's; that they reach those plans and can show a wrong kernel is what
tests/test_spark_op_cases_host.py asserts on the CPU. References are float64 on the CPU; limits: 2e-5 of the result's maximum for BatchNorm
(badly conditioned cases: max(2e-5, 4 x torch fp32's own distance from float64)), 5e-6 for a convolution on random operands and nothing on
integer operands, 2e-6 for the loss and AdamW. Every test prints the restated plan and the measured errors.

Every output lies between two sentinel guard bands (tests/test_gpu_encoder_ops_edges.py's Banded), inputs are held between bands and compared
with what was passed afterwards; an output passed as NULL is simply absent; a refused call leaves its outputs as they were."""
import ctypes as C

import pytest
import torch

import spark_op_cases as S
from conftest import load_pkg
from test_gpu_encoder_ops_edges import Banded, held, nchw, nhwc, ok, p
from test_gpu_spark_ops import ops  # noqa: F401  (the module's fixture handle)

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.float().cuda().contiguous()


def unchanged(h, t, what):
    assert torch.equal(h.check(what), t.float().cpu() if t.is_cuda else t.float()), what + " was modified"


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def run_bn(ops, name):
    """forward and backward through the C ABI with exactly the optional pointers of the case -> {result: float64, NHWC / per channel}"""
    lib, h = ops.lib, ops.h
    c, o = S.BN_CASES[name], S.bn_operands(name)
    B, H, W, f, Cc = c["B"], c["H"], c["W"], c["f"], c["C"]
    N, band = B * H * W, 64 * Cc
    zg, dyg = held(dev(o["z"]), band), held(dev(o["dy"]), band)
    resg = held(dev(o["res"]), band) if c["res"] else None
    sg, fillg, gam, bet = dev(o["s"]), dev(o["fill"]), dev(o["gamma"]), dev(o["beta"])
    cells = o["active"].to(torch.uint8).cuda().contiguous() if c["sparse"] else None
    rm, rv = (held(dev(o["rm"]), 64), held(dev(o["rv"]), 64)) if (c["run"] or not c["training"]) else (None, None)
    mr, y = Banded((2, Cc), 64), Banded((B, H, W, Cc), band)
    ok(ops, lib.cddpm_op_spark_bn_forward(h, zg.ptr(), p(gam), p(bet), p(sg), resg and resg.ptr(), c["act"], C.c_float(S.EPS), C.c_float(S.MOM), rm and rm.ptr(),
                                          rv and rv.ptr(), mr.ptr(), y.ptr(), N, H * W, Cc, p(cells), f, H, W, p(fillg), c["training"], None))
    dz, dres = Banded((B, H, W, Cc), band), Banded((B, H, W, Cc), band) if c["dres"] else None
    dgam, dbet, dfill = Banded((Cc,), 64), Banded((Cc,), 64), Banded((Cc,), 64) if c["fill"] else None
    ok(ops, lib.cddpm_op_spark_bn_backward(h, zg.ptr(), None if c["y_null"] else y.ptr(), dyg.ptr(), mr.ptr(), p(gam), p(sg), c["act"], dz.ptr(), dres and dres.ptr(),
                                           dgam.ptr(), dbet.ptr(), N, H * W, Cc, p(cells), f, H, W, dfill and dfill.ptr(), c["training"], None))
    torch.cuda.synchronize()
    unchanged(zg, o["z"], name + " z"), unchanged(dyg, o["dy"], name + " dy")
    if resg:
        unchanged(resg, o["res"], name + " res")
    mrc = mr.check(name + " mean|rstd").double()
    got = dict(y=y.check(name + " y").double(), mean=mrc[0], rstd=mrc[1], dz=dz.check(name + " dz").double(), dgamma=dgam.check(name + " dgamma").double(),
               dbeta=dbet.check(name + " dbeta").double())
    if rm:
        got["run_mean"], got["run_var"] = rm.check(name + " running_mean").double(), rv.check(name + " running_var").double()
    if dres:
        got["dres"] = dres.check(name + " dres").double()
    if dfill:
        got["dfill"] = dfill.check(name + " dfill").double()
    return got


@pytest.mark.parametrize("name", list(S.BN_CASES))
def test_batchnorm_forward_and_backward(ops, name):
    """float64 from the definition, the activation's slope taken on the implementation's own y"""
    c, o, pl = S.BN_CASES[name], S.bn_operands(name), S.bn_plan(name)
    got = run_bn(ops, name)
    ref = S.bn_ref(name, y_impl=got["y"])
    limits = S.bn_limits(name, ref, y_impl=got["y"])
    assert set(got) == set(ref)
    e = {k: S.rel(got[k], ref[k]) for k in ref}
    print(name, {k: pl[k] for k in ("N", "cells", "chunks", "qpb", "rows", "yblocks")}, "trips", S.count_trips(pl["cells"]),
          {k: f"{e[k]:.1e}" + (f" (torch fp32 {limits[k][1]:.1e})" if limits[k][1] is not None else "") for k in ref})
    for k in ref:
        assert e[k] <= limits[k][0], (name, k, e[k], limits[k])
    on = S.cell_mask(o["active"], c["H"], c["W"]) if c["sparse"] else torch.ones(c["B"], c["H"], c["W"], dtype=torch.bool)
    assert bool((got["dz"][~on] == 0).all())                                    # exactly 0 at inactive pixels
    if not c["training"]:                                                        # evaluation leaves the running statistics alone
        assert torch.equal(got["run_mean"], o["rm"]) and torch.equal(got["run_var"], o["rv"])
    if c["ss"] and not c["res"]:
        assert float(got["y"][1].abs().max()) == 0.0                             # the dropped sample: fill * 0 as well
    if c["const"]:                                                               # the constant channels: variance 0, y = beta at the active pixels
        for ch_ in (1, 5):
            assert abs(float(got["rstd"][ch_]) - S.EPS ** -0.5) <= 1e-5 * S.EPS ** -0.5
            assert float((got["y"][..., ch_][on] - o["beta"][ch_]).abs().max()) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------- convolution family
def run_conv(ops, case, kind):
    """every role the case has, twice -> two {role: float64 in PyTorch layout}"""
    lib, h = ops.lib, ops.h
    Cin, Cout, K, tc, B, H, W, bias = case
    _, _, (Ho, Wo), wshape = S.conv_geom(case)
    x, w, b, dy = S.conv_operands(case, kind)
    band = 64 * max(Cin, Cout)
    xg, dyg, wg, bg = held(nhwc(x), band), held(nhwc(dy), band), held(dev(w), band), dev(b)
    runs = []
    for _ in range(2):
        y, dx, dw, db = Banded((B, Ho, Wo, Cout), band), Banded((B, H, W, Cin), band), Banded(wshape, band), Banded((Cout,), 64) if bias else None
        ok(ops, lib.cddpm_op_spark_conv(h, xg.ptr(), wg.ptr(), p(bg) if bias else None, y.ptr(), B, H, W, Cin, Cout, K, tc, 0, None))
        ok(ops, lib.cddpm_op_spark_conv(h, dyg.ptr(), wg.ptr(), None, dx.ptr(), B, H, W, Cin, Cout, K, tc, 1, None))
        ok(ops, lib.cddpm_op_spark_conv_wgrad(h, xg.ptr(), dyg.ptr(), dw.ptr(), db and db.ptr(), B, H, W, Cin, Cout, K, tc, None))
        torch.cuda.synchronize()
        what = S.conv_id(case) + " " + kind
        out = dict(y=nchw(y.check(what + " y")), dx=nchw(dx.check(what + " dx")), dw=dw.check(what + " dw").double())
        if bias:
            out["db"] = db.check(what + " db").double()
        runs.append(out)
    assert torch.equal(nchw(xg.check("x")), x) and torch.equal(nchw(dyg.check("dy")), dy) and torch.equal(wg.check("w").double(), w.float().double())
    return runs


@pytest.mark.parametrize("case", list(S.CONV_CASES), ids=S.conv_id)
def test_convolution_roles_on_random_operands(ops, case):
    a, b = run_conv(ops, case, "random")
    ref = S.conv_ref(case, "random")
    e = {r: S.rel(a[r], ref[r]) for r in ref}
    print(S.conv_id(case), S.CONV_CASES[case], S.conv_plan(case), {r: f"{v:.1e}" for r, v in e.items()})
    assert set(a) == set(ref)
    for r in ref:
        assert torch.equal(a[r], b[r]), (r, "two calls differ")
        assert e[r] <= S.CONV_LIMIT, (r, e[r])


@pytest.mark.parametrize("case", list(S.CONV_CASES), ids=S.conv_id)
def test_convolution_roles_are_exact_on_integer_operands(ops, case):
    """operands in -2..2: every partial sum is an integer below 2^24 (asserted on the host), exact in fp32 in any order -- a dropped, doubled
    or misplaced term is an integer difference with no tolerance to hide in"""
    assert S.integer_sum_bound(case) < 2 ** 24
    a, b = run_conv(ops, case, "integer")
    ref = S.conv_ref(case, "integer")
    print(S.conv_id(case), S.CONV_CASES[case], S.conv_plan(case), "largest |result|", {r: int(v.abs().max()) for r, v in ref.items()})
    for r in ref:
        bad = a[r] != ref[r]
        assert a[r].shape == ref[r].shape and not bool(bad.any()), (r, int(bad.sum()), "elements differ, first at", bad.nonzero()[0].tolist(), "by up to",
                                                                    float((a[r] - ref[r]).abs().max()))
        assert torch.equal(a[r], b[r]), (r, "two calls differ")


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("name", list(S.LOSS_CASES))
def test_loss(ops, name):
    lib, h = ops.lib, ops.h
    B, H, W, f, mask, (wm, wl), with_drec = S.LOSS_CASES[name]
    rec, inp, active = S.loss_operands(name)
    l_mask, l_l1, drec_ref = S.loss_ref(name)
    recg, inpg = held(dev(rec), 256), held(dev(inp), 256)
    cells = active.to(torch.uint8).cuda().contiguous()
    loss, drec = Banded((2,), 64), Banded((B, H, W), 256)
    call = lambda l, d: lib.cddpm_op_spark_loss(h, recg.ptr(), inpg.ptr(), p(cells), f, B, H, W, C.c_float(wm), C.c_float(wl), l.ptr(), d and d.ptr(), None)
    ok(ops, call(loss, drec if with_drec else None))
    torch.cuda.synchronize()
    got = loss.check(name + " loss")
    unchanged(recg, rec, "rec"), unchanged(inpg, inp, "inp")
    e_mask = abs(float(got[0]) - float(l_mask)) / max(float(l_mask), 1e-30)
    e_l1 = abs(float(got[1]) - float(l_l1)) / float(l_l1)
    pl = S.loss_plan(name)
    print(name, {k: pl[k] for k in ("total", "cells", "chunks")}, "trips", S.count_trips(pl["cells"]), f"masked {e_mask:.1e} l1 {e_l1:.1e}", end=" ")
    assert bool(torch.isfinite(got).all())
    if mask == "nothing_masked":
        assert float(got[0]) == 0.0 and float(l_mask) == 0.0
    else:
        assert e_mask <= S.LOSS_LIMIT
    assert e_l1 <= S.LOSS_LIMIT
    if with_drec:
        d = drec.check(name + " drec").double()
        print(f"drec {S.rel(d, drec_ref):.1e}")
        assert S.rel(d, drec_ref) <= S.LOSS_LIMIT
        assert bool((d[rec == inp] == 0).all())                                                            # sign(0) = 0, exactly
    else:                                                     # without a gradient: nothing written there, and the same scalars as with one
        drec.check(name + " drec of a call without one", written=False)
        loss2 = Banded((2,), 64)
        ok(ops, call(loss2, drec))
        torch.cuda.synchronize()
        assert torch.equal(loss2.check("loss"), got) and S.rel(drec.check("drec").double(), drec_ref) <= S.LOSS_LIMIT
        print()


# ---------------------------------------------------------------------------------------------------------------- mask multiply
@pytest.mark.parametrize("case", S.MASK_MUL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mask_multiply(ops, case):
    B, H, W, Cc, f = case
    x, active = S.mask_mul_operands(case)
    want = S.mask_mul_ref(case).float()
    xg, y = held(dev(x), 256), Banded((B, H, W, Cc), 256)
    cells = active.to(torch.uint8).cuda().contiguous()
    ok(ops, ops.lib.cddpm_op_spark_mask_mul(ops.h, xg.ptr(), p(cells), y.ptr(), B, H, W, Cc, f, None))
    torch.cuda.synchronize()
    unchanged(xg, x, "x")
    ok(ops, ops.lib.cddpm_op_spark_mask_mul(ops.h, xg.ptr(), p(cells), xg.ptr(), B, H, W, Cc, f, None))         # in place
    torch.cuda.synchronize()
    print(case, "cells", B * f * f, "trips", S.count_trips(B * f * f))
    assert torch.equal(y.check("mask_mul"), want) and torch.equal(xg.check("mask_mul in place"), want)


# ---------------------------------------------------------------------------------------------------------------- AdamW
def adam_steps(ops, case, op):
    """ADAM_STEPS guarded updates, then one with an inf in its gradient -> (p, m, v) before the skipped step, and after it, and ctrl"""
    lib, h = ops.lib, ops.h
    n, wd, unscale = case
    lr, (b1, b2), eps = S.ADAM_HYPER["lr"], S.ADAM_HYPER["betas"], S.ADAM_HYPER["eps"]
    p0, grads, bad = S.adam_operands(n)
    pg, m, v = held(dev(p0), 64), Banded((n,), 64), Banded((n,), 64)
    m.out.zero_(), v.out.zero_()
    ctrl = torch.zeros(8, dtype=torch.int32).cuda()

    def step(grad):
        gg = held(grad, 64)
        ok(ops, lib.cddpm_op_grad_check(h, gg.ptr(), n, p(ctrl), None))
        ok(ops, lib.cddpm_op_guard_commit(h, p(ctrl), C.c_float(b1), C.c_float(b2), None))
        tail = (C.c_float(wd), C.c_float(unscale)) if op == "adamw" else (C.c_float(unscale),)
        fn = lib.cddpm_op_adamw_guarded if op == "adamw" else lib.cddpm_op_adam_guarded
        ok(ops, fn(h, pg.ptr(), gg.ptr(), m.ptr(), v.ptr(), n, C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps), *tail, p(ctrl), None))
        torch.cuda.synchronize()
        assert torch.equal(gg.check("gradient"), grad.cpu())

    for t in range(S.ADAM_STEPS):
        step(dev(grads[t]))
    served = [b.check(k).clone() for b, k in ((pg, "p"), (m, "m"), (v, "v"))]
    step(dev(bad))
    after = [b.check(k).clone() for b, k in ((pg, "p"), (m, "m"), (v, "v"))]
    return served, after, ctrl.cpu().tolist()


@pytest.mark.parametrize("case", S.ADAM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_adamw(ops, case):
    """against torch.optim.AdamW's rule in float64 with grad_unscale = 0.5; a skipped step moves and decays nothing; weight_decay = 0 gives the
    bits of cddpm_op_adam_guarded"""
    n, wd, unscale = case
    served, after, ctrl = adam_steps(ops, case, "adamw")
    ref = S.adam_ref(case)
    e = [S.rel(g, r) for g, r in zip(served, ref)]
    print(case, "workgroups", (n + 255) // 256, "p %.1e m %.1e v %.1e" % tuple(e))
    assert max(e) <= S.ADAM_LIMIT
    for a, b in zip(served, after):
        assert torch.equal(a, b)
    assert ctrl[1:4] == [S.ADAM_STEPS, 1, 1]
    if wd == 0.0:
        plain, _, _ = adam_steps(ops, case, "adam")
        for a, b in zip(served, plain):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- what the ABI refuses
def test_refused_calls_leave_their_outputs_alone(ops):
    """a misaligned pointer, src = dst, an activation without y, f dividing H but not W, a negative weight decay: non-zero, a message that
    names the operator, nothing written"""
    lib, h = ops.lib, ops.h
    src = torch.zeros(1 << 16, device="cuda")
    cells = torch.ones(64, dtype=torch.uint8, device="cuda")
    s = src.data_ptr()
    eps, mom = C.c_float(S.EPS), C.c_float(S.MOM)

    def refused(name, call, *outs):
        assert lib.cddpm_op_spark_mask_mul(h, None, None, None, 1, 2, 2, 1, 1, None) != 0 and b"mask_mul" in lib.cddpm_last_error(h)     # another message first
        assert call(*[o.ptr() for o in outs]) != 0, name
        msg = lib.cddpm_last_error(h)
        assert msg.startswith(name.encode() + b":"), (name, msg)
        torch.cuda.synchronize()
        for o in outs:
            o.check(name, written=False)

    new = lambda: Banded((1 << 12,), 1 << 10)
    B, H, W, Cc = 2, 6, 6, 8
    N, HW = B * H * W, H * W
    fwd = lambda z, f, Wd: (lambda rm, rv, mr, y: lib.cddpm_op_spark_bn_forward(h, z, s, s, None, None, 1, eps, mom, rm, rv, mr, y, B * H * Wd, H * Wd, Cc, p(cells), f, H,
                                                                                Wd, None, 1, None))
    refused("cddpm_op_spark_bn_forward", fwd(s + 4, 3, W), new(), new(), new(), new())                       # z not 16-byte aligned
    refused("cddpm_op_spark_bn_forward", fwd(s, 3, 8), new(), new(), new(), new())                           # f = 3 divides H = 6, not W = 8
    refused("cddpm_op_spark_bn_forward", lambda rm, rv, mr, y: lib.cddpm_op_spark_bn_forward(h, s, s, s, None, None, 1, eps, mom, rm, rv, mr, y + 4, N, HW, Cc,
                                                                                             p(cells), 3, H, W, None, 1, None), new(), new(), new(), new())
    bwd = lambda z, y, f, Wd: (lambda dz, dg, db: lib.cddpm_op_spark_bn_backward(h, z, y, s, s, s, None, 1, dz, None, dg, db, B * H * Wd, H * Wd, Cc, p(cells), f, H, Wd,
                                                                                 None, 1, None))
    refused("cddpm_op_spark_bn_backward", bwd(s, None, 3, W), new(), new(), new())                            # act = 1 with y_dev = NULL
    refused("cddpm_op_spark_bn_backward", bwd(s + 4, s, 3, W), new(), new(), new())
    refused("cddpm_op_spark_bn_backward", bwd(s, s, 3, 8), new(), new(), new())
    conv = lambda a, Wd=W: (lambda o: lib.cddpm_op_spark_conv(h, a, s, None, o, B, H, Wd, 8, 4, 3, 0, 0, None))
    refused("cddpm_op_spark_conv", conv(s + 4), new())
    o = new()
    refused("cddpm_op_spark_conv", lambda dst: lib.cddpm_op_spark_conv(h, dst, s, None, dst, B, H, W, 8, 4, 3, 0, 0, None), o)      # src = dst
    refused("cddpm_op_spark_conv", lambda dst: lib.cddpm_op_spark_conv(h, s, s, None, dst + 4, B, H, W, 8, 4, 3, 0, 0, None), new())
    refused("cddpm_op_spark_conv_wgrad", lambda dw: lib.cddpm_op_spark_conv_wgrad(h, s + 4, s, dw, None, B, H, W, 8, 4, 3, 0, None), new())
    refused("cddpm_op_spark_conv_wgrad", lambda dw: lib.cddpm_op_spark_conv_wgrad(h, s, s + 8, dw, None, B, H, W, 8, 4, 3, 0, None), new())
    refused("cddpm_op_spark_mask_mul", lambda y: lib.cddpm_op_spark_mask_mul(h, s, p(cells), y, B, H, 8, Cc, 3, None), new())
    refused("cddpm_op_spark_loss", lambda l, d: lib.cddpm_op_spark_loss(h, s, s, p(cells), 3, B, H, 8, C.c_float(1.0), C.c_float(0.0), l, d, None), new(), new())
    ctrl = torch.zeros(8, dtype=torch.int32, device="cuda")
    refused("cddpm_op_adamw_guarded", lambda pp, m, v: lib.cddpm_op_adamw_guarded(h, pp, s, m, v, 64, C.c_float(1e-2), C.c_float(0.9), C.c_float(0.95), C.c_float(1e-8),
                                                                                  C.c_float(-0.05), C.c_float(1.0), p(ctrl), None), new(), new(), new())
    assert not bool(src.any()) and not bool(ctrl.any())


# ---------------------------------------------------------------------------------------------------------------- the arena without slack
FILL = -7.0


@pytest.fixture()
def eng():
    e = load_pkg("engine").CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16)       # a fresh handle: only its arena is used
    yield e
    e.close()


def both_sides(eng, q, call, outputs):
    """tests/test_gpu_operator_scratch.py's rule for the five SparK size queries: an arena of exactly q bytes serves the call; with 256 bytes
    less (where that still is an arena) it is refused with the arena message before anything is launched"""
    lib, h = eng.lib, eng._h
    assert q > 0 and q % 256 == 0
    if q > 256:
        assert lib.cddpm_op_set_scratch(h, q - 256) == 0
        assert call() != 0
        msg = lib.cddpm_last_error(h).decode()
        assert f"operator scratch: {q} bytes needed, arena holds {q - 256}" in msg, msg
        torch.cuda.synchronize()
        for o in outputs:
            assert bool((o == FILL).all()), "a refused call wrote to an output"
    assert lib.cddpm_op_set_scratch(h, q) == 0
    assert call() == 0, lib.cddpm_last_error(h).decode()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool(torch.isfinite(o).all()) and not bool((o == FILL).any())


def test_an_arena_of_exactly_the_queried_size_serves_the_call(eng):
    lib, h = eng.lib, eng._h
    q = load_pkg("_lib").scratch_query
    out = lambda *shape: torch.full(shape, FILL, device="cuda")
    g = torch.Generator().manual_seed(3)
    rnd = lambda *shape: torch.randn(*shape, generator=g).cuda()
    # BatchNorm: N = 3 x 33 x 45, C = 40: 10 chunks
    B, H, W, Cc = 3, 33, 45, 40
    N = B * H * W
    z, dy, gam, bet = rnd(B, H, W, Cc), rnd(B, H, W, Cc), rnd(Cc), rnd(Cc)
    mr, y = out(2, Cc), out(B, H, W, Cc)
    both_sides(eng, q("spark_bn_forward", N, H * W, Cc),
               lambda: lib.cddpm_op_spark_bn_forward(h, p(z), p(gam), p(bet), None, None, 1, C.c_float(S.EPS), C.c_float(S.MOM), None, None, p(mr), p(y), N, H * W, Cc,
                                                     None, 1, H, W, None, 1, None), [mr, y])
    dz, dg, db = out(B, H, W, Cc), out(Cc), out(Cc)
    both_sides(eng, q("spark_bn_backward", N, H * W, Cc),
               lambda: lib.cddpm_op_spark_bn_backward(h, p(z), p(y), p(dy), p(mr), p(gam), None, 1, p(dz), None, p(dg), p(db), N, H * W, Cc, None, 1, H, W, None, 1, None),
               [dz, dg, db])
    # convolution: 72 -> 72, 3x3 at 30 pixels: Z = 4 planes; its weight gradient; a bias gradient of 2 chunks
    B, H, W, Cin, Cout = 2, 3, 5, 72, 72
    x, w, dyc = rnd(B, H, W, Cin), rnd(Cout, Cin, 3, 3), rnd(B, H, W, Cout)
    yc, dw = out(B, H, W, Cout), out(Cout, Cin, 3, 3)
    assert S.conv_split(B * H * W, Cout, Cin, 3)[0] == 4
    both_sides(eng, q("spark_conv", B, H, W, Cin, Cout, 3, 0, 0), lambda: lib.cddpm_op_spark_conv(h, p(x), p(w), None, p(yc), B, H, W, Cin, Cout, 3, 0, 0, None), [yc])
    both_sides(eng, q("spark_conv_wgrad", B, H, W, Cin, Cout, 3, 0, 0),
               lambda: lib.cddpm_op_spark_conv_wgrad(h, p(x), p(dyc), p(dw), None, B, H, W, Cin, Cout, 3, 0, None), [dw])
    B, H, W, Cin, Cout = 3, 15, 17, 4, 24
    x, dyc, dw, dbias = rnd(B, H, W, Cin), rnd(B, H, W, Cout), out(Cout, Cin, 1, 1), out(Cout)
    both_sides(eng, q("spark_conv_wgrad", B, H, W, Cin, Cout, 1, 0, 1),
               lambda: lib.cddpm_op_spark_conv_wgrad(h, p(x), p(dyc), p(dw), p(dbias), B, H, W, Cin, Cout, 1, 0, None), [dw, dbias])
    # loss: 1 x 1026 x 1026: 256 chunks
    B, H, W, f = 1, 1026, 1026, 2
    rec, inp, cells = rnd(B, H, W), rnd(B, H, W), torch.tensor([1, 0, 0, 1], dtype=torch.uint8).cuda()
    loss, drec = out(2), out(B, H, W)
    both_sides(eng, q("spark_loss", B, H, W, f),
               lambda: lib.cddpm_op_spark_loss(h, p(rec), p(inp), p(cells), f, B, H, W, C.c_float(1.0), C.c_float(0.5), p(loss), p(drec), None), [loss, drec])
