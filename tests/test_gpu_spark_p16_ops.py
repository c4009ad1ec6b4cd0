"""GPU: the two operators precision-16 SparK pre-training adds to the C ABI (include/cddpm.h, "Under Dynamic loss scaling"), one call at a
time against the calls they are defined by -- no tolerance, the contract is bit identity:

  cddpm_op_spark_loss_scaled  at device scale S == cddpm_op_spark_loss with weights S w_mask, S w_l1 (terms and drec);
  cddpm_op_adamw_scaled       at device scale S == cddpm_op_adamw_guarded with grad_unscale = extra_unscale / S (p, m, v).

S is a power of two and the operands are N(0, 1) / U(0, 1): S w and extra_unscale / S are exact in fp32 and nothing under- or overflows
(2^24 x a loss gradient of at most 2 / 1 is far from 3.4e38). Outputs lie between sentinel guard bands; refused calls write nothing."""
import ctypes as C

import pytest
import torch

from conftest import load_pkg
from test_gpu_encoder_ops_edges import Banded, held, ok, p

pytestmark = pytest.mark.gpu

LOSS_SHAPES = [(2, 64, 2), (3, 96, 3), (1, 32, 1)]          # (B, H = W, f): 2 / 6 / 1 chunks of 4096 pixels, 8 / 27 / 1 cells
WEIGHTS = [(1.0, 0.0), (0.5, 1.0)]
SCALES = [2.0 ** 0, 2.0 ** 16, 2.0 ** 24]


@pytest.fixture(scope="module")
def ops():
    o = load_pkg("training").UNetTrainer({"w": torch.zeros(64)}, device=torch.device("cuda", 0))
    o._fit(4, 64, 64)
    yield o
    o.close()


def scaler_block(scale, tracker=0, skips=0):
    return load_pkg("training")._scaler_block(scale, tracker, skips, torch.device("cuda", 0))


def loss_operands(B, H, f):
    g = torch.Generator().manual_seed(100 * B + H + f)
    rec, inp = torch.randn(B, H, H, generator=g), torch.rand(B, H, H, generator=g)
    rec[0, 1, :5] = inp[0, 1, :5]                                     # sign(0) = 0 at any scale
    active = torch.rand(B, f * f, generator=g) < 0.35
    active[0, 0] = False                                              # something is masked
    return rec, inp, active.view(B, f, f).to(torch.uint8)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("weights", WEIGHTS, ids=lambda w: f"w{w[0]:g}-{w[1]:g}")
def test_loss_scaled_is_the_plain_loss_at_scaled_weights(ops, shape, weights):
    lib, h = ops.lib, ops.h
    B, H, f = shape
    wm, wl = weights
    rec, inp, active = loss_operands(B, H, f)
    recg, inpg, cells = held(rec.cuda(), 256), held(inp.cuda(), 256), active.cuda().contiguous()
    for S in SCALES:
        blk = scaler_block(S, tracker=5, skips=2)
        blk0 = blk.clone()
        want_l, want_d, got_l, got_d, got_l2 = Banded((2,), 64), Banded((B, H, H), 256), Banded((2,), 64), Banded((B, H, H), 256), Banded((2,), 64)
        ok(ops, lib.cddpm_op_spark_loss(h, recg.ptr(), inpg.ptr(), p(cells), f, B, H, H, C.c_float(S * wm), C.c_float(S * wl), want_l.ptr(), want_d.ptr(), None))
        ok(ops, lib.cddpm_op_spark_loss_scaled(h, recg.ptr(), inpg.ptr(), p(cells), f, B, H, H, C.c_float(wm), C.c_float(wl), p(blk), got_l.ptr(), got_d.ptr(), None))
        ok(ops, lib.cddpm_op_spark_loss_scaled(h, recg.ptr(), inpg.ptr(), p(cells), f, B, H, H, C.c_float(wm), C.c_float(wl), p(blk), got_l2.ptr(), None, None))
        torch.cuda.synchronize()
        wl_, wd_, gl_, gd_ = want_l.check("loss"), want_d.check("drec"), got_l.check("scaled loss"), got_d.check("scaled drec")
        assert torch.equal(gl_.view(torch.int32), wl_.view(torch.int32)), (S, gl_, wl_)
        assert torch.equal(gd_.view(torch.int32), wd_.view(torch.int32)), (S, float((gd_ - wd_).abs().max()))
        assert torch.equal(got_l2.check("scaled loss without drec").view(torch.int32), wl_.view(torch.int32))      # drec_dev NULL works
        assert bool(torch.isfinite(gd_).all()) and bool(gd_.any()) and torch.equal(blk, blk0)                          # the block is only read
        # the terms do not carry the scale: they are those of the unscaled call
        plain = Banded((2,), 64)
        ok(ops, lib.cddpm_op_spark_loss(h, recg.ptr(), inpg.ptr(), p(cells), f, B, H, H, C.c_float(wm), C.c_float(wl), plain.ptr(), None, None))
        torch.cuda.synchronize()
        assert torch.equal(plain.check("plain loss").view(torch.int32), gl_.view(torch.int32))
    assert torch.equal(recg.check("rec"), rec) and torch.equal(inpg.check("inp"), inp)


def test_loss_scaled_refuses_a_null_scaler(ops):
    lib, h = ops.lib, ops.h
    B, H, f = 2, 64, 2
    rec, inp, active = loss_operands(B, H, f)
    recg, inpg, cells = rec.cuda(), inp.cuda(), active.cuda().contiguous()
    loss, drec = Banded((2,), 64), Banded((B, H, H), 256)
    assert lib.cddpm_op_spark_mask_mul(h, None, None, None, 1, 2, 2, 1, 1, None) != 0                     # another message first
    assert lib.cddpm_op_spark_loss_scaled(h, p(recg), p(inpg), p(cells), f, B, H, H, C.c_float(1.0), C.c_float(0.0), None, loss.ptr(), drec.ptr(), None) != 0
    assert lib.cddpm_last_error(h).startswith(b"cddpm_op_spark_loss_scaled:")
    blk = scaler_block(2.0)
    assert lib.cddpm_op_spark_loss_scaled(h, p(recg), p(inpg), p(cells), 3, B, H, H, C.c_float(1.0), C.c_float(0.0), p(blk), loss.ptr(), drec.ptr(), None) != 0
    assert b"unsupported shape" in lib.cddpm_last_error(h)                                                 # f = 3 does not divide 64
    torch.cuda.synchronize()
    loss.check("loss", written=False), drec.check("drec", written=False)


# ---------------------------------------------------------------------------------------------------------------- AdamW
HYPER = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
S16 = 2.0 ** 16


def adamw_run(ops, n, wd, extra, scaled, grads):
    """len(grads) updates through the guard -> (p, m, v) on the host, ctrl"""
    lib, h = ops.lib, ops.h
    g = torch.Generator().manual_seed(n)
    pg, m, v = held(torch.randn(n, generator=g).cuda(), 64), Banded((n,), 64), Banded((n,), 64)
    m.out.zero_(), v.out.zero_()
    ctrl, blk = torch.zeros(8, dtype=torch.int32, device="cuda"), scaler_block(S16)
    lr, (b1, b2), eps = HYPER["lr"], HYPER["betas"], HYPER["eps"]
    for grad in grads:
        gg = held(grad.cuda(), 64)
        ok(ops, lib.cddpm_op_grad_check(h, gg.ptr(), n, p(ctrl), None))
        ok(ops, lib.cddpm_op_guard_commit(h, p(ctrl), C.c_float(b1), C.c_float(b2), None))
        head = (h, pg.ptr(), gg.ptr(), m.ptr(), v.ptr(), n, C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps), C.c_float(wd))
        if scaled:
            ok(ops, lib.cddpm_op_adamw_scaled(*head, C.c_float(extra), p(ctrl), p(blk), None))
        else:
            ok(ops, lib.cddpm_op_adamw_guarded(*head, C.c_float(extra / S16), p(ctrl), None))
        torch.cuda.synchronize()
        assert torch.equal(gg.check("gradient"), grad)
    assert torch.equal(blk.cpu(), scaler_block(S16).cpu())                                                  # the update only reads the scale
    return [b.check(k).clone() for b, k in ((pg, "p"), (m, "m"), (v, "v"))], ctrl.cpu().tolist()


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
@pytest.mark.parametrize("wd", [0.05, 0.0])
@pytest.mark.parametrize("extra", [1.0, 0.5])
def test_adamw_scaled_is_adamw_guarded_at_the_unscale(ops, n, wd, extra):
    """two clean updates on gradients that carry the scale, then one with an inf: bit for bit the guarded form's; the skipped one moves nothing"""
    g = torch.Generator().manual_seed(7 * n + 1)
    grads = [S16 * torch.randn(n, generator=g) for _ in range(2)]
    got, ctrl = adamw_run(ops, n, wd, extra, True, grads)
    want, _ = adamw_run(ops, n, wd, extra, False, grads)
    for a, b, k in zip(got, want, "pmv"):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, float((a - b).abs().max()))
    assert ctrl[1:4] == [2, 0, 0] and bool(got[1].any()) and bool(torch.isfinite(torch.stack(got)).all())
    # the moments are those of the UNSCALED gradient: |m| after two steps is far below the scale
    assert float(got[1].abs().max()) < 1.0
    bad = grads[0].clone()
    bad[n // 2] = float("inf")
    after, ctrl = adamw_run(ops, n, wd, extra, True, grads + [bad])
    for a, b in zip(after, got):
        assert torch.equal(a, b)                                                                            # with the skip flag set nothing moves
    assert ctrl[1:4] == [2, 1, 1]


def test_adamw_scaled_refuses_a_null_scaler_and_a_negative_decay(ops):
    lib, h = ops.lib, ops.h
    n = 64
    src, ctrl, blk = torch.zeros(n, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), scaler_block(S16)
    for wd, scaler in ((0.05, None), (-0.05, blk)):
        pp, m, v = Banded((n,), 64), Banded((n,), 64), Banded((n,), 64)
        assert lib.cddpm_op_spark_mask_mul(h, None, None, None, 1, 2, 2, 1, 1, None) != 0
        assert lib.cddpm_op_adamw_scaled(h, pp.ptr(), p(src), m.ptr(), v.ptr(), n, C.c_float(1e-2), C.c_float(0.9), C.c_float(0.95), C.c_float(1e-8), C.c_float(wd),
                                         C.c_float(1.0), p(ctrl), p(scaler), None) != 0
        assert lib.cddpm_last_error(h).startswith(b"cddpm_op_adamw_scaled:")
        torch.cuda.synchronize()
        for o in (pp, m, v):
            o.check("adamw_scaled", written=False)


# ---------------------------------------------------------------------------------------------------------------- the arena without slack
FILL = -7.0


def test_an_arena_of_exactly_the_queried_size_serves_the_new_calls():
    """cddpm_op_spark_loss_scaled takes what cddpm_op_spark_loss_scratch says (18 chunks at 2 x 192 x 192: two fp64 partial sums each, 512
    bytes): served by exactly that, refused with 256 bytes less before anything is launched. cddpm_op_adamw_scaled has no size query: it
    takes nothing from the arena and runs on the same handle."""
    eng = load_pkg("engine").CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16)          # a fresh handle: only its arena is used
    try:
        lib, h = eng.lib, eng._h
        B, H, f = 2, 192, 6
        q = load_pkg("_lib").scratch_query("spark_loss", B, H, H, f)
        assert q > 256 and q % 256 == 0
        rec, inp, active = loss_operands(B, H, f)
        recg, inpg, cells, blk = rec.cuda(), inp.cuda(), active.cuda().contiguous(), scaler_block(S16)
        loss, drec = torch.full((2,), FILL, device="cuda"), torch.full((B, H, H), FILL, device="cuda")
        call = lambda: lib.cddpm_op_spark_loss_scaled(h, p(recg), p(inpg), p(cells), f, B, H, H, C.c_float(0.5), C.c_float(1.0), p(blk), p(loss), p(drec), None)
        assert lib.cddpm_op_set_scratch(h, q - 256) == 0
        assert call() != 0
        msg = lib.cddpm_last_error(h).decode()
        assert f"operator scratch: {q} bytes needed, arena holds {q - 256}" in msg, msg
        torch.cuda.synchronize()
        assert bool((loss == FILL).all()) and bool((drec == FILL).all())
        assert lib.cddpm_op_set_scratch(h, q) == 0
        assert call() == 0, lib.cddpm_last_error(h).decode()
        n = 257
        pp, g, m, v = torch.ones(n, device="cuda"), torch.full((n,), S16, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        ctrl = torch.zeros(8, dtype=torch.int32, device="cuda")
        assert lib.cddpm_op_grad_check(h, p(g), n, p(ctrl), None) == 0 and lib.cddpm_op_guard_commit(h, p(ctrl), C.c_float(0.9), C.c_float(0.95), None) == 0
        assert lib.cddpm_op_adamw_scaled(h, p(pp), p(g), p(m), p(v), n, C.c_float(1e-2), C.c_float(0.9), C.c_float(0.95), C.c_float(1e-8), C.c_float(0.05), C.c_float(1.0),
                                         p(ctrl), p(blk), None) == 0, lib.cddpm_last_error(h).decode()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(drec).all()) and not bool((drec == FILL).any())
        # the first AdamW step from zero moments at unscaled gradient 1: m = 0.1, p = 1 (1 - lr wd) - lr to fp32 rounding
        assert torch.allclose(m, torch.full_like(m, 0.1), rtol=1e-6) and torch.allclose(pp, torch.full_like(pp, 1.0 * (1 - 1e-2 * 0.05) - 1e-2), rtol=1e-5)
    finally:
        eng.close()
