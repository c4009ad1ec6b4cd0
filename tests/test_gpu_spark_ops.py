"""GPU: the operators of SparK masked pre-training (csrc/spark_train.hip behind cddpm_op_spark_* and cddpm_op_adamw_guarded) one call at a
time against float64 torch on the host: the sparse / dense BatchNorm with fill value and ReLU6, the mask multiply, the small-channel
convolution family (Conv2d 1x1 / 3x3 and ConvTranspose2d 4/2/1: forward, input gradient, weight and bias gradient), the masked loss and
the decoupled-decay Adam update.

Limits are those of tests/test_gpu_encoder_ops.py for the same arithmetic (fp32 elementwise work over fp64 sums; fp32 FMA contractions):
2e-5 of the result's maximum for BatchNorm, 5e-6 for a convolution. The loss scalars are fp64 sums of fp32 differences: 2e-6 relative.
Every output lies between sentinel guard bands (tests/test_gpu_encoder_ops_edges.py's Banded)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg
from test_gpu_encoder_ops_edges import Banded, held, nchw, nhwc, ok, p

pytestmark = pytest.mark.gpu

BN_LIMIT, CONV_LIMIT, LOSS_LIMIT = 2e-5, 5e-6, 2e-6
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def ops():
    tr = load_pkg("training")
    o = tr.UNetTrainer({"w": torch.zeros(64)}, device=torch.device("cuda", 0))
    o._fit(4, 64, 64)
    return o


def close(got, want, limit, what):
    scale = float(want.abs().max())
    err = float((got.double() - want.double()).abs().max())
    print(f"{what}: max error {err:.3e} against a maximum of {scale:.3e} (limit {limit:g} of it)")
    assert err <= limit * max(scale, 1e-30), what


def dilate(active, H, W):
    """bool [B, f, f] -> bool [B, 1, H, W]: the mask at a tensor's resolution (spark/encoder.py:13-16)"""
    f = active.shape[-1]
    return active.repeat_interleave(H // f, 1).repeat_interleave(W // f, 2).unsqueeze(1)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def bn_reference(z, gamma, beta, mask, fill, s, res, act, training, rm, rv):
    """float64: y = act((active ? bn(z) : fill) s_b + res) with BatchNorm1d over the active pixels (sp_bn_forward); -> y, new running stats"""
    B, Cc, H, W = z.shape
    rows = z.permute(0, 2, 3, 1)[mask[:, 0]]
    n = rows.shape[0]
    if training:
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        new_rm, new_rv = (1 - MOM) * rm + MOM * mean.detach(), (1 - MOM) * rv + MOM * var.detach() * n / (n - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    v = (z - mean.view(1, Cc, 1, 1)) / torch.sqrt(var.view(1, Cc, 1, 1) + EPS) * gamma.view(1, Cc, 1, 1) + beta.view(1, Cc, 1, 1)
    v = torch.where(mask, v, fill.view(1, Cc, 1, 1).expand_as(v))
    v = v * s.view(B, 1, 1, 1) + res
    y = F.relu(v) if act == 1 else F.relu6(v) if act == 2 else v
    return y, new_rm, new_rv


BN_CASES = {
    # name: (B, H, W, f, C, active cells per sample or None (dense), act, fill, res and s_b, training)
    "sparse_unequal_relu_res": (2, 8, 8, 2, 64, (3, 1), 1, False, True, 1),
    "sparse_one_cell_each_2048_fill": (3, 3, 3, 3, 2048, (1, 1, 1), 0, True, False, 1),
    "dense_relu6": (2, 16, 16, 1, 4, None, 2, False, False, 1),
    "sparse_relu6_fill_res_8": (2, 12, 12, 3, 8, (4, 2), 2, True, True, 1),
    "sparse_eval": (2, 8, 8, 2, 64, (3, 1), 1, False, True, 0),
    "dense_eval_fill_ignored": (2, 6, 6, 1, 12, None, 0, False, False, 0),
}


def bn_operands(name):
    B, H, W, f, Cc, cells, act, has_fill, has_res, training = BN_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z = r(B, Cc, H, W) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * r(Cc), 0.1 * r(Cc)
    if act == 2:
        gamma, beta = gamma * 3.0, beta + 3.0          # outputs straddle both 0 and 6
    if cells is None:
        active = None
        mask = torch.ones(B, 1, H, W, dtype=torch.bool)
    else:
        active = torch.zeros(B, f * f, dtype=torch.bool)
        for b, k in enumerate(cells):
            active[b, torch.randperm(f * f, generator=g)[:k]] = True
        active = active.view(B, f, f)
        mask = dilate(active, H, W)
    fill = 0.5 * r(Cc) if has_fill else torch.zeros(Cc, dtype=torch.float64)
    s = (torch.tensor([1.25, 0.0, 1.0][:B], dtype=torch.float64) if has_res else torch.ones(B, dtype=torch.float64))
    res = r(B, Cc, H, W) * (2.0 if act == 2 else 1.0) if has_res else torch.zeros(B, Cc, H, W, dtype=torch.float64)
    rm, rv = 0.2 * r(Cc), 0.5 + torch.rand(Cc, generator=g, dtype=torch.float64)
    dy = r(B, Cc, H, W)
    return dict(z=z, gamma=gamma, beta=beta, active=active, mask=mask, fill=fill, s=s, res=res, rm=rm, rv=rv, dy=dy, act=act, training=training,
                has_fill=has_fill, has_res=has_res, dims=(B, H, W, f, Cc))


@pytest.mark.parametrize("name", list(BN_CASES))
def test_batchnorm_forward_and_backward(ops, name):
    lib, h = ops.lib, ops.h
    o = bn_operands(name)
    B, H, W, f, Cc = o["dims"]
    leaves = {k: o[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta", "fill", "res")}
    y_ref, rm_ref, rv_ref = bn_reference(leaves["z"], leaves["gamma"], leaves["beta"], o["mask"], leaves["fill"], o["s"], leaves["res"], o["act"],
                                         o["training"], o["rm"], o["rv"])
    y_ref.backward(o["dy"])

    dev = lambda t: t.float().cuda().contiguous()
    band = 64 * Cc
    zg, dyg = held(nhwc(o["z"]), band), held(nhwc(o["dy"]), band)
    resg = held(nhwc(o["res"]), band) if o["has_res"] else None
    sg = dev(o["s"]) if o["has_res"] else None
    fillg = dev(o["fill"]) if o["has_fill"] else None
    act_g = None if o["active"] is None else o["active"].to(torch.uint8).cuda().contiguous()
    gam, bet, rm, rv = dev(o["gamma"]), dev(o["beta"]), dev(o["rm"]), dev(o["rv"])
    mr, y = Banded((2, Cc), 64), Banded((B, H, W, Cc), band)
    N = B * H * W
    ok(ops, lib.cddpm_op_spark_bn_forward(h, zg.ptr(), p(gam), p(bet), p(sg), None if resg is None else resg.ptr(), o["act"], C.c_float(EPS),
                                          C.c_float(MOM), p(rm), p(rv), mr.ptr(), y.ptr(), N, H * W, Cc, p(act_g), f, H, W, p(fillg), o["training"], None))
    dz, dres = Banded((B, H, W, Cc), band), Banded((B, H, W, Cc), band)
    dgam, dbet, dfill = Banded((Cc,), 64), Banded((Cc,), 64), Banded((Cc,), 64)
    ok(ops, lib.cddpm_op_spark_bn_backward(h, zg.ptr(), y.ptr(), dyg.ptr(), mr.ptr(), p(gam), p(sg), o["act"], dz.ptr(), dres.ptr(), dgam.ptr(),
                                           dbet.ptr(), N, H * W, Cc, p(act_g), f, H, W, dfill.ptr(), o["training"], None))
    torch.cuda.synchronize()
    close(nchw(y.check(name + " y")), y_ref.detach(), BN_LIMIT, name + " y")
    close(rm.cpu(), rm_ref, BN_LIMIT, name + " running_mean")
    close(rv.cpu(), rv_ref, BN_LIMIT, name + " running_var")
    if not o["training"]:
        assert torch.equal(rm.cpu(), o["rm"].float()) and torch.equal(rv.cpu(), o["rv"].float())      # evaluation leaves them alone
    dz_ref = leaves["z"].grad
    close(nchw(dz.check(name + " dz")), dz_ref, BN_LIMIT, name + " dz")
    assert bool((nchw(dz.out.cpu())[~o["mask"].expand_as(dz_ref)] == 0).all())                           # exactly 0 at inactive pixels
    close(nchw(dres.check(name + " dres")), leaves["res"].grad, BN_LIMIT, name + " dres")
    close(dgam.check(name + " dgamma"), leaves["gamma"].grad, BN_LIMIT, name + " dgamma")
    close(dbet.check(name + " dbeta"), leaves["beta"].grad, BN_LIMIT, name + " dbeta")
    dfill_ref = leaves["fill"].grad
    got = dfill.check(name + " dfill")
    if float(dfill_ref.abs().max()) > 0:
        close(got, dfill_ref, BN_LIMIT, name + " dfill")
    else:
        assert bool((got == 0).all())


def test_batchnorm_refuses_one_active_pixel(ops):
    """torch's BatchNorm1d raises on one row in training mode; so does the operator, before anything is written"""
    lib, h = ops.lib, ops.h
    Cc = 8
    z = held(torch.randn(1, 2, 2, Cc).cuda(), 64)
    active = torch.tensor([[[0, 1], [0, 0]]], dtype=torch.uint8).cuda()
    gam, bet = torch.ones(Cc).cuda(), torch.zeros(Cc).cuda()
    rm, rv = torch.full((Cc,), 0.25).cuda(), torch.full((Cc,), 2.0).cuda()
    mr, y = Banded((2, Cc), 64), Banded((1, 2, 2, Cc), 64)
    args = lambda act_ptr, f, training: (h, z.ptr(), p(gam), p(bet), None, None, 0, C.c_float(EPS), C.c_float(MOM), p(rm), p(rv), mr.ptr(), y.ptr(), 4, 4, Cc,
                                         act_ptr, f, 2, 2, None, training, None)
    assert lib.cddpm_op_spark_bn_forward(*args(p(active), 2, 1)) != 0
    msg = lib.cddpm_last_error(h).decode()
    assert "1 active pixel" in msg and "BatchNorm1d" in msg, msg
    torch.cuda.synchronize()
    y.check("refused y", written=False)
    assert bool((rm == 0.25).all()) and bool((rv == 2.0).all())
    ok(ops, lib.cddpm_op_spark_bn_forward(*args(p(active), 2, 0)))               # the same call in evaluation mode is served
    # a dense call over one pixel is refused on the host
    assert lib.cddpm_op_spark_bn_forward(h, z.ptr(), p(gam), p(bet), None, None, 0, C.c_float(EPS), C.c_float(MOM), p(rm), p(rv), mr.ptr(), y.ptr(), 1, 1, Cc,
                                         None, 1, 1, 1, None, 1, None) != 0
    # C = 6 is no multiple of 4; f = 3 does not divide 2
    assert lib.cddpm_op_spark_bn_forward(h, z.ptr(), p(gam), p(bet), None, None, 0, C.c_float(EPS), C.c_float(MOM), p(rm), p(rv), mr.ptr(), y.ptr(), 4, 4, 6,
                                         None, 1, 2, 2, None, 1, None) != 0
    assert lib.cddpm_op_spark_bn_forward(*args(p(active), 3, 1)) != 0


# ---------------------------------------------------------------------------------------------------------------- mask multiply
@pytest.mark.parametrize("dims", [(3, 64, 64, 1, 2), (2, 24, 24, 64, 3), (1, 6, 9, 5, 3)])
def test_mask_multiply(ops, dims):
    B, H, W, Cc, f = dims
    g = torch.Generator().manual_seed(B * H + Cc)
    x = torch.randn(B, H, W, Cc, generator=g)
    active = torch.rand(B, f, f, generator=g) < 0.5
    want = x * dilate(active, H, W).permute(0, 2, 3, 1)
    xg, y = held(x.cuda(), 256), Banded((B, H, W, Cc), 256)
    ag = active.to(torch.uint8).cuda()
    ok(ops, ops.lib.cddpm_op_spark_mask_mul(ops.h, xg.ptr(), p(ag), y.ptr(), B, H, W, Cc, f, None))
    ok(ops, ops.lib.cddpm_op_spark_mask_mul(ops.h, xg.ptr(), p(ag), xg.ptr(), B, H, W, Cc, f, None))         # in place
    torch.cuda.synchronize()
    assert torch.equal(y.check("mask_mul"), want) and torch.equal(xg.check("mask_mul in place"), want)


# ---------------------------------------------------------------------------------------------------------------- convolution family
CONV_CASES = [
    # (Cin, Cout, K, transposed, H, W, bias)
    (8, 4, 3, 0, 10, 7, False), (16, 16, 3, 0, 10, 7, False), (1024, 64, 3, 0, 4, 6, True),
    (2048, 128, 1, 0, 2, 2, True), (4, 1, 1, 0, 9, 5, True),
    (8, 8, 4, 1, 3, 3, True), (128, 128, 4, 1, 2, 3, True),
]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_convolution_family(ops, case, B):
    lib, h = ops.lib, ops.h
    Cin, Cout, K, tconv, H, W, has_bias = case
    g = torch.Generator().manual_seed(Cin + 7 * Cout + K)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    wshape = (Cin, Cout, K, K) if tconv else (Cout, Cin, K, K)
    w = (torch.randn(wshape, generator=g, dtype=torch.float64) / (Cin * K * K) ** 0.5).requires_grad_(True)
    b = (0.3 * torch.randn(Cout, generator=g, dtype=torch.float64)).requires_grad_(True)
    y_ref = F.conv_transpose2d(x, w, b if has_bias else None, 2, 1) if tconv else F.conv2d(x, w, b if has_bias else None, 1, K // 2)
    Ho, Wo = y_ref.shape[2:]
    dy = torch.randn(B, Cout, Ho, Wo, generator=g, dtype=torch.float64)
    y_ref.backward(dy)

    band = 64 * max(Cin, Cout)
    xg, dyg = held(nhwc(x.detach()), band), held(nhwc(dy), band)
    wg, bg = held(w.detach().float().cuda(), band), b.detach().float().cuda()
    runs = []
    for _ in range(2):
        y, dx = Banded((B, Ho, Wo, Cout), band), Banded((B, H, W, Cin), band)
        dw, db = Banded(wshape, band), Banded((Cout,), 64)
        ok(ops, lib.cddpm_op_spark_conv(h, xg.ptr(), wg.ptr(), p(bg) if has_bias else None, y.ptr(), B, H, W, Cin, Cout, K, tconv, 0, None))
        ok(ops, lib.cddpm_op_spark_conv(h, dyg.ptr(), wg.ptr(), None, dx.ptr(), B, H, W, Cin, Cout, K, tconv, 1, None))
        ok(ops, lib.cddpm_op_spark_conv_wgrad(h, xg.ptr(), dyg.ptr(), dw.ptr(), db.ptr() if has_bias else None, B, H, W, Cin, Cout, K, tconv, None))
        torch.cuda.synchronize()
        runs.append((y.check("y"), dx.check("dx"), dw.check("dw"), db.check("db", written=has_bias)))
    xg.check("x"), dyg.check("dy"), wg.check("w")                                 # the inputs and their bands are as they were
    for a, c in zip(*runs):
        assert torch.equal(a, c)                                                   # two calls: the same bits
    y, dx, dw, db = runs[0]
    close(nchw(y), y_ref.detach(), CONV_LIMIT, "y")
    close(nchw(dx), x.grad, CONV_LIMIT, "dx")
    close(dw, w.grad, CONV_LIMIT, "dw")
    if has_bias:
        close(db, b.grad, CONV_LIMIT, "db")


def test_convolution_family_refuses_other_geometries(ops):
    lib, h = ops.lib, ops.h
    t = torch.zeros(4096, device="cuda")
    for Cin, Cout, K, tconv in ((8, 8, 5, 0), (8, 8, 2, 0), (8, 8, 3, 1), (8, 8, 1, 1), (0, 8, 3, 0), (8, 0, 3, 0)):
        assert lib.cddpm_op_spark_conv(h, p(t), p(t), None, p(t[2048:]), 1, 4, 4, Cin, Cout, K, tconv, 0, None) != 0
        assert lib.cddpm_op_spark_conv_wgrad(h, p(t), p(t), p(t[2048:]), None, 1, 4, 4, Cin, Cout, K, tconv, None) != 0
    assert lib.cddpm_op_spark_conv_wgrad(h, p(t), p(t), p(t[2048:]), p(t[1024:]), 1, 1, 1, 4, 512, 1, 0, None) != 0       # bias gradient beyond 256 channels


# ---------------------------------------------------------------------------------------------------------------- loss
LOSS_MASKS = {
    "mixed": [[1, 0, 0, 1], [0, 0, 1, 0], [1, 1, 0, 1]],
    "one_sample_fully_active": [[1, 1, 1, 1], [0, 1, 0, 0], [0, 0, 1, 1]],
    "nothing_masked": [[1, 1, 1, 1]] * 3,
}


@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.5, 1.0)])
@pytest.mark.parametrize("name", list(LOSS_MASKS))
def test_loss(ops, name, weights):
    B, H, W, f = 3, 64, 64, 2
    w_mask, w_l1 = weights
    g = torch.Generator().manual_seed(5)
    rec = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    inp = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64).float().double()
    active = torch.tensor(LOSS_MASKS[name], dtype=torch.bool).view(B, f, f)
    masked = ~dilate(active, H, W)
    pp = (H // f) * (W // f)
    l_mask = ((rec - inp) ** 2 * masked).sum() / (pp * ((~active).sum() + 1e-8))          # spatial_loss, pix_norm 0 (spark/Spark_2D.py:192-199)
    l_l1 = (rec - inp).abs().mean()
    (w_mask * l_mask + w_l1 * l_l1).backward()
    l_mask, l_l1 = l_mask.detach(), l_l1.detach()
    recg, inpg = held(rec.detach().float().cuda().view(B, H, W), 256), held(inp.float().cuda().view(B, H, W), 256)
    loss, drec = Banded((2,), 64), Banded((B, H, W), 256)
    ok(ops, ops.lib.cddpm_op_spark_loss(ops.h, recg.ptr(), inpg.ptr(), p(active.to(torch.uint8).cuda()), f, B, H, W, C.c_float(w_mask), C.c_float(w_l1),
                                        loss.ptr(), drec.ptr(), None))
    torch.cuda.synchronize()
    got = loss.check("loss").double()
    print(f"{name}: masked {float(got[0]):.8e} (float64 {float(l_mask):.8e}), l1 {float(got[1]):.8e} (float64 {float(l_l1):.8e})")
    assert bool(torch.isfinite(got).all())
    if name == "nothing_masked":
        assert float(got[0]) == 0.0 and float(l_mask) == 0.0
    else:
        assert abs(float(got[0]) - float(l_mask)) <= LOSS_LIMIT * float(l_mask)
    assert abs(float(got[1]) - float(l_l1)) <= LOSS_LIMIT * float(l_l1)
    close(drec.check("drec").view(B, 1, H, W), rec.grad, LOSS_LIMIT, "drec")


# ---------------------------------------------------------------------------------------------------------------- AdamW
def test_adamw_follows_torch_and_a_skipped_step_decays_nothing(ops):
    """three guarded updates against torch.optim.AdamW(lr, weight_decay 0.05, betas (0.9, 0.95)) (src/models/Spark_2D.py:123-124) in
    float64; then a gradient with an inf: no update, no decay, no step"""
    lib, h = ops.lib, ops.h
    n, lr, wd, betas = 1000, 1e-2, 0.05, (0.9, 0.95)
    g = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=g)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd, betas=betas)
    pg, m, v = p0.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    ctrl = torch.zeros(8, dtype=torch.int32).cuda()

    def step(grad):
        ok(ops, lib.cddpm_op_grad_check(h, p(grad), n, p(ctrl), None))
        ok(ops, lib.cddpm_op_guard_commit(h, p(ctrl), C.c_float(betas[0]), C.c_float(betas[1]), None))
        ok(ops, lib.cddpm_op_adamw_guarded(h, p(pg), p(grad), p(m), p(v), n, C.c_float(lr), C.c_float(betas[0]), C.c_float(betas[1]), C.c_float(1e-8),
                                           C.c_float(wd), C.c_float(1.0), p(ctrl), None))

    for _ in range(3):
        grad = torch.randn(n, generator=g)
        ref.grad = grad.double()
        opt.step()
        step(grad.cuda())
    close(pg.cpu(), ref.detach(), 2e-6, "three AdamW steps")
    before, bad = pg.clone(), torch.randn(n, generator=g)
    bad[17] = float("inf")
    step(bad.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pg, before) and ctrl.cpu().tolist()[1:4] == [3, 1, 1]
