"""GPU: the training operators of the context encoder (csrc/encoder_train.hip, encoder_train_p16.hip and batchnorm_train.hip behind cddpm_op_enc_*) one call at a
time at the edges of their plans: many row tiles with a ragged last one, every contraction split, weight-gradient pixel ranges from one to the
cap, chunked BatchNorm reductions, max-pool inputs full of ties. The cases are tests/encoder_op_cases.py's; that they reach those plans is
what tests/test_encoder_op_cases_host.py asserts on the CPU. References are float64 on the CPU (for precision 16 on the operands rounded to
fp16: the yardstick of tests/test_gpu_encoder_ops_p16.py), the limits those of tests/test_gpu_encoder_ops.py: 5e-6 of the result's maximum
for a convolution and the stem, 2e-5 for BatchNorm, 1e-6 for the average pool. On integer operands every convolution result is exact in
both arithmetics, so a dropped, duplicated or misplaced element is an integer difference with no tolerance to hide in.

Every output lies between two guard bands (at least 64 rows of the produced width) pre-filled, like the output, with a sentinel: the bands
come back unchanged and no sentinel is left in the output; a refused call leaves the output as it was."""
import ctypes as C
import math

import pytest
import torch

import encoder_op_cases as EC
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CONV_LIMIT, BN_LIMIT, AVG_LIMIT = 5e-6, 2e-5, 1e-6
SENTINEL = -6.02e23          # an fp32 number no operator here produces; fp16 (weight images): -60200, as unlikely


@pytest.fixture(scope="module")
def ops():
    tr = load_pkg("training")
    o = tr.UNetTrainer({"w": torch.zeros(64)}, device=torch.device("cuda", 0))
    o._fit(4, 64, 64)
    return o


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().double()


def p(t):
    return None if t is None else t.data_ptr()


class Banded:
    """an output tensor between two guard bands of `band` elements (rounded up to 64), all three filled with a sentinel"""

    def __init__(self, shape, band, dtype=torch.float32):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.band = (max(band, 64) + 63) // 64 * 64
        self.fill = -60200.0 if dtype == torch.float16 else SENTINEL
        self.buf = torch.full((2 * self.band + self.n,), self.fill, dtype=dtype, device="cuda")
        self.out = self.buf[self.band:self.band + self.n].view(self.shape)

    def ptr(self):
        return self.out.data_ptr()

    def check(self, what, written=True):
        """-> the output on the host (fp32 / fp16 as it is); call after a synchronisation"""
        cpu = self.buf.cpu()
        lo, mid, hi = cpu[:self.band], cpu[self.band:self.band + self.n], cpu[self.band + self.n:]
        assert bool((lo == self.fill).all()) and bool((hi == self.fill).all()), f"{what}: a guard band was written"
        if written:
            assert not bool((mid == self.fill).any()), f"{what}: {int((mid == self.fill).sum())} elements were not written"
        else:
            assert bool((mid == self.fill).all()), f"{what}: a refused call wrote its output"
        return mid.view(self.shape)


def held(t, band):
    """an input between two sentinel bands: a read past either end meets the sentinel, not whatever a neighbouring tensor holds"""
    b = Banded(t.shape, band)
    b.out.copy_(t)
    return b


def ok(ops, rc):
    assert rc == 0, ops.lib.cddpm_last_error(ops.h)


# ---------------------------------------------------------------------------------------------------------------- convolutions
def run_conv(ops, case, kind, precision):
    """the roles the operators of `precision` take `case` in, from conv_operands(case, kind) -> {role: float64 result in PyTorch layout}"""
    lib, h = ops.lib, ops.h
    B, Cin, Cout, K, st, H, W = case
    Ho, Wo = EC.out_hw(case)
    roles = EC.CONV_CASES[case] if precision == 32 else "ydw"
    x, w, dy = EC.conv_operands(case, kind)
    band, nw = 64 * max(Cin, Cout), Cout * Cin * K * K
    wg = w.float().cuda().contiguous()
    if precision == 32:
        wf, wd = Banded((K * K, Cin, Cout), band), Banded((K * K, Cout, Cin), band)
        ok(ops, lib.cddpm_op_enc_pack_w(h, wg.data_ptr(), Cout, Cin, K, wf.ptr(), wd.ptr(), None))
        conv, wgrad = lib.cddpm_op_enc_conv, lib.cddpm_op_enc_conv_wgrad
    else:
        wf, wd = Banded((nw,), band, torch.float16), Banded((nw,), band, torch.float16)
        ok(ops, lib.cddpm_op_enc_pack_w_p16(h, wg.data_ptr(), Cout, Cin, K, wf.ptr(), wd.ptr(), None))
        conv, wgrad = lib.cddpm_op_enc_conv_p16, lib.cddpm_op_enc_conv_wgrad_p16
    xg, dyg = held(nhwc(x), band), held(nhwc(dy), band)
    out = {}
    if "y" in roles:
        out["y"] = Banded((B, Ho, Wo, Cout), band)
        ok(ops, conv(h, xg.ptr(), wf.ptr(), out["y"].ptr(), B, H, W, Cin, Cout, K, st, 0, None))
    if "d" in roles:
        out["d"] = Banded((B, H, W, Cin), band)
        ok(ops, conv(h, dyg.ptr(), wd.ptr(), out["d"].ptr(), B, H, W, Cin, Cout, K, st, 1, None))
    if "w" in roles:
        out["w"] = Banded((Cout, Cin, K, K), band)
        ok(ops, wgrad(h, xg.ptr(), dyg.ptr(), out["w"].ptr(), B, H, W, Cin, Cout, K, st, None))
    torch.cuda.synchronize()
    what = f"{EC.conv_id(case)} precision {precision}"
    if precision == 32:          # the two weight images are permutations of w
        assert torch.equal(wf.check(what + " wf"), w.float().permute(2, 3, 1, 0).reshape(K * K, Cin, Cout))
        assert torch.equal(wd.check(what + " wd"), w.float().permute(2, 3, 0, 1).reshape(K * K, Cout, Cin))
    else:
        wf.check(what + " wf"), wd.check(what + " wd")
    res = {r: b.check(f"{what} {EC.ROLES[r]}") for r, b in out.items()}
    return {r: (t.double() if r == "w" else nchw(t)) for r, t in res.items()}


CONV_RUNS = [(c, 32) for c in EC.CONV_CASES] + [(c, 16) for c in EC.CONV_CASES if EC.p16_accepts(c)]
_conv_run_id = lambda v: EC.conv_id(v) if isinstance(v, tuple) else f"p{v}"


@pytest.mark.parametrize("case,precision", CONV_RUNS, ids=_conv_run_id)
def test_convolution_roles_on_random_operands(ops, case, precision):
    got = run_conv(ops, case, "random", precision)
    ref = dict(zip("ydw", EC.conv_reference(case, "random", precision)))
    e = {r: EC.rel(g, ref[r]) for r, g in got.items()}
    print(EC.conv_id(case), f"precision {precision}", EC.conv_plan(case, precision), {EC.ROLES[r]: f"{v:.1e}" for r, v in e.items()})
    assert set(got) == set(EC.CONV_CASES[case] if precision == 32 else "ydw")
    assert max(e.values()) < CONV_LIMIT


@pytest.mark.parametrize("case,precision", CONV_RUNS, ids=_conv_run_id)
def test_convolution_roles_are_exact_on_integer_operands(ops, case, precision):
    got = run_conv(ops, case, "integer", precision)
    ref = dict(zip("ydw", EC.conv_reference(case, "integer")))
    for r, g in got.items():
        bad = g != ref[r]
        assert g.shape == ref[r].shape and not bool(bad.any()), (EC.ROLES[r], int(bad.sum()), "elements differ, first at", bad.nonzero()[0].tolist(),
                                                                 "by up to", float((g - ref[r]).abs().max()))


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("case", EC.SPLIT_CASES, ids=EC.conv_id)
def test_two_calls_return_identical_bits(ops, case, precision):
    plan = EC.conv_plan(case, precision)
    assert max(plan.values()) > 1
    a, b = run_conv(ops, case, "random", precision), run_conv(ops, case, "random", precision)
    for r in a:
        assert torch.equal(a[r].float().view(torch.int32), b[r].float().view(torch.int32)), EC.ROLES[r]


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def run_bn(ops, case, o, opt, entry="enc"):
    """forward and backward on the device -> dict of float64 NCHW / per-channel results (keys as EC.bn_reference). entry "spark": the same
    call through cddpm_op_spark_bn_forward / _backward without a mask or a fill value, f = 1, in training mode, act = relu"""
    lib, h = ops.lib, ops.h
    B, C_, H, W = case
    N, HW = B * H * W, H * W
    band = 64 * C_
    zg, dyg = held(nhwc(o["z"]), band), held(nhwc(o["dy"]), band)
    gam, bet = o["gamma"].float().cuda(), o["beta"].float().cuda()
    rg = held(nhwc(o["res"]), band) if opt["res"] else None
    ssg = EC.sample_scale(B).float().cuda() if opt["drop"] else None
    rm, rv = (Banded((C_,), 64), Banded((C_,), 64)) if opt["run"] else (None, None)
    if opt["run"]:
        rm.out.copy_(o["run_mean"].float()), rv.out.copy_(o["run_var"].float())
    relu = int(opt["relu"])
    mr, y = Banded((2, C_), band), Banded((B, H, W, C_), band)
    forward, backward = (lib.cddpm_op_enc_bn_forward, lib.cddpm_op_enc_bn_backward) if entry == "enc" else (lib.cddpm_op_spark_bn_forward, lib.cddpm_op_spark_bn_backward)
    tail = (None,) if entry == "enc" else (None, 1, H, W, None, 1, None)          # stream | active, f, H, W, fill / dfill, training, stream
    ok(ops, forward(h, zg.ptr(), gam.data_ptr(), bet.data_ptr(), p(ssg), rg and rg.ptr(), relu, C.c_float(EC.BN_EPS), C.c_float(EC.BN_MOMENTUM),
                    rm and rm.ptr(), rv and rv.ptr(), mr.ptr(), y.ptr(), N, HW, C_, *tail))
    dz, dres = Banded((B, H, W, C_), band), (Banded((B, H, W, C_), band) if opt["dres"] else None)
    dg, db = Banded((C_,), 64), Banded((C_,), 64)
    assert not (opt["y_null"] and relu)
    ok(ops, backward(h, zg.ptr(), None if opt["y_null"] else y.ptr(), dyg.ptr(), mr.ptr(), gam.data_ptr(), p(ssg), relu, dz.ptr(),
                     dres and dres.ptr(), dg.ptr(), db.ptr(), N, HW, C_, *tail))
    torch.cuda.synchronize()
    what = "x".join(map(str, case)) + " " + EC.bn_option_id(opt)
    mrc = mr.check(what + " mean|rstd").double()
    got = dict(y=nchw(y.check(what + " y")), mean=mrc[0], rstd=mrc[1], dz=nchw(dz.check(what + " dz")), dgamma=dg.check(what + " dgamma").double(),
               dbeta=db.check(what + " dbeta").double())
    if opt["dres"]:
        got["dres"] = nchw(dres.check(what + " dres"))
    if opt["run"]:
        got["run_mean"], got["run_var"] = rm.check(what + " run_mean").double(), rv.check(what + " run_var").double()
    return got


def bn_refs(case, o, opt, got, dtype=torch.float64):
    B = case[0]
    return EC.bn_reference(o["z"], o["gamma"], o["beta"], o["dy"], opt["relu"], mask=got["y"] > 0, res=o["res"] if opt["res"] else None,
                           ss=EC.sample_scale(B) if opt["drop"] else None, run_mean=o["run_mean"] if opt["run"] else None,
                           run_var=o["run_var"] if opt["run"] else None, dtype=dtype)


@pytest.mark.parametrize("opt", EC.BN_OPTIONS, ids=EC.bn_option_id)
@pytest.mark.parametrize("case", EC.BN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_forward_and_backward(ops, case, opt):
    """float64 autograd on the implementation's ReLU mask; running statistics start from random values"""
    o = EC.bn_operands(case)
    got = run_bn(ops, case, o, opt)
    ref = bn_refs(case, o, opt, got)
    e = {k: EC.rel(v, ref[k]) for k, v in got.items()}
    print(case, EC.bn_option_id(opt), "chunks", EC.bn_chunks(case), {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < BN_LIMIT, e
    if opt["relu"]:
        assert 0.2 < float((got["y"] > 0).double().mean()) < 0.8
    if opt["drop"] and not opt["res"]:
        assert float(got["y"][1].abs().max()) == 0.0


@pytest.mark.parametrize("ratio", [10.0, 100.0])
@pytest.mark.parametrize("case", [(3, 64, 19, 9), (2, 64, 65, 65)], ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_with_a_large_mean(ops, case, ratio):
    """|mean| / sigma of 10 and 100, against float64 on the same fp32 inputs. No number is fixed in advance: the limit of every result is
    max(2e-5, 4 x the distance of torch's own fp32 CPU batch_norm / autograd from float64 on these inputs) -- the factor 4 covers the kernel's
    different summation order and its fp32 elementwise pass. Measured on an MI355X, kernel (torch fp32), worst of the two cases: ratio 10: y 1.5e-7
    (2.0e-7), dz 1.2e-7 (1.5e-7), dgamma 3.3e-7 (4.2e-7), dbeta 4.3e-8 (3.1e-7); ratio 100: y 1.3e-6 (2.5e-6), dz 3.1e-7 (3.3e-7), dgamma 5.4e-6
    (5.4e-6), dbeta 4.9e-8 (3.0e-7); mean, rstd and the running statistics below 1e-7 (below 2e-7) throughout. So 2e-5 is the limit that
    binds everywhere; DESIGN.md section 4b, "The encoder's operators at plan edges"."""
    opt = dict(relu=True, res=False, drop=False, dres=True, run=True, y_null=False)
    o = EC.bn_operands(case, ratio)
    got = run_bn(ops, case, o, opt)
    ref = bn_refs(case, o, opt, got)
    yard = bn_refs(case, o, opt, got, dtype=torch.float32)
    rows = {k: (EC.rel(v, ref[k]), EC.rel(yard[k].double(), ref[k])) for k, v in got.items()}
    print(case, "ratio", ratio, {k: f"{e:.1e} (torch fp32 {t:.1e})" for k, (e, t) in rows.items()})
    for k, (e, t) in rows.items():
        assert e < max(BN_LIMIT, 4 * t), (k, e, t)


@pytest.mark.parametrize("opt", [EC.BN_OPTIONS[1], EC.BN_OPTIONS[2]], ids=EC.bn_option_id)        # everything on; nothing on (no ReLU: y may be NULL)
@pytest.mark.parametrize("case", [(2, 64, 9, 7),          # N = 126: one chunk, a ragged lane tail
                                  (2, 64, 23, 29)],       # N = 1334: five chunks, the last ragged, a sample boundary inside a chunk
                         ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_entries_are_one_implementation(ops, case, opt):
    """cddpm_op_enc_bn_* and cddpm_op_spark_bn_* (no mask, f = 1, no fill, training) run the same kernels (csrc/batchnorm_train.hip); what
    differs is the plan each entry hands them. At C = 64 and N <= 8192 both chunk rules give N / 256 chunks (N 64 / 16384), so every
    result has the same bits: the fp64 partial sums are taken and folded in the same order, the elementwise passes are the same code."""
    B, C_, H, W = case
    N, HW = B * H * W, H * W
    q = lambda name: getattr(ops.lib, f"cddpm_op_{name}_scratch")(N, HW, C_)
    r256 = lambda n: (n + 255) // 256 * 256
    nchunk = max(1, N // 256)
    assert q("enc_bn_forward") == r256(nchunk * 2 * C_ * 8)                           # the two rules agree here: nchunk chunks of 2 planes ...
    assert q("spark_bn_forward") == r256(nchunk * 2 * C_ * 8) + 256                   # ... + the status words
    assert q("spark_bn_backward") == r256(nchunk * 3 * C_ * 8) + r256(2 * C_ * 4)     # 3 planes in the spark entry's backward
    o = EC.bn_operands(case)
    enc, spark = run_bn(ops, case, o, opt, "enc"), run_bn(ops, case, o, opt, "spark")
    assert set(enc) == set(spark) >= {"y", "mean", "rstd", "dz", "dgamma", "dbeta"}
    for k in enc:
        assert torch.equal(enc[k].float().view(torch.int32), spark[k].float().view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("C_", EC.MAXPOOL_CHANNELS)
@pytest.mark.parametrize("H,W", EC.MAXPOOL_SHAPES)
def test_maxpool_equals_torch_float64(ops, H, W, C_, kind):
    """exactly: the inputs are fp32 numbers, dy is integer-valued, nothing rounds -- on `ties` only torch's rule (the first maximum of a
    window in row-major order takes the gradient) gives this dx"""
    lib, h = ops.lib, ops.h
    B = 2
    x, dy = EC.maxpool_input(kind, B, C_, H, W)
    ty, tdx = EC.maxpool_torch(x, dy)
    xg, dyg = held(nhwc(x), 64 * C_), held(nhwc(dy), 64 * C_)
    y, dx = Banded((B, (H + 1) // 2, (W + 1) // 2, C_), 64 * C_), Banded((B, H, W, C_), 64 * C_)
    ok(ops, lib.cddpm_op_enc_maxpool(h, xg.ptr(), y.ptr(), B, H, W, C_, 0, None, None, None))
    ok(ops, lib.cddpm_op_enc_maxpool(h, xg.ptr(), None, B, H, W, C_, 1, dyg.ptr(), dx.ptr(), None))
    torch.cuda.synchronize()
    gy, gdx = nchw(y.check("max pool")), nchw(dx.check("max pool backward"))
    assert gy.shape == ty.shape and not bool((gy != ty).any())
    bad = gdx != tdx
    assert gdx.shape == tdx.shape and not bool(bad.any()), (int(bad.sum()), "of", bad.numel(), "elements differ")
    assert float(gdx.sum()) == float(dy.sum())               # every window's gradient went to exactly one element


@pytest.mark.parametrize("B,C_,HW", EC.AVGPOOL_CASES)
def test_avgpool_both_directions(ops, B, C_, HW):
    lib, h = ops.lib, ops.h
    g = torch.Generator().manual_seed(B + C_ + HW)
    x = torch.randn(B, HW, C_, generator=g)
    dg = torch.randn(B, C_, generator=g)
    out, dx = Banded((B, C_), 64 * C_), Banded((B, HW, C_), 64 * C_)
    xg, dgg = held(x.cuda(), 64 * C_), held(dg.cuda(), 64 * C_)
    ok(ops, lib.cddpm_op_enc_avgpool(h, xg.ptr(), out.ptr(), B, HW, C_, 0, None))
    ok(ops, lib.cddpm_op_enc_avgpool(h, dgg.ptr(), dx.ptr(), B, HW, C_, 1, None))
    torch.cuda.synchronize()
    e = (EC.rel(out.check("average pool").double(), x.double().mean(dim=1)),
         EC.rel(dx.check("average pool backward").double(), (dg.double() / HW)[:, None, :].expand(B, HW, C_)))
    print((B, C_, HW), "g %.1e dx %.1e" % e)
    assert max(e) < AVG_LIMIT


# ---------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("case", EC.STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_forward_and_weight_gradient(ops, case, kind):
    """integer operands: the forward is an fp32 FMA chain of at most 49 integer products, the weight gradient accumulates in fp64 -- both exact"""
    lib, h = ops.lib, ops.h
    B, H, W = case
    x, w, dz = EC.stem_operands(case, kind)
    rz, rdw = EC.stem_reference(case, kind)
    xg, wg, dzg = held(x.float().cuda(), 64 * 64), w.float().cuda().contiguous(), held(nhwc(dz), 64 * 64)
    z, dw = Banded((B, (H + 1) // 2, (W + 1) // 2, 64), 64 * 64), Banded((64, 1, 7, 7), 64 * 64)
    ok(ops, lib.cddpm_op_enc_stem(h, xg.ptr(), wg.data_ptr(), z.ptr(), B, H, W, None))
    ok(ops, lib.cddpm_op_enc_stem_wgrad(h, xg.ptr(), dzg.ptr(), dw.ptr(), B, H, W, None))
    torch.cuda.synchronize()
    gz, gdw = nchw(z.check("stem")), dw.check("stem weight gradient").double()
    if kind == "integer":
        assert torch.equal(gz, rz) and torch.equal(gdw, rdw)
    else:
        e = (EC.rel(gz, rz), EC.rel(gdw, rdw))
        print(case, "z %.1e dw %.1e" % e)
        assert max(e) < CONV_LIMIT


# ---------------------------------------------------------------------------------------------------------------- what the ABI refuses
def test_refused_calls_leave_their_outputs_alone(ops):
    """argument checks on the host, before any launch: non-zero, cddpm_last_error names the operator, the sentinel-filled output is as it was"""
    lib, h = ops.lib, ops.h
    src = torch.zeros(1 << 20, device="cuda")          # larger than any operand a call below names
    img = torch.zeros(1 << 20, device="cuda")
    s, i = src.data_ptr(), img.data_ptr()
    B, H, W = 2, 4, 4

    def refused(name, call, *outs):
        assert lib.cddpm_op_enc_avgpool(h, None, None, 0, 0, 0, 0, None) != 0 and b"avgpool" in lib.cddpm_last_error(h)     # another message first
        rc = call(*[o.ptr() for o in outs])
        assert rc != 0, name
        msg = lib.cddpm_last_error(h)
        assert msg.startswith(name.encode() + b":"), (name, msg)
        torch.cuda.synchronize()
        for o in outs:
            o.check(name, written=False)

    new = lambda: Banded((1 << 16,), 1 << 12)
    bad = [("Cin = 40", dict(Cin=40)), ("Cout = 96", dict(Cout=96)), ("K = 5", dict(K=5)), ("stride = 3", dict(st=3))]
    for what, kw in bad:
        a = dict(Cin=64, Cout=64, K=3, st=1)
        a.update(kw)
        Cin, Cout, K, st = a["Cin"], a["Cout"], a["K"], a["st"]
        for sfx in ("", "_p16"):
            conv, wgrad = getattr(lib, "cddpm_op_enc_conv" + sfx), getattr(lib, "cddpm_op_enc_conv_wgrad" + sfx)
            for transposed in (0, 1):
                if sfx == "" and transposed and what == "Cout = 96":
                    continue          # a contraction of 96 channels is a multiple of 16: the fp32 input gradient takes it
                refused("cddpm_op_enc_conv" + sfx, lambda o: conv(h, s, i, o, B, H, W, Cin, Cout, K, st, transposed, None), new())
            refused("cddpm_op_enc_conv_wgrad" + sfx, lambda o: wgrad(h, s, s, o, B, H, W, Cin, Cout, K, st, None), new())
        if what != "stride = 3":
            refused("cddpm_op_enc_pack_w_p16", lambda o, q: lib.cddpm_op_enc_pack_w_p16(h, s, Cout, Cin, K, o, q, None), new(), new())
    refused("cddpm_op_enc_pack_w", lambda o, q: lib.cddpm_op_enc_pack_w(h, s, 64, 64, 5, o, q, None), new(), new())
    # the roles the case table leaves out are the ones the fp32 operators refuse
    for case, roles in EC.CONV_CASES.items():
        Bc, Cin, Cout, K, st, Hc, Wc = case
        if "y" not in roles:
            refused("cddpm_op_enc_conv", lambda o: lib.cddpm_op_enc_conv(h, s, i, o, Bc, Hc, Wc, Cin, Cout, K, st, 0, None), new())
        if "d" not in roles:
            refused("cddpm_op_enc_conv", lambda o: lib.cddpm_op_enc_conv(h, s, i, o, Bc, Hc, Wc, Cin, Cout, K, st, 1, None), new())
        if "w" not in roles:
            refused("cddpm_op_enc_conv_wgrad", lambda o: lib.cddpm_op_enc_conv_wgrad(h, s, s, o, Bc, Hc, Wc, Cin, Cout, K, st, None), new())
    # NULL for a required pointer
    refused("cddpm_op_enc_conv", lambda o: lib.cddpm_op_enc_conv(h, None, i, o, B, H, W, 64, 64, 3, 1, 0, None), new())
    refused("cddpm_op_enc_conv", lambda o: lib.cddpm_op_enc_conv(h, s, None, o, B, H, W, 64, 64, 3, 1, 0, None), new())
    refused("cddpm_op_enc_conv_p16", lambda o: lib.cddpm_op_enc_conv_p16(h, s, None, o, B, H, W, 64, 64, 3, 1, 1, None), new())
    refused("cddpm_op_enc_conv_wgrad", lambda o: lib.cddpm_op_enc_conv_wgrad(h, s, None, o, B, H, W, 64, 64, 3, 1, None), new())
    refused("cddpm_op_enc_conv_wgrad_p16", lambda o: lib.cddpm_op_enc_conv_wgrad_p16(h, None, s, o, B, H, W, 64, 64, 3, 1, None), new())
    refused("cddpm_op_enc_conv", lambda: lib.cddpm_op_enc_conv(h, s, i, None, B, H, W, 64, 64, 3, 1, 0, None))
    refused("cddpm_op_enc_stem", lambda o: lib.cddpm_op_enc_stem(h, s, None, o, B, H, W, None), new())
    refused("cddpm_op_enc_stem_wgrad", lambda o: lib.cddpm_op_enc_stem_wgrad(h, None, s, o, B, H, W, None), new())
    refused("cddpm_op_enc_avgpool", lambda o: lib.cddpm_op_enc_avgpool(h, None, o, B, 16, 64, 0, None), new())
    # BatchNorm: C = 32, a NULL gamma, one running statistic without the other, relu without y
    eps, mom, N, HW = C.c_float(EC.BN_EPS), C.c_float(EC.BN_MOMENTUM), B * H * W, H * W
    fwd = lambda Cc, gamma, rm, rv: (lambda mr, y: lib.cddpm_op_enc_bn_forward(h, s, gamma, i, None, None, 1, eps, mom, rm, rv, mr, y, N, HW, Cc, None))
    run = new()
    refused("cddpm_op_enc_bn_forward", fwd(32, i, None, None), new(), new())
    refused("cddpm_op_enc_bn_forward", fwd(64, None, None, None), new(), new())
    refused("cddpm_op_enc_bn_forward", fwd(64, i, run.ptr(), None), new(), new())
    refused("cddpm_op_enc_bn_forward", fwd(64, i, None, run.ptr()), new(), new())
    torch.cuda.synchronize()
    run.check("the running statistic of a refused call", written=False)
    bwd = lambda Cc, y, relu: (lambda dz, dres, dg, db: lib.cddpm_op_enc_bn_backward(h, s, y, s, i, i, None, relu, dz, dres, dg, db, N, HW, Cc, None))
    refused("cddpm_op_enc_bn_backward", bwd(32, s, 1), new(), new(), new(), new())
    refused("cddpm_op_enc_bn_backward", bwd(64, None, 1), new(), new(), new(), new())
    refused("cddpm_op_enc_bn_backward", lambda dres, dg, db: lib.cddpm_op_enc_bn_backward(h, s, s, s, i, i, None, 1, None, dres, dg, db, N, HW, 64, None),
            new(), new(), new())
    # max pool: C = 6, a direction without its pointers
    refused("cddpm_op_enc_maxpool", lambda o: lib.cddpm_op_enc_maxpool(h, s, o, B, H, W, 6, 0, None, None, None), new())
    refused("cddpm_op_enc_maxpool", lambda o: lib.cddpm_op_enc_maxpool(h, s, None, B, H, W, 6, 1, s, o, None), new())
    refused("cddpm_op_enc_maxpool", lambda o: lib.cddpm_op_enc_maxpool(h, s, None, B, H, W, 64, 1, None, o, None), new())
    refused("cddpm_op_enc_maxpool", lambda o: lib.cddpm_op_enc_maxpool(h, None, o, B, H, W, 64, 0, None, None, None), new())
    refused("cddpm_op_enc_maxpool", lambda: lib.cddpm_op_enc_maxpool(h, s, None, B, H, W, 64, 0, None, None, None))
