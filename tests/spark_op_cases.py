"""What the tests of the SparK operators share (tests/test_spark_op_cases_host.py, tests/test_gpu_spark_ops_edges.py): the plan rules of
csrc/spark_train.hip, of the BatchNorm behind cddpm_op_spark_bn_* (csrc/batchnorm_train.hip) and of that entry (csrc/cddpm_ops.hip) restated in
Python with the source line beside each, one table of cases per operator (a comment states the edge each
case is there for), seeded operands, float64 references written from each operation's definition, and the results a wrong kernel of a
given kind would produce (`mut`). Nothing here needs a GPU; everything is computed once per process (lru_cache) and never modified.

Operands are fp32 numbers held in float64. Layouts are the kernels': activations NHWC [B,H,W,C], the cell mask uint8 / bool [B,f,f],
one-channel images [B,H,W], weights in PyTorch's layout (Conv2d [Cout][Cin][K][K], ConvTranspose2d [Cin][Cout][K][K]).

Limits are the project's for this arithmetic (tests/test_gpu_spark_ops.py): 2e-5 of a result's maximum for BatchNorm, 5e-6 for a
convolution on random operands (0 on integer operands), 2e-6 for the loss and AdamW. The badly conditioned BatchNorm cases (`yardstick`:
|mean| / sigma of 10 and 100, a channel that is constant over the active pixels) take max(2e-5, 4 x the distance of torch's fp32 CPU run of
the same reference from float64): the rule of tests/test_gpu_encoder_ops_edges.py::test_batchnorm_with_a_large_mean."""
import functools
import zlib

import torch
import torch.nn.functional as F

BN_LIMIT, CONV_LIMIT, LOSS_LIMIT, ADAM_LIMIT = 2e-5, 5e-6, 2e-6, 2e-6
EPS, MOM = 1e-5, 0.1


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().double()


def rel(got, want):
    """the project's measure: the largest difference over the result's largest magnitude"""
    return float((got.double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- the plan rules
def r256(nbytes):
    """the operator arena hands out multiples of 256 bytes"""
    return (nbytes + 255) // 256 * 256


def count_trips(ncell):
    """count_active_cells, kernels.h:362: for (i = threadIdx.x; i < ncell; i += 256) -> trips of thread 0"""
    return len(range(0, ncell, 256))


def bn_chunks(N, C):
    """spark_bn_chunks, cddpm_ops.hip:836-840: the chunk rule of the cddpm_op_spark_bn_* entries"""
    return max(1, min(128, N * C // 16384))


def bn_lanes(C):
    """bn_train_args / launch_bn_chan_partial, batchnorm_train.hip:238, 243 -> (qpb, rows, blockIdx.y blocks)"""
    qpb = min(C // 4, 16)
    return qpb, 256 // qpb, (C // 4 + qpb - 1) // qpb


def chunk_ranges(N, nchunk):
    """per = ceil(N / nchunk), [per k, min(per k + per, N)): batchnorm_train.hip:54 (BatchNorm), spark_train.hip:227 (channel sum), :274 (loss).
    A range whose start is at or beyond N is empty"""
    per = (N + nchunk - 1) // nchunk
    return [(per * k, max(per * k, min(per * k + per, N))) for k in range(nchunk)]


def conv_split(M, Cd, Cs, K):
    """spark_conv_split, spark_train.hip:124-130 -> (Z, nstep)"""
    wgs = ((M + 63) // 64) * ((Cd + 63) // 64)
    nstep = K * K * ((Cs + 15) // 16)
    Z = 1
    while Z < 32 and wgs * Z * 2 <= 512 and nstep // (Z * 2) >= 8:
        Z *= 2
    return Z, nstep


def step_ranges(nstep, Z):
    """spark_conv_kernel, spark_train.hip:82: s0 = nstep z / Z, s1 = nstep (z + 1) / Z; step = tap nck + 16-channel chunk (:57)"""
    return [(nstep * z // Z, nstep * (z + 1) // Z) for z in range(Z)]


def wgrad_parts(M, Cd, Cg, K):
    """spark_wgrad_parts, spark_train.hip:211-217"""
    per = ((Cd + 63) // 64) * ((Cg + 63) // 64) * K * K
    return max(1, min((512 + per - 1) // per, M // 64, 64))


def pixel_ranges(M, P):
    """spark_wgrad_kernel, spark_train.hip:153: m0 = M part / P, m1 = M (part + 1) / P, walked in steps of 16 pixels (:161)"""
    return [(M * k // P, M * (k + 1) // P) for k in range(P)]


def chan_sum_chunks(M, C):
    """spark_chan_sum_chunks, spark_train.hip:246-250"""
    return max(1, min(256, M * C // 8192))


def loss_chunks(total):
    """spark_loss_chunks, spark_train.hip:304-308"""
    return max(1, min(256, total // 4096))


def cell_mask(active, H, W, swap=False):
    """bool [B,f,f] -> bool [B,H,W] by the kernels' own index ((b f + y / ch) f + x / cw), ch = H / f, cw = W / f (batchnorm_train.hip:38-40,
    spark_train.hip:26, :281). swap: ch and cw exchanged; an index that then leaves the mask reads 0"""
    B, f = active.shape[0], active.shape[1]
    ch, cw = (W // f, H // f) if swap else (H // f, W // f)
    b, y, x = torch.arange(B).view(B, 1, 1), torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    idx = (b * f + y // ch) * f + x // cw
    flat = active.reshape(-1)
    flat = torch.cat([flat, torch.zeros(max(0, int(idx.max()) + 1 - flat.numel()), dtype=flat.dtype)])
    return flat[idx]


def random_cells(g, B, f, density=0.5):
    """bool [B,f,f]: about `density` of the cells set, two or more per sample"""
    a = torch.rand(B, f * f, generator=g) < density
    if f * f >= 2:
        for b in range(B):
            a[b, torch.randperm(f * f, generator=g)[:2]] |= a[b].sum() < 2
    else:
        a[:] = True
    return a.view(B, f, f)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def _bn(B, H, W, f, C, sparse, act, **kw):
    d = dict(B=B, H=H, W=W, f=f, C=C, sparse=sparse, act=act, res=False, ss=False, fill=False, dres=False, run=True, y_null=False, training=1,
             ratio=None, const=False, yardstick=False, density=0.5)
    d.update(kw)
    d["yardstick"] = d["ratio"] is not None or d["const"]
    assert not (d["y_null"] and act) and (sparse or f == 1)
    return d


BN_CASES = {
    # 297 cells, one pixel each: count_active_cells' second trip; active cells at index >= 256. Residual, sample scale, dres, running statistics
    "cells297_relu_res_ss": _bn(33, 3, 3, 3, 64, True, 1, res=True, ss=True, dres=True),
    # H != W with ch = 5 != cw = 7; C = 72: 18 quads over two blockIdx.y blocks, the second partial. ReLU6 with fill and residual
    "rect_c72_relu6_fill_res": _bn(2, 10, 14, 2, 72, True, 2, res=True, fill=True, dres=True),
    # 32 chunks of 9 pixels over N = 261: 3 trailing chunks empty; 261 cells; running statistics a NULL pair; y = NULL with act 0; no dres
    "empty_chunks_c2048_norun_ynull": _bn(29, 3, 3, 3, 2048, True, 0, fill=True, run=False, y_null=True),
    # qpb 10, rows 25 (6 idle threads) in training; 10 chunks of 446, the last 441; boundaries inside a row and inside a sample; ch 11 != cw 15
    "c40_ragged_sparse_relu_ss_res_fill": _bn(3, 33, 45, 3, 40, True, 1, res=True, ss=True, fill=True, dres=True),
    "c40_ragged_dense_relu6": _bn(3, 33, 45, 1, 40, False, 2, dres=True),
    # qpb 3, rows 85 (thread 255 idle), sparse, training
    "c12_sparse_relu6_fill_res": _bn(2, 12, 18, 6, 12, True, 2, res=True, fill=True),
    # the cap of 128 chunks: per 2097, the last 2001; qpb 2, rows 128
    "cap128_c8_relu": _bn(1, 520, 516, 4, 8, True, 1, fill=True),
    # channels 1 and 5 constant over the active pixels (0.75: exact in fp32; fp32(0.1): not short), varying over the inactive ones
    "constant_channels": _bn(2, 8, 12, 2, 8, True, 0, fill=True, const=True, dres=True),
    # a sample scale with a 0 entry, fill, no residual: the dropped sample's inactive pixels are fill * 0
    "dropped_sample_fill_nores": _bn(3, 6, 6, 3, 16, True, 0, ss=True, fill=True),
    # evaluation mode, sparse, with fill and dfill
    "eval_sparse_fill": _bn(2, 8, 12, 2, 24, True, 1, res=True, ss=True, fill=True, dres=True, training=0),
    # the trainer's decoder call: dense, no activation, y = NULL, no dres, no running statistics
    "dense_norun_ynull": _bn(2, 5, 7, 1, 4, False, 0, run=False, y_null=True),
    # |mean| / sigma of 10 and 100 on a sparse and on a dense shape (several chunks on the dense one)
    "large_mean_10_sparse": _bn(2, 10, 14, 2, 72, True, 1, ratio=10.0, dres=True),
    "large_mean_100_sparse": _bn(2, 10, 14, 2, 72, True, 1, ratio=100.0, dres=True),
    "large_mean_10_dense": _bn(3, 33, 45, 1, 40, False, 1, ratio=10.0, dres=True),
    "large_mean_100_dense": _bn(3, 33, 45, 1, 40, False, 1, ratio=100.0, dres=True),
}
BN_MUTATIONS = ("count255", "swap", "last_chunk", "ragged", "last_quad", "all_pixels")


def sample_scale(B):
    return torch.tensor([1.25, 0.0, 1.0] * (B // 3 + 1), dtype=torch.float64)[:B]


@functools.lru_cache(maxsize=None)
def bn_operands(name):
    c = BN_CASES[name]
    B, H, W, f, C = c["B"], c["H"], c["W"], c["f"], c["C"]
    g = _gen("bn", name)
    active = random_cells(g, B, f, c["density"]) if c["sparse"] else None
    on = cell_mask(active, H, W) if c["sparse"] else torch.ones(B, H, W, dtype=torch.bool)
    z = _randn(g, B, H, W, C) * 1.5 + 0.3
    if c["ratio"] is not None:
        sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
        z = (_randn(g, B, H, W, C) * 1.5 + c["ratio"] * 1.5 * sign).float().double()
    gamma, beta = 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    if c["const"]:
        for ch_, val in ((1, 0.75), (5, float(torch.tensor(0.1, dtype=torch.float32)))):
            z[..., ch_] = torch.where(on, torch.full_like(z[..., ch_], val), z[..., ch_])
            gamma[ch_] = 0.004          # rstd is 1 / sqrt(eps) = 316 there: keeps that channel's dz at the size of the others'
    fill = 0.5 * _randn(g, C) if c["fill"] else None
    res = _randn(g, B, H, W, C) if c["res"] else None
    if c["act"] == 2:                 # outputs straddle both 0 and 6, at active and at inactive pixels
        gamma, beta = gamma * 3.0, beta + 3.0
        fill = None if fill is None else fill + 3.0
        res = None if res is None else res * 2.0
        if c["res"] and not c["fill"]:
            res = res + 1.5
    o = dict(z=z, dy=_randn(g, B, H, W, C), gamma=gamma.float().double(), beta=beta.float().double(), active=active,
             fill=None if fill is None else fill.float().double(), res=None if res is None else res.float().double(),
             s=sample_scale(B) if c["ss"] else None, rm=(0.2 * _randn(g, C)).float().double(),
             rv=(0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double())
    return o


def bn_plan(name):
    c = BN_CASES[name]
    N = c["B"] * c["H"] * c["W"]
    qpb, rows, yblocks = bn_lanes(c["C"])
    ranges = chunk_ranges(N, bn_chunks(N, c["C"]))
    return dict(N=N, cells=c["B"] * c["f"] ** 2 if c["sparse"] else 0, chunks=len(ranges), ranges=ranges, qpb=qpb, rows=rows, yblocks=yblocks)


def bn_mutations(name):
    """the mutations that change what a kernel of that kind would compute for this case"""
    c, pl = BN_CASES[name], bn_plan(name)
    out = ["last_quad"]
    if c["sparse"] and c["training"]:
        out.append("all_pixels")
        if pl["cells"] > 256:
            out.append("count255")
    if c["sparse"] and c["H"] // c["f"] != c["W"] // c["f"]:
        out.append("swap")
    if pl["chunks"] > 1 and pl["ranges"][-1][0] < pl["N"]:
        out.append("last_chunk")
    if pl["N"] % pl["chunks"]:
        out.append("ragged")
    return out


def bn_ref(name, mut=None, dtype=torch.float64, y_impl=None):
    """y = act((active ? bn(z) : fill) s[b] + res) with the statistics of the active pixels (training) or the running ones, and its
    backward from the definition: g = dy act'(y) s[b]; dbeta = sum_active g, dgamma = sum_active g zhat, dfill = sum_inactive g,
    dz = active ? gamma rstd (g - dbeta / n - zhat dgamma / n) : 0 (evaluation: without the two means), dres = dy act'(y).
    y_impl (NHWC): take act' on the implementation's own output. dtype float32: torch's fp32 CPU run of the same formulas (the yardstick).
    mut: a wrong kernel -- cells counted up to index 255 only, ch and cw swapped, the last chunk / the ragged remainder of the pixel ranges
    dropped from every sum, the sums of the last channel quad missing, statistics over all pixels. -> dict of results, NHWC / per channel"""
    c, o = BN_CASES[name], bn_operands(name)
    B, H, W, f, C, act, training = c["B"], c["H"], c["W"], c["f"], c["C"], c["act"], c["training"]
    N = B * H * W
    t = lambda k: None if o[k] is None else o[k].to(dtype)
    z, dy, gamma, beta = t("z").reshape(N, C), t("dy").reshape(N, C), t("gamma"), t("beta")
    on = cell_mask(o["active"], H, W, swap=mut == "swap").reshape(N) if c["sparse"] else torch.ones(N, dtype=torch.bool)
    n = N
    if c["sparse"]:
        cells = o["active"].reshape(-1)
        n = int((cells[:256] if mut == "count255" else cells).sum()) * (H // f) * (W // f)
    sel = torch.ones(N, dtype=torch.bool)
    nchunk = bn_chunks(N, C)
    if mut == "last_chunk":
        sel[chunk_ranges(N, nchunk)[-1][0]:] = False
    if mut == "ragged":
        sel[nchunk * (N // nchunk):] = False
    chan = torch.ones(C, dtype=dtype)
    if mut == "last_quad":
        chan[-4:] = 0
    stat_on = torch.ones(N, dtype=torch.bool) if mut == "all_pixels" else on
    if mut == "all_pixels":
        n = N
    out = {}
    if training:
        w = (stat_on & sel).to(dtype)[:, None]
        mean = (z * w).sum(0) * chan / n
        if mut is None:
            var = (((z - mean) ** 2) * w).sum(0) / n                        # the definition
        else:
            var = ((z * z * w).sum(0) * chan / n - mean * mean).clamp_min(0)   # what the kernel makes of its two sums
        rstd = 1 / torch.sqrt(var + EPS)
        if c["run"]:
            out["run_mean"] = (1 - MOM) * t("rm") + MOM * mean
            out["run_var"] = (1 - MOM) * t("rv") + MOM * var * n / (n - 1)
    else:
        mean, rstd = t("rm"), 1 / torch.sqrt(t("rv") + EPS)
        out["run_mean"], out["run_var"] = t("rm"), t("rv")
    zhat = (z - mean) * rstd
    inactive = t("fill").expand(N, C) if c["fill"] else torch.zeros(N, C, dtype=dtype)
    v = torch.where(on[:, None], zhat * gamma + beta, inactive)
    sb = t("s").repeat_interleave(H * W)[:, None] if c["ss"] else torch.ones(N, 1, dtype=dtype)
    v = v * sb
    if c["res"]:
        v = v + t("res").reshape(N, C)
    y = v.clamp_min(0) if act == 1 else v.clamp(0, 6) if act == 2 else v
    ya = y if y_impl is None else y_impl.reshape(N, C).to(dtype)
    slope = (ya > 0) if act == 1 else ((ya > 0) & (ya < 6)) if act == 2 else torch.ones(N, C, dtype=torch.bool)
    g0 = dy * slope.to(dtype)
    g = g0 * sb
    w_on, w_off = (on & sel).to(dtype)[:, None], (~on & sel).to(dtype)[:, None]
    dbeta, dgamma = (g * w_on).sum(0) * chan, (g * zhat * w_on).sum(0) * chan
    k0, k1 = (dbeta / n, dgamma / n) if training else (torch.zeros(C, dtype=dtype),) * 2
    dz = torch.where(on[:, None], gamma * rstd * (g - k0 - zhat * k1), torch.zeros(N, C, dtype=dtype))
    out.update(y=y.view(B, H, W, C), mean=mean, rstd=rstd, dz=dz.view(B, H, W, C), dgamma=dgamma, dbeta=dbeta)
    if c["dres"]:
        out["dres"] = g0.view(B, H, W, C)
    if c["fill"]:
        out["dfill"] = (g * w_off).sum(0) * chan
    return out


def bn_limits(name, ref, y_impl=None):
    """per result: 2e-5, or for the yardstick cases max(2e-5, 4 x torch fp32's distance from float64) -> {key: (limit, torch's distance or None)}"""
    if not BN_CASES[name]["yardstick"]:
        return {k: (BN_LIMIT, None) for k in ref}
    yard = bn_ref(name, dtype=torch.float32, y_impl=y_impl)
    return {k: (max(BN_LIMIT, 4 * rel(yard[k], ref[k])), rel(yard[k], ref[k])) for k in ref}


# ---------------------------------------------------------------------------------------------------------------- convolution family
CONV_CASES = {
    # (Cin, Cout, K, transposed, B, H, W, bias): the edge. Every case runs forward, input gradient, weight gradient (and bias gradient)
    # the scalar gather path (Cs, Cd or Cg no multiple of 4) with 3x3 taps
    (6, 3, 3, 0, 2, 5, 4, True): "scalar path, 3x3, both channel counts ragged",
    (1, 7, 3, 0, 2, 5, 4, False): "scalar path, one source channel",
    (17, 5, 3, 0, 5, 7, 1, True): "35 pixels: Z = 2 over 18 steps, a last step of one channel",
    (72, 72, 3, 0, 2, 3, 5, False): "30 pixels: Z = 4 with step ranges 11/11/11/12, partial second 64-channel tiles in both directions",
    (1025, 64, 3, 0, 2, 3, 4, True): "24 pixels: Z = 32 over 585 steps (uneven ranges) on the scalar path",
    (2050, 128, 1, 0, 2, 1, 2, True): "4 pixels: Z = 16 over 129 steps",
    (8, 4, 3, 0, 2, 4, 8, False): "exactly 64 pixels: one full pixel tile",
    (8, 4, 3, 0, 5, 13, 1, False): "65 pixels: a second tile of one pixel",
    # ConvTranspose2d with Cin != Cout: a [Cin][Cout] / [Cout][Cin] mix-up shows
    (12, 20, 4, 1, 2, 3, 5, True): "transposed, non-square, Cin != Cout",
    (20, 6, 4, 1, 2, 3, 5, True): "transposed, Cout no multiple of 4",
    (20, 72, 4, 1, 5, 7, 1, True): "transposed, 140 output pixels: Z = 4, a partial second channel tile",
    # the weight gradient's pixel ranges
    (4, 1, 1, 0, 5, 13, 65, True): "4225 pixels: P at its cap of 64, ranges of 66 or 67 pixels (no multiple of the 16-pixel step)",
    (8, 4, 3, 0, 127, 1, 1, False): "127 pixels: P = 1, the last below P's first step",
    (8, 4, 3, 0, 2, 8, 8, False): "128 pixels: P = 2",
    # the bias gradient: rows = 256 / C with idle threads, one channel, C = 256
    (4, 1, 1, 0, 2, 3, 5, True): "bias gradient C = 1",
    (4, 3, 1, 0, 2, 3, 5, True): "bias gradient C = 3: rows 85, one idle thread",
    (4, 24, 1, 0, 2, 3, 5, True): "bias gradient C = 24: rows 10, 16 idle threads",
    (4, 96, 1, 0, 2, 3, 5, True): "bias gradient C = 96: rows 2, 64 idle threads",
    (4, 255, 1, 0, 2, 3, 5, True): "bias gradient C = 255: one row, one idle thread",
    (4, 256, 1, 0, 2, 3, 5, True): "bias gradient C = 256",
    (4, 24, 1, 0, 3, 15, 17, True): "bias gradient over 765 pixels: 2 ragged chunks of 383 and 382",
    (8, 8, 4, 1, 2, 129, 258, True): "266256 output pixels: the bias gradient's cap, 256 chunks of 1041, the last 801",
}
CONV_ROLES = ("y", "dx", "dw", "db")


def conv_id(case):
    return "x".join(map(str, case[:7])) + ("b" if case[7] else "")


def conv_geom(case):
    """-> stride, pad, (Ho, Wo), weight shape. H, W: the layer's input size; a ConvTranspose2d 4/2/1 doubles it"""
    Cin, Cout, K, tc, B, H, W, _ = case
    return (2, 1, (2 * H, 2 * W), (Cin, Cout, K, K)) if tc else (1, K // 2, (H, W), (Cout, Cin, K, K))


def conv_plan(case):
    """-> Z and step count of the forward (y) and the input gradient (dx), P of the weight gradient, the bias gradient's chunks"""
    Cin, Cout, K, tc, B, H, W, bias = case
    _, _, (Ho, Wo), _ = conv_geom(case)
    Zy, ny = conv_split(B * Ho * Wo, Cout, Cin, K)
    Zd, nd = conv_split(B * H * W, Cin, Cout, K)
    Cd, Cg = (Cin, Cout) if tc else (Cout, Cin)            # cddpm_ops.hip:968
    return dict(Zy=Zy, steps_y=ny, Zdx=Zd, steps_dx=nd, P=wgrad_parts(B * H * W, Cd, Cg, K), db_chunks=chan_sum_chunks(B * Ho * Wo, Cout) if bias else 0)


@functools.lru_cache(maxsize=None)
def conv_operands(case, kind):
    """-> x [B,Cin,H,W], w, bias [Cout], dy [B,Cout,Ho,Wo] (NCHW, float64). integer: values in -2..2"""
    Cin, Cout, K, tc, B, H, W, _ = case
    _, _, (Ho, Wo), wshape = conv_geom(case)
    g = _gen("conv", case, kind)
    if kind == "integer":
        r = lambda *s: torch.randint(-2, 3, s, generator=g).double()
        return r(B, Cin, H, W), r(*wshape), r(Cout), r(B, Cout, Ho, Wo)
    return _randn(g, B, Cin, H, W), (_randn(g, *wshape) / (Cin * K * K) ** 0.5).float().double(), 0.3 * _randn(g, Cout), _randn(g, B, Cout, Ho, Wo)


def integer_sum_bound(case):
    """no partial sum of the integer run exceeds this: |x|, |w|, |dy|, |b| <= 2, at most K K Cs terms per output element and at most as
    many terms as pixels per weight-gradient element"""
    Cin, Cout, K, tc, B, H, W, _ = case
    return 4 * max(K * K * Cin, K * K * Cout, B * H * W) + 2


def _corr(big, wt, s, p, hs, ws):
    """out[n,a,i,j] = sum_{b,ky,kx} big[n,b,i s + ky - p, j s + kx - p] wt[a,b,ky,kx] (zero outside)"""
    K = wt.shape[-1]
    bp = F.pad(big, (p, p, p, p))
    out = torch.zeros(big.shape[0], wt.shape[0], hs, ws, dtype=big.dtype)
    for ky in range(K):
        for kx in range(K):
            out += torch.einsum("nbij,ab->naij", bp[:, :, ky:ky + s * hs:s, kx:kx + s * ws:s], wt[:, :, ky, kx])
    return out


def _scat(small, wt, s, p, Hb, Wb):
    """out[n,b,i s + ky - p, j s + kx - p] += small[n,a,i,j] wt[a,b,ky,kx]: the adjoint of _corr"""
    K, (hs, ws) = wt.shape[-1], small.shape[2:]
    out = torch.zeros(small.shape[0], wt.shape[1], Hb + 2 * p, Wb + 2 * p, dtype=small.dtype)
    for ky in range(K):
        for kx in range(K):
            out[:, :, ky:ky + s * hs:s, kx:kx + s * ws:s] += torch.einsum("naij,ab->nbij", small, wt[:, :, ky, kx])
    return out[:, :, p:p + Hb, p:p + Wb]


def _wg(small, big, s, p, K):
    """dW[a,b,ky,kx] = sum_{n,i,j} small[n,a,i,j] big[n,b,i s + ky - p, j s + kx - p]"""
    hs, ws = small.shape[2:]
    bp = F.pad(big, (p, p, p, p))
    out = torch.zeros(small.shape[1], big.shape[1], K, K, dtype=small.dtype)
    for ky in range(K):
        for kx in range(K):
            out[:, :, ky, kx] = torch.einsum("naij,nbij->ab", small, bp[:, :, ky:ky + s * hs:s, kx:kx + s * ws:s])
    return out


def _drop_pixels(t, start):
    """NCHW t with the pixels of flat NHWC index >= start zeroed"""
    n, c, h, w = t.shape
    keep = (torch.arange(n * h * w) < start).view(n, 1, h, w)
    return t * keep


def _step_keep(Cs, K, Z, nstep):
    """[Cs][K K] float: 0 where step = tap nck + cs / 16 lies in the last of the Z step ranges"""
    nck = (Cs + 15) // 16
    step = torch.arange(K * K).view(1, -1) * nck + (torch.arange(Cs) // 16).view(-1, 1)
    s0, s1 = step_ranges(nstep, Z)[-1]
    return (~((step >= s0) & (step < s1))).double()


def conv_mutations(case):
    Cin, Cout, K, tc, B, H, W, bias = case
    pl = conv_plan(case)
    _, _, (Ho, Wo), _ = conv_geom(case)
    out = []
    if Cin % 16 or Cout % 16:
        out.append("tail16")
    if Cin % 4 or Cout % 4:
        out += ["tail4", "wgrad_tail4"]
    if pl["Zy"] > 1 or pl["Zdx"] > 1:
        out.append("split_last")
    if pl["P"] > 1:
        out.append("wgrad_last_range")
    if tc and Cin != Cout:
        out.append("transposed_weight")
    if bias and pl["db_chunks"] > 1:
        out.append("db_last_chunk")
        if (B * Ho * Wo) % pl["db_chunks"]:
            out.append("db_ragged")
    return out


@functools.lru_cache(maxsize=None)
def conv_ref(case, kind, mut=None):
    """float64 from the definitions -> {y [B,Cout,Ho,Wo], dx [B,Cin,H,W], dw (PyTorch layout), db}. With wt [a][b][K][K] the layer's weight:
    Conv2d (a = Cout): y = corr(x, wt) + bias, dx = scat(dy, wt), dW = wg(dy, x); ConvTranspose2d (a = Cin): y = scat(x, wt) + bias,
    dx = corr(dy, wt), dW = wg(x, dy). mut: the last Cs % 16 / Cs % 4 source channels of a gather dropped (tail16 / tail4), the last Cd % 4 or
    Cg % 4 channels of the weight gradient dropped, the last step range of a contraction split dropped, the last pixel range of the weight
    gradient dropped, the transposed weight read as [Cout][Cin], the last chunk / the ragged remainder of the bias gradient dropped"""
    Cin, Cout, K, tc, B, H, W, bias = case
    s, p, (Ho, Wo), wshape = conv_geom(case)
    x, w, b, dy = conv_operands(case, kind)
    pl = conv_plan(case)

    def gather_weight(Cs, Z, nstep, cs_axis):
        """the weight a mutated gather over Cs source channels sees; cs_axis: the axis of w that is the source channel"""
        keep = torch.ones(Cs, K * K, dtype=torch.float64)
        if mut in ("tail16", "tail4"):
            m = 16 if mut == "tail16" else 4
            keep[Cs - Cs % m:] = 0
        if mut == "split_last" and Z > 1:
            keep = _step_keep(Cs, K, Z, nstep)
        keep = keep.view(Cs, 1, K, K) if cs_axis == 0 else keep.view(1, Cs, K, K)
        wt = w
        if mut == "transposed_weight":
            wt = w.reshape(Cout, Cin, K, K).permute(1, 0, 2, 3)
        return wt * keep

    # the forward contracts over Cin, the input gradient over Cout; Conv2d: w[Cout][Cin], ConvTranspose2d: w[Cin][Cout]
    wy = gather_weight(Cin, pl["Zy"], pl["steps_y"], 0 if tc else 1)
    wd = gather_weight(Cout, pl["Zdx"], pl["steps_dx"], 1 if tc else 0)
    small, big = (x, dy) if tc else (dy, x)
    if mut == "wgrad_last_range":
        small = _drop_pixels(small, pixel_ranges(B * H * W, pl["P"])[-1][0])
    if tc:
        y, dx = _scat(x, wy, s, p, Ho, Wo), _corr(dy, wd, s, p, H, W)
    else:
        y, dx = _corr(x, wy, s, p, Ho, Wo), _scat(dy, wd, s, p, H, W)
    dw = _wg(small, big, s, p, K)
    if mut == "wgrad_tail4":
        dw = dw.clone()
        dw[dw.shape[0] - dw.shape[0] % 4:] = 0
        dw[:, dw.shape[1] - dw.shape[1] % 4:] = 0
    if mut == "transposed_weight":
        dw = dw.permute(1, 0, 2, 3).contiguous().view(wshape)
    out = dict(y=y + (b.view(1, -1, 1, 1) if bias else 0), dx=dx, dw=dw)
    if bias:
        M, nchunk = B * Ho * Wo, pl["db_chunks"]
        d = dy
        if mut == "db_last_chunk":
            d = _drop_pixels(dy, chunk_ranges(M, nchunk)[-1][0])
        if mut == "db_ragged":
            d = _drop_pixels(dy, nchunk * (M // nchunk))
        out["db"] = d.sum(dim=(0, 2, 3))
    return out


# ---------------------------------------------------------------------------------------------------------------- loss
LOSS_CASES = {
    # name: (B, H, W, f, mask, (w_mask, w_l1), drec). In every case rec == inp exactly at a tenth of the pixels (sign(0) = 0)
    # total 9639: chunks of 4820 and 4819 with the boundary inside a row; ch = 17 != cw = 21
    "ragged_mixed_1_0": (3, 51, 63, 3, "mixed", (1.0, 0.0), True),
    "ragged_mixed_0_1": (3, 51, 63, 3, "mixed", (0.0, 1.0), True),
    "ragged_mixed_half_1": (3, 51, 63, 3, "mixed", (0.5, 1.0), True),
    "ragged_all_masked": (3, 51, 63, 3, "all_masked", (0.5, 1.0), True),
    "ragged_nothing_masked": (3, 51, 63, 3, "nothing_masked", (0.5, 1.0), True),
    "ragged_no_gradient": (3, 51, 63, 3, "mixed", (0.5, 1.0), False),            # drec_dev = NULL: the scalars are unchanged
    # 320 cells: count_active_cells' second trip; total 1280 < 4096: one chunk
    "cells320_below_4096": (5, 16, 16, 8, "mixed", (0.5, 1.0), True),
    # the cap: 256 chunks of 4113, the last 3861
    "cap256": (1, 1026, 1026, 2, "mixed", (0.5, 1.0), True),
}


@functools.lru_cache(maxsize=None)
def loss_operands(name):
    B, H, W, f, mask, _, _ = LOSS_CASES[name]
    g = _gen("loss", B, H, W, f, mask)
    rec, inp = _randn(g, B, H, W), torch.rand(B, H, W, generator=g, dtype=torch.float64).float().double()
    tie = torch.rand(B, H, W, generator=g) < 0.1
    rec = torch.where(tie, inp, rec)
    if mask == "mixed":
        active = random_cells(g, B, f, 0.4)
        if B * f * f > 256:
            active.view(-1)[-3:] = torch.tensor([True, False, True])       # cells beyond index 255 of both kinds
    else:
        active = torch.full((B, f, f), mask == "nothing_masked")
    return rec, inp, active


def loss_plan(name):
    B, H, W, f = LOSS_CASES[name][:4]
    ranges = chunk_ranges(B * H * W, loss_chunks(B * H * W))
    return dict(total=B * H * W, cells=B * f * f, chunks=len(ranges), ranges=ranges)


def loss_mutations(name):
    B, H, W, f, mask, (wm, wl), drec = LOSS_CASES[name]
    pl = loss_plan(name)
    out = []
    if pl["cells"] > 256 and mask != "nothing_masked" and wm:
        out.append("count255")
    if H // f != W // f and mask == "mixed":
        out.append("swap")
    if pl["chunks"] > 1:
        out.append("last_chunk")
    if pl["total"] % pl["chunks"]:
        out.append("ragged")
    if wl and drec:
        out.append("sign0")
    return out


def loss_ref(name, mut=None):
    """masked = sum over the pixels of masked cells of (rec - inp)^2 / (ch cw (n_masked + 1e-8)), l1 = mean |rec - inp|,
    drec = d (w_mask masked + w_l1 l1) / d rec (Spark_2D.py:180-199 with pix_norm 0) -> (masked, l1, drec [B,H,W])"""
    B, H, W, f, _, (wm, wl), _ = LOSS_CASES[name]
    rec, inp, active = loss_operands(name)
    total, pl = B * H * W, loss_plan(name)
    masked = ~cell_mask(active, H, W, swap=mut == "swap")
    cells = active.reshape(-1)
    n_masked = cells.numel() - int((cells[:256] if mut == "count255" else cells).sum())
    sel = torch.ones(total, dtype=torch.bool)
    if mut == "last_chunk":
        sel[pl["ranges"][-1][0]:] = False
    if mut == "ragged":
        sel[pl["chunks"] * (total // pl["chunks"]):] = False
    sel = sel.view(B, H, W)
    d = rec - inp
    den = (H // f) * (W // f) * (n_masked + 1e-8)
    l_mask, l_l1 = (d * d * (masked & sel)).sum() / den, (d.abs() * sel).sum() / total
    sign = torch.sign(d) if mut != "sign0" else torch.where(d >= 0, 1.0, -1.0).double()
    drec = (wm * 2 * d * masked / den + wl * sign / total) * sel
    return l_mask, l_l1, drec


# ---------------------------------------------------------------------------------------------------------------- mask multiply
MASK_MUL_CASES = [
    # (B, H, W, C, f)
    (33, 3, 3, 5, 3),        # 297 cells; C no multiple of 4
    (2, 6, 9, 1, 3),         # one channel; ch = 2 != cw = 3
    (3, 8, 12, 6, 4),        # C = 6; ch = 2 != cw = 3; more than one workgroup
]


def mask_mul_operands(case):
    B, H, W, C, f = case
    g = _gen("mask_mul", case)
    return _randn(g, B, H, W, C), random_cells(g, B, f)


def mask_mul_ref(case, mut=None):
    x, active = mask_mul_operands(case)
    return x * cell_mask(active, case[1], case[2], swap=mut == "swap").unsqueeze(-1)


# ---------------------------------------------------------------------------------------------------------------- AdamW
# adam_guarded_kernel (train_kernels.hip:1334-1352) takes one element per thread in workgroups of 256, no vector accesses: n on either side
# of 256 and of 2 x 256; grad_check_kernel beside it (:1313-1322) reads float4 with a scalar tail of n & 3: n on either side of 4
ADAM_LENGTHS = (1, 3, 4, 5, 255, 256, 257, 511, 513, 1027)
ADAM_HYPER = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
ADAM_CASES = [(n, wd, 0.5) for n in ADAM_LENGTHS for wd in (0.05, 0.0)]        # (n, weight_decay, grad_unscale)
ADAM_STEPS = 3


@functools.lru_cache(maxsize=None)
def adam_operands(n):
    """-> p0 [n], the gradients of ADAM_STEPS served steps [steps][n] (as stored: before the unscale), a gradient with an inf"""
    g = _gen("adamw", n)
    p0, grads, bad = _randn(g, n), _randn(g, ADAM_STEPS, n) * 2.0, _randn(g, n)
    bad[n // 2] = float("inf")
    return p0, grads, bad


def adam_ref(case, mut=None):
    """torch.optim.AdamW's rule written out: p <- p (1 - lr wd); m, v moments of g = grad unscale; p <- p - lr / (1 - b1^t) m / (sqrt(v) /
    sqrt(1 - b2^t) + eps); then a step whose gradient holds an inf: nothing moves (mut decay_on_skip: the decay is applied all the same)"""
    n, wd, unscale = case
    lr, (b1, b2), eps = ADAM_HYPER["lr"], ADAM_HYPER["betas"], ADAM_HYPER["eps"]
    p0, grads, _ = adam_operands(n)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, ADAM_STEPS + 1):
        g = grads[t - 1] * unscale
        p = p * (1 - lr * wd)
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    if mut == "decay_on_skip":
        p = p * (1 - lr * wd)
    return p, m, v
