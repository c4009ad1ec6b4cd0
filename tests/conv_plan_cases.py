"""The fused convolution as a HANDLE plans it (csrc/cddpm_api.hip::conv_launch): the planning arithmetic written out again in plain
Python, the cases of tests/test_gpu_conv_planned.py with their inputs, and their float64 references and error bounds. Pure torch /
Python on the CPU; tests/test_conv_plan_host.py pins the port to the library, tests/test_conv_plan_cases_host.py the references to
torch's own operators.

Error bound of a precision-32 call, element by element (S = the split-K factor the plan took, s1 = sum |a||w| over the element's whole
contraction, main and skip segment):
    conv_bound                      2^-20 s1 (+ 2^-24 sum |w| in the h3 family): tests/test_gpu_kernels.py::conv_bound, per segment
  + 2^-20 s1(main)                  where `coef` is used: the device evaluates the affine + SiLU transform in fp32
                                    (test_conv_domain_mixed_magnitudes_and_weight_outliers)
  + 2^-23 |ref|                     the store
  + (S + 1) 2^-24 (s1 + |bias| + |res|)
                                    the combine: conv_reduce_kernel performs S - 1 plane adds, one bias add and one residual add, S + 1
                                    fp32 additions in a fixed order. Every partial result is a sum of a subset of the element's terms
                                    (plane sums, bias, residual), so its magnitude is at most s1 + |bias| + |res| (up to the planes' own
                                    rounding, which conv_bound covers), and each addition rounds to at most 2^-24 of its result. With
                                    S = 1 the convolution's own epilogue does the bias and residual adds: the same term with S = 1.
Precision 16 (a handle at cddpm_set_precision(h, 16)): conv_p16_reference.py::p16_forward_ref and its bound."""
import torch
import torch.nn.functional as F

from conv_p16_reference import p16_forward_ref

MAX_KSPLIT = 8
FAMILY_CODE = {"f32": 0, "x6": 1, "h3": 2}
PLANE_FLOATS = 256 * 256 * 128          # the handle's split-K plane workspace (csrc/cddpm_ctx.h::KSPLIT_PLANE_FLOATS)


# ---- the plan, in plain Python ----------------------------------------------------------------------------------------------------------
def ksplit_rule(family, workgroups, Cin, Cskip, taps):
    """cddpm_api.hip::ksplit_rule -> (S, kbound[0 .. S]). family: 'h3' | 'x6' | 'f32'; workgroups: of the 128-cout form at the handle's
    maximum geometry; taps: 9, 1, or 4 (folded upsample). The K loop runs over 32-channel chunks, the main segment's (each `taps`
    multiplications per tile) and then the skip segment's (one each)."""
    nch_main, nch_skip = Cin // 32, Cskip // 32
    nch = nch_main + nch_skip
    if family != "h3":
        return 1, [0, nch]
    units = nch_main * taps + nch_skip
    S = 1
    while S < MAX_KSPLIT and workgroups * (S * 2) <= 256 and units // (S * 2) >= 9 and S * 2 <= nch:
        S *= 2
    if S == 1:
        return 1, [0, nch]
    cost = lambda c: taps if c < nch_main else 1
    kb, c, acc = [0], 0, 0
    for j in range(1, S):
        target = units * j // S
        while c < nch - (S - j) and acc + cost(c) // 2 < target:
            acc += cost(c)
            c += 1
        if c <= kb[j - 1]:
            acc += cost(c)
            c += 1
        kb.append(c)
    kb.append(nch)
    return S, kb


def conv_workgroups(Cout, taps, B, H, W):
    """cddpm_ctx.h::conv_workgroups: tiles of 32 x 8 output pixels x 128 couts; the folded upsample (taps 4) runs four parity classes
    on the half-resolution grid"""
    up2 = taps == 4
    gh, gw = (H // 2, W // 2) if up2 else (H, W)
    return B * (4 if up2 else 1) * ((gw + 31) // 32) * ((gh + 7) // 8) * (Cout // 128)


def workgroups_at_max(geom, img_hw, Cout, taps, H, W):
    """cddpm_api.hip::conv_workgroups_at_max: the layer's extent scaled by maximum / current image size, at max_batch.
    geom = (max_batch, max_h, max_w)"""
    mb, mh, mw = geom
    return conv_workgroups(Cout, taps, mb, H * mh // img_hw[0], W * mw // img_hw[1])


def nb2_planned(family, wanted, workgroups, Cout, taps, S):
    """256-cout workgroups (cddpm_ctx.h::conv_set_nb2 under NB2_HANDLE_PLAN, CDDPM_NB2 unset; conv_x6.hip::launch_split): h3, unsplit K,
    Cout a multiple of 256, not the 1x1 loop, >= 512 workgroups of the 128-cout form at the maximum geometry, and a step / handle that
    wants them"""
    return bool(wanted and family == "h3" and S == 1 and Cout % 256 == 0 and taps != 1 and workgroups >= 512)


def unet_convs(model_channels, channel_mult, num_res_blocks, attention_resolutions, **_):
    """every convolution conv_launch plans in a forward of this descriptor (cddpm_api.hip::build_program / run_res / run_attn):
    -> [(name, Cin, Cskip, Cout, taps, ds of the OUTPUT)]"""
    C, out = model_channels, []

    def res(name, cin, cout, ds, up=False, down=False):
        ds_out = ds * 2 if down else ds // 2 if up else ds
        out.append((name + ".in_layers.2", cin, 0, cout, 4 if up else 9, ds_out))
        out.append((name + ".out_layers.3", cout, cin if cin != cout else 0, cout, 9, ds_out))

    def attn(name, c, ds):
        out.append((name + ".qkv", c, 0, 3 * c, 1, ds))
        out.append((name + ".proj_out", c, 0, c, 1, ds))

    chans, ch, ds, idx = [C], C, 1, 1
    for level, mult in enumerate(channel_mult):
        for _i in range(num_res_blocks):
            res(f"input_blocks.{idx}.0", ch, mult * C, ds)
            ch = mult * C
            if ds in attention_resolutions:
                attn(f"input_blocks.{idx}.1", ch, ds)
            chans.append(ch)
            idx += 1
        if level != len(channel_mult) - 1:
            res(f"input_blocks.{idx}.0", ch, ch, ds, down=True)
            ds *= 2
            chans.append(ch)
            idx += 1
    res("middle_block.0", ch, ch, ds)
    attn("middle_block.1", ch, ds)
    res("middle_block.2", ch, ch, ds)
    idx = 0
    for level in reversed(range(len(channel_mult))):
        co = channel_mult[level] * C
        for i in range(num_res_blocks + 1):
            res(f"output_blocks.{idx}.0", ch + chans.pop(), co, ds)
            ch, sub = co, 1
            if ds in attention_resolutions:
                attn(f"output_blocks.{idx}.{sub}", ch, ds)
                sub += 1
            if level > 0 and i == num_res_blocks:
                res(f"output_blocks.{idx}.{sub}", ch, ch, ds, up=True)
                ds //= 2
            idx += 1
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# handles: (max_batch, max_h, max_w)
GEOM_P = (2, 32, 32)          # the small-batch handle of most of the suite: every layer is split
GEOM_R = (2, 48, 80)          # a geometry with a 12 x 20 layer at ds = 4
GEOM_Q = (16, 64, 64)         # the smallest geometry at which a Cout = 256 full-resolution layer has exactly 512 workgroups
GEOM_Q15 = (15, 64, 64)       # one slice fewer: 480


def _c(name, geom, img, B, H, W, C0, Cout, k, *, coef=False, silu=False, folded=False, res=None, S0=0, S1=0, skip_scale=None, gn_ratio=None,
       expect_S, kbound=None, ranges=None):
    return dict(name=name, geom=geom, img=img, B=B, H=H, W=W, C0=C0, Cout=Cout, k=k, coef=coef, silu=silu, folded=folded, res=res, S0=S0, S1=S1,
                skip_scale=skip_scale, gn_ratio=gn_ratio, expect_S=expect_S, kbound=kbound, ranges=ranges)


# expect_S / kbound: what the rule gives TODAY for the case (from the port above; tests/test_conv_plan_host.py pins both to the library).
# The GPU test asserts, before it looks at any number, what the case NEEDS of the plan the launch reports: S, valid ranges, and `ranges`,
# the property of kbound the case exists for (check_ranges) -- so a change of the rule fails the test instead of silently moving the case
# off its path, while any valid bounds with that property still have to give the right numbers: they are data to the kernel.
CASES_P = [
    _c("3x3_128_8x8_plain", GEOM_P, (32, 32), 2, 8, 8, 128, 128, 3, expect_S=4, kbound=[0, 1, 2, 3, 4],
       ranges="one_chunk_each"),
    _c("3x3_256_16x16_act_res", GEOM_P, (32, 32), 2, 16, 16, 256, 256, 3, coef=True, silu=True, res="same", expect_S=8),
    # main 256 (8 chunks of 9 taps) | skip 256 + 128 (12 chunks of 1): range 6 = chunks 7, 8 straddles main / skip, range 7 = chunks 9 .. 19
    # lies inside the skip segment and crosses from skip0 into skip1 at chunk 16
    _c("3x3_256_skip_256_128_16x16", GEOM_P, (32, 32), 2, 16, 16, 256, 256, 3, coef=True, silu=True, S0=256, S1=128, skip_scale=1e3,
       expect_S=8, kbound=[0, 1, 2, 3, 5, 6, 7, 9, 20], ranges="straddle_and_inside_skip"),
    _c("folded_256_16x16_to_32x32_res_up", GEOM_P, (32, 32), 2, 32, 32, 256, 256, 3, coef=True, silu=True, folded=True, res="up", expect_S=2),
    _c("1x1_640_to_128_8x8_res", GEOM_P, (32, 32), 2, 8, 8, 640, 128, 1, res="same", expect_S=2),                    # the 1x1 loop's split
    _c("1x1_256_qkv_8x8", GEOM_P, (32, 32), 2, 8, 8, 256, 768, 1, coef=True, expect_S=1),                           # unsplit, same entry
]
# H % 8, W % 32 and H W % 64 all non-zero: ragged tiles in the convolution, a tail record in the combine (240 = 3 x 64 + 48 pixels)
CASE_RAGGED = _c("3x3_128_to_256_12x20_ragged_gn", GEOM_R, (48, 80), 2, 12, 20, 128, 256, 3, gn_ratio=100.0, expect_S=4)
P16_NAMES = ("3x3_256_16x16_act_res", "3x3_256_skip_256_128_16x16", "folded_256_16x16_to_32x32_res_up")
# Cout = 256 at full resolution, B = 1 calls: 512 workgroups at the maximum geometry of GEOM_Q, 480 at GEOM_Q15's
CASES_Q = [
    _c("3x3_64_to_256_64x64_gn", GEOM_Q, (64, 64), 1, 64, 64, 64, 256, 3, coef=True, silu=True, gn_ratio=10.0, expect_S=1),
    _c("folded_64_to_256_32x32_to_64x64_gn", GEOM_Q, (64, 64), 1, 64, 64, 64, 256, 3, coef=True, silu=True, folded=True, gn_ratio=10.0, expect_S=1),
]
ALL_CASES = CASES_P + [CASE_RAGGED] + CASES_Q


def check_ranges(case, S, kb, prop=True):
    """the chunk bounds a launch reports are usable by the kernel (start at 0, end at the last chunk, no empty range) and, with `prop`
    (the split plan of the default family), have the property the case was written for"""
    nmain, nch = case["C0"] // 32, (case["C0"] + case["S0"] + case["S1"]) // 32
    assert len(kb) == S + 1 and kb[0] == 0 and kb[S] == nch and all(kb[j] < kb[j + 1] for j in range(S)), (case["name"], S, kb)
    if not prop:
        return
    if case["ranges"] == "one_chunk_each":
        assert all(kb[j + 1] - kb[j] == 1 for j in range(S)), (case["name"], kb)
    elif case["ranges"] == "straddle_and_inside_skip":
        assert any(kb[j] < nmain < kb[j + 1] for j in range(S)), (case["name"], kb, "no range straddles the main / skip boundary")
        assert any(kb[j] >= nmain for j in range(S)), (case["name"], kb, "no range lies wholly inside the skip segment")
    else:
        assert case["ranges"] is None


def case_plan(case, family="h3", geom=None):
    """(workgroups at the maximum geometry, S, kbound) of a case by the port"""
    taps = 4 if case["folded"] else case["k"] ** 2
    nwg = workgroups_at_max(geom or case["geom"], case["img"], case["Cout"], taps, case["H"], case["W"])
    S, kb = ksplit_rule(family, nwg, case["C0"], case["S0"] + case["S1"], taps)
    return nwg, S, kb


def make_inputs(case):
    """seeded fp32 CPU tensors of a case (NCHW): x, coef [3,B,Cin] | None, wt, bias, res | None, skip [B, S0 + S1, H, W] | None,
    wskip | None, gamma / beta | None"""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, case["name"])))
    rn = lambda *s: torch.randn(*s, generator=g)
    B, H, W, Cin, Cout, k = case["B"], case["H"], case["W"], case["C0"], case["Cout"], case["k"]
    h, w = (H // 2, W // 2) if case["folded"] else (H, W)
    d = dict(x=rn(B, Cin, h, w) * 1.3 + 0.2, wt=rn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5, bias=rn(Cout) * 0.1,
             coef=None, res=None, skip=None, wskip=None, gamma=None, beta=None)
    if case["coef"]:
        d["coef"] = torch.stack([rn(B, Cin) * 0.2, 1 + 0.2 * rn(B, Cin), rn(B, Cin) * 0.2])
    if case["res"] == "same":
        d["res"] = rn(B, Cout, H, W)
    elif case["res"] == "up":
        d["res"] = rn(B, Cout, H // 2, W // 2)
    if case["S0"]:
        Sk = case["S0"] + case["S1"]
        # the RAW residual stream (no GroupNorm in front of the skip_connection): magnitudes of skip_scale .. 10 skip_scale
        d["skip"] = rn(B, Sk, H, W) * case["skip_scale"] * 10.0 ** torch.rand(B, Sk, H, W, generator=g)
        d["wskip"] = rn(Cout, Sk, 1, 1) / Sk ** 0.5
    if case["gn_ratio"] is not None:
        d["bias"] = case["gn_ratio"] * (1 + 0.05 * rn(Cout))            # output sigma ~ 1: |mean| / sigma = gn_ratio
        d["gamma"], d["beta"] = 1 + 0.1 * rn(Cout), 0.1 * rn(Cout)
    return d


def take(d, b):
    """the inputs of the B = 1 call of slice b"""
    out = dict(d)
    for key in ("x", "res", "skip"):
        if d[key] is not None:
            out[key] = d[key][b:b + 1].contiguous()
    if d["coef"] is not None:
        out["coef"] = d["coef"][:, b:b + 1].contiguous()
    return out


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def act64(x, coef, silu):
    v = x.double()
    if coef is not None:
        m, a, dd = (coef[i].double()[:, :, None, None] for i in range(3))
        v = (v - m) * a + dd
    return F.silu(v) if silu else v


def conv_bound(v64, w64, pad, family):
    """tests/test_gpu_kernels.py::conv_bound, the family a parameter (there: the process default)"""
    s1 = F.conv2d(v64.abs(), w64.abs(), None, padding=pad)
    s2 = F.conv2d(torch.ones_like(v64), w64.abs(), None, padding=pad)
    rel, ab = (2.0 ** -18 if family == "f32" else 2.0 ** -20), (2.0 ** -24 if family == "h3" else 0.0)
    return rel * s1 + ab * s2 + 1e-30


def skip64(skip0, skip1, wskip):
    """the two-source skip segment: each source against its own slice of the ONE weight tensor [Cout, S0 + S1, 1, 1]"""
    S0 = skip0.shape[1]
    out = F.conv2d(skip0.double(), wskip.double()[:, :S0])
    if skip1 is not None:
        out = out + F.conv2d(skip1.double(), wskip.double()[:, S0:])
    return out


def reference32(case, d, S, family="h3"):
    """(ref, bound) float64 NCHW of a precision-32 call that took split-K factor S; see the module docstring"""
    pad = case["k"] // 2
    v = act64(d["x"], d["coef"], case["silu"])
    if case["folded"]:
        v = F.interpolate(v, scale_factor=2, mode="nearest")
    w64 = d["wt"].double()
    s1 = F.conv2d(v.abs(), w64.abs(), None, padding=pad)
    ref = F.conv2d(v, w64, d["bias"].double(), padding=pad)
    lim = conv_bound(v, w64, pad, family)
    if case["coef"]:
        lim = lim + 2.0 ** -20 * s1
    add = d["bias"].double().abs()[None, :, None, None].expand_as(ref)
    if d["skip"] is not None:
        S0 = case["S0"]
        sk0, sk1 = d["skip"][:, :S0], (d["skip"][:, S0:] if case["S1"] else None)
        ref = ref + skip64(sk0, sk1, d["wskip"])
        lim = lim + conv_bound(d["skip"].double(), d["wskip"].double(), 0, family)
        s1 = s1 + F.conv2d(d["skip"].double().abs(), d["wskip"].double().abs())
    if d["res"] is not None:
        r = d["res"].double()
        r = F.interpolate(r, scale_factor=2, mode="nearest") if case["res"] == "up" else r
        ref = ref + r
        add = add + r.abs()
    lim = lim + 2.0 ** -23 * ref.abs() + (S + 1) * 2.0 ** -24 * (s1 + add)
    return ref, lim


def reference16(case, d, scale_exp):
    """(ref, bound) of a call on a precision-16 handle: p16_forward_ref with the pre-scale exponent the library reports"""
    return p16_forward_ref(d["x"], d["coef"], case["silu"], d["wt"], scale_exp, case["k"], d["bias"], folded=case["folded"], skip=d["skip"],
                           ws=d["wskip"], res=d["res"], res_up=case["res"] == "up")


def gn_error(out_nchw, coef_out, gamma, beta):
    """largest error of the normalised value the returned (mean, a, d) imply, against float64 GroupNorm32 of the output AS STORED
    (test_groupnorm_statistics_from_the_conv_epilogue_with_large_mean: bound 1e-5 (1 + ratio))"""
    o64, cf = out_nchw.double(), coef_out.double()
    ref = F.group_norm(o64, 32, gamma.double(), beta.double(), eps=1e-5)
    got = (o64 - cf[0][:, :, None, None]) * cf[1][:, :, None, None] + cf[2][:, :, None, None]
    return float((got - ref).abs().max())
