"""The fused convolution's two epilogue paths (csrc/conv_x6.hip): a workgroup whose 8 x 32 tile lies inside the image requests its residual
and stores its tile without per-lane predicates, a ragged one keeps the masked code. Shapes at which each path occurs alone and both in
one launch:
    8 x 32   one full tile                                  full path alone
    16 x 40  a full tile column beside a ragged one         both paths in one launch
    12 x 20  all ragged                                     masked path alone
    16 x 64  four full tiles                                records of two 4-row bands per tile
(the grid the tiles cover; the folded upsample runs on the half-resolution grid, so its OUTPUT is 2H x 2W). B = 2, 128 channels.

Per shape, through cddpm_op_conv_planned with the helpers, float64 references and bounds of tests/test_gpu_conv_planned.py /
conv_plan_cases.py (no tolerance of its own): every call into a sentinel-filled buffer whose margins must come back untouched, against
float64 element by element, and slice b of the B = 2 call bit-equal to its B = 1 call. 3x3 with and without residual, with and without
statistics; the folded 2x2 form with a half-resolution residual; 1x1; a split-K plan (plane stores and the combine); a precision-16
handle; an x6-family handle. The statistics RECORDS are guarded through cddpm_op_conv_packed, which takes their buffer from the caller.

Bit-identity with the commit before the full-tile path: tests/golden/conv_bits_epilogue_parent.json holds the digests tools/conv_bits.py
--set epilogue printed with a build of that commit; recomputed here with the product library, the 256-cout plan (CDDPM_NB2=force, read
once per process) in a child."""
import importlib.util
import json
import os

import pytest
import torch

import conv_plan_cases as P
import test_gpu_conv_planned as T
from conftest import GOLD, ROOT

engines = T.engines            # the module-scoped handle cache of the planned-convolution tests, an instance of its own here

SHAPES = {"8x32": (8, 32), "16x40": (16, 40), "12x20": (12, 20), "16x64": (16, 64)}
FULL = {"8x32": [[True]], "16x40": [[True, False], [True, False]], "12x20": [[False], [False]], "16x64": [[True, True], [True, True]]}
GEOM_U = (16, 64, 128)         # >= 512 workgroups at the maximum geometry for every case below: K is not split
C = 128                        # the smallest channel counts the entries accept (Cout a multiple of 128)


def full_tiles(H, W):
    """conv_x6.hip: full = (y0 + 8 <= gridH) && (x0 + 32 <= gridW), per tile (ty, tx)"""
    return [[(8 * ty + 8 <= H) and (32 * tx + 32 <= W) for tx in range((W + 31) // 32)] for ty in range((H + 7) // 8)]


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_take_the_paths_they_are_listed_for(shape):
    assert full_tiles(*SHAPES[shape]) == FULL[shape]


def case_of(shape, kind, *, res=False, stats=False, geom=GEOM_U):
    H, W = SHAPES[shape]
    name = f"epilogue_{kind}_{shape}{'_res' if res else ''}{'_gn' if stats else ''}{'_split' if geom != GEOM_U else ''}"
    gn = 10.0 if stats else None
    if kind == "folded":
        c = P._c(name, geom, (2 * H, 2 * W), 2, 2 * H, 2 * W, C, C, 3, coef=True, silu=True, folded=True, res="up", gn_ratio=gn, expect_S=0)
    elif kind == "1x1":
        c = P._c(name, geom, (H, W), 2, H, W, C, C, 1, coef=True, res="same" if res else None, gn_ratio=gn, expect_S=0)
    else:
        c = P._c(name, geom, (H, W), 2, H, W, C, C, 3, coef=True, silu=True, res="same" if res else None, gn_ratio=gn, expect_S=0)
    return c


def check(eng, case, *, split=False, **kw):
    c = dict(case, expect_S=P.case_plan(case, kw.get("family", "h3"))[1])
    assert (c["expect_S"] > 1) == split, (c["name"], c["expect_S"])
    return T.check_case(eng, c, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True], ids=["", "stats"])
@pytest.mark.parametrize("res", [False, True], ids=["", "res"])
@pytest.mark.parametrize("shape", SHAPES)
def test_3x3(engines, shape, res, stats):
    check(engines(GEOM_U), case_of(shape, "3x3", res=res, stats=stats))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_folded_upsample_with_half_resolution_residual(engines, shape):
    check(engines(GEOM_U), case_of(shape, "folded", stats=True))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_1x1(engines, shape):
    check(engines(GEOM_U), case_of(shape, "1x1", res=True))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_split_k_plane_stores_and_combine(engines, shape):
    """a handle of max_batch 2 at the layer's own size: S > 1, the kernel stores raw planes, conv_reduce_kernel adds bias and residual"""
    H, W = SHAPES[shape]
    geom = (2, H, W)
    check(engines(geom), case_of(shape, "3x3", res=True, stats=True, geom=geom), split=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_precision16_handle(engines, shape):
    check(engines(GEOM_U, "p16"), case_of(shape, "3x3", res=True), bits=16)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_x6_family_handle(engines, shape):
    check(engines(GEOM_U, "x6"), case_of(shape, "3x3", res=True, stats=True), family="x6")


# ---- the statistics records in a guarded buffer ------------------------------------------------------------------------------------------
def _packed_call(eng, B, H, W, folded, x, coef, img, wexp, bias, res, guarded=True):
    """cddpm_op_conv_packed with out and the records in the middle of sentinel-filled buffers -> (out bits, record bits)"""
    lib, p = eng.lib, (lambda t: None if t is None else t.data_ptr())
    nrec = lib.cddpm_stat_records(H, W, 1 if folded else 0)
    n_out, n_rec, M = B * H * W * C, B * nrec * C * 2, T.MARGIN
    bufs = [torch.full((M + n + M,), T.SENTINEL, dtype=torch.int32, device="cuda") for n in (n_out, n_rec)]
    out, rec = (b[M:M + n].view(torch.float32) for b, n in zip(bufs, (n_out, n_rec)))
    rc = lib.cddpm_op_conv_packed(eng._h, p(x), C, None, 0, p(coef), 1, int(folded), p(img), wexp, p(bias), C, 3, p(res), int(folded), None, 0,
                                  None, 0, None, p(out), p(rec), B, H, W, None)
    assert rc == 0, lib.cddpm_last_error(eng._h)
    torch.cuda.synchronize()
    for b, n, what in zip(bufs, (n_out, n_rec), ("output", "statistics records")):
        assert bool((b[:M] == T.SENTINEL).all()) and bool((b[M + n:] == T.SENTINEL).all()), f"a margin of the {what} was written"
        assert not bool((b[M:M + n] == T.SENTINEL).any()), f"part of the {what} was not written"
    return bufs[0][M:M + n_out].view(B, H, W, C).clone(), bufs[1][M:M + n_rec].view(B, nrec, C, 2).clone()


@pytest.mark.gpu
@pytest.mark.parametrize("folded", [False, True], ids=["3x3", "folded"])
@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_records_stay_inside_their_buffer(engines, shape, folded):
    """out and the records between sentinel margins; every record written; slice b of the B = 2 call equals its B = 1 call, records
    included; and the output equals, bit for bit, the planned entry's on the same inputs (one kernel, one packed image)"""
    eng = engines(GEOM_U)
    case = case_of(shape, "folded" if folded else "3x3", res=True)
    d = P.make_inputs(case)
    H, W = case["H"], case["W"]
    ref_out, _, plan = T.run(eng, case, d)
    wexp = plan["scale_exp"]
    wd = d["wt"].cuda().contiguous()
    taps = 4 if folded else 9
    img = torch.zeros((4 if folded else 1) * eng.lib.cddpm_packed_conv_bytes(C, C, taps), dtype=torch.uint8, device="cuda")
    assert eng.lib.cddpm_op_pack_conv(eng._h, wd.data_ptr(), C, C, 3, 2 if folded else 0, wexp, img.data_ptr(), None) == 0, eng.lib.cddpm_last_error(eng._h)
    x, res, coef, bias = T.nhwc(d["x"]), T.nhwc(d["res"]), d["coef"].cuda().contiguous(), d["bias"].cuda()
    out, rec = _packed_call(eng, 2, H, W, folded, x, coef, img, wexp, bias, res)
    assert torch.equal(T.nchw(out.view(torch.float32)).view(torch.int32), ref_out.view(torch.int32))
    for b in range(2):
        o1, r1 = _packed_call(eng, 1, H, W, folded, x[b:b + 1].contiguous(), coef[:, b:b + 1].contiguous(), img, wexp, bias, res[b:b + 1].contiguous())
        assert torch.equal(o1[0], out[b]) and torch.equal(r1[0], rec[b]), f"slice {b} depends on the batch it is in"


# ---- bit-identity with the parent commit ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLD, "conv_bits_epilogue_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tool(parent):
    spec = importlib.util.spec_from_file_location("conv_bits", os.path.join(ROOT, "tools", "conv_bits.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    assert parent["seed"] == t.SEED and parent["shapes"] == {k: list(v) for k, v in t.EPILOGUE_SHAPES.items()}      # the digests are of THESE inputs
    assert parent["ops"] == {k: list(v) for k, v in t.EPILOGUE_OPS.items()} and t.EPILOGUE_SHAPES == SHAPES
    return t


def _compare(got, want):
    assert sorted(got) == sorted(want)
    bad = [name for name in want if got[name] != want[name]]
    assert not bad, f"digests differ from the parent commit's: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "p16", "x6"])
def test_epilogue_bits_equal_parent(tool, parent, mode, monkeypatch):
    monkeypatch.delenv("CDDPM_NB2", raising=False)
    _compare(tool.epilogue_digests(mode), parent["modes"][mode])


@pytest.mark.gpu
def test_epilogue_bits_equal_parent_256_cout_plan(tool, parent):
    _compare(tool.digests_in_child("nb2", "epilogue"), parent["modes"]["nb2"])
