"""Host side of the encoder operator tests (no GPU): the conditions tests/test_gpu_encoder_ops_edges.py rests on. The case tables of
encoder_op_cases.py reach the plans they are there for -- as the library's own size queries state them, not as a formula restated in
Python --, the inputs have the properties the device tests lean on (ties, integer exactness), and the brute-force references agree with
torch's float64 operators bit for bit."""
import pytest
import torch

import encoder_op_cases as EC

# the plans the cases were chosen for, (Z forward, Z input gradient, P) at precision 32 and P at precision 16 (None: role not taken)
CLAIMED = {
    (5, 64, 64, 3, 1, 19, 21): ((4, 4, 16), 15),
    (2, 64, 64, 1, 1, 23, 29): ((1, 1, 16), 10),
    (2, 128, 64, 3, 2, 33, 31): ((8, 4, 8), 4),
    (2, 192, 192, 3, 1, 21, 20): ((4, 4, 13), 6),
    (3, 192, 64, 3, 2, 5, 5): ((8, 4, 1), 1),
    (2, 48, 64, 3, 1, 9, 11): ((2, None, None), None),
    (2, 64, 80, 3, 2, 9, 11): ((None, 4, None), None),
    (3, 64, 64, 3, 1, 7, 9): ((4, 4, 2), 1),
    (3, 128, 64, 1, 1, 5, 6): ((1, 1, 1), 1),
    (3, 512, 2048, 1, 1, 2, 2): ((4, 8, 1), 1),
}


def test_the_table_holds_the_cases_of_the_two_operator_files():
    ops32 = [(3, 64, 64, 3, 1, 7, 9), (3, 64, 128, 3, 2, 9, 7), (3, 128, 64, 1, 1, 5, 6), (3, 64, 128, 1, 2, 8, 5), (3, 256, 64, 3, 2, 4, 4)]
    ops16 = ops32 + [(3, 512, 2048, 1, 1, 2, 2), (3, 2048, 512, 1, 1, 2, 2), (3, 512, 512, 3, 2, 3, 3), (1, 64, 64, 3, 1, 1, 1)]
    assert all(EC.CONV_CASES[c] == "ydw" and EC.p16_accepts(c) for c in ops16)
    assert len(EC.CONV_CASES) == 17 and all(c in EC.CONV_CASES for c in EC.SPLIT_CASES)


@pytest.mark.parametrize("case", list(CLAIMED), ids=EC.conv_id)
def test_a_case_reaches_the_plan_it_is_there_for(case):
    (zy, zd, p), p16 = CLAIMED[case]
    plan = EC.conv_plan(case)
    assert (plan.get("y"), plan.get("d"), plan.get("w")) == (zy, zd, p)
    assert EC.conv_plan(case, 16).get("w") == p16


def test_fp32_forward_and_input_gradient_plans():
    seen, uneven, ragged_tiles = set(), [], []
    for case, roles in EC.CONV_CASES.items():
        plan = EC.conv_plan(case)
        assert set(plan) == set(roles)
        for role in "yd":
            if role not in roles:
                continue
            Z, M, nstep = plan[role], EC.conv_rows(case, role), EC.conv_steps(case, role)
            seen.add(Z)
            if Z > 1 and nstep % Z:
                uneven.append((case, role, nstep, Z))
            if M % 64 and (M + 63) // 64 > 8:
                ragged_tiles.append((case, role, M))
    assert seen == {1, 2, 4, 8}
    assert ((3, 192, 64, 3, 2, 5, 5), "y", 108, 8) in uneven
    assert ((5, 64, 64, 3, 1, 19, 21), "y", 1995) in ragged_tiles and 1995 % 64 == 11 and (1995 + 63) // 64 == 32
    # contraction widths that are multiples of 16 and not of 64, in both roles
    assert any("y" in r and c[1] % 64 and c[1] % 16 == 0 for c, r in EC.CONV_CASES.items())
    assert any("d" in r and c[2] % 64 and c[2] % 16 == 0 for c, r in EC.CONV_CASES.items())
    # a stride-2 input gradient over an odd size has rows in all four parity classes and the two roles plan differently
    assert EC.conv_plan((2, 128, 64, 3, 2, 33, 31))["y"] != EC.conv_plan((2, 128, 64, 3, 2, 33, 31))["d"]


def test_fp32_weight_gradient_plans():
    plans = {c: (EC.conv_plan(c)["w"], EC.conv_rows(c, "w")) for c, r in EC.CONV_CASES.items() if "w" in r}
    ps = {p for p, _m in plans.values()}
    assert 1 in ps and 16 in ps and any(2 < p < 15 for p in ps) and max(ps) == 16
    # ranges [M p / P, M (p + 1) / P) that are no multiples of the kernel's 16-pixel step: M itself is no multiple of 16 P
    for want in (16, 13, 8):
        assert any(p == want and m % (16 * p) for p, m in plans.values()), want
    for want in (16, 13):                                                            # ... and ranges of unequal length
        assert any(p == want and m % p for p, m in plans.values()), want
    for k in (1, 3):
        assert any(p == 16 for c, (p, _m) in plans.items() if c[3] == k), k


def test_precision_16_plans():
    cases = [c for c in EC.CONV_CASES if EC.p16_accepts(c)]
    assert len(cases) == 15 and all(EC.CONV_CASES[c] == "ydw" for c in cases)
    plans = {c: EC.conv_plan(c, 16) for c in cases}
    for k in (1, 3):
        assert any(pl["w"] >= 2 for c, pl in plans.items() if c[3] == k), k          # the multi-plane folds of both kernel sizes
    assert any(pl["w"] >= 2 and EC.conv_rows(c, "w") % (64 * pl["w"]) for c, pl in plans.items())      # ranges that end inside a 64-pixel step
    assert any(pl["y"] > 1 for pl in plans.values()) and any(pl["d"] > 1 for pl in plans.values())
    assert any(pl[r] > 1 and EC.conv_steps(c, r, 16) % pl[r] for c, pl in plans.items() for r in "yd")
    for c in EC.CONV_CASES:
        if not EC.p16_accepts(c):
            assert EC.conv_plan(c, 16) == {}


def test_batchnorm_chunk_plans():
    chunks = {c: EC.bn_chunks(c) for c in EC.BN_CASES}
    assert all(EC.bn_chunks(c, backward=True) == n for c, n in chunks.items())
    assert chunks == {(4, 64, 6, 5): 1, (3, 64, 19, 9): 2, (2, 128, 23, 29): 5, (2, 64, 65, 65): 32, (16, 2048, 1, 1): 1}
    assert sorted(set(chunks.values())) == [1, 2, 5, 32] and 3 <= 5 <= 31
    ragged = [c for c, n in chunks.items() if (c[0] * c[2] * c[3]) % n]
    assert len(ragged) >= 2
    # a per-sample scale changes inside a chunk: HW is no multiple of the chunk length
    B, _c, H, W = (2, 64, 65, 65)
    assert (H * W) % -(-B * H * W // 32) != 0
    for B in (2, 3, 4, 16):
        s = EC.sample_scale(B)
        assert float(s[1]) == 0.0 and len(set(s.tolist())) >= min(B, 3) and float(s[0]) == 1.0


def test_pooling_and_stem_tables():
    assert set(EC.MAXPOOL_SHAPES) == {(9, 11), (8, 6), (1, 1), (2, 5), (32, 32)} and EC.MAXPOOL_CHANNELS == [4, 64]
    assert {hw for _b, _c, hw in EC.AVGPOOL_CASES} == {1, 4, 99} and any((b * c) % 256 for b, c, _hw in EC.AVGPOOL_CASES)
    assert set(EC.STEM_CASES) == {(3, 21, 18), (1, 7, 7), (2, 32, 32), (2, 33, 47)}
    B, H, W = (1, 7, 7)
    assert B * ((H + 1) // 2) * ((W + 1) // 2) < 32           # fewer output pixels than pixel ranges: some ranges are empty


# ---------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("H,W", EC.MAXPOOL_SHAPES)
def test_first_maximum_in_row_major_order_is_torchs_rule(H, W):
    """the brute-force pool and its backward equal torch's float64 max_pool2d bit for bit on inputs full of ties"""
    for C_ in EC.MAXPOOL_CHANNELS if H < 32 else [4]:
        x, dy = EC.maxpool_input("ties", 2, C_, H, W)
        assert EC.tie_share(x) >= 0.5 or H * W == 1              # (1, 1): one window of one element
        y, dx = EC.maxpool_first(x, dy)
        ty, tdx = EC.maxpool_torch(x, dy)
        assert torch.equal(y, ty) and torch.equal(dx, tdx)
        assert torch.equal(EC.maxpool_backward_fp32_order(x, dy), tdx)        # integer dy: the fp32 order of the sums does not matter
    for x in (torch.zeros(2, 4, H, W, dtype=torch.float64), torch.zeros(2, 4, H, W, dtype=torch.float64).index_fill_(3, torch.tensor([0]), -0.0)):
        dy = EC.maxpool_input("ties", 2, 4, H, W)[1]
        y, dx = EC.maxpool_first(x, dy)
        ty, tdx = EC.maxpool_torch(x, dy)
        assert torch.equal(y, ty) and torch.equal(dx, tdx)


def test_tie_share_of_the_tie_inputs():
    shares = []
    for H, W in EC.MAXPOOL_SHAPES:
        for C_ in EC.MAXPOOL_CHANNELS:
            if H * W > 1:
                shares.append(EC.tie_share(EC.maxpool_input("ties", 2, C_, H, W)[0]))
    assert min(shares) >= 0.5, shares
    # the inputs the earlier test drew have none, and ReLU of randn far fewer: not what pins the rule
    assert EC.tie_share(EC.maxpool_input("random", 2, 64, 9, 11)[0]) == 0.0
    assert EC.tie_share(torch.randn(3, 64, 9, 11, generator=torch.Generator().manual_seed(0)).clamp_min(0).double()) < 0.1


def test_fp32_order_backward_differs_from_float64_only_by_rounding():
    """random dy: the fp32-ordered sum is the float64 backward rounded -- within one fp32 ulp of the sum of magnitudes -- and equal where an
    element collects one window"""
    x = EC.maxpool_input("ties", 2, 4, 9, 11)[0]
    dy = torch.randn(2, 4, 5, 6, generator=torch.Generator().manual_seed(3)).double()
    a, b = EC.maxpool_backward_fp32_order(x, dy), EC.maxpool_torch(x, dy)[1]
    bound = 3 * 2.0 ** -24 * EC.maxpool_torch(x, dy.abs())[1]
    assert bool(((a - b).abs() <= bound).all()) and not torch.equal(a, b)
    assert torch.equal(a.float().double(), a)


@pytest.mark.parametrize("case", list(EC.CONV_CASES), ids=EC.conv_id)
def test_integer_operands_are_exact_in_both_arithmetics(case):
    """x, w, dy from -2 .. 2: fp16 holds every operand, and every result -- and every partial sum, in any order: at most 4 x the length of
    the contraction -- is below 2^24, so fp32 accumulation of any split, range or fold order is exact"""
    B, Cin, Cout, K, st, H, W = case
    ops = EC.conv_operands(case, "integer")
    for t in ops:
        assert torch.equal(t, t.round()) and float(t.abs().max()) == 2.0 and torch.equal(EC.rounded(t), t)
    assert 4 * max(K * K * Cin, K * K * Cout, EC.conv_rows(case, "w")) < 2 ** 24
    ref = EC.conv_reference(case, "integer")
    assert all(torch.equal(r, r.round()) and float(r.abs().max()) < 2 ** 24 for r in ref)
    assert all(torch.equal(a, b) for a, b in zip(ref, EC.conv_reference(case, "integer", 16)))
    if case == (5, 64, 64, 3, 1, 19, 21):
        print("max |y|", float(ref[0].abs().max()), "max |dw|", float(ref[2].abs().max()))
        assert float(ref[0].abs().max()) < 1000 and float(ref[2].abs().max()) < 2000
    # random operands are fp32 numbers, and fp16 rounds them
    r = EC.conv_operands(case, "random")
    assert all(torch.equal(t.float().double(), t) for t in r) and not torch.equal(EC.rounded(r[0]), r[0])
    assert EC.conv_reference(case, "random") is EC.conv_reference(case, "random")          # computed once


def test_stem_integer_operands_are_exact():
    for case in EC.STEM_CASES:
        x, w, dz = EC.stem_operands(case, "integer")
        z, dw = EC.stem_reference(case, "integer")
        assert 4 * max(49, dz.shape[0] * dz.shape[2] * dz.shape[3]) < 2 ** 24
        assert torch.equal(z, z.round()) and torch.equal(dw, dw.round()) and float(dw.abs().max()) > 0


def test_batchnorm_reference_is_torchs_training_mode_module():
    case = (3, 64, 19, 9)
    o = EC.bn_operands(case)
    bn = torch.nn.BatchNorm2d(64, eps=EC.BN_EPS, momentum=EC.BN_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(o["gamma"]); bn.bias.copy_(o["beta"]); bn.running_mean.copy_(o["run_mean"]); bn.running_var.copy_(o["run_var"])
    y = torch.relu(bn(o["z"]) + o["res"])
    r = EC.bn_reference(o["z"], o["gamma"], o["beta"], o["dy"], True, mask=y > 0, res=o["res"], run_mean=o["run_mean"], run_var=o["run_var"])
    assert torch.equal(r["y"], y.detach()) and torch.equal(r["run_mean"], bn.running_mean) and torch.equal(r["run_var"], bn.running_var)
    assert not torch.equal(r["run_mean"], o["run_mean"])                     # the operands themselves are left alone
    assert EC.rel(r["mean"], o["z"].mean(dim=(0, 2, 3))) < 1e-14
    # large |mean| / sigma: the operand really has it
    for ratio in (10.0, 100.0):
        z = EC.bn_operands(case, ratio)["z"]
        got = z.mean(dim=(0, 2, 3)).abs() / z.std(dim=(0, 2, 3))
        assert float((got / ratio - 1).abs().max()) < 0.1
