"""Host: the case tables, references and plan rules of tests/spark_op_cases.py are themselves checked here, with no GPU.
1. every float64 reference agrees to 1e-12 with an independent torch formulation of the same operation (F.batch_norm over the gathered rows
   plus torch.where, F.conv2d / F.conv_transpose2d, autograd, torch.optim.AdamW);
2. every case reaches the edge it is listed for, recomputed from the restated plan rules and, where the library states a size itself, from
   its own size queries (bytes = the restated chunk, plane and part counts, each request rounded up to 256);
3. sensitivity: the result a wrong kernel of a given kind would give -- cells counted only up to index 255, ch and cw swapped, the last chunk
   or its ragged remainder dropped, the last channel quad dropped, the last Cs % 16 / Cs % 4 source channels dropped, the last step range of a
   split or the last pixel range of the weight gradient dropped, the transposed weight read as [Cout][Cin], sign(0) = 1, decay applied on a
   skipped step, statistics over all pixels -- differs from the reference by MORE than 4 limits in one result or more (on integer operands:
   differs at all), for every case the mutation applies to; and every mutation is applied to a case or more."""
import pytest
import torch
import torch.nn.functional as F

import spark_op_cases as S
from conftest import load_pkg


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


@pytest.fixture(scope="module")
def q():
    return load_pkg("_lib").scratch_query


# ---------------------------------------------------------------------------------------------------------------- the plan rules
def test_the_benchmarked_step_reaches_what_the_issue_names():
    """32 x 96 x 96 with f = 3: 288 cells (two trips of the count), the BatchNorm cap at C = 8, the bias gradient's cap at the last layer"""
    assert S.count_trips(32 * 3 * 3) == 2 and S.count_trips(48) == 1 and S.count_trips(256) == 1 and S.count_trips(257) == 2
    assert S.bn_chunks(32 * 96 * 96, 8) == 128
    assert S.chan_sum_chunks(32 * 96 * 96, 8) == 256          # dense_decoder.dec.4.up: 8 channels at 96 x 96
    assert S.bn_chunks(261, 2048) == 32 and S.chunk_ranges(261, 32)[28:] == [(252, 261), (261, 261), (270, 270), (279, 279)]
    assert [b - a for a, b in S.step_ranges(45, 4)] == [11, 11, 11, 12]
    assert S.loss_chunks(12288) == 3 and S.loss_chunks(4095) == 1


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def bn_by_torch(name):
    """F.batch_norm over the gathered rows (the reference's BatchNorm1d, encoder.py:25-35), torch.where for the fill, autograd"""
    c, o = S.BN_CASES[name], S.bn_operands(name)
    B, H, W, f, C = c["B"], c["H"], c["W"], c["f"], c["C"]
    on = S.cell_mask(o["active"], H, W) if c["sparse"] else torch.ones(B, H, W, dtype=torch.bool)
    leaf = {k: o[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta", "fill", "res") if o[k] is not None}
    rm, rv = o["rm"].clone(), o["rv"].clone()
    rows = leaf["z"][on]
    normed = F.batch_norm(rows, rm if (c["run"] or not c["training"]) else None, rv if (c["run"] or not c["training"]) else None, leaf["gamma"], leaf["beta"],
                          bool(c["training"]), S.MOM, S.EPS)
    # the statistics of the rows applied to every pixel: only the active ones are kept
    mean = rows.mean(0) if c["training"] else o["rm"]
    var = rows.var(0, unbiased=False) if c["training"] else o["rv"]
    everywhere = (leaf["z"] - mean) / torch.sqrt(var + S.EPS) * leaf["gamma"] + leaf["beta"]
    close(everywhere[on].detach(), normed.detach())
    inactive = leaf["fill"].expand(B, H, W, C) if c["fill"] else torch.zeros(B, H, W, C, dtype=torch.float64)
    v = torch.where(on.unsqueeze(-1), everywhere, inactive)
    if c["ss"]:
        v = v * o["s"].view(B, 1, 1, 1)
    if c["res"]:
        v = v + leaf["res"]
    if c["dres"] and not c["res"]:
        extra = torch.zeros_like(v, requires_grad=True)          # dres without a residual: the gradient at the activation's input
        v = v + extra
        leaf["res"] = extra
    y = F.relu(v) if c["act"] == 1 else F.relu6(v) if c["act"] == 2 else v
    y.backward(o["dy"])
    out = dict(y=y.detach(), dz=leaf["z"].grad, dgamma=leaf["gamma"].grad, dbeta=leaf["beta"].grad, mean=mean.detach(),
               rstd=1 / torch.sqrt(var.detach() + S.EPS))
    if c["run"] or not c["training"]:
        out["run_mean"], out["run_var"] = rm, rv
    if c["dres"]:
        out["dres"] = leaf["res"].grad
    if c["fill"]:
        out["dfill"] = leaf["fill"].grad
    return out


@pytest.mark.parametrize("name", list(S.BN_CASES))
def test_batchnorm_reference_and_sensitivity(name):
    c = S.BN_CASES[name]
    ref, ind = S.bn_ref(name), bn_by_torch(name)
    assert set(ref) == set(ind)
    for k in ref:
        close(ref[k], ind[k], 1e-12 if c["ratio"] is None else 1e-10)        # float64's own cancellation at |mean| / sigma = 100
    if c["act"] == 2:                                                         # each branch of ReLU6 holds its share
        y = ref["y"]
        for part in (y == 0, (y > 0) & (y < 6), y == 6):
            assert 0.10 < float(part.double().mean()) < 0.80, (name, float(part.double().mean()))
    if c["act"] == 1:
        assert 0.10 < float((ref["y"] > 0).double().mean()) < 0.90
    limits = S.bn_limits(name, ref)
    muts = S.bn_mutations(name)
    for mut in muts:
        wrong = S.bn_ref(name, mut)
        worst = max(S.rel(wrong[k], ref[k]) / limits[k][0] for k in ref)
        assert worst > 4, (name, mut, worst)


def test_every_batchnorm_mutation_has_a_case():
    applied = {m for name in S.BN_CASES for m in S.bn_mutations(name)}
    assert applied == set(S.BN_MUTATIONS)


def test_batchnorm_cases_reach_their_edges(q):
    P = {name: S.bn_plan(name) for name in S.BN_CASES}
    O = {name: S.bn_operands(name) for name in S.BN_CASES if name != "cap128_c8_relu"}
    C_ = S.BN_CASES
    # the library's own chunk counts
    for name, pl in P.items():
        c = C_[name]
        N, HW, C = pl["N"], c["H"] * c["W"], c["C"]
        assert q("spark_bn_forward", N, HW, C) == S.r256(pl["chunks"] * 2 * C * 8) + S.r256(2 * 4), name
        assert q("spark_bn_backward", N, HW, C) == S.r256(pl["chunks"] * 3 * C * 8) + S.r256(2 * C * 4), name
        assert pl["qpb"] * pl["rows"] <= 256 and pl["yblocks"] * pl["qpb"] >= C // 4
    # more than 256 cells, no multiple of 256, active cells beyond index 255
    for name in ("cells297_relu_res_ss", "empty_chunks_c2048_norun_ynull"):
        cells = O[name]["active"].reshape(-1)
        assert P[name]["cells"] > 256 and P[name]["cells"] % 256 and S.count_trips(P[name]["cells"]) == 2
        assert 0 < int(cells[256:].sum()) < cells.numel() - 256 and int(cells.sum()) != int(cells[:256].sum())
    assert P["cells297_relu_res_ss"]["cells"] == 297
    # H != W, ch != cw, a partial second channel block
    c, pl = C_["rect_c72_relu6_fill_res"], P["rect_c72_relu6_fill_res"]
    assert c["H"] != c["W"] and c["H"] // c["f"] != c["W"] // c["f"] and pl["yblocks"] == 2 and c["C"] // 4 == 18 and 18 % pl["qpb"]
    # empty trailing chunks
    pl = P["empty_chunks_c2048_norun_ynull"]
    assert pl["chunks"] == 32 and pl["ranges"][0] == (0, 9) and sum(a >= pl["N"] for a, b in pl["ranges"]) == 3 and pl["N"] == 261
    # qpb not dividing 256, in training; ragged last chunk; boundaries inside a row and inside a sample
    for name in ("c40_ragged_sparse_relu_ss_res_fill", "c40_ragged_dense_relu6"):
        c, pl = C_[name], P[name]
        assert (pl["qpb"], pl["rows"]) == (10, 25) and 256 % pl["qpb"] and c["training"]
        sizes = [b - a for a, b in pl["ranges"]]
        assert sizes == [446] * 9 + [441]
        assert any(a % c["W"] for a, b in pl["ranges"][1:]) and any(a // (c["H"] * c["W"]) != (b - 1) // (c["H"] * c["W"]) for a, b in pl["ranges"])
    c, pl = C_["c12_sparse_relu6_fill_res"], P["c12_sparse_relu6_fill_res"]
    assert (pl["qpb"], pl["rows"]) == (3, 85) and c["sparse"] and c["training"]
    # the cap with a ragged chunk
    pl = P["cap128_c8_relu"]
    assert pl["chunks"] == 128 and pl["N"] * 8 // 16384 > 128 and pl["ranges"][0] == (0, 2097) and pl["ranges"][-1][1] - pl["ranges"][-1][0] == 2001
    assert (pl["qpb"], pl["rows"]) == (2, 128) and any(a % 516 for a, b in pl["ranges"][1:])
    # constant channels: constant over the active pixels, varying over the inactive ones; one constant exact in few bits, one not
    o, c = O["constant_channels"], C_["constant_channels"]
    on = S.cell_mask(o["active"], c["H"], c["W"])
    for ch_ in (1, 5):
        assert float(o["z"][..., ch_][on].std()) == 0 and float(o["z"][..., ch_][~on].std()) > 0.5
    assert float(o["z"][..., 1][on][0]) == 0.75 and float(o["z"][..., 5][on][0]) not in (0.1, 0.75)
    assert float(S.bn_ref("constant_channels")["rstd"][1]) == pytest.approx(S.EPS ** -0.5)
    # a dropped sample with fill and without a residual: its inactive pixels are fill * 0
    c, o = C_["dropped_sample_fill_nores"], O["dropped_sample_fill_nores"]
    assert c["ss"] and c["fill"] and not c["res"] and float(o["s"][1]) == 0 and float(S.bn_ref("dropped_sample_fill_nores")["y"][1].abs().max()) == 0
    assert float(S.bn_ref("dropped_sample_fill_nores")["dfill"].abs().min()) > 0
    c = C_["eval_sparse_fill"]
    assert not c["training"] and c["sparse"] and c["fill"]
    # the option set: with and without each of res, ss, fill, dres, running statistics, y; act 0 / 1 / 2; sparse and dense
    for key in ("res", "ss", "fill", "dres", "run", "y_null", "sparse"):
        assert {bool(c[key]) for c in C_.values()} == {False, True}, key
    assert {c["act"] for c in C_.values()} == {0, 1, 2} and all(c["act"] == 0 for c in C_.values() if c["y_null"])
    assert any(c["ss"] and not c["res"] for c in C_.values()) and any(not c["run"] and c["training"] for c in C_.values())
    # |mean| / sigma
    for name, ratio in (("large_mean_10_sparse", 10), ("large_mean_100_sparse", 100), ("large_mean_10_dense", 10), ("large_mean_100_dense", 100)):
        r = S.bn_ref(name)
        got = (r["mean"].abs() * r["rstd"])
        assert 0.8 * ratio < float(got.min()) and float(got.max()) < 1.25 * ratio, (name, float(got.min()), float(got.max()))
    assert C_["large_mean_10_sparse"]["sparse"] and not C_["large_mean_10_dense"]["sparse"]


# ---------------------------------------------------------------------------------------------------------------- convolution family
def conv_by_torch(case, kind):
    Cin, Cout, K, tc, B, H, W, bias = case
    x, w, b, dy = S.conv_operands(case, kind)
    x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv_transpose2d(x, w, b if bias else None, 2, 1) if tc else F.conv2d(x, w, b if bias else None, 1, K // 2)
    y.backward(dy)
    out = dict(y=y.detach(), dx=x.grad, dw=w.grad)
    if bias:
        out["db"] = b.grad
    return out


@pytest.mark.parametrize("case", list(S.CONV_CASES), ids=S.conv_id)
def test_convolution_reference_and_sensitivity(case):
    assert case[4] >= 2                                      # a tile crosses a sample boundary
    for kind in ("random", "integer"):
        ref, ind = S.conv_ref(case, kind), conv_by_torch(case, kind)
        assert set(ref) == set(ind) == set(S.CONV_ROLES[:4 if case[7] else 3])
        for k in ref:
            close(ref[k], ind[k])
    assert S.integer_sum_bound(case) < 2 ** 24
    ref = S.conv_ref(case, "integer")
    assert all(float(v.abs().max()) <= S.integer_sum_bound(case) and bool((v == v.round()).all()) for v in ref.values())
    for mut in S.conv_mutations(case):
        for kind in ("random", "integer"):
            ref, wrong = S.conv_ref(case, kind), S.conv_ref(case, kind, mut)
            if kind == "integer":
                assert any(not torch.equal(wrong[k], ref[k]) for k in ref), (case, mut)
            else:
                assert max(S.rel(wrong[k], ref[k]) for k in ref) > 4 * S.CONV_LIMIT, (case, mut)


def test_convolution_cases_reach_their_edges(q):
    plans = {case: S.conv_plan(case) for case in S.CONV_CASES}
    applied = {m for case in S.CONV_CASES for m in S.conv_mutations(case)}
    assert applied == {"tail16", "tail4", "wgrad_tail4", "split_last", "wgrad_last_range", "transposed_weight", "db_last_chunk", "db_ragged"}
    # the library's own plans: Z planes of the result, P parts of dW, the bias gradient's chunks
    for case, pl in plans.items():
        Cin, Cout, K, tc, B, H, W, bias = case
        _, _, (Ho, Wo), _ = S.conv_geom(case)
        assert q("spark_conv", B, H, W, Cin, Cout, K, tc, 0) == (S.r256(pl["Zy"] * B * Ho * Wo * Cout * 4) if pl["Zy"] > 1 else 0), case
        assert q("spark_conv", B, H, W, Cin, Cout, K, tc, 1) == (S.r256(pl["Zdx"] * B * H * W * Cin * 4) if pl["Zdx"] > 1 else 0), case
        parts = S.r256(pl["P"] * Cin * Cout * K * K * 4)
        assert q("spark_conv_wgrad", B, H, W, Cin, Cout, K, tc, 0) == parts, case
        assert q("spark_conv_wgrad", B, H, W, Cin, Cout, K, tc, 1) == parts + S.r256(S.chan_sum_chunks(B * Ho * Wo, Cout) * Cout * 8), case
    by = lambda *head: next(c for c in S.CONV_CASES if c[:len(head)] == head)
    # the scalar path with 3x3 and 4x4 taps; a ragged last 16-channel step
    assert all(by(*h)[2] == 3 and (h[0] % 4 or h[1] % 4) for h in ((6, 3), (1, 7), (17, 5)))
    pl = plans[by(17, 5)]
    assert pl["Zy"] == 2 and pl["steps_y"] == 18 and 17 % 16 == 1 and by(17, 5)[4] * by(17, 5)[5] * by(17, 5)[6] == 35
    pl = plans[by(72, 72)]
    assert pl["Zy"] == pl["Zdx"] == 4 and [b - a for a, b in S.step_ranges(pl["steps_y"], 4)] == [11, 11, 11, 12] and 64 < 72 < 128
    pl = plans[by(1025, 64)]
    assert pl["Zy"] == 32 and pl["steps_y"] == 585 and len({b - a for a, b in S.step_ranges(585, 32)}) == 2 and 1025 % 4
    pl = plans[by(2050, 128)]
    assert pl["Zy"] == 16 and pl["steps_y"] == 129 and len({b - a for a, b in S.step_ranges(129, 16)}) == 2
    assert {c[4] * c[5] * c[6] for c in S.CONV_CASES} >= {64, 65, 127, 128}
    # transposed: Cin != Cout, one of them no multiple of 4, non-square
    tcs = [c for c in S.CONV_CASES if c[3]]
    assert {c[:2] for c in tcs} >= {(12, 20), (20, 6), (20, 72)} and all(c[5] != c[6] for c in tcs) and any(c[1] % 4 for c in tcs)
    pl = plans[by(20, 72)]
    assert pl["Zy"] == 4 and 5 * 14 * 2 == 140
    # the weight gradient's parts: the cap with ranges of 66 and 67 pixels; either side of the first step
    c = by(4, 1, 1, 0, 5, 13, 65)
    assert plans[c]["P"] == 64 and {b - a for a, b in S.pixel_ranges(4225, 64)} == {66, 67} and c[7]
    assert plans[by(8, 4, 3, 0, 127)]["P"] == 1 and plans[by(8, 4, 3, 0, 2, 8, 8)]["P"] == 2
    assert any(pl["P"] > 1 and (b - a) % 16 for pl_case, pl in plans.items() for a, b in S.pixel_ranges(pl_case[4] * pl_case[5] * pl_case[6], pl["P"]))
    # the bias gradient
    assert {c[1] for c in S.CONV_CASES if c[7]} >= {1, 3, 24, 96, 255, 256}
    c = by(4, 24, 1, 0, 3, 15, 17)
    assert plans[c]["db_chunks"] == 2 and [b - a for a, b in S.chunk_ranges(765, 2)] == [383, 382]
    c = by(8, 8, 4, 1)
    sizes = [b - a for a, b in S.chunk_ranges(266256, plans[c]["db_chunks"])]
    assert plans[c]["db_chunks"] == 256 and 266256 * 8 // 8192 > 256 and sizes[0] == 1041 and sizes[-1] == 801 and c[4] * c[5] * c[6] * 4 == 266256


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("name", list(S.LOSS_CASES))
def test_loss_reference_and_sensitivity(name):
    B, H, W, f, mask, (wm, wl), _ = S.LOSS_CASES[name]
    rec, inp, active = S.loss_operands(name)
    l_mask, l_l1, drec = S.loss_ref(name)
    r = rec.clone().requires_grad_(True)
    up = active.repeat_interleave(H // f, 1).repeat_interleave(W // f, 2)              # the mask at the image's resolution (encoder.py:13-16)
    t_mask = ((r - inp) ** 2 * ~up).sum() / ((H // f) * (W // f) * ((~active).sum().double() + 1e-8))
    t_l1 = (r - inp).abs().mean()
    (wm * t_mask + wl * t_l1).backward()
    t_mask, t_l1 = t_mask.detach(), t_l1.detach()
    assert abs(float(l_mask - t_mask)) <= 1e-12 * float(t_mask) and abs(float(l_l1 - t_l1)) <= 1e-12 * float(t_l1)
    close(drec, r.grad)
    assert 0.05 < float((rec == inp).double().mean()) < 0.15
    assert (float(l_mask) == 0) == (mask == "nothing_masked")
    for mut in S.loss_mutations(name):
        m_mask, m_l1, m_drec = S.loss_ref(name, mut)
        shows = [abs(float(m_l1 - l_l1)) > 4 * S.LOSS_LIMIT * float(l_l1), S.rel(m_drec, drec) > 4 * S.LOSS_LIMIT]
        if mask != "nothing_masked":
            shows.append(abs(float(m_mask - l_mask)) > 4 * S.LOSS_LIMIT * float(l_mask))
        assert any(shows), (name, mut)


def test_loss_cases_reach_their_edges(q):
    P = {name: S.loss_plan(name) for name in S.LOSS_CASES}
    for name, pl in P.items():
        B, H, W, f = S.LOSS_CASES[name][:4]
        assert q("spark_loss", B, H, W, f) == S.r256(pl["chunks"] * 2 * 8), name
    assert {m for name in S.LOSS_CASES for m in S.loss_mutations(name)} == {"count255", "swap", "last_chunk", "ragged", "sign0"}
    pl = P["ragged_mixed_1_0"]
    assert [b - a for a, b in pl["ranges"]] == [4820, 4819] and 4820 % 63 and 51 // 3 != 63 // 3
    pl = P["cells320_below_4096"]
    assert pl["cells"] == 320 and pl["total"] < 4096 and pl["chunks"] == 1
    cells = S.loss_operands("cells320_below_4096")[2].reshape(-1)
    assert int(cells[256:].sum()) > 0 and int((~cells[256:]).sum()) > 0
    pl = P["cap256"]
    sizes = [b - a for a, b in pl["ranges"]]
    assert pl["chunks"] == 256 and pl["total"] // 4096 > 256 and sizes[0] == 4113 and sizes[-1] == 3861
    masks = {c[4] for c in S.LOSS_CASES.values()}
    assert masks == {"mixed", "all_masked", "nothing_masked"} and {c[5] for c in S.LOSS_CASES.values()} == {(1.0, 0.0), (0.0, 1.0), (0.5, 1.0)}
    assert not S.loss_operands("ragged_all_masked")[2].any() and S.loss_operands("ragged_nothing_masked")[2].all()
    assert any(not c[6] for c in S.LOSS_CASES.values())


# ---------------------------------------------------------------------------------------------------------------- mask multiply
@pytest.mark.parametrize("case", S.MASK_MUL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mask_multiply_reference_and_sensitivity(case):
    B, H, W, C, f = case
    x, active = S.mask_mul_operands(case)
    ref = S.mask_mul_ref(case)
    up = active.repeat_interleave(H // f, 1).repeat_interleave(W // f, 2)
    assert torch.equal(ref, x * up.unsqueeze(-1)) and 0 < int(active.sum()) < active.numel()
    if H // f != W // f:
        assert not torch.equal(S.mask_mul_ref(case, "swap"), ref)


def test_mask_multiply_cases_reach_their_edges():
    assert any(B * f * f > 256 for B, H, W, C, f in S.MASK_MUL_CASES) and any(C == 1 for B, H, W, C, f in S.MASK_MUL_CASES)
    assert any(C % 4 and C > 1 for B, H, W, C, f in S.MASK_MUL_CASES) and any(H // f != W // f for B, H, W, C, f in S.MASK_MUL_CASES)
    assert any(B * H * W * C > 256 for B, H, W, C, f in S.MASK_MUL_CASES)


# ---------------------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("case", S.ADAM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_adamw_reference_and_sensitivity(case):
    n, wd, unscale = case
    p0, grads, bad = S.adam_operands(n)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=S.ADAM_HYPER["lr"], weight_decay=wd, betas=S.ADAM_HYPER["betas"], eps=S.ADAM_HYPER["eps"])
    for t in range(S.ADAM_STEPS):
        ref.grad = grads[t] * unscale
        opt.step()
    p, m, v = S.adam_ref(case)
    close(p, ref.detach())
    close(m, opt.state[ref]["exp_avg"])
    close(v, opt.state[ref]["exp_avg_sq"])
    assert unscale == 0.5 and not bool(torch.isfinite(bad).all())
    if wd:
        assert S.rel(S.adam_ref(case, "decay_on_skip")[0], p) > 4 * S.ADAM_LIMIT
    else:
        assert torch.equal(S.adam_ref(case, "decay_on_skip")[0], p)


def test_adamw_lengths_straddle_the_kernels_steps():
    """one element per thread, 256 threads per workgroup (adam_guarded_kernel); float4 with a scalar tail (grad_check_kernel)"""
    ns = set(S.ADAM_LENGTHS)
    assert {1, 3, 4, 5, 255, 256, 257} <= ns and any(n > 512 and n % 256 and n % 4 for n in ns)
    assert {wd for _, wd, _ in S.ADAM_CASES} == {0.0, 0.05}
