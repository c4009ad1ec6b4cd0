"""GPU: the operator arenas without slack. (1) For every operator that takes shape-dependent temporaries, at the smallest shapes that
reach each branch of its plan: on a handle whose arena is exactly the bytes its size query (cddpm_op_*_scratch) names, the operator
runs and its outputs are finite; with 256 bytes less it is refused with the arena message before anything is launched (the outputs
keep their fill). (2) With training.ARENA_FLOOR at 0 the trainer's arenas are the largest queried call and nothing more: whole steps
then run unrefused and give bit for bit the gradients and the parameters of the same step with the floor in place -- no kernel
knows the arena's size."""
import ctypes as C

import pytest
import torch

import arch_cases as A
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FILL = -7.0


@pytest.fixture()
def eng():
    e = load_pkg("engine").CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16)       # a fresh handle: only its arena is used
    yield e
    e.close()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + len(shape))).cuda()


def out(*shape):
    return torch.full(shape, FILL, device="cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def both_sides(eng, q, call, outputs):
    """call() runs the operator on eng's handle. Arena = q bytes: returns 0, outputs finite. Arena = q - 256: refused, nothing written."""
    lib, h = eng.lib, eng._h
    assert q % 256 == 0
    assert lib.cddpm_op_set_scratch(h, q) == 0
    if q:
        assert q > 256                         # (an arena of 0 bytes is no arena: the operator would allocate for the call)
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
        assert bool(torch.isfinite(o).all()) and not bool((o == FILL).all())


@pytest.fixture()
def train_precision():
    lib = load_pkg("_lib").load_library()
    yield lambda bits: lib.cddpm_set_train_precision(bits)
    lib.cddpm_set_train_precision(32)


# B = 9: two batch groups, one ragged; 5 x 9 pixels: ragged tiles. k 3 (images, CK 32); k 1 with Cin 96 (the register-staged kernel, no
# images) and with Cin 128 (images, CK 64)
@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("k,cin,cout", [(3, 32, 64), (1, 96, 64), (1, 128, 64)], ids=["k3", "k1_staged", "k1_images"])
def test_conv_wgrad(eng, train_precision, k, cin, cout, with_db, bits):
    B, H, W = 9, 5, 9
    train_precision(bits)
    lib = eng.lib
    q = lib.cddpm_op_conv_wgrad_scratch(cin, 0, 0, cout, k, B, H, W, 0)
    assert q == lib.cddpm_op_conv_wgrad_scratch(cin, 0, 0, cout, k, B, H, W, bits) <= lib.cddpm_op_conv_wgrad_scratch(cin, 0, 0, cout, k, B, H, W, 32)
    images = k == 3 or cin % 64 == 0
    assert (q < lib.cddpm_op_conv_wgrad_scratch(cin, 0, 0, cout, k, B, H, W, 32)) == (bits == 16 and images)
    x, dy = rnd(B, H, W, cin), rnd(B, H, W, cout, seed=1)
    dw, db = out(cout, cin, k, k), out(cout) if with_db else None
    both_sides(eng, q, lambda: lib.cddpm_op_conv_wgrad(eng._h, _p(x), cin, None, 0, None, 0, 0, _p(dy), cout, k, _p(dw), _p(db), B, H, W, None),
               [dw] + ([db] if with_db else []))


@pytest.mark.parametrize("hw", [(65, 63), (64, 64)], ids=["4095", "4096"])          # the step of gn_nsplit: 64 ranges of 64 pixels | 16 of 256
@pytest.mark.parametrize("records", [False, True], ids=["swept", "records"])
def test_gn_silu_backward(eng, hw, records):
    B, (H, W), Cc = 1, hw, 32
    lib = eng.lib
    q = lib.cddpm_op_gn_silu_backward_scratch(int(records), B, H * W, Cc)
    assert lib.cddpm_op_gn_silu_backward_scratch(0, B, H * W, Cc) > lib.cddpm_op_gn_silu_backward_scratch(1, B, H * W, Cc)
    x, da, gamma, beta = rnd(B, H, W, Cc), rnd(B, H, W, Cc, seed=1), rnd(Cc, seed=2), rnd(Cc, seed=3)
    rec = torch.stack([x.sum(dim=(1, 2)), (x * x).sum(dim=(1, 2))], dim=-1).reshape(B, 1, Cc, 2).contiguous() if records else None
    dx, dg, dbt = out(B, H, W, Cc), out(Cc), out(Cc)
    both_sides(eng, q, lambda: lib.cddpm_op_gn_silu_backward(eng._h, _p(x), None, 0, _p(da), _p(gamma), _p(beta), None, 1, _p(dx), None, _p(dg), _p(dbt),
                                                             None, _p(rec), 1 if records else 0, None, B, H * W, Cc, None), [dx, dg, dbt])


@pytest.mark.parametrize("two", [False, True], ids=["one_source", "two_sources"])
def test_gn_coef(eng, two):
    B, HW, C0, C1 = 2, 70, 32, 32 if two else 0
    lib = eng.lib
    q = lib.cddpm_op_gn_coef_scratch(C0, int(two), C1, B, HW)
    x0, x1 = rnd(B, HW, C0), rnd(B, HW, C1, seed=1) if two else None
    gamma, beta, coef = rnd(C0 + C1, seed=2), rnd(C0 + C1, seed=3), out(3, B, C0 + C1)
    both_sides(eng, q, lambda: lib.cddpm_op_gn_coef(eng._h, _p(x0), C0, _p(x1), C1, _p(gamma), _p(beta), None, _p(coef), B, HW, None), [coef])


@pytest.mark.parametrize("p16", [False, True], ids=["fp32", "p16"])
def test_attention_backward(eng, p16):
    B, N, Cc = 1, 65, 64
    lib = eng.lib
    q = lib.cddpm_op_attention_backward_scratch(B, N, Cc)
    qkv, da, dqkv = rnd(B, N, 3 * Cc), rnd(B, N, Cc, seed=1), out(B, N, 3 * Cc)
    op = lib.cddpm_op_attention_backward_p16 if p16 else lib.cddpm_op_attention_backward
    both_sides(eng, q, lambda: op(eng._h, _p(qkv), _p(da), _p(dqkv), B, N, Cc, None), [dqkv])


# (2, 1024, 64) with SiLU: the activated copy of x and the split-K partial sums; (65, 64, 64) without: nothing
@pytest.mark.parametrize("M,N,K,silu", [(2, 1024, 64, 1), (65, 64, 64, 0)], ids=["split_k_silu", "plain"])
def test_linear_backward(eng, M, N, K, silu):
    lib = eng.lib
    q = lib.cddpm_op_linear_backward_scratch(M, N, K, silu)
    assert (q == 0) == (not silu)
    x, w, dy = rnd(M, K), rnd(N, K, seed=1), rnd(M, N, seed=2)
    dw, db, dx = out(N, K), out(N), out(M, K)
    both_sides(eng, q, lambda: lib.cddpm_op_linear_backward(eng._h, _p(x), _p(w), _p(dy), M, N, K, silu, _p(dw), _p(db), _p(dx), None), [dw, db, dx])


def test_head_and_small_reductions(eng):
    B, H, W, Cc = 1, 4, 4, 128
    lib = eng.lib
    x, w9, bias, o = rnd(B, H, W, Cc), rnd(9, Cc, seed=1), rnd(1, seed=2), out(B, 1, H, W)
    coef = torch.stack([torch.zeros(B, Cc), torch.ones(B, Cc), torch.zeros(B, Cc)]).cuda()
    both_sides(eng, lib.cddpm_op_head_scratch(B, H, W, Cc),
               lambda: lib.cddpm_op_head(eng._h, _p(x), _p(coef), _p(w9), C.c_float(0.0), _p(bias), _p(o), B, H, W, Cc, None), [o])
    img, dw = rnd(B, H, W, seed=3), out(Cc * 9)
    both_sides(eng, lib.cddpm_op_chan_image_corr_scratch(B, H, W, Cc),
               lambda: lib.cddpm_op_chan_image_corr(eng._h, _p(x), _p(coef), 1, _p(img), -1, _p(dw), B, H, W, Cc, None), [dw])
    db = out(Cc)
    both_sides(eng, lib.cddpm_op_bias_grad_scratch(B * H * W, Cc), lambda: lib.cddpm_op_bias_grad(eng._h, _p(x), B * H * W, Cc, _p(db), None), [db])


# 1 x 8 x 8 pixels = one row tile: Cin 256 splits the contraction in two (16 steps of 16 channels), Cin 64 does not (no temporaries)
@pytest.mark.parametrize("cin", [256, 64], ids=["split_k", "direct"])
def test_enc_conv(eng, cin):
    B, H, W, cout = 1, 8, 8, 64
    lib = eng.lib
    q = lib.cddpm_op_enc_conv_scratch(B, H, W, cin, cout, 1, 1, 0)
    assert q == (2 * B * H * W * cout * 4 if cin == 256 else 0)
    w, wf, wd = rnd(cout, cin, 1, 1), torch.zeros(cout * cin, device="cuda"), torch.zeros(cout * cin, device="cuda")
    assert lib.cddpm_op_enc_pack_w(eng._h, _p(w), cout, cin, 1, _p(wf), _p(wd), None) == 0
    x, y = rnd(B, H, W, cin, seed=1), out(B, H, W, cout)
    both_sides(eng, q, lambda: lib.cddpm_op_enc_conv(eng._h, _p(x), _p(wf), _p(y), B, H, W, cin, cout, 1, 1, 0, None), [y])


def test_enc_weight_gradients(eng):
    B, H, W, cin, cout = 1, 8, 8, 64, 64
    lib = eng.lib
    x, dz, dw = rnd(B, H, W, cin), rnd(B, H, W, cout, seed=1), out(cout, cin, 3, 3)
    both_sides(eng, lib.cddpm_op_enc_conv_wgrad_scratch(B, H, W, cin, cout, 3, 1),
               lambda: lib.cddpm_op_enc_conv_wgrad(eng._h, _p(x), _p(dz), _p(dw), B, H, W, cin, cout, 3, 1, None), [dw])
    img, dz0, dw0 = rnd(B, 1, 2 * H, 2 * W, seed=2), rnd(B, H, W, 64, seed=3), out(64, 1, 7, 7)
    both_sides(eng, lib.cddpm_op_enc_stem_wgrad_scratch(B, 2 * H, 2 * W),
               lambda: lib.cddpm_op_enc_stem_wgrad(eng._h, _p(img), _p(dz0), _p(dw0), B, 2 * H, 2 * W, None), [dw0])


@pytest.mark.parametrize("N", [255, 256 * 33], ids=["one_chunk", "32_chunks"])        # enc_bn_chunks: N / 256, at least 1, at most 32
def test_enc_batchnorm(eng, N):
    Cc = 64
    lib = eng.lib
    qf, qb = lib.cddpm_op_enc_bn_forward_scratch(N, N, Cc), lib.cddpm_op_enc_bn_backward_scratch(N, N, Cc)
    assert qf == (1 if N == 255 else 32) * 2 * Cc * 8 and qb == qf + 2 * Cc * 4
    z, gamma, beta, dy = rnd(1, N, 1, Cc), rnd(Cc, seed=1), rnd(Cc, seed=2), rnd(1, N, 1, Cc, seed=3)
    mr, y = out(2, Cc), out(1, N, 1, Cc)
    both_sides(eng, qf, lambda: lib.cddpm_op_enc_bn_forward(eng._h, _p(z), _p(gamma), _p(beta), None, None, 1, C.c_float(1e-5), C.c_float(0.1), None, None,
                                                            _p(mr), _p(y), N, N, Cc, None), [mr, y])
    dz, dg, dbt = out(1, N, 1, Cc), out(Cc), out(Cc)
    both_sides(eng, qb, lambda: lib.cddpm_op_enc_bn_backward(eng._h, _p(z), _p(y), _p(dy), _p(mr), _p(gamma), None, 1, _p(dz), None, _p(dg), _p(dbt),
                                                             N, N, Cc, None), [dz, dg, dbt])


# ---------------------------------------------------------------------------------------------- (2) the rule without slack
ONE_LEVEL_0 = dict(model_channels=128, channel_mult=(1, 1), num_res_blocks=1, attention_resolutions=(1,), cond_dim=128, geometry=(2, 16, 24))
STEP_CASES = {"cond4": A.CASES["cond4"], "attn_levels": A.CASES["attn_levels"], "mult0_2": A.CASES["mult0_2"], "one_level_0": ONE_LEVEL_0,
              # cond4's UNet with the ResNet-50 trained jointly, at a geometry the encoder's own tests run
              "cond4+encoder": dict(A.CASES["cond4"], geometry=(3, 64, 96), encoder=True)}


def _step(tr, synth, case, overlap):
    """one training.training_step from freshly built trainers -> (gflat, flat[, the encoder's]) and the two arena sizes"""
    dev = torch.device("cuda", 0)
    B, H, W = case["geometry"]
    sd = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    trainer = tr.UNetTrainer({k: torch.from_numpy(v) for k, v in sd.items()}, device=dev, overlap_wgrad=overlap,
                             attention_resolutions=case["attention_resolutions"], **A.trainer_kw(case))
    enc = None
    try:
        if case.get("encoder"):
            esd = synth.synth_encoder_state_dict(0, num_classes=case["cond_dim"])
            enc = load_pkg("encoder_training").EncoderTrainer({k: torch.from_numpy(v) for k, v in esd.items()}, trainer)
        x01 = torch.from_numpy(synth.synth_slices(3, 0, B, H, W)).reshape(B, 1, H, W).to(dev)
        cond = torch.from_numpy(synth.synth_cond(3, 0, B, case["cond_dim"])).to(dev)
        noise = torch.from_numpy(synth.noise_xT(3, 0, B, H, W)).reshape(B, 1, H, W).to(dev)
        t = torch.tensor([(137 * (i + 1)) % 1000 for i in range(B)], dtype=torch.long, device=dev)
        loss = float(tr.training_step(trainer, x01, cond, t=t, noise=noise, encoder=enc))
        torch.cuda.synchronize(dev)
        assert loss == loss and trainer.step_count == 1 and trainer.skipped_steps == 0
        bits = [trainer.gflat.cpu(), trainer.flat.cpu()] + ([enc.gflat.cpu(), enc.flat.cpu()] if enc else [])
        return bits, tr.arena_bytes(trainer.program, B, H, W, 8 * trainer.C, trainer.cond_dim or 0)
    finally:
        trainer.close()


@pytest.mark.parametrize("overlap", [True, False], ids=["side_stream", "one_stream"])
@pytest.mark.parametrize("bits", [32, 16])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_steps_run_on_arenas_of_exactly_the_largest_call(synth, monkeypatch, train_precision, name, bits, overlap):
    tr = load_pkg("training")
    case = STEP_CASES[name]
    train_precision(bits)
    with_floor, arena = _step(tr, synth, case, overlap)
    assert arena == (tr.ARENA_FLOOR, tr.ARENA_FLOOR)           # at these geometries the floor is what the handles got
    monkeypatch.setattr(tr, "ARENA_FLOOR", 0)
    exact, arena0 = _step(tr, synth, case, overlap)             # no operator is refused (training_step raises on a refusal)
    assert 0 < arena0[1] <= arena0[0] < arena[0]
    for a, b in zip(with_floor, exact):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
        assert torch.equal(a, b)
