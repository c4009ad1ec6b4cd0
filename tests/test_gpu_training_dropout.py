"""GPU: training the UNet with dropout (`dropout_unet`; nn.Dropout between the SiLU and the second convolution of every ResBlock,
reference OpenAI_Unet.py:255). The device mask (csrc/train_kernels.hip: act_dropout / dropout_scale) against its host restatement
synth.dropout_mask bit for bit; the forward and every gradient against float64 autograd through the oracle given the same masks; dropout 0
is the trainer as it was; the mask sequence replays, resumes from optimizer_state() and does not depend on how slices are batched."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
T = 1000
SEED = 20240611
MASK_SHAPES = [(2, 16, 48, 128), (1, 8, 8, 256)]      # a 48-pixel row (no multiple of the convolution's 32-pixel tile); 256 channels


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=50, max_batch=2, max_h=16, max_w=48)


def _keep(synth, step, layer, slice0, shape, p):
    """mask / (1 - p) as the device forms it: the uint8 mask times the fp32 scale"""
    return torch.from_numpy(synth.dropout_mask(SEED, step, layer, slice0, *shape, p).astype(np.float32) * synth.dropout_scale(p))


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("slice0", [0, 5])
def test_mask_bits_and_dropout_scale_equal_the_host_restatement(eng, synth, shape, p, slice0):
    step, layer = 3, 7
    kw = dict(seed=SEED, step=step, slice0=slice0, stream_id=synth.STREAM_DROPOUT + layer, p=p)
    keep = _keep(synth, step, layer, slice0, shape, p)
    got = eng.op_act_dropout(torch.ones(shape, device="cuda"), None, False, **kw).cpu()
    assert torch.equal(got, keep)
    assert 0 < int((got == 0).sum()) < got.numel()
    torch.manual_seed(int(p * 10) + slice0)
    x = torch.randn(shape)
    assert torch.equal(eng.op_dropout_scale(x.cuda(), **kw).cpu(), x * keep)     # one fp32 product per kept element: exact


@pytest.mark.parametrize("seed", [(1 << 32) + SEED, (1 << 64) - 1], ids=["2^32+seed", "2^64-1"])
def test_mask_reads_the_high_word_of_a_64_bit_seed(eng, synth, seed):
    """the Philox key is (seed mod 2^32, seed >> 32): every other seed of this file is below 2^32 and leaves the second word zero"""
    shape, p, step, layer, slice0 = MASK_SHAPES[1], 0.5, 3, 7, 5
    kw = dict(step=step, slice0=slice0, stream_id=synth.STREAM_DROPOUT + layer, p=p)
    keep = torch.from_numpy(synth.dropout_mask(seed, step, layer, slice0, *shape, p).astype(np.float32) * synth.dropout_scale(p))
    got = eng.op_act_dropout(torch.ones(shape, device="cuda"), None, False, seed=seed, **kw).cpu()
    assert torch.equal(got, keep)
    low = eng.op_act_dropout(torch.ones(shape, device="cuda"), None, False, seed=seed & 0xFFFFFFFF, **kw).cpu()
    assert not torch.equal(got, low) and 0 < int((got == 0).sum()) < got.numel()


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act_dropout_with_coefficients_and_silu_vs_float64(eng, synth, shape):
    """out = mask s SiLU((x - m) a + d) with s = fp32(1 / (1 - p)), against float64 on the SAME fp32 coefficient plane. Bound, from the
    kernel's operations, each one fp32 rounding (2^-24 relative) of its result, results bounded by M = |x - m| |a| + |d| >= |u|:
    u = (x - m) a + d: three roundings, carried through SiLU (|SiLU'| <= 1.1): 3.3; sigmoid(u) = 1 / (1 + exp2(-u log2 e)): the constant
    and the product (their effect on u sigmoid(u) is |u|^2 s (1 - s) <= 0.9 of a rounding of |u| each): 2, exp2 and the reciprocal
    (hardware approximations, 1 ulp = 2 roundings each): 4, the addition: 1; u * sigmoid: 1; the scale's own rounding and the product
    with it: 2. Sum 13.3 -> |error| <= 14 * 2^-24 * s * M. Dropped elements are exactly 0."""
    B, H, W, C = shape
    p, step, layer, slice0 = 0.1, 1, 4, 2
    torch.manual_seed(C)
    x = (torch.randn(shape) * 1.7 + 0.6).cuda()
    gamma, beta, film = 1 + 0.1 * torch.randn(C), 0.1 * torch.randn(C), (0.3 * torch.randn(B, 2 * C)).cuda()
    coef = eng.op_gn_coef(x, None, gamma, beta, film)
    got = eng.op_act_dropout(x, coef, True, seed=SEED, step=step, slice0=slice0, stream_id=synth.STREAM_DROPOUT + layer, p=p).double().cpu()
    m, a, d = (coef[i].double().cpu()[:, None, None, :] for i in range(3))
    x64 = x.double().cpu()
    u = (x64 - m) * a + d
    mask = torch.from_numpy(synth.dropout_mask(SEED, step, layer, slice0, B, H, W, C, p)).double()
    s = float(synth.dropout_scale(p))
    ref = mask * s * u * torch.sigmoid(u)
    lim = 14 * 2.0 ** -24 * s * ((x64 - m).abs() * a.abs() + d.abs())
    ratio = float(((got - ref).abs() / lim).max())
    print(f"{shape}: max |error| / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert bool((got[mask == 0] == 0).all())


def test_bad_arguments_are_refused_with_a_message(eng, synth):
    x = torch.ones(1, 8, 8, 128, device="cuda")
    for bad in (1.0, -0.25, float("nan")):
        with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
            eng.op_act_dropout(x, None, False, seed=1, step=0, slice0=0, stream_id=synth.STREAM_DROPOUT, p=bad)
        with pytest.raises(RuntimeError, match=r"\[0, 1\)"):
            eng.op_dropout_scale(x, seed=1, step=0, slice0=0, stream_id=synth.STREAM_DROPOUT, p=bad)
    lib, h = eng.lib, eng._h
    assert lib.cddpm_op_act_dropout(h, None, None, 0, x.data_ptr(), 1, 0, 0, 0, 0.1, 1, 64, 128, None) != 0
    assert b"NULL" in lib.cddpm_last_error(h)
    assert lib.cddpm_op_dropout_scale(h, None, 1, 0, 0, 0, 0.1, 1, 64, 128, None) != 0
    assert b"NULL" in lib.cddpm_last_error(h)


# ---------------------------------------------------------------------------------------------------------------- the training step
def _inputs(synth, B, H, W, seed, slice0=0):
    x01 = torch.from_numpy(synth.synth_slices(seed, slice0, B, H, W)).reshape(B, 1, H, W)
    cond = torch.from_numpy(synth.synth_cond(seed, slice0, B))
    noise = torch.from_numpy(synth.noise_xT(seed, slice0, B, H, W)).reshape(B, 1, H, W)
    t = torch.tensor([(137 * (i + slice0 + 1) + seed) % T for i in range(B)], dtype=torch.long)
    return x01, cond, noise, t


def _loss_of(out, target, p2w, loss_type):
    d = out - target
    per = (d.abs() if loss_type == "l1" else d ** 2).reshape(d.shape[0], -1).mean(dim=1) * p2w
    return per.mean()


class _MaskedOracle:
    """the oracle's UNet with the trainer's dropout: while active, oracle._conv multiplies the input of every `*.out_layers.3`
    convolution by that ResBlock's synth.dropout_mask / (1 - p) (the oracle itself has no dropout: Dropout(p = 0) is the identity)"""

    def __init__(self, oracle, synth, program, seed, step, slice0, p):
        self.oracle, self.synth, self.key = oracle, synth, (seed, step, slice0, p)
        self.ordinal = {n: i for i, n in enumerate(n for kind, n, _a in program if kind == "res")}

    def __enter__(self):
        inner, (seed, step, slice0, p) = self.oracle._conv, self.key
        self.inner, self.seen = inner, 0

        def conv(x, sd, prefix, pad):
            if prefix.endswith(".out_layers.3"):
                B, C, H, W = x.shape
                m = self.synth.dropout_mask(seed, step, self.ordinal[prefix[:-len(".out_layers.3")]], slice0, B, H, W, C, p)
                keep = torch.from_numpy(m.astype(np.float32) * self.synth.dropout_scale(p)).permute(0, 3, 1, 2)
                x = x * keep.to(x.dtype)
                self.seen += 1
            return inner(x, sd, prefix, pad)

        self.oracle._conv = conv
        return self

    def __exit__(self, *exc):
        self.oracle._conv = self.inner
        assert exc[0] is not None or self.seen == len(self.ordinal)


def _check_against_autograd(oracle, synth, sd_np, B, H, W, objective, loss_type, p):
    """tests/test_gpu_training.py::test_loss_and_all_gradients_vs_autograd, link for link, with dropout p on both sides;
    -> (forward max|delta|, the fp32 oracle's own max|delta| or None, worst relative gradient errors, median)"""
    tr = load_pkg("training")
    x01, cond, noise, t = _inputs(synth, B, H, W, 3)
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
    buf64 = oracle.to_float64(oracle.schedule_buffers(T))
    x0 = x01 * 2 - 1
    dev = torch.device("cuda", 0)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, dropout=p, dropout_seed=SEED)
    try:
        masked = _MaskedOracle(oracle, synth, trainer.program, SEED, trainer.dropout_step, 0, p)
        with masked:
            ref_out = oracle.unet_forward(oracle.q_sample(x0.double(), t, noise.double(), buf64), t, cond.double(), sd)
        target = noise if objective == "pred_noise" else x0
        ref_loss = float(_loss_of(ref_out.detach(), target.double(), buf64["p2_loss_weight"][t], loss_type))
        buf = load_pkg("schedule").schedule_buffers(T)
        xt = (buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise)
        out = trainer.forward(xt.to(dev), t.to(dev), cond.to(dev))
        fwd = float((out.double().cpu() - ref_out.detach()).abs().max())
        yard = None
        if not fwd < 2e-5:       # the fp32 oracle's own distance from float64 on the same masked forward
            with masked, torch.no_grad():
                o32 = oracle.unet_forward(oracle.q_sample(x0, t, noise, oracle.schedule_buffers(T)), t, cond, {k: torch.from_numpy(v) for k, v in sd_np.items()})
            yard = float((o32.double() - ref_out.detach()).abs().max())
        # link 1: the loss kernel
        loss, dout = trainer.loss_and_grad(out, target.to(dev), buf["p2_loss_weight"][t].to(dev).contiguous(), loss_type)
        loss_err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
        o64 = out.double().cpu().requires_grad_(True)
        _loss_of(o64, target.double(), buf64["p2_loss_weight"][t], loss_type).backward()
        S = trainer.grad_scale
        assert S == 2 ** round(np.log2(S)) and S >= B * H * W
        assert float((dout.double().cpu() / S - o64.grad).abs().max()) <= 1e-6 * float(o64.grad.abs().max())
        # link 2: the backward pass
        grads = trainer.backward(dout)
        torch.cuda.synchronize()
        ref_out.backward(dout.double().cpu() / S)
        ref_g = {k: v.grad for k, v in sd.items()}
        assert set(grads) == set(ref_g), (set(ref_g) - set(grads), set(grads) - set(ref_g))
        worst = []
        for k in sorted(ref_g):
            r = ref_g[k]
            g = grads[k].double().cpu().reshape(r.shape) / S
            assert torch.isfinite(g).all(), k
            worst.append((float((g - r).abs().max() / (r.abs().max() + 1e-30)), k))
        worst.sort(reverse=True)
        return fwd, yard, loss_err, worst, float(np.median([e for e, _ in worst]))
    finally:
        trainer.close()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,W,objective,loss_type", [(2, 32, 32, "pred_x0", "l1"), (2, 16, 48, "pred_noise", "l2")])
def test_loss_and_all_gradients_vs_autograd_with_dropout(oracle, synth, sd_np, B, H, W, objective, loss_type, p):
    """The limits of tests/test_gpu_training.py::test_loss_and_all_gradients_vs_autograd: output within 2e-5 of float64, worst relative
    gradient error below 1e-4, median below 1e-5. At p = 0.5 (kept activations doubled in every ResBlock) an output over 2e-5 is held
    against the descriptor tests' yardstick instead: 4 x the fp32 oracle's own distance from float64 on the same masked forward."""
    fwd, yard, loss_err, worst, median = _check_against_autograd(oracle, synth, sd_np, B, H, W, objective, loss_type, p)
    print(f"p {p} {B}x{H}x{W} {objective}/{loss_type}: forward max|delta| {fwd:.3e}" + (f" (fp32 oracle {yard:.3e})" if yard is not None else ""),
          "worst relative gradient errors", [(f"{e:.2e}", k) for e, k in worst[:3]], f"median {median:.2e}")
    if p == 0.5 and yard is not None:
        assert fwd <= 4.0 * yard, (fwd, yard)
    else:
        assert fwd < 2e-5
    assert loss_err < 2e-6
    assert worst[0][0] < 1e-4, worst[:5]
    assert median < 1e-5


def test_precision16_gradients_with_dropout_are_fp16_grade(oracle, synth, sd_np):
    """one case in the reference trainer's precision-16 arithmetic, against the limits of
    tests/test_gpu_training.py::test_precision16_mode_gradients_are_fp16_grade"""
    tr = load_pkg("training")
    try:
        assert tr.set_precision(16) == 16
        fwd, _yard, _loss_err, worst, median = _check_against_autograd(oracle, synth, sd_np, 2, 32, 32, "pred_noise", "l2", 0.1)
    finally:
        tr.set_precision(32)
    print(f"precision 16, p 0.1: forward {fwd:.3e} worst {worst[0][0]:.3e} median {median:.3e}")
    assert len(worst) == 316
    assert fwd < 5e-3 and worst[0][0] < 2e-2 and median < 3e-3
    assert median > 1e-5


def _trainer(sd_np, **kw):
    dev = torch.device("cuda", 0)
    return load_pkg("training").UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **kw)


def _xt(synth, B, H, W, seed, slice0=0):
    x01, cond, noise, t = _inputs(synth, B, H, W, seed, slice0)
    buf = load_pkg("schedule").schedule_buffers(T)
    x0 = x01 * 2 - 1
    xt = buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise
    return xt.cuda(), t.cuda(), cond.cuda(), noise.cuda()


def test_dropout_zero_is_the_trainer_without_the_argument(synth, sd_np):
    a, b = _trainer(sd_np), _trainer(sd_np, dropout=0.0, dropout_seed=SEED)
    try:
        def refuse(*_a, **_k):
            raise AssertionError("act_dropout launched at dropout 0")
        b.act_dropout = b.dropout_scale_ = refuse
        xt, t, cond, noise = _xt(synth, 2, 32, 32, 5)
        res = []
        for tr_ in (a, b):
            out = tr_.forward(xt, t, cond)
            assert not any("a2" in v for v in tr_.saved.values() if isinstance(v, dict)) and "drop" not in tr_.saved
            loss, dout = tr_.loss_and_grad(out, noise, None, "l2")
            tr_.backward(dout)
            torch.cuda.synchronize()
            res.append((out, loss, dout, tr_.gflat.clone()))
        for u, v in zip(*res):
            assert torch.equal(u, v)
        assert b.dropout_step == 0 and "dropout" not in b.optimizer_state()
    finally:
        a.close(); b.close()


def test_mask_replays_in_backward_and_advances_with_every_forward(synth, sd_np):
    tr_ = _trainer(sd_np, dropout=0.1, dropout_seed=SEED)
    try:
        xt, t, cond, noise = _xt(synth, 2, 32, 32, 5)
        out0 = tr_.forward(xt, t, cond)
        saved = tr_.saved
        _loss, dout = tr_.loss_and_grad(out0, noise, None, "l2")
        tr_.backward(dout)
        g0 = tr_.gflat.clone()
        tr_.saved = saved                 # the same forward once more: the masks come from its counters, not from stored state
        tr_.backward(dout)
        assert torch.equal(tr_.gflat, g0)
        out1 = tr_.forward(xt, t, cond)   # the next dropout step
        assert tr_.dropout_step == 2 and not torch.equal(out0, out1)
        tr_.dropout_step = 0              # ... and step 0 again
        assert torch.equal(tr_.forward(xt, t, cond), out0)
    finally:
        tr_.close()


def test_a_resumed_run_continues_the_mask_sequence(synth, sd_np):
    tr = load_pkg("training")
    dev = torch.device("cuda", 0)
    a = _trainer(sd_np, dropout=0.1, dropout_seed=SEED)
    b = None
    try:
        batches = [tuple(v.to(dev) for v in _inputs(synth, 2, 32, 32, 11 + s)) for s in range(3)]
        step = lambda tr_, s: float(tr.training_step(tr_, batches[s][0], batches[s][1], t=batches[s][3], noise=batches[s][2], lr=1e-4))
        for s in range(2):
            step(a, s)
        params, state = {k: v.clone() for k, v in a.p.items()}, a.optimizer_state()
        assert state["dropout"] == {"seed": SEED, "step": 2}
        loss_a = step(a, 2)
        b = tr.UNetTrainer(params, device=dev, dropout=0.1, dropout_seed=SEED + 99)      # the seed comes back with the state
        b.load_optimizer_state(state)
        assert (b.dropout_seed, b.dropout_step) == (SEED, 2)
        loss_b = step(b, 2)
        assert loss_a == loss_b and torch.equal(a.flat, b.flat)
        c = dict(state); del c["dropout"]        # a state saved without dropout loads as before: seed and step stay
        b.load_optimizer_state(c)
        assert (b.dropout_seed, b.dropout_step) == (SEED, 3)
    finally:
        a.close()
        if b is not None:
            b.close()


def test_a_slices_mask_does_not_depend_on_its_batch(synth, sd_np):
    """slices 2-3 of a B = 4 forward equal a B = 2 forward with slice0 = 2 (same dropout step, the same handle: the trainer's handle
    keeps the geometry of the larger batch)"""
    tr_ = _trainer(sd_np, dropout=0.1, dropout_seed=SEED)
    try:
        xt, t, cond, _n = _xt(synth, 4, 32, 32, 5)
        full = tr_.forward(xt, t, cond, slice0=0)
        tr_.dropout_step = 0
        part = tr_.forward(xt[2:].contiguous(), t[2:].contiguous(), cond[2:].contiguous(), slice0=2)
        assert tr_.eng.max_batch == 4 and torch.equal(full[2:], part)
        tr_.dropout_step = 0
        assert not torch.equal(tr_.forward(xt[2:].contiguous(), t[2:].contiguous(), cond[2:].contiguous(), slice0=0), part)
    finally:
        tr_.close()


def test_mirror_passes_dropout_unet_to_training_only(sd_np, synth):
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=1000)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return x.flatten(1)[:, :128].contiguous()

    inp = torch.from_numpy(synth.synth_slices(2, 0, 3, 32, 32)).cuda()
    noise = torch.from_numpy(synth.noise_xT(3, 0, 3, 32, 32)).cuda()
    recos = []
    for p in (0.1, 0):
        mod = M.DDPM_2D(dict(cfg, dropout_unet=p), encoder=Enc())
        mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        mod = mod.cuda()
        trainer = mod.hip_trainer(inp.device)
        assert trainer.dropout == p
        _loss, reco = mod.reconstruct(inp, noise=noise)          # evaluation: no dropout, as under .eval()
        recos.append(reco.clone())
        trainer.close()
        mod.diffusion.model._hip.close()
    assert torch.equal(recos[0], recos[1])
