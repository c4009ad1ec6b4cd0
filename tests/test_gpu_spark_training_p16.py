"""GPU: SparK pre-training with `SparKTrainer(..., precision=16)` -- every convolution of the sparse ResNet-50 but the stem on the fp16-MFMA
operators, under a dynamic loss scale on the device -- and the Spark_2D mirror at `cfg.precision: 16`.

No end-to-end tolerance is asked of the precision-16 step: training-mode BatchNorm over as few as four active rows per channel amplifies one
convolution's fp16-grade difference beyond any meaningful bound (tests/test_gpu_encoder_training_p16.py explains it for the dense encoder,
which has more rows). What is checked instead: every convolution call of a real masked step on its own, at its real shape, against float64
on its own fp16-rounded inputs with the operator test's limit (tests/encoder_step_calls.py); the switch; and everything the loss scale
adds, bit for bit -- a step at device scale S against the same step driven by hand through the unscaled operators, the scale's trajectory
against torch._amp_update_scale_, a real overflow backing off, a checkpoint round trip."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import spark_reference as R
from conftest import load_pkg
from encoder_step_calls import check, record

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MASK_RATIO = 0.65
STAGE_SCALES = {"layer2.1": [1 / 0.9, 0.0, 1 / 0.9], "layer4.2": [0.0, 1 / 0.95, 1 / 0.95]}      # two fixed drop scales (B = 3)
FP16_MIN_NORMAL = 2.0 ** -14


@pytest.fixture(scope="module")
def params(synth):
    return {k[len("model."):]: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_spark_state_dict(0).items()}


def make(params, **kw):
    return load_pkg("spark_training").SparKTrainer(params, DEV, **kw)


def batch(B, side, seed=None):
    """x [B,1,side,side] in [0, 1] and the reference's cell mask at ratio 0.65 under a fixed seed"""
    torch.manual_seed(B + side if seed is None else seed)
    x = torch.rand(B, 1, side, side)
    return x.to(DEV), R.draw_mask(B, side // 32, MASK_RATIO).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def state(tr):
    return [t.clone() for t in (tr.flat, tr.enc.flat, tr.state["m"], tr.state["v"], tr.enc.state["m"], tr.enc.state["v"])]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def device_scale(tr):
    return tr.scaler[:1].view(torch.float32).cpu()


# ---------------------------------------------------------------------------------------------------------------- call by call
def underflow_by_stage(calls):
    """share of the non-zero elements of each stage's `dz` operands (the input gradient's source, the weight gradient's second operand)
    whose magnitude lies below fp16's smallest normal BEFORE rounding, and the largest magnitude"""
    out = {}
    for role, name, a, b, _hw, _o in calls:
        if role == "y":
            continue
        dz = (a if role == "dx" else b).abs()
        nz = dz[dz > 0]
        n, small, top = out.get(name.split(".")[0], (0, 0, 0.0))
        out[name.split(".")[0]] = (n + nz.numel(), small + int((nz < FP16_MIN_NORMAL).sum()), max(top, float(dz.max())))
    return {k: (small / max(n, 1), top) for k, (n, small, top) in sorted(out.items())}


@pytest.mark.parametrize("B,side,drop", [(4, 64, False), (3, 96, True)])
def test_every_convolution_of_a_masked_step_at_its_real_shape(params, B, side, drop):
    """52 forward convolutions, 52 input gradients, 52 weight gradients of one forward + backward under the default loss scaling. The
    (3, 96) case runs at the default start 65536 and prints, per stage, the share of non-zero dz operand elements below 2^-14 before
    rounding; the (4, 64) case overflows there and is checked at the scale the scaler backs off to."""
    x, active = batch(B, side)
    scales = {k: torch.tensor(v) for k, v in STAGE_SCALES.items()} if drop else {}
    names = {}
    for precision in (32, 16):
        tr = make(params, precision=precision)
        try:
            assert tr.precision == precision and tr.enc.precision == precision and tr.loss_scaling == (precision == 16)
            if precision == 16:
                assert tr.loss_scale == 65536.0 and all(t.dtype == torch.float16 for t in list(tr.enc.wf.values()) + list(tr.enc.wd.values()))
            calls = record(tr.enc)
            while True:
                calls.clear()
                loss, reco, latent = tr.forward(x, active, drop_scales=scales)
                grads = tr.backward()
                if precision == 32 or (bool(torch.isfinite(tr.gflat).all()) and bool(torch.isfinite(tr.enc.gflat).all())):
                    break
                # B = 4 with ONE active cell per sample: the gradient of a mean over so few pixels is large, 65536 x it passes 65504 inside
                # layer1..3 (fp32 run: largest |dz| 2.99 unscaled) and the step is one the scaler skips. The step that is checked is the
                # first one that would be applied, at the scale the scaler reaches for it.
                assert not drop and tr.consecutive_skips < 3, "the step does not go through at 2^13"
                tr.adamw_step(lr=1e-3)              # skipped: only the scale moves
            torch.cuda.synchronize()
            names[precision] = sorted((role, name) for role, name, *_ in calls)
            if precision == 32:
                continue
            print(f"{B} x {side} x {side}: checked at loss scale {tr.loss_scale:g} after {tr.skipped_steps} skipped steps")
            assert tr.step_count == 0 and (tr.loss_scale == 65536.0 or not drop)
            seen = check(tr.enc, calls)
            print({k: (n, f"{e:.1e}") for k, (n, e) in seen.items()})
            assert {k: n for k, (n, _e) in seen.items()} == {"y": 52, "dx": 52, "dw": 52}
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(reco).all()) and bool(torch.isfinite(latent).all())
            assert all(bool(torch.isfinite(g).all()) for g in list(grads.values()) + list(tr.enc.g.values()))
            shares = underflow_by_stage(calls)
            print(f"dz operands at scale {tr.loss_scale:g}, {B} x {side} x {side}: " +
                  ", ".join(f"{k}: {100 * s:.3f} % below 2^-14, largest {top:.3g}" for k, (s, top) in shares.items()))
            assert max(top for _s, top in shares.values()) < 65504.0
        finally:
            tr.close()
    assert names[16] == names[32] and len(names[16]) == 156             # the set of calls the same trainer issues at precision 32


# ---------------------------------------------------------------------------------------------------------------- the switch
def test_the_switch_and_the_repacked_images(params):
    """default == precision 32, bit for bit (loss, reconstruction, both gradient buffers); 16 differs in all of them; after adamw_step the
    fp16 images carry the updated weights (the next forward's calls are checked against the CURRENT parameters)"""
    B, side = 4, 64
    x, active = batch(B, side)
    res = []
    for kw in ({}, {"precision": 32}, {"precision": 16}):
        tr = make(params, **kw)
        if kw.get("precision") == 16:
            tr.enable_loss_scaling(init_scale=1.0)          # the same gradient scale as the other two: what differs is the arithmetic
        loss, reco, _latent = tr.forward(x, active, drop_scales={})
        tr.backward()
        torch.cuda.synchronize()
        res.append((tr, loss.clone(), reco.clone(), tr.gflat.clone(), tr.enc.gflat.clone()))
    try:
        (a, *ra), (b, *rb), (c, *rc) = res
        assert a.precision == b.precision == 32 and c.precision == 16 and not a.loss_scaling and not b.loss_scaling and c.loss_scaling
        assert all(t.dtype == torch.float32 for t in a.enc.wf.values()) and all(t.dtype == torch.float16 for t in list(c.enc.wf.values()) + list(c.enc.wd.values()))
        for u, v, w, what in zip(ra, rb, rc, ("loss", "reco", "gflat", "enc.gflat")):
            assert torch.equal(u, v), what
            assert not torch.equal(u, w), what
        flat0 = c.enc.flat.clone()
        c.adamw_step(lr=1e-3)
        assert not torch.equal(c.enc.flat, flat0) and c.step_count == 1
        calls = record(c.enc)
        loss2, _reco, _latent = c.forward(x, active, drop_scales={})
        seen = check(c.enc, calls)                 # stale images would miss the limit
        assert seen["y"][0] == 52 and bool(torch.isfinite(loss2)) and not torch.equal(loss2, rc[0])
        # evaluation-mode forwards run the same convolutions
        calls.clear()
        loss3, _reco, _latent = c.forward(x, active, training=False)
        seen = check(c.enc, calls)
        assert seen["y"][0] == 52 and set(seen) == {"y"} and bool(torch.isfinite(loss3))
    finally:
        for tr, *_ in res:
            tr.close()


# ---------------------------------------------------------------------------------------------------------------- a step at scale S
def test_a_step_at_device_scale_is_the_same_step_driven_by_hand(params):
    """S = 2^16, growth and back-off out of play: both flat parameter buffers and both pairs of moments equal, bit for bit, those of the
    existing operators driven by hand -- weights x S in cddpm_op_spark_loss, grad_unscale 1 / S in cddpm_op_adamw_guarded"""
    S, B, side = 2.0 ** 16, 3, 96                  # 3 x 96 x 96: nothing overflows at 2^16 (largest dz operand 1.4e4), both steps are applied
    lr, wd, betas, eps = 1e-3, 0.05, (0.9, 0.95), 1e-8
    x, active = batch(B, side)
    wm, wl = 0.5, 1.0
    dyn = make(params, precision=16, loss_weights=(wm, wl))
    hand = make(params, precision=16, loss_weights=(S * wm, S * wl))
    try:
        dyn.enable_loss_scaling(init_scale=S)
        hand.disable_loss_scaling()
        for step in range(2):
            loss_d, reco_d, _l = dyn.forward(x, active, drop_scales={})
            dyn.backward()
            dyn.adamw_step(lr=lr, weight_decay=wd, betas=betas, eps=eps)
            loss_h, reco_h, _l = hand.forward(x, active, drop_scales={})
            hand.backward()
            assert torch.equal(dyn.gflat, hand.gflat) and torch.equal(dyn.enc.gflat, hand.enc.gflat)         # both carry S
            lib, ctrl = hand.lib, hand.ctrl
            for t in (hand, hand.enc):
                if "m" not in t.state:
                    t.state["m"], t.state["v"] = torch.zeros_like(t.flat), torch.zeros_like(t.flat)
                assert lib.cddpm_op_grad_check(hand.h, _p(t.gflat), t.gflat.numel(), _p(ctrl), None) == 0
            assert lib.cddpm_op_guard_commit(hand.h, _p(ctrl), C.c_float(betas[0]), C.c_float(betas[1]), None) == 0
            for t in (hand, hand.enc):
                assert lib.cddpm_op_adamw_guarded(hand.h, _p(t.flat), _p(t.gflat), _p(t.state["m"]), _p(t.state["v"]), t.flat.numel(), C.c_float(lr),
                                                  C.c_float(betas[0]), C.c_float(betas[1]), C.c_float(eps), C.c_float(wd), C.c_float(1.0 / S), _p(ctrl), None) == 0
            hand.enc.repack()
            torch.cuda.synchronize()
            assert torch.equal(reco_d, reco_h) and float(loss_h) == pytest.approx(S * float(loss_d), rel=1e-6)       # the loss itself is unscaled
            assert same(state(dyn), state(hand)), step
        assert dyn.step_count == hand.step_count == 2 and dyn.skipped_steps == 0
        assert dyn.loss_scale == S and dyn.growth_tracker == 2 and dyn.consecutive_skips == 0
        assert bool(dyn.state["m"].any()) and bool(dyn.enc.state["m"].any())
    finally:
        dyn.close(), hand.close()


# ---------------------------------------------------------------------------------------------------------------- scaler dynamics
def test_the_scale_follows_torch_amp_update_scale(params):
    """10 steps at 4 x 64 x 64, growth interval 3, an inf written from the host into one gradient entry on steps 2, 3 and 7: after every
    step the device scale, tracker and consecutive skips are torch._amp_update_scale_'s on the same found-inf sequence (GradScaler's
    arithmetic); a skipped step moves and decays nothing and does not count. found-inf is taken from the gradient buffers by torch on
    every step, so the steps this small batch overflows by itself at the default start (the first two: one active cell per sample)
    are part of the sequence."""
    B, side = 4, 64
    x, active = batch(B, side)
    tr = make(params, precision=16)
    try:
        tr.enable_loss_scaling(growth_interval=3)
        assert tr.loss_scale == 65536.0
        inject = {2, 3, 7}
        scale_ref, tracker_ref = torch.tensor([65536.0]), torch.zeros(1, dtype=torch.int32)
        steps = skipped = run = 0
        seen, founds = [], []
        for t in (tr, tr.enc):
            t.state["m"], t.state["v"] = torch.zeros_like(t.flat), torch.zeros_like(t.flat)
        for i in range(10):
            tr.forward(x, active, drop_scales={})
            tr.backward()
            if i in inject:
                (tr.g["mask_tokens.1"] if i != 3 else tr.enc.g["layer3.2.conv2.weight"]).view(-1)[7] = float("inf")
            found = not (bool(torch.isfinite(tr.gflat).all()) and bool(torch.isfinite(tr.enc.gflat).all()))
            assert found or i not in inject
            before = state(tr)
            tr.adamw_step(lr=1e-3)
            torch._amp_update_scale_(scale_ref, tracker_ref, torch.tensor([1.0 if found else 0.0]), 2.0, 0.5, 3)
            steps, skipped, run = steps + (not found), skipped + found, (run + 1 if found else 0)
            assert torch.equal(device_scale(tr), scale_ref), (i, device_scale(tr), scale_ref)
            assert tr.growth_tracker == int(tracker_ref[0]) and tr.consecutive_skips == run, i
            assert tr.step_count == steps and tr.skipped_steps == skipped, i
            if found:
                assert same(state(tr), before), i
            else:
                assert bool(torch.isfinite(tr.flat).all()) and bool(torch.isfinite(tr.enc.flat).all())
                assert not torch.equal(tr.enc.flat, before[1]) and not torch.equal(tr.state["m"], before[2])
            seen.append(float(scale_ref[0]))
            founds.append(found)
        print("found inf", founds, "scale after each step", seen)
        assert steps >= 4 and any(b > a for a, b in zip(seen, seen[1:])) and any(b < a for a, b in zip(seen, seen[1:]))      # it backed off and grew
        assert tr.loss_scale == float(scale_ref[0])
    finally:
        tr.close()


def test_a_real_overflow_backs_off_until_a_step_goes_through(params):
    """init scale 2^40: the fp16 operands of the backward pass overflow, steps are skipped while the scale halves, then one goes through"""
    B, side = 4, 64
    x, active = batch(B, side)
    tr = make(params, precision=16)
    try:
        tr.enable_loss_scaling(init_scale=2.0 ** 40)
        flat0, enc0 = tr.flat.clone(), tr.enc.flat.clone()
        k = 0
        while tr.step_count == 0:
            assert k < 40, "no step went through within 40"
            S = tr.loss_scale
            tr.forward(x, active, drop_scales={})
            tr.backward()
            tr.adamw_step(lr=1e-3)
            if tr.step_count == 0:
                k += 1
                assert torch.equal(tr.flat, flat0) and torch.equal(tr.enc.flat, enc0) and tr.loss_scale == S / 2 and tr.consecutive_skips == k
        print(f"back-offs: {k} (2^40 -> 2^{int(math.log2(S))})")
        assert k >= 1 and tr.skipped_steps == k and tr.consecutive_skips == 0 and S == 2.0 ** (40 - k)
        assert bool(torch.isfinite(tr.flat).all()) and bool(torch.isfinite(tr.enc.flat).all())
        assert not torch.equal(tr.enc.flat, enc0)
    finally:
        tr.close()


def test_five_steps_train(params):
    """one fixed 4 x 64 x 64 batch, one fixed mask, default loss scaling: finite losses, the last clean step's below the first's"""
    x, active = batch(4, 64)
    tr = make(params, precision=16)
    try:
        losses, skipped = [], []
        for _ in range(5):
            loss, _reco, _latent = tr.forward(x, active, drop_scales={})
            tr.backward()
            n = tr.skipped_steps
            tr.adamw_step(lr=1e-3)
            losses.append(float(loss))
            skipped.append(tr.skipped_steps > n)
        print("losses", losses, "skipped", skipped, "loss scale", tr.loss_scale)
        assert np.isfinite(losses).all() and bool(torch.isfinite(tr.flat).all()) and bool(torch.isfinite(tr.enc.flat).all())
        clean = [v for v, s in zip(losses, skipped) if not s]
        assert len(clean) >= 2 and clean[-1] < clean[0]
    finally:
        tr.close()


def test_optimizer_state_carries_the_scaler(params):
    """the "scaler" key in UNetTrainer's layout; a state saved without it leaves the scaler as it is"""
    x, active = batch(4, 64)
    a, b = make(params, precision=16), make(params, precision=32)
    try:
        a.enable_loss_scaling(init_scale=2.0 ** 11, growth_interval=2)
        for _ in range(3):
            a.forward(x, active, drop_scales={})
            a.backward()
            a.adamw_step(lr=1e-3)
        st = a.optimizer_state()
        assert set(st["scaler"]) == {"init_scale", "growth_factor", "backoff_factor", "growth_interval", "growth_tracker", "state"}
        assert st["scaler"]["growth_interval"] == 2 and a.loss_scale == 2.0 ** 12 and a.growth_tracker == 1
        plain = b.optimizer_state()
        assert "scaler" not in plain and not b.loss_scaling
        b.load_optimizer_state({k: v for k, v in st.items() if k != "scaler"})
        assert not b.loss_scaling and b.step_count == 3                       # left as it was: off
        b.load_optimizer_state(st)                                             # loss scaling is available at 32 too
        assert b.loss_scaling and b.scaler_cfg == (2.0, 0.5, 2) and b.loss_scale == 2.0 ** 12 and b.growth_tracker == 1
        assert torch.equal(b.enc.state["m"], a.enc.state["m"]) and torch.equal(b.state["v"], a.state["v"])
        a.load_optimizer_state({k: v for k, v in plain.items()})
        assert a.loss_scaling and a.loss_scale == 2.0 ** 12                    # no "scaler" key: left as it was, on
        with pytest.raises(ValueError, match="power of two"):
            a.enable_loss_scaling(init_scale=1000.0)
        with pytest.raises(ValueError, match="growth_factor"):
            a.enable_loss_scaling(growth_factor=3.0)
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- the mirror
CFG = dict(backbone="resnet50", imageDim=[128, 128, 100], rescaleFactor=2, mask_ratio=0.65, pix_norm=False, lr=1e-3, loss_on_mask=True, precision=16)


def mirror(params, **over):
    """the mirror at a 64 x 64 input with the synthetic weights (only the image-norm buffer `norm_black` has the input's size: zeros)"""
    m = load_pkg("Spark_2D").Spark_2D(dict(CFG, **over), prefix="")
    sd = {"model." + k: v for k, v in params.items()}
    sd["model.norm_black"] = torch.zeros(1, 3, 64, 64)
    m.load_state_dict(sd)
    return m


def batch_of(x):
    return {"vol": {"data": x.unsqueeze(-1)}}


def test_the_mirror_warns_once_when_every_step_is_skipped(params):
    """a batch holding a NaN: every step is skipped; the consecutive skips are read every 50 steps and the first read that sees 30 or
    more warns, once (the DDPM_2D mirror's rule, tests/test_gpu_loss_scaling.py)"""
    import warnings
    m = mirror(params)
    try:
        x = torch.rand(4, 1, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
        x[0, 0, 5, 5] = float("nan")
        m.train()
        ours = lambda seen: [w for w in seen if issubclass(w.category, RuntimeWarning) and "skipped" in str(w.message)]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.manual_seed(1)
            for i in range(49):
                m.training_step(batch_of(x), i)
            assert ours(seen) == []
            m.training_step(batch_of(x), 49)
            assert len(ours(seen)) == 1, [str(w.message) for w in seen]
        tr = m._hip_spark_trainer
        assert tr.step_count == 0 and tr.skipped_steps == 50 and tr.consecutive_skips == 50 and tr.loss_scale == 65536.0 * 2.0 ** -50
        assert float(m.logged["train/skipped_steps"]) == 50.0
    finally:
        if m._hip_spark_trainer is not None:
            m._hip_spark_trainer.close()


def test_the_mirror_at_precision_16(params):
    m = mirror(params)
    made = [m]
    try:
        torch.manual_seed(21)
        x = torch.rand(4, 1, 64, 64).cuda()
        m.train()
        torch.manual_seed(5)
        losses = [float(m.training_step(batch_of(x), i)["loss"]) for i in range(3)]
        tr = m._hip_spark_trainer
        assert tr.precision == 16 and tr.enc.precision == 16 and tr.loss_scaling and tr.scaler_cfg == (2.0, 0.5, 2000)
        assert np.isfinite(losses).all() and tr.step_count + tr.skipped_steps == 3
        assert m.logged["train/loss_scale"].is_cuda and float(m.logged["train/loss_scale"]) == tr.loss_scale == 65536.0 * 0.5 ** tr.skipped_steps
        assert float(m.logged["train/skipped_steps"]) == tr.skipped_steps and float(m.logged["train/Loss_comb"]) == losses[-1]
        m.eval()
        out = m.validation_step(batch_of(x), 0)
        assert np.isfinite(float(out["loss"])) and float(m.logged["val/Loss_comb"]) == float(out["loss"])
        # checkpoint: weights, AdamW's moments, scale and tracker travel; a restored mirror continues bit for bit
        ckpt = {"state_dict": {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}}
        m.on_save_checkpoint(ckpt)
        sc = ckpt["hip_optimizer_state"]["spark"]["scaler"]
        assert sc["state"].device.type == "cpu" and ckpt["hip_optimizer_state"]["spark"]["step"] == tr.step_count
        m3 = mirror(params)
        made.append(m3)
        m3.load_state_dict(ckpt["state_dict"])
        m3.on_load_checkpoint(ckpt)
        m.train(), m3.train()
        for mod in (m, m3):
            torch.manual_seed(13)                   # mask (host generator) and stochastic depth (device generator) from the same seed
            for i in range(3):
                last = mod.training_step(batch_of(x), 3 + i)["loss"]
            mod.last_loss = last
        tr3 = m3._hip_spark_trainer
        assert torch.equal(tr3.scaler, tr.scaler) and tr3.growth_tracker == tr.growth_tracker and tr3.step_count == tr.step_count
        assert tr3.step_count + tr3.skipped_steps == 6 and torch.equal(m.last_loss, m3.last_loss)
        assert same(state(tr), state(tr3))
        for (ka, va), (kb, vb) in zip(m.state_dict().items(), m3.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        # a reference checkpoint: Lightning 1.5's GradScaler state seeds scale and tracker
        m4 = mirror(params)
        made.append(m4)
        m4.on_load_checkpoint({"native_amp_scaling_state": {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                                                             "_growth_tracker": 7}})
        m4.train()
        m4.training_step(batch_of(x), 0)
        tr4 = m4._hip_spark_trainer
        assert tr4.loss_scale == 1024.0 and tr4.growth_tracker == 8 and tr4.step_count == 1
    finally:
        for mod in made:
            if mod._hip_spark_trainer is not None:
                mod._hip_spark_trainer.close()
