"""GPU: the patched DDPM on the HIP path -- the three box kernels (cddpm_box_q_sample, cddpm_box_stitch, cddpm_op_loss_box) against the
torch restatement of tests/test_patched_host.py, GaussianDiffusion.p_losses_grid against the reference's recorded test_step
(tests/golden/patched) and against the per-box loop over the existing p_losses, the box training step against float64 autograd, and
the DDPM_2D_patched mirror. Shapes: 3 slices of 32 x 32, one 16 x 48 case (W = 48: vector path with another row length)."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from test_patched_host import (SAMPLER_OF, STITCH_OF, box_mask, patched_golden, ref_box_q_sample, ref_box_stitch, ref_loss_box)

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # tests/test_gpu_mirror.py::test_p_losses_box_and_inpaint_variants_vs_reference_golden, on its recos
S, H, W, T = 3, 32, 32, 1000
# one box per slice, two rounds (N = 6): 1 x 1 at the corner, past the edge, the full image | empty after clipping, zero width, odd start
ODD_BOXES = [[31, 31, 47, 47], [20, 25, 36, 41], [0, 0, 32, 32], [40, 40, 56, 56], [5, 5, 5, 9], [3, 7, 16, 20]]


def _bits_equal(a, b):
    """bitwise equal, NaN positions aside (which must coincide)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


def _data(synth, s=S, h=H, w=W):
    x01 = torch.from_numpy(synth.synth_slices(2, 0, s, h, w)).reshape(s, 1, h, w).cuda()
    noise = torch.from_numpy(synth.noise_z(3, 0, 0, s, h, w)).reshape(s, 1, h, w).cuda()
    return x01, noise


def _grid(patch, overlap, s, h, w):
    bs = load_pkg("patch_sampling").BoxSampler(dict(patch_size=patch, overlap=overlap))
    img = torch.zeros(s, 1, h, w)
    return bs.sample_grid(img).permute(1, 0, 2).contiguous(), bs.sample_grid_cut(img).permute(1, 0, 2).contiguous()     # box-major [K,S,4]


BOX_CASES = {"grid16": (S, H, W, 16, False), "grid12_ragged": (S, H, W, 12, False), "grid12_overlap": (S, H, W, 12, True),
             "odd": (S, H, W, None, None), "w48": (2, 16, 48, 16, False)}


def _case(name):
    s, h, w, patch, overlap = BOX_CASES[name]
    if patch is None:
        b = torch.tensor(ODD_BOXES).reshape(2, s, 4)
        return s, h, w, b, b
    return (s, h, w) + _grid(patch, overlap, s, h, w)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory(timesteps=T, max_batch=S, max_h=32, max_w=48)


@pytest.mark.parametrize("name", sorted(BOX_CASES))
def test_box_q_sample_is_q_sample_pasted_bitwise(eng, synth, name):
    s, h, w, boxes, _cut = _case(name)
    x01, noise = _data(synth, s, h, w)
    for t in (torch.tensor([350, 7, 999][:s]), 350):
        q = eng.q_sample(x01, t, noise)                          # the existing kernel: the arithmetic inside the box, to the bit
        K = boxes.shape[0]
        want = torch.where(box_mask(boxes.cuda(), h, w), q.repeat(K, 1, 1, 1), (x01 * 2 - 1).repeat(K, 1, 1, 1))
        got = eng.box_q_sample(x01, t.cuda() if isinstance(t, torch.Tensor) else t, noise, boxes)
        assert got.shape == (K * s, 1, h, w) and torch.equal(got, want), name
        sa, s1 = (torch.from_numpy(a).cuda() for a in eng._qs)
        tt = t.cuda() if isinstance(t, torch.Tensor) else torch.full((s,), t).cuda()
        ref = ref_box_q_sample(x01, noise, sa[tt], s1[tt], boxes.cuda())            # float64: within two fp32 roundings of values < 8
        assert float((got.double() - ref).abs().max()) < 1e-6 and torch.equal(got.double()[~box_mask(boxes.cuda(), h, w)], ref[~box_mask(boxes.cuda(), h, w)])
    if name == "odd":
        assert torch.equal(got[3], x01[0] * 2 - 1) and torch.equal(got[4], x01[1] * 2 - 1)        # empty boxes select nothing
        assert int((got[0] != x01[0] * 2 - 1).sum()) == 1                                          # the 1 x 1 box at (31, 31)
    with pytest.raises(RuntimeError):
        eng.box_q_sample(x01, 350, noise, boxes.reshape(-1, 4)[:s + 1])       # not a multiple of the slices
    with pytest.raises(RuntimeError, match="outside"):
        eng.box_q_sample(x01, T, noise, boxes)
    with pytest.raises(IndexError):
        eng.box_q_sample(x01, torch.tensor([0, T, 1][:s]), noise, boxes)


@pytest.mark.parametrize("mode", ["paste", "cut", "avg"])
@pytest.mark.parametrize("name", sorted(BOX_CASES))
def test_box_stitch_equals_the_restatement_bitwise(eng, synth, name, mode):
    s, h, w, boxes, cut = _case(name)
    K = boxes.shape[0]
    reco = torch.from_numpy(synth.noise_z(5, 0, 0, K * s, h, w)).reshape(K * s, 1, h, w).cuda() * 0.3 + 0.5
    got = eng.box_stitch(reco, boxes, cut, mode)
    want = ref_box_stitch(reco, boxes, cut, mode, s)            # on the device: torch's own division
    assert got.shape == (s, 1, h, w) and _bits_equal(got, want), (name, mode)
    if name == "odd":
        assert bool(torch.isnan(got).any()) == (mode == "avg")  # pixels in no box: 0 / 0 under 'avg', 0 under the paste modes
    if mode == "cut":
        with pytest.raises(RuntimeError):
            eng.box_stitch(reco, boxes, None, "cut")
    with pytest.raises(ValueError):
        eng.box_stitch(reco, boxes, cut, "mean")


@pytest.mark.parametrize("objective,loss_type,inpaint", [("pred_x0", "l1", True), ("pred_noise", "l2", False), ("pred_noise", "l1", True),
                                                          ("pred_x0", "l2", False)])
@pytest.mark.parametrize("name", ["odd", "w48"])
def test_loss_box_vs_float64(eng, synth, name, objective, loss_type, inpaint):
    s, h, w, boxes, _cut = _case(name)
    boxes = boxes.reshape(-1, 4)[[1, 5, 3][:s]] if name == "odd" else boxes[1]       # past the edge, odd start, empty | a grid cell
    x01, noise = _data(synth, s, h, w)
    x0 = x01 * 2 - 1
    out = torch.from_numpy(synth.noise_z(6, 0, 0, s, h, w)).reshape(s, 1, h, w).cuda() * 0.5
    w_b = torch.tensor([1.0, 0.5, 2.0][:s]).cuda()
    scale = 4096.0
    loss_b, dout = eng.loss_box(out, x0, noise, boxes, objective=objective, loss_type=loss_type, inpaint=inpaint, w_b=w_b, grad_scale=scale)
    o64 = out.double().requires_grad_(True)
    ref = ref_loss_box(o64, x0.double(), noise.double(), boxes.cuda(), objective == "pred_noise", inpaint, loss_type == "l2", w_b.double()).mean()
    ref.backward()
    loss = float(loss_b.double().mean())
    print(name, objective, loss_type, inpaint, "loss", loss, "ref", float(ref))
    assert abs(loss - float(ref)) < 2e-6 * max(1.0, abs(float(ref)))
    assert float((dout.double() / scale - o64.grad).abs().max()) <= 1e-6 * float(o64.grad.abs().max())
    if inpaint:
        assert float(dout[~box_mask(boxes.cuda(), h, w)].abs().max()) == 0.0
    only, none = eng.loss_box(out, x0, noise, boxes, objective=objective, loss_type=loss_type, inpaint=inpaint, w_b=w_b, want_grad=False)
    assert none is None and torch.equal(only, loss_b)
    scaler = load_pkg("training")._scaler_block(scale, 0, 0, out.device)
    l2_, d2_ = eng.loss_box(out, x0, noise, boxes, objective=objective, loss_type=loss_type, inpaint=inpaint, w_b=w_b, scaler=scaler)
    assert torch.equal(l2_, loss_b) and torch.equal(d2_, dout)                     # the device loss scale: the same bits


# ---- p_losses_grid ---------------------------------------------------------------------------------------------------------------
def _uncond_diffusion(synth, objective, loss_type, inpaint):
    U, D = load_pkg("OpenAI_Unet"), load_pkg("cond_DDPM")
    m = U.UNetModel(image_size=(H, W), in_channels=1, model_channels=128, out_channels=1, num_res_blocks=3,
                    attention_resolutions=(3, 6, 12), dropout=0, channel_mult=[1, 2, 2], conv_resample=True, dims=2,
                    num_classes=None, use_checkpoint=False, use_fp16=True, num_heads=1, num_head_channels=64,
                    num_heads_upsample=-1, use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True,
                    use_spatial_transformer=False, transformer_depth=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, num_classes=None).items()}, strict=True)
    return D.GaussianDiffusion(m, image_size=(H, W), timesteps=T, sampling_timesteps=T, objective=objective, channels=1,
                               loss_type=loss_type, p2_loss_weight_gamma=0, inpaint=inpaint, cfg=None).cuda()


OBJ = {"x0_l1_inpaint": ("pred_x0", "l1", True), "noise_l2_box": ("pred_noise", "l2", False)}


@pytest.mark.parametrize("oname", sorted(OBJ))
def test_p_losses_grid_vs_reference_test_step_and_the_per_box_loop(synth, oname):
    """every stitch combination of the fixture on ONE handle, created by the batched call first (chunk = K S = 27 at the most). Against
    the reference: reco within TOL, loss within 1e-5. Against the per-box loop over the existing p_losses + torch paste, for chunk in
    {K S, 5, 1}: the stitched volume bit for bit (the engine's batch invariance on one handle); the loss, which the loop forms with
    torch's fp32 mean and p_losses_grid with cddpm_op_loss_box's fixed-order float64 sum, within that kernel's own bound."""
    PS = load_pkg("patch_sampling")
    d = _uncond_diffusion(synth, *OBJ[oname])
    x01, noise = _data(synth)
    x_start = x01 * 2 - 1
    t = torch.full((S,), 350, device="cuda", dtype=torch.long)
    try:
        for sname in ("p12_overlap_avg", "p12_overlap_cut", "p12_ragged_paste", "p16_paste"):      # K = 9 first: the largest handle
            g = patched_golden(f"{sname}__{oname}")
            bs = PS.BoxSampler(dict(SAMPLER_OF[sname]))
            boxes, cut = bs.sample_grid(x01), bs.sample_grid_cut(x01)              # [S,K,4]
            K, mode = boxes.shape[1], STITCH_OF[sname]
            loss, reco = d.p_losses_grid(x_start, t, boxes, noise, stitch=mode, cut=cut, chunk=K * S)
            handle = d.model._hip.engine
            vol = torch.from_numpy(g["final_volume"])[0, 0].permute(2, 0, 1).unsqueeze(1)
            e_reco, e_loss = float((reco.cpu() - vol).abs().max()), abs(float(loss) - float(g["loss_diff"]))
            print(sname, oname, "reco", e_reco, "loss", e_loss)
            assert e_reco < TOL and e_loss < 1e-5
            recos = []
            for k in range(K):
                loop_loss, r = d.p_losses(x_start, t, noise=noise, box=boxes[:, k])
                recos.append(r)
            want = ref_box_stitch(torch.cat(recos), boxes.permute(1, 0, 2), cut.permute(1, 0, 2), mode, S)
            assert d.model._hip.engine is handle                                   # not rebuilt in between
            assert abs(float(loss) - float(loop_loss)) < 2e-6 * max(1.0, abs(float(loop_loss)))
            for chunk in (K * S, 5, 1):
                l2_, r2_ = d.p_losses_grid(x_start, t, boxes, noise, stitch=mode, cut=cut, chunk=chunk)
                assert _bits_equal(r2_, want), (sname, chunk)
                assert torch.equal(l2_, loss)
        with pytest.raises(RuntimeError):
            d.p_losses_grid(x_start, t, boxes, noise, stitch="cut")                # no cut boxes
        with pytest.raises(ValueError):
            d.p_losses_grid(x_start, t, boxes, noise, stitch="mean")
    finally:
        d.model._hip.close()


# ---- training ----------------------------------------------------------------------------------------------------------------------
TRAIN_BOXES = [[6, 9, 22, 21], [24, 20, 40, 36]]          # a 16 x 12 box, and a 16 x 16 box clipped at the edge to 8 x 12


@pytest.mark.parametrize("objective,loss_type,inpaint", [("pred_x0", "l1", True), ("pred_noise", "l2", False)])
def test_box_training_step_gradients_vs_autograd(oracle, synth, objective, loss_type, inpaint):
    """the two-link check of tests/test_gpu_training.py on the box-noised input: (1) cddpm_op_loss_box against autograd of the loss formula
    at the HIP forward's own output, (2) the backward pass against the float64 oracle's vector-Jacobian product for that dL/d(out)."""
    tr = load_pkg("training")
    B = 2
    sd_np = synth.synth_state_dict(0, num_classes=None)
    x01 = torch.from_numpy(synth.synth_slices(3, 0, B, H, W)).reshape(B, 1, H, W)
    noise = torch.from_numpy(synth.noise_xT(3, 0, B, H, W)).reshape(B, 1, H, W)
    t = torch.tensor([(137 * (i + 1) + 3) % T for i in range(B)], dtype=torch.long)
    boxes = torch.tensor(TRAIN_BOXES)
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
    buf64 = oracle.to_float64(oracle.schedule_buffers(T))
    x0 = x01 * 2 - 1
    m = box_mask(boxes, H, W)
    xt64 = torch.where(m, oracle.q_sample(x0.double(), t, noise.double(), buf64), x0.double())
    ref_out = oracle.unet_forward(xt64, t, None, sd)
    p2w64 = buf64["p2_loss_weight"][t]
    ref_loss = float(ref_loss_box(ref_out.detach(), x0.double(), noise.double(), boxes, objective == "pred_noise", inpaint, loss_type == "l2", p2w64).mean())

    dev = torch.device("cuda", 0)
    trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, cond_dim=None, device=dev)
    buf = load_pkg("schedule").schedule_buffers(T)
    trainer._fit(B, H, W)
    tables = tuple(buf[k].to(dev) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"))
    xt = trainer.eng.box_q_sample(x01.to(dev), t.to(dev), noise.to(dev), boxes, tables=tables)
    assert float((xt.double().cpu() - xt64).abs().max()) < 1e-6
    out = trainer.forward(xt, t.to(dev), None)
    assert float((out.double().cpu() - ref_out.detach()).abs().max()) < 2e-5
    loss, dout = trainer.loss_and_grad_box(out, x0.to(dev), noise.to(dev), boxes.to(dev, torch.int32), buf["p2_loss_weight"][t].to(dev).contiguous(),
                                           loss_type, objective, inpaint)
    assert abs(float(loss) - ref_loss) < 2e-6 * max(1.0, abs(ref_loss))
    o64 = out.double().cpu().requires_grad_(True)
    ref_loss_box(o64, x0.double(), noise.double(), boxes, objective == "pred_noise", inpaint, loss_type == "l2", p2w64).mean().backward()
    Sc = trainer.grad_scale
    assert float((dout.double().cpu() / Sc - o64.grad).abs().max()) <= 1e-6 * float(o64.grad.abs().max())
    grads = trainer.backward(dout)
    torch.cuda.synchronize()
    ref_out.backward(dout.double().cpu() / Sc)
    worst = []
    for k, v in sd.items():
        r = v.grad
        assert float(r.abs().max()) > 1e-12, k          # the precondition: a small box must not turn the relative measure into noise
        gk = grads[k].double().cpu().reshape(r.shape) / Sc
        assert torch.isfinite(gk).all(), k
        worst.append((float((gk - r).abs().max() / r.abs().max()), k))
    worst.sort(reverse=True)
    print("worst relative gradient errors:", [(f"{e:.2e}", k) for e, k in worst[:5]], "median", float(np.median([e for e, _ in worst])))
    assert worst[0][0] < 1e-4, worst[:5]
    assert float(np.median([e for e, _ in worst])) < 1e-5
    trainer.close()


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------
def _mirror(synth, **extra):
    P = load_pkg("DDPM_2D_patched")
    cfg = dict(imageDim=[96, 96, 5], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], patch_size=16, grid_boxes=True, inpaint=True,
               objective="pred_x0", loss="l1", test_timesteps=351, lr=1e-4, resizedEvaluation=True, erodeBrainmask=True, medianFiltering=True,
               evalSeg=True, threshold="auto", **extra)
    mod = P.DDPM_2D(cfg)
    mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, num_classes=None).items()}, strict=True)
    return mod.cuda()


def test_mirror_trains_evaluates_and_checkpoints(synth):
    mod = _mirror(synth, num_eval_slices=3)
    try:
        x01, _n = _data(synth, 2)
        batch = {"vol": {"data": x01.unsqueeze(-1)}}

        def probe():
            torch.manual_seed(5)
            return float(mod.validation_step(batch, 0)["loss"])
        before = probe()
        torch.manual_seed(0)
        for i in range(6):
            assert np.isfinite(float(mod.training_step(batch, i)["loss"]))
        after = probe()
        print("probe validation loss", before, "->", after)
        assert after < before
        # checkpoint round trip: Adam's state travels
        ck = {}
        mod.on_save_checkpoint(ck)
        st = ck["hip_optimizer_state"]["unet"]
        assert int(st["ctrl"][1]) == 6 and float(st["m"].abs().max()) > 0
        other = _mirror(synth, num_eval_slices=3)
        other.load_state_dict(mod.state_dict())
        other.on_load_checkpoint(ck)
        tr2 = other.hip_trainer(torch.device("cuda", 0))
        assert tr2.step_count == 6 and torch.equal(tr2.state["m"].cpu(), st["m"]) and torch.equal(tr2.state["v"].cpu(), st["v"])
        tr2.close()
        other.diffusion.model._hip.close()
        # test_step: the 3 centre slices of 5, equal to p_losses_grid on them; eval_dict filled through the native _test_step
        vol5, _n = _data(synth, 5)
        vol = vol5[:, 0].permute(1, 2, 0)[None, None].contiguous()                 # [1,1,32,32,5]
        mod.on_test_start()
        tb = {"Dataset": ["synthetic"], "vol": {"data": vol}, "vol_orig": {"data": vol}, "seg_orig": {"data": (vol > 0.9).float()},
              "mask_orig": {"data": torch.ones_like(vol)}, "seg_available": True, "ID": ["v0"], "stage": "val", "label": 1}
        torch.manual_seed(9)
        out = mod.test_step(tb, 0)
        assert out["final_volume"].shape == (1, 1, 32, 32, 3) and out["ind_offset"] == 1
        sl = vol5[1:4]
        torch.manual_seed(9)
        noise = torch.randn_like(sl)
        t = torch.full((3,), 350, device="cuda", dtype=torch.long)
        loss, reco = mod.diffusion.p_losses_grid(sl * 2 - 1, t, mod.boxes.sample_grid(sl), noise)
        assert torch.equal(out["final_volume"][0, 0].permute(2, 0, 1).unsqueeze(1), reco) and torch.equal(out["loss"], loss)
        ed = mod.eval_dict
        assert len(ed["AnomalyScoreRegPerVol"]) == 1 and abs(ed["AnomalyScoreRegPerVol"][0] - float(loss)) < 1e-7
        assert len(ed["l1recoErrorAll"]) == 1 and np.isfinite(ed["l1recoErrorAll"][0]) and ed["labelPerVol"] == [1]      # the native _test_step
        assert len(ed["AUPRCPerVol"]) == 1 and ed["IDs"] == ["v0"]
    finally:
        if getattr(mod, "_hip_unet_trainer", None) is not None:
            mod._hip_unet_trainer.close()
        mod.diffusion.model._hip.close()
