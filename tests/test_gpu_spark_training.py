"""GPU: one whole SparK pre-training step (spark_training.SparKTrainer over csrc/spark_train.hip and the encoder's training operators)
against float64 autograd through tests/spark_reference.py's restatement, at synth_spark_state_dict(0), with the implementation's own
cell mask and activation masks (the yardstick differentiates the branch the implementation is on: oracle/encoder_oracle.py's docstring).

Bounds. tools/spark_fp32_yardstick.py measures, on the CPU, how far torch's own fp32 run of the restatement lies from its float64 run at
these two cases in these metrics (tests/spark_step_cases.py); the step is allowed 4 x that (the dense encoder's test allows 3.6 x its
measured 5.6e-5; a sparse BatchNorm over 12 rows per channel is worse conditioned than the dense network's 16 and more):

    case      loss      reco      latent    running   worst gradient   median gradient
    b12_64    1.11e-06  1.71e-04  9.77e-05  3.06e-05  4.62e-04         2.59e-04      measured
    b4_96     5.63e-07  1.21e-04  7.09e-05  2.22e-05  7.75e-04         3.77e-04      measured
    bounds    4 x each figure of the case's row (BOUNDS below)

The 64 x 64 case runs at B = 12, not 8: at B = 8 (one active cell per sample, 8 rows per channel in layer4) torch's fp32 run itself is
1.25e-3 from float64 in its worst gradient (layer1.1.bn1.weight; loss 6.2e-6, reco 1.9e-4, median gradient 4.8e-4); at B = 12 it is stable
under 1e-3 (the row above; B = 16: worst 5.4e-4, median 2.7e-4). Both cases then have 12 active rows per channel in layer4."""
import numpy as np
import pytest
import torch

import spark_reference as R
from conftest import load_pkg
from spark_step_cases import CASES, case_inputs, step_metrics

pytestmark = pytest.mark.gpu

# 4 x the measured fp32 figures above, per case: (loss, reco, latent, running, worst gradient, median gradient)
BOUNDS = {
    "b12_64": (4 * 1.11e-06, 4 * 1.71e-04, 4 * 9.77e-05, 4 * 3.06e-05, 4 * 4.62e-04, 4 * 2.59e-04),
    "b4_96": (4 * 5.63e-07, 4 * 1.21e-04, 4 * 7.09e-05, 4 * 2.22e-05, 4 * 7.75e-04, 4 * 3.77e-04),
}
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sd_np(synth):
    return synth.synth_spark_state_dict(0)


def make_trainer(sd_np, **kw):
    st = load_pkg("spark_training")
    return st.SparKTrainer({k[len("model."):]: torch.from_numpy(v) for k, v in sd_np.items()}, DEV, **kw)


def implementation_masks(tr, reco, x):
    """the branch the HIP forward is on, from the activations it saved (NHWC) and its reconstruction -> spark_reference's act_masks"""
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu()
    sv = tr.enc.saved_pyramid
    acts = {"bn1": nchw(sv["a0"])}
    for bk in tr.enc.blocks:
        r, n = sv[bk["name"]], bk["name"]
        acts[n + ".bn1"], acts[n + ".bn2"], acts[n + ".out"] = nchw(r["a1"]), nchw(r["a2"]), nchw(r["out"])
    for i, r in enumerate(tr.saved["dec"]):
        acts[f"dec.{i}"] = nchw(r["a1"])
    acts["l1"] = reco.cpu() - x                                   # fp32, as the loss kernel forms it
    return R.masks_of(acts)


def implementation_result(tr, loss, reco, latent, grads_of):
    """the trainer's outputs under the reference's names"""
    pre = "model." + load_pkg("spark_training").ENC_PREFIX
    stats = {pre + k: v.cpu() for k, v in tr.enc.buf.items()}
    stats.update({"model." + k: v.cpu() for k, v in tr.buf.items()})
    grads = {pre + k: v.cpu() for k, v in grads_of(tr.enc).items()}
    grads.update({"model." + k: v.cpu() for k, v in grads_of(tr).items()})
    return dict(loss=loss.cpu(), reco=reco.cpu(), latent=latent.cpu(), stats=stats, grads=grads)


@pytest.mark.parametrize("name", list(CASES))
def test_whole_step_against_float64_autograd(sd_np, name):
    B, S, on_mask, delta, drop = CASES[name]
    x, active, scales, kw = case_inputs(name)
    tr = make_trainer(sd_np, loss_weights=(1.0, 0.0) if on_mask else (delta, 1.0), drop_path_rate=0.0)
    try:
        loss, reco, latent = tr.forward(x.to(DEV), active.to(DEV), drop_scales=scales)
        masks = implementation_masks(tr, reco, x)
        tr.backward()
        torch.cuda.synchronize()
        got = implementation_result(tr, loss, reco, latent, lambda t: t.g)
    finally:
        tr.close()
    sd = R.to_torch(sd_np, torch.float64)
    leaves = {k: v.requires_grad_(True) for k, v in sd.items()
              if v.dtype == torch.float64 and "running" not in k and k.split(".")[1] not in ("imn_m", "imn_s", "norm_black")}
    stats = {}
    ref = R.spark_forward(x.double(), sd, active, drop_scales=scales, stats=stats, act_masks=masks, **kw)
    ref["loss"].backward()
    assert set(got["grads"]) == set(leaves) and set(got["stats"]) == set(stats)
    for k, g in got["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    m = step_metrics(got, dict(loss=ref["loss"].detach(), reco=ref["reco"].detach(), latent=ref["latent"].detach(), stats=stats,
                               grads={k: v.grad for k, v in leaves.items()}))
    print(name, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in m.items()})
    b = BOUNDS[name]
    assert m["grad_tensors"] == 221
    assert m["loss"] <= b[0] and m["reco"] <= b[1] and m["latent"] <= b[2] and m["running"] <= b[3]
    assert m["grad_worst"] <= b[4] and m["grad_median"] <= b[5]


def test_three_adamw_steps_follow_torch_and_the_loss_falls(sd_np):
    """Adam's first updates are lr * sign(g) for every element, however small g is, so parameters after a step are not a continuous function
    of the gradients and cannot be compared with a float64 run element by element. What is compared instead is well conditioned:
    (a) the update itself: torch.optim.AdamW(lr, weight_decay 0.05, betas (0.9, 0.95)) over the restatement's parameters (fp32, as the
        reference runs it), fed the implementation's gradients, lands where adamw_step lands -- every tensor of both buffers, decay
        included (fp32 rounding of three updates: 2e-6 of the tensor's maximum, the limit of tests/test_gpu_spark_ops.py's AdamW test);
    (b) the loss the implementation reports at every step is the restatement's float64 loss at the implementation's current parameters,
        within the whole-step bound on the loss;
    and the loss falls. Then an inf in one gradient: nothing moves, nothing decays, the step does not count."""
    name = "b4_96"
    B, S, on_mask, delta, drop = CASES[name]
    x, active, scales, kw = case_inputs(name)
    lr, wd, betas = 1e-3, 0.05, (0.9, 0.95)
    tr = make_trainer(sd_np, loss_weights=(delta, 1.0), drop_path_rate=0.0)
    pre = "model." + load_pkg("spark_training").ENC_PREFIX
    try:
        sd = R.to_torch(sd_np, torch.float32)
        names = [pre + k for k in tr.enc.p] + ["model." + k for k in tr.p]
        params = [sd[k].requires_grad_(True) for k in names]
        opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd, betas=betas)
        losses = []
        for step in range(3):
            loss, _reco, _latent = tr.forward(x.to(DEV), active.to(DEV), drop_scales={})
            cur = {k: v.detach().double().cpu() for k, v in tr.state_dict().items()}
            with torch.no_grad():
                ref = R.spark_forward(x.double(), {"model." + k: v for k, v in cur.items()}, active, **kw)
            losses.append(float(loss))
            assert abs(losses[-1] - float(ref["loss"])) <= BOUNDS[name][0] * abs(float(ref["loss"])), (step, losses[-1], float(ref["loss"]))
            tr.backward()
            for k, p_ in zip(names, params):
                g = tr.enc.g[k[len(pre):]] if k.startswith(pre) else tr.g[k[len("model."):]]
                p_.grad = g.cpu().reshape(p_.shape).clone()
            opt.step()
            tr.adamw_step(lr=lr, weight_decay=wd, betas=betas)
        torch.cuda.synchronize()
        now = tr.state_dict()
        worst = max(R_rel(now[k[len("model."):]], p_.detach()) for k, p_ in zip(names, params))
        print("losses", losses, "worst parameter difference after three steps", worst)
        assert worst <= 2e-6 and losses[2] < losses[0] and tr.step_count == 3
        # a non-finite gradient anywhere: no update, no decay, no step
        tr.forward(x.to(DEV), active.to(DEV), drop_scales={})
        tr.backward()
        tr.g["mask_tokens.2"].view(-1)[5] = float("inf")
        before = (tr.flat.clone(), tr.enc.flat.clone())
        tr.adamw_step(lr=lr, weight_decay=wd, betas=betas)
        torch.cuda.synchronize()
        assert torch.equal(tr.flat, before[0]) and torch.equal(tr.enc.flat, before[1])
        assert tr.step_count == 3 and tr.skipped_steps == 1
    finally:
        tr.close()


def R_rel(got, want):
    want = want.double()
    return float((got.double().cpu().reshape(want.shape) - want).abs().max() / (want.abs().max() + 1e-30))


def test_evaluation_forward_uses_and_keeps_the_running_statistics(sd_np):
    x, active, _scales, kw = case_inputs("b4_96")
    tr = make_trainer(sd_np, loss_weights=(0.5, 1.0))
    try:
        before = {k: v.clone() for k, v in {**tr.buf, **tr.enc.buf}.items()}
        loss, reco, latent = tr.forward(x.to(DEV), active.to(DEV), training=False)
        torch.cuda.synchronize()
        assert all(torch.equal(v, {**tr.buf, **tr.enc.buf}[k]) for k, v in before.items())
        with pytest.raises(RuntimeError, match="no training-mode forward"):
            tr.backward()
    finally:
        tr.close()
    with torch.no_grad():
        ref = R.spark_forward(x.double(), R.to_torch(sd_np, torch.float64), active, training=False, **kw)
    e = [R_rel(loss, ref["loss"]), R_rel(reco, ref["reco"]), R_rel(latent, ref["latent"])]
    print("evaluation mode: loss, reco, latent rel err", e)
    b = BOUNDS["b4_96"]         # running statistics are better conditioned than 12-row batch statistics: the training-mode scale bounds it
    assert e[0] <= b[0] and e[1] <= b[1] and e[2] <= b[2]
