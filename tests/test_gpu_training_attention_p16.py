"""GPU: the training step with `attention_precision=16` -- every attention core of the program, forward and backward, on the fp16-MFMA
kernels (cddpm_op_attention_p16, cddpm_op_attention_backward_p16) -- at `attn_levels` (2 x 16 x 24, ten attention blocks) in a
precision-16 process, against float64 autograd through the oracle, with the limits of the project's precision-16 training tests
(test_gpu_training_attention.py::test_precision16_mode_gradients_are_fp16_grade_with_level_attention) unchanged; that the switch
reaches the trainer; and that `attention_precision=32` is the default trainer, bit for bit. The gradient checks run in processes of
their own through tools/train_grad_check.py: the convolutions' arithmetic is chosen once per process."""
import json
import os
import subprocess
import sys

import pytest
import torch

import arch_cases as A
from conftest import load_pkg
from test_gpu_training_attention import DESCRIPTORS, ONE_LEVEL, T, _inputs, _trainer_kw

pytestmark = pytest.mark.gpu

PROBE = "middle_block.1.qkv.weight"


def _grad_check(attention_precision):
    case = DESCRIPTORS["attn_levels"]
    B, H, W = case["geometry"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    desc = json.dumps({k: case[k] for k in ("model_channels", "channel_mult", "num_res_blocks", "cond_dim", "attention_resolutions")})
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_grad_check.py"), "--attention-precision", str(attention_precision),
                        "--gradient", PROBE, str(B), str(H), str(W), desc],
                       env=dict(os.environ, CDDPM_TRAIN_PRECISION="16"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs():
    """the two processes, once: precision-16 convolutions with p16 attention and with fp32 attention"""
    return {bits: _grad_check(bits) for bits in (16, 32)}


def test_precision16_gradients_with_p16_attention_are_fp16_grade(runs):
    """Measured on an MI355X (attn_levels, 2 x 16 x 24, CDDPM_TRAIN_PRECISION=16): forward 1.42e-3, worst relative
    gradient error 3.29e-3, median 1.08e-3, all 238 finite; with fp32 attention in the same visit 1.13e-3 / 4.23e-3 / 1.10e-3."""
    res = runs[16]
    print("precision 16, attention precision 16, attn_levels:", res)
    print("precision 16, attention precision 32, attn_levels:", runs[32])
    assert res["attention_precision"] == 16
    n = len(load_pkg("synth").unet_param_shapes(**A.synth_kw(DESCRIPTORS["attn_levels"])))
    assert n == 238
    assert res["finite"] and res["n"] == n
    assert res["forward_max_abs_err"] < 5e-3 and res["worst"] < 2e-2 and res["median"] < 3e-3
    assert res["median"] > 1e-5


def test_attention_precision_reaches_the_trainer(runs):
    a, b = runs[16], runs[32]
    assert a["attention_precision"] == 16 and b["attention_precision"] == 32
    assert b["finite"] and b["n"] == a["n"]
    assert a["gradient_sha256"] != b["gradient_sha256"]


def test_attention_precision_32_is_the_default_trainer(synth):
    """in-process, precision 32: a default trainer and one built with attention_precision=32 give bit-identical gradients"""
    tr = load_pkg("training")
    assert tr.get_precision() == 32
    case = ONE_LEVEL
    sd_np = synth.synth_state_dict(A.SEED_W, **A.synth_kw(case))
    x01, cond, noise, t = _inputs(synth, case, 3)
    dev = torch.device("cuda", 0)
    buf = load_pkg("schedule").schedule_buffers(T)
    x0 = x01 * 2 - 1
    xt = (buf["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * x0 + buf["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1, 1) * noise).to(dev)
    flats = []
    for kw in ({}, {"attention_precision": 32}):
        trainer = tr.UNetTrainer({k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}, device=dev, **_trainer_kw(case), **kw)
        try:
            assert trainer.attention_precision == 32
            out = trainer.forward(xt, t.to(dev), cond.to(dev))
            _loss, dout = trainer.loss_and_grad(out, noise.to(dev), buf["p2_loss_weight"][t].to(dev).contiguous(), "l2")
            trainer.backward(dout)
            torch.cuda.synchronize()
            flats.append((out.clone(), trainer.gflat.clone()))
        finally:
            trainer.close()
    assert torch.equal(flats[0][0], flats[1][0])
    assert torch.equal(flats[0][1], flats[1][1]) and bool(torch.isfinite(flats[0][1]).all()) and float(flats[0][1].abs().max()) > 0
