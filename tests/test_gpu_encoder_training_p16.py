"""GPU: the context encoder's training step with `EncoderTrainer(..., precision=16)` -- every convolution but the stem on the fp16-MFMA
operators (csrc/encoder_train_p16.hip), what the reference's `precision: 16` autocast computes for self.encoder
(configs/trainer/default.yaml:7; src/models/DDPM_2D.py:114-135). No end-to-end tolerance against an independent run means anything here:
training-mode BatchNorm over as few as 16 samples per channel amplifies one convolution's fp16-grade difference to several percent of the
context and tens of percent of a median gradient (a float64 run with fp32- against fp64-accumulated convolutions already differs by 2e-2).
So every convolution call of a real step is recorded at its real shape and checked on its own, against float64 arithmetic on its own
rounded inputs, with the operator test's limit (tests/test_gpu_encoder_ops_p16.py)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from encoder_step_calls import build, check, record

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W,drop", [(4, 64, 64, False), (3, 64, 96, True)])
def test_every_convolution_of_a_step_at_its_real_shape(synth, B, H, W, drop):
    """52 forward convolutions, their 52 input gradients (the trainer issues the first block's too: the max pool's backward needs it) and 52
    weight gradients. The upstream gradient is 8 randn: measured on the CPU, the rounded backward is the same at scale 8 and 64 to 1e-10,
    loses 1e-3 to underflow at 1 and overflows at 2^10."""
    enc = build(synth, B, H, W, precision=16)
    assert enc.precision == 16 and all(t.dtype == torch.float16 for t in list(enc.wf.values()) + list(enc.wd.values()))
    torch.manual_seed(B + H)
    x = torch.rand(B, 1, H, W).cuda()
    dcond = (8 * torch.randn(B, 128)).cuda()
    scales = None
    if drop:
        scales = {"layer2.1": torch.tensor([1 / 0.9, 0.0, 1 / 0.9][:B]), "layer4.2": torch.tensor([0.0, 1 / 0.95, 1 / 0.95][:B])}
    calls = record(enc)
    out = enc.forward(x, drop_scales=scales)
    grads = enc.backward(dcond)
    seen = check(enc, calls)
    print({k: (n, f"{e:.1e}") for k, (n, e) in seen.items()})
    assert {k: n for k, (n, _e) in seen.items()} == {"y": 52, "dx": 52, "dw": 52}
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())


def test_the_switch_and_the_repacked_images(synth):
    """default == precision 32, bit for bit; 16 differs; after adam_step the p16 images carry the updated weights"""
    B, H, W = 4, 64, 64
    torch.manual_seed(3)
    x = torch.rand(B, 1, H, W).cuda()
    dcond = (8 * torch.randn(B, 128)).cuda()
    res = []
    for kw in ({}, {"precision": 32}, {"precision": 16}):
        enc = build(synth, B, H, W, **kw)
        out = enc.forward(x)
        enc.backward(dcond)
        torch.cuda.synchronize()
        res.append((enc, out.clone(), enc.gflat.clone()))
    assert res[0][0].precision == res[1][0].precision == 32 and res[2][0].precision == 16
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert not torch.equal(res[0][1], res[2][1]) and not torch.equal(res[0][2], res[2][2])
    enc = res[2][0]
    flat0 = enc.flat.clone()
    enc.adam_step(lr=1e-3)
    assert not torch.equal(enc.flat, flat0)
    calls = record(enc)                     # the forward's reference weights are the CURRENT parameters: stale images would miss the limit
    out = enc.forward(x)
    seen = check(enc, calls)
    assert seen["y"][0] == 52 and torch.isfinite(out).all() and not torch.equal(out, res[2][1])


def test_the_joint_step_trains_with_the_encoder_in_precision_16():
    """five joint steps (training_step(..., encoder=enc)) on one fixed 4 x 64 x 64 batch in a precision-16 process, dynamic loss scaling
    on: finite losses, and the last clean step's loss is below the first's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_grad_check.py"), "--encoder-precision", "16", "--joint-steps", "5", "4", "64", "64"],
                       env=dict(os.environ, CDDPM_TRAIN_PRECISION="16"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    print("skipped_steps", res["skipped_steps"], "loss_scale", res["loss_scale"])
    assert res["precision"] == 16 and res["encoder_precision"] == 16
    assert all(v == v and abs(v) != float("inf") for v in res["losses"]) and res["finite_parameters"]
    clean = [v for v, s in zip(res["losses"], res["skipped"]) if not s]
    assert len(clean) >= 2 and clean[-1] < clean[0]
