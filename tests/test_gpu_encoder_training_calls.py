"""GPU: every operator call of the context encoder's training step at the default precision (fp32 FMA convolutions, csrc/encoder_train.hip),
each at its real shape and checked on its own. tests/test_gpu_encoder_training.py compares whole-network gradients and has to allow 2e-4 to
1e-3, because training-mode BatchNorm amplifies whatever one operator adds; here each of the 156 convolution calls, the 53 + 53 BatchNorm
calls, the stem, the two pools and the stem's weight gradient is held to the limit of its operator test (tests/test_gpu_encoder_ops.py),
against float64 arithmetic on the call's own inputs (the same construction as tests/test_gpu_encoder_training_p16.py, whose helpers this
shares: tests/encoder_step_calls.py)."""
import pytest
import torch
import torch.nn.functional as F

import encoder_op_cases as EC
from encoder_step_calls import BN_LIMIT, LIMIT, build, check, check_bn, nchw, record, record_bn, unrounded

pytestmark = pytest.mark.gpu

AVG_LIMIT = 1e-6             # tests/test_gpu_encoder_ops.py
LINEAR_LIMIT = 1e-5          # tests/test_gpu_train_ops.py::test_linear_backward_vs_autograd


@pytest.mark.parametrize("B,H,W,drop", [(4, 64, 64, False), (3, 64, 96, True)])
def test_every_operator_call_of_a_step_at_precision_32(synth, B, H, W, drop):
    """52 forward convolutions, 52 input gradients, 52 weight gradients at 5e-6 of the maximum; 53 BatchNorm forward and 53 backward calls
    at 2e-5 for y, mean, rstd, the updated running statistics, dz, dres, dgamma, dbeta, each on the call's own ReLU mask; stem and its weight
    gradient at 5e-6; average pool at 1e-6; max pool exact.

    Max pool backward: its input a0 is a ReLU output -- where a whole window is at zero the maximum is tied (1 to 2 % of the windows with
    the synthetic weights; the operator test has the inputs made of ties) --, its dy the result of the last shortcut add. An input element
    collects up to four windows, and a sum of four fp32 numbers rounds, so the yardstick is torch's float64 backward with those (at most
    four) terms added in fp32 in the row-major order of the windows (EC.maxpool_backward_fp32_order: per parity class of the windows the
    float64 backward holds single fp32 values, nothing rounds there); the result is equal to it bit for bit.

    Average pool backward: its input is the fc layer's input gradient, which only the library computes; checked are that all pixels of a
    (sample, channel) carry the same bits, and the value against float64 fc-backward / HW at the sum of the two operators' limits."""
    enc = build(synth, B, H, W, precision=32)
    assert enc.precision == 32 and all(t.dtype == torch.float32 for t in list(enc.wf.values()) + list(enc.wd.values()))
    torch.manual_seed(B + H)
    x = torch.rand(B, 1, H, W).cuda()
    dcond = torch.randn(B, 128).cuda()
    scales = None
    if drop:
        scales = {"layer2.1": torch.tensor([1 / 0.9, 0.0, 1 / 0.9][:B]), "layer4.2": torch.tensor([0.0, 1 / 0.95, 1 / 0.95][:B])}
    calls = record(enc)
    fwd, bwd, last = record_bn(enc)
    out = enc.forward(x, drop_scales=scales)
    sv = dict(enc.saved)                                    # backward() drops it
    grads = enc.backward(dcond)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())

    seen = check(enc, calls, rounding=unrounded, limit=LIMIT)
    assert {k: n for k, (n, _e) in seen.items()} == {"y": 52, "dx": 52, "dw": 52}
    assert [r["name"] for r in fwd][:2] == ["bn1", "layer1.0.bn1"] and bwd[0]["name"] == "layer4.2.bn3" and bwd[-1]["name"] == "bn1"
    seen_bn = check_bn(enc, fwd, bwd, limit=BN_LIMIT)
    assert len(fwd) == 53 and len(bwd) == 53
    assert {k: n for k, (n, _e) in seen_bn.items()} == {"bn y": 53, "bn mean": 53, "bn rstd": 53, "bn run_mean": 53, "bn run_var": 53, "bn dz": 53,
                                                        "bn dres": 16, "bn dgamma": 53, "bn dbeta": 53}
    if drop:
        assert sum(r["ss"] is not None for r in fwd) == 2 and sum(r["ss"] is not None for r in bwd) == 2
    seen.update(seen_bn)

    host = lambda t: t.double().cpu()
    img = lambda t: nchw(t.double().cpu())
    rest = {}
    # stem: x -> z0, and its weight gradient from dz0, the output of bn1's backward
    w1 = host(enc.p["conv1.weight"])
    rest["stem y"] = EC.rel(img(sv["z0"]), F.conv2d(host(x), w1, None, stride=2, padding=3))
    rest["stem dw"] = EC.rel(host(grads["conv1.weight"]), torch.nn.grad.conv2d_weight(host(x), w1.shape, img(bwd[-1]["dz"]), stride=2, padding=3))
    assert rest["stem y"] < LIMIT and rest["stem dw"] < LIMIT, rest
    # max pool: a0 -> the first block's input; backward: the last add's result -> the dy of bn1's backward
    a0, dpool = img(sv["a0"]), img(last["add"])
    assert last["add"].shape == sv["layer1.0"]["inp"].shape and bwd[-1]["dy"].shape == sv["a0"].shape
    share = EC.tie_share(a0)
    pooled = img(sv["layer1.0"]["inp"])
    assert pooled.shape == (B, 64, (a0.shape[2] + 1) // 2, (a0.shape[3] + 1) // 2) and not bool((pooled != F.max_pool2d(a0, 3, 2, 1)).any())
    want = EC.maxpool_backward_fp32_order(a0, dpool)
    got = img(bwd[-1]["dy"])
    bad = got != want
    assert got.shape == want.shape and not bool(bad.any()), (int(bad.sum()), "of", bad.numel(), "elements of the max pool's input gradient differ")
    f64 = EC.maxpool_torch(a0, dpool)[1]
    rest["maxpool dx vs float64"] = EC.rel(got, f64)
    assert bool(((got - f64).abs() <= 3 * 2.0 ** -24 * EC.maxpool_torch(a0, dpool.abs())[1]).all())
    rest["maxpool y"] = rest["maxpool dx"] = 0.0
    # average pool: the last block's output -> gap; backward: fc's input gradient -> the dy of the last block's bn3
    Bc, Hc, Wc, Cc = sv["last"].shape
    rest["avgpool g"] = EC.rel(host(sv["gap"]), host(sv["last"]).mean(dim=(1, 2)))
    d = host(bwd[0]["dy"]).reshape(Bc, Hc * Wc, Cc)
    assert all(torch.equal(d[:, 0], d[:, i]) for i in range(1, Hc * Wc))
    dgap = host(dcond) @ host(enc.p["fc.weight"])
    rest["avgpool dx (with fc backward)"] = EC.rel(d[:, 0], dgap / (Hc * Wc))
    assert rest["avgpool g"] < AVG_LIMIT and rest["avgpool dx (with fc backward)"] < AVG_LIMIT + LINEAR_LIMIT, rest
    print((B, H, W), "worst error per operator and role:", {k: (n, f"{e:.1e}") for k, (n, e) in seen.items()}, {k: f"{e:.1e}" for k, e in rest.items()},
          f"windows of a0 with a tied maximum: {share:.2f}")
