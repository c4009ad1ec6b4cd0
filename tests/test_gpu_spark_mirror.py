"""GPU: the Spark_2D mirror end to end on a synthetic batch: training_step (forward, backward, AdamW) and validation_step with their logs,
the reference's mask under torch.manual_seed, evaluation mode on untouched running statistics, the state_dict round trip and the
checkpoint hooks that carry AdamW's state."""
import numpy as np
import pytest
import torch

import spark_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CFG = dict(backbone="resnet50", imageDim=[192, 192, 100], rescaleFactor=2, mask_ratio=0.65, pix_norm=False, lr=1e-3, loss_on_mask=True)


@pytest.fixture(scope="module")
def syn(synth):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_spark_state_dict(0).items()}


def make(syn, **over):
    m = load_pkg("Spark_2D").Spark_2D(dict(CFG, **over), prefix="")
    m.load_state_dict(syn)
    return m


def batch_of(x):
    return {"vol": {"data": x.unsqueeze(-1)}}           # [B,1,H,W,1], torchio's layout of a slice batch


def test_training_and_validation_steps(syn):
    m = make(syn)
    try:
        torch.manual_seed(21)
        x = torch.rand(4, 1, 96, 96).cuda()
        torch.manual_seed(5)
        want_mask = R.draw_mask(4, 3, 0.65)
        torch.manual_seed(5)
        m.train()
        losses = []
        for step in range(3):
            out = m.training_step(batch_of(x), step)
            losses.append(float(out["loss"]))
            if step == 0:
                assert torch.equal(m.last_active, want_mask)                       # the reference's cells under the seed
        assert np.isfinite(losses).all() and float(m.logged["train/Loss_comb"]) == losses[-1]
        sd = m.state_dict()
        assert all(int(v) == 3 for k, v in sd.items() if k.endswith("num_batches_tracked"))
        moved = [k for k, v in sd.items() if v.is_floating_point() and "running" not in k and k not in ("model.imn_m", "model.imn_s", "model.norm_black")
                 and not torch.equal(v.cpu(), syn[k])]
        assert len(moved) == 221                                                   # AdamW moved (at least decayed) every parameter
        assert not torch.equal(sd["model.en_de_norms.0.running_mean"].cpu(), syn["model.en_de_norms.0.running_mean"])
        tr = m._hip_spark_trainer
        assert tr.step_count == 3 and tr.skipped_steps == 0
        # the same mask at every step: the loss of the masked cells falls
        m2 = make(syn)
        fixed = []
        for step in range(3):
            torch.manual_seed(9)
            fixed.append(float(m2.training_step(batch_of(x), step)["loss"]))
        print("losses with a fresh mask per step", losses, "with one mask", fixed)
        assert fixed[2] < fixed[0]
        m2._hip_spark_trainer.close()
        # validation: evaluation mode, running statistics used and left alone
        m.eval()
        before = {k: v.clone() for k, v in m.state_dict().items()}
        out = m.validation_step(batch_of(x), 0)
        assert np.isfinite(float(out["loss"])) and float(m.logged["val/Loss_comb"]) == float(out["loss"])
        assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
        with pytest.raises(NotImplementedError, match="test_after_training"):
            m.test_step(batch_of(x), 0)
        with pytest.raises(ValueError, match="96"):
            m(torch.rand(2, 1, 64, 64).cuda())
        # checkpoint: weights and AdamW's state travel; a restored mirror continues bit for bit
        ckpt = {"state_dict": {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}}
        m.on_save_checkpoint(ckpt)
        assert set(ckpt["hip_optimizer_state"]) == {"spark"} and ckpt["hip_optimizer_state"]["spark"]["step"] == 3
        m3 = make(syn)
        m3.load_state_dict(ckpt["state_dict"])
        m3.on_load_checkpoint(ckpt)
        m.train(), m3.train()
        torch.manual_seed(13)
        a = m.training_step(batch_of(x), 3)["loss"]
        torch.manual_seed(13)
        b = m3.training_step(batch_of(x), 3)["loss"]
        # stochastic depth draws on the device generator: both runs start it from the same seed above
        assert m3._hip_spark_trainer.step_count == 4
        assert torch.equal(a, b)
        for (ka, va), (kb, vb) in zip(m.state_dict().items(), m3.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        m3._hip_spark_trainer.close()
    finally:
        if m._hip_spark_trainer is not None:
            m._hip_spark_trainer.close()


def test_loss_strategy_and_delta_mask_reach_the_loss(syn):
    """loss_on_mask False: L1_AE's recon_error + delta_mask * the masked term (src/models/Spark_2D.py:28-31), evaluation mode, one mask"""
    x = torch.rand(2, 1, 96, 96, generator=torch.Generator().manual_seed(2)).cuda()
    got = {}
    for key, over in dict(on_mask={}, mean=dict(loss_on_mask=False, delta_mask=0.5, lossStrategy="mean"),
                          sum=dict(loss_on_mask=False, delta_mask=0.5, lossStrategy="sum")).items():
        m = make(syn, **over).eval()
        torch.manual_seed(3)
        loss, reco, latent = m(x)
        got[key] = (float(loss), m._hip_spark_trainer.terms.cpu().double())
        assert reco.shape == (2, 1, 96, 96) and latent.shape == (2, 2048)
        m._hip_spark_trainer.close()
    masked, l1 = got["on_mask"][1]
    assert got["on_mask"][0] == pytest.approx(float(masked), rel=1e-6)
    assert got["mean"][0] == pytest.approx(float(l1 + 0.5 * masked), rel=1e-6)
    assert got["sum"][0] == pytest.approx(float(l1 * 96 * 96 + 0.5 * masked), rel=1e-6)
