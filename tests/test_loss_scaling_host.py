"""Host logic of the dynamic loss scaling (CPU): the checked settings of UNetTrainer.enable_loss_scaling, the seed taken from a
Lightning 1.5 native-AMP checkpoint (`native_amp_scaling_state` = a torch GradScaler.state_dict()), the DDPM_2D mirror's bookkeeping --
when it turns the scaler on, the every-50-steps read of the consecutive skips and its one warning, optimizer states with and without the
scaler key. The device side is tests/test_gpu_loss_scaling.py."""
import warnings

import pytest
import torch

from conftest import load_pkg

CFG = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500,
           noise_ensemble=True, spatial_transformer=False, backbone="Spark_Encoder_2D", version="resnet50", cond_dim=128)


def _mirror():
    return load_pkg("DDPM_2D").DDPM_2D(CFG, encoder=torch.nn.Identity())


class _Trainer:
    """a stand-in for training.UNetTrainer: records what the mirror asks of it"""

    def __init__(self, skips=0):
        self.loss_scaling, self.enabled, self.skips, self.reads, self.loaded = False, [], skips, 0, None
        self.loss_scale = 1.0

    def enable_loss_scaling(self, **kw):
        self.enabled.append(kw)
        self.loss_scaling = True

    @property
    def consecutive_skips(self):
        self.reads += 1
        return self.skips

    def optimizer_state(self):
        return {"m": torch.ones(3), "v": torch.zeros(3), "ctrl": torch.tensor([0, 7, 0, 1, 0, 0, 0, 0], dtype=torch.int32),
                "layout": [("a", 3)]}

    def load_optimizer_state(self, st):
        self.loaded = st


def test_settings_default_to_torch_grad_scaler():
    tr = load_pkg("training")
    gs = torch.amp.GradScaler("cpu")
    assert tr.loss_scaling_settings() == {"init_scale": None, "growth_factor": gs.get_growth_factor(),
                                          "backoff_factor": gs.get_backoff_factor(), "growth_interval": gs.get_growth_interval(),
                                          "growth_tracker": 0}
    assert tr.loss_scaling_settings(2.0 ** -3, 4.0, 0.25, 1, 0)["init_scale"] == 0.125


@pytest.mark.parametrize("kw", [dict(init_scale=3.0), dict(init_scale=0.0), dict(init_scale=-4.0), dict(init_scale=float("inf")),
                                dict(init_scale=float("nan")), dict(init_scale=2.0 ** 127 * 1.5), dict(growth_factor=3.0),
                                dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=0.3), dict(backoff_factor=1.0),
                                dict(backoff_factor=2.0), dict(growth_interval=0), dict(growth_interval=2.5), dict(growth_interval=True),
                                dict(growth_tracker=-1), dict(init_scale="big")])
def test_settings_reject_what_is_not_an_exact_power_of_two_scaler(kw):
    tr = load_pkg("training")
    with pytest.raises(ValueError):
        tr.loss_scaling_settings(**kw)


def test_seed_from_a_grad_scaler_state_dict():
    tr = load_pkg("training")
    gs = torch.amp.GradScaler("cpu", init_scale=2.0 ** 10, growth_interval=500)
    sd = gs.state_dict()
    sd["_growth_tracker"] = 17
    assert tr.loss_scaling_from_grad_scaler(sd) == {"init_scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                                                    "growth_interval": 500, "growth_tracker": 17}
    with pytest.raises(ValueError):
        tr.loss_scaling_from_grad_scaler(dict(sd, scale=1000.0))


@pytest.mark.parametrize("start", [None, 65536.0])
def test_scaler_state_round_trips_with_and_without_the_device_block(start):
    """optimizer.FlatOptimizer on the CPU, for both kinds of trainer (no default start: the block waits for the first loss; a default
    start: made at once): scaler_state() -> load_scaler_state() restores settings and block; no "scaler" entry leaves the scaler alone"""
    opt = load_pkg("optimizer")
    cls = type("T", (opt.FlatOptimizer,), {"DEFAULT_INIT_SCALE": start})
    make = lambda: cls({"w": torch.arange(3.0)}, ["w"], "cpu")
    src = make()
    assert not src.loss_scaling and src.scaler is None and src.loss_scale is None and src.growth_tracker == src.consecutive_skips == 0
    src.enable_loss_scaling(growth_interval=7, growth_tracker=3)
    assert (src.scaler is None) == (start is None) and src.loss_scale == start and src.growth_tracker == 3
    for with_block in (start is not None, True):
        if with_block:
            src._start_scaler(256.0)                # the first loss of a trainer without a default start
            src.scaler[2] = 2
        st = {"scaler": src.scaler_state()}
        assert set(st["scaler"]) == {"init_scale", "growth_factor", "backoff_factor", "growth_interval", "growth_tracker", "state"}
        assert (st["scaler"]["state"] is not None) == with_block and st["scaler"]["init_scale"] == start
        dst = make()
        dst.load_scaler_state(st.get("scaler"))
        assert dst.loss_scaling and dst.scaler_cfg == (2.0, 0.5, 7) and dst.growth_tracker == 3
        assert dst.loss_scale == src.loss_scale and dst.consecutive_skips == src.consecutive_skips == (2 if with_block else 0)
        if with_block:
            assert torch.equal(dst.scaler, src.scaler) and dst.scaler is not st["scaler"]["state"] and dst.scaler.dtype == torch.int32
            assert dst.loss_scale == (start or 256.0)
        block = dst.scaler
        dst.load_scaler_state({}.get("scaler"))     # a state saved without dynamic loss scaling
        assert dst.loss_scaling and dst.scaler is block and dst.scaler_cfg == (2.0, 0.5, 7)
    off = make()
    off.load_scaler_state({}.get("scaler"))
    assert not off.loss_scaling and off.scaler is None
    src.disable_loss_scaling()
    assert not src.loss_scaling and src.scaler is None and src.loss_scale is None


def test_mirror_keeps_a_native_amp_seed_pending_until_precision_16():
    mod = _mirror()
    sd = {"scale": 2.0 ** 12, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 5}
    mod.on_load_checkpoint({"native_amp_scaling_state": sd})
    seed = {"init_scale": 4096.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "growth_tracker": 5}
    assert mod._pending_amp_scaler == seed
    t32 = _Trainer()
    mod._loss_scaling(t32, 32)                      # precision 32: nothing changes, the seed waits
    assert t32.enabled == [] and mod._pending_amp_scaler == seed
    t16 = _Trainer()
    mod._loss_scaling(t16, 16)
    assert t16.enabled == [seed] and mod._pending_amp_scaler is None
    mod._loss_scaling(t16, 16)                      # already on: left alone
    assert t16.enabled == [seed]
    fresh = _Trainer()
    mod._loss_scaling(fresh, 16)                    # no seed: torch's defaults, the batch-size start
    assert fresh.enabled == [{}]


def test_hip_optimizer_state_wins_over_the_native_amp_seed():
    mod = _mirror()
    mod.on_load_checkpoint({"hip_optimizer_state": {"unet": {"m": torch.ones(1)}}, "native_amp_scaling_state": {"scale": 8.0}})
    assert getattr(mod, "_pending_amp_scaler", None) is None and "unet" in mod._pending_opt_state


def test_an_optimizer_state_without_the_scaler_key_loads_as_before():
    """a checkpoint written before the scaler existed: passed to the trainer as it is, no seed; a state with the key is saved host-side"""
    mod = _mirror()
    src = _Trainer()
    mod._hip_unet_trainer = src
    ck = {}
    mod.on_save_checkpoint(ck)
    assert "scaler" not in ck["hip_optimizer_state"]["unet"]
    fresh = _mirror()
    fresh.on_load_checkpoint(ck)
    assert getattr(fresh, "_pending_amp_scaler", None) is None
    fresh._hip_unet_trainer = _Trainer()
    fresh._load_pending_optimizer_state()
    assert set(fresh._hip_unet_trainer.loaded) == {"m", "v", "ctrl", "layout"}
    st = src.optimizer_state()
    st["scaler"] = {"init_scale": None, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "growth_tracker": 0,
                    "state": torch.tensor([0, 3, 0, 0], dtype=torch.int32)}
    src.optimizer_state = lambda: st
    mod.on_save_checkpoint(ck)
    saved = ck["hip_optimizer_state"]["unet"]["scaler"]
    assert saved["state"].device.type == "cpu" and torch.equal(saved["state"], st["scaler"]["state"])


def test_mirror_reads_the_skips_every_50_steps_and_warns_once():
    mod = _mirror()
    tr_ = _Trainer(skips=49)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(49):
            mod._watch_loss_scale(tr_)
        assert tr_.reads == 0 and seen == []
        mod._watch_loss_scale(tr_)                  # step 50: one read, 49 skips in a row >= 30
        assert tr_.reads == 1 and len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning)
        tr_.skips = 99
        for _ in range(50):
            mod._watch_loss_scale(tr_)
        assert tr_.reads == 2 and len(seen) == 1    # still stalled: not repeated
        tr_.skips = 0
        for _ in range(50):
            mod._watch_loss_scale(tr_)
        tr_.skips = 30
        for _ in range(50):
            mod._watch_loss_scale(tr_)
        assert tr_.reads == 4 and len(seen) == 2    # recovered in between: a new stall warns again
    below, other = _Trainer(skips=29), _mirror()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(100):
            other._watch_loss_scale(below)
        assert below.reads == 2 and seen == []
