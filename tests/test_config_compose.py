"""CPU: the Hydra-less composer on the cDDPM experiment's config tree. tests/golden/configs holds that tree's layout (root
defaults list, group files, the `# @package _global_` experiment overlay) with the values of the experiment's model-shaping keys."""
import os

import torch

from conftest import GOLD, load_pkg

CFG_DIR = os.path.join(GOLD, "configs")


def test_compose_cddpm_experiment():
    config = load_pkg("config")
    cfg = config.compose(CFG_DIR, "cDDPM/DDPM_cond_spark_2D", overrides=["model.cfg.pretrained_encoder=False"])
    m = cfg["model"]["cfg"]
    assert cfg["model"]["_target_"] == "src.models.DDPM_2D.DDPM_2D"
    assert m["unet_dim"] == 128 and m["dim_mults"] == [1, 2, 2] and m["test_timesteps"] == 500
    assert m["imageDim"] == [192, 192, 100] and m["rescaleFactor"] == 2          # ${datamodule.cfg.*} resolved
    assert m["pretrained_encoder"] is False and m["noisetype"] == "simplex"
    assert cfg["trainer"]["max_epochs"] == 1200                                  # experiment overlay over the group file
    assert cfg["data_dir"] == "${oc.env:DATA_DIR}"                               # resolver syntax is left as written
    enc = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.LazyLinear(128))
    mod = config.instantiate_model(cfg, encoder=enc)
    assert mod.diffusion.model.image_size == (96, 96) and mod.diffusion.num_timesteps == 1000
    assert mod.diffusion.model.channel_mult == (1, 2, 2) and mod.test_timesteps == 500
