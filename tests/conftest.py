"""Shared fixtures. Tests marked `gpu` need an MI355X and call the HIP path through the C ABI;
everything else runs on CPU (oracle vs golden vectors, host logic, library symbol check)."""
import importlib
import os
import sys

# The golden vectors were written with MKL on its COMPATIBLE code path (MANIFEST.json "mkl_cbwr"). Left to itself MKL picks a
# branch per CPU vendor and ISA, and its exp / sin / cos differ between them by an ulp, which the timestep embedding turns into
# 3e-5; pinned, Intel and AMD hosts compute the same bits. Set before torch (and with it MKL) is loaded.
os.environ["MKL_CBWR"] = "COMPATIBLE"

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

PKG_NAME = "conditioned-diffusion-models-uad_amd"
GOLD = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # The CPU oracle is compared with reference outputs at 2e-6: torch's CPU convolutions sum in an order that depends on the
    # thread count, so the oracle runs with the thread count the fixtures were generated with (MANIFEST.json "threads": 8),
    # whatever the host offers (measured: 3 threads move a 50-step chain by 8e-6).
    try:
        import torch
        torch.set_num_threads(8)
    except Exception:
        pass


def load_pkg(sub: str = ""):
    return importlib.import_module(PKG_NAME + (("." + sub) if sub else ""))


@pytest.fixture(scope="session")
def synth():
    return load_pkg("synth")


@pytest.fixture(scope="session")
def oracle():
    import cddpm_oracle
    return cddpm_oracle


@pytest.fixture(scope="session")
def sd_np(synth):
    """synthetic UNet weights, seed 0 (the seed every golden fixture was made with)"""
    return synth.synth_state_dict(0)


@pytest.fixture(scope="session")
def sd_torch(sd_np, oracle):
    return oracle.to_torch_sd(sd_np)


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


@pytest.fixture(scope="session")
def engine_factory(sd_np):
    """builds CddpmEngine objects with the synthetic weights loaded (GPU tests only)"""
    import torch
    eng_mod = load_pkg("engine")
    sched = load_pkg("schedule")
    made = []

    def make(timesteps=1000, max_batch=4, max_h=128, max_w=128, objective="pred_x0", beta_schedule="cosine"):
        e = eng_mod.CddpmEngine(timesteps=timesteps, max_batch=max_batch, max_h=max_h, max_w=max_w)
        e.load_weights(sd_np)
        e.set_schedule(sched.schedule_buffers(timesteps, beta_schedule), objective)
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()
