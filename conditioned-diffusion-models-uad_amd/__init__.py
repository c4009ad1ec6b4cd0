"""MI355X-native cDDPM reverse-diffusion reconstruction path (hand-written HIP behind a C ABI).

Import this package with importlib (the directory name carries a hyphen):
    pkg = importlib.import_module("conditioned-diffusion-models-uad_amd")
Submodules: synth (counter RNG + synthetic weights), schedule, engine (ctypes owner of the HIP handle),
OpenAI_Unet / cond_DDPM / DDPM_2D / DDPM_2D_patched (host-side mirrors of the reference classes; the patched DDPM's class is
DDPM_2D_patched.DDPM_2D, its box sampler patch_sampling.BoxSampler -- both also reachable as pkg.DDPM_2D_patched / pkg.BoxSampler),
Spark_2D (the mirror of the SparK pre-training LightningModule) over spark_training, sharding, config, build.
Nothing here imports oracle/ and nothing computes on the CPU: without the HIP library the path raises.
"""
__all__ = ["synth", "schedule", "engine", "build", "DDPM_2D_patched", "BoxSampler"]


def __getattr__(name):
    # lazy: importing the package must not import torch-heavy mirrors (nor need the HIP library)
    if name == "BoxSampler":
        from .patch_sampling import BoxSampler
        return BoxSampler
    if name == "DDPM_2D_patched":
        import importlib
        return importlib.import_module(__name__ + ".DDPM_2D_patched")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
