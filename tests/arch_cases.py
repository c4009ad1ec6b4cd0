"""UNet descriptors beyond the experiment's 128-channel (1, 2, 2) model, shared by oracle/make_golden_arch.py (which records the
reference's outputs at them), the CPU tests that pin the oracle and the synthetic weights to those records, and the GPU tests that
run the engine and the trainer at them (tests/test_gpu_unet_descriptors.py, tests/test_gpu_training_descriptors.py).

A case is the constructor arguments of one UNet, ONE test geometry (B, H, W) and the code path it exists for. H and W are multiples
of 4 and of 2^(levels - 1), non-square and not a multiple of the convolution's 32 x 8 pixel tile. Every case is small enough that the
float64 oracle forward and one float64 autograd pass each take under ten seconds on 16 CPU threads (the slowest is w384_limit).

`attention_resolutions` DEFAULT_ATT is the experiment's (3, 6, 12): no power of two, so attention in the middle block only."""
import numpy as np
import torch

DEFAULT_ATT = (3, 6, 12)
SEED_W, SEED_COND, SEED_X = 0, 1, 2         # the seeds of every other fixture under tests/golden
GOLDEN_T = ("t500", "tmixed")               # the two timestep vectors recorded per case: uniform 500, and mixed per sample


def _case(model_channels, channel_mult, num_res_blocks, cond_dim, geometry, attention_resolutions=DEFAULT_ATT):
    return dict(model_channels=model_channels, channel_mult=tuple(channel_mult), num_res_blocks=num_res_blocks,
                attention_resolutions=tuple(attention_resolutions), cond_dim=cond_dim, geometry=geometry)


CASES = {
    # head_dots_kernel's dynamic LDS at C = 256 (75 KB: above the 64 KB a kernel gets without asking); Cout 512; concatenations of 1024
    "w256": _case(256, (1, 2), 1, 128, (2, 16, 24)),
    # conv_in1_kernel at C = 384 (256 threads are not a multiple of the 96 channel quads); Cout 768; the deepest output block concatenates
    # 768 + 768 = 1536 channels: exactly MAX_CONCAT_CHANNELS
    "w384_limit": _case(384, (1, 2), 1, 128, (2, 16, 24)),
    # head LDS at C = 512 (150 KB); embedding width E = 2048; no label_emb (the unconditioned model)
    "w512_uncond": _case(512, (1, 1), 1, 0, (2, 16, 24)),
    # four levels: ds = 8, 3 x 5 = 15 tokens in the middle attention (not a multiple of 16), two ResBlocks per level
    "deep4": _case(128, (1, 1, 2, 2), 2, 128, (2, 24, 40)),
    # attention inside input and output blocks at C = 128 (2 heads, N = H W tokens at ds = 1) and C = 256; an attention followed by an
    # up-ResBlock in one output block (sub-index 2); attention outputs pushed on the skip stack
    "attn_levels": _case(128, (1, 2, 2), 1, 128, (2, 16, 24), attention_resolutions=(1, 2, 4)),
    # channel_mult[0] != 1: the head (out.0 / out.2) reads 256 channels, not model_channels
    "mult0_2": _case(128, (2, 2), 1, 128, (2, 16, 24)),
    # the smallest context vector the library accepts; also the B = 3 case (6 x 10 = 60 tokens in the middle attention)
    "cond4": _case(128, (1, 2), 1, 4, (3, 12, 20)),
}

# descriptors cddpm_create must refuse, each with the words its message must contain (validate_desc / check_program of cddpm_api.hip).
# `desc` overrides a valid base descriptor: 128 x (1, 2), one ResBlock per level, cond_dim 128, max geometry 2 x 16 x 24.
REFUSALS = {
    # 256 x (1, 4), three ResBlocks: the deepest output blocks concatenate 1024 + 1024 channels
    "concat_2048": dict(desc=dict(model_channels=256, channel_mult=(1, 4), num_res_blocks=3), message="at most 1536"),
    "model_channels_640": dict(desc=dict(model_channels=640), message="model_channels must be 128, 256, 384 or 512"),
    # 512 x 4 = 2048 channels at level 1
    "mult_x_c_2048": dict(desc=dict(model_channels=512, channel_mult=(1, 4)), message="channel_mult[1] * model_channels = 2048 exceeds 1024"),
    "cond_dim_6": dict(desc=dict(cond_dim=6), message="cond_dim must be a non-negative multiple of 4"),
    # four levels need H, W that are multiples of 8
    "max_h_20_of_4_levels": dict(desc=dict(channel_mult=(1, 1, 2, 2), max_h=20, max_w=40), message="multiples of 8"),
}
REFUSAL_BASE = dict(model_channels=128, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=DEFAULT_ATT, cond_dim=128,
                    max_batch=2, max_h=16, max_w=24)


# ---- the one case dict as the arguments of each layer ---------------------------------------------------------------------------------
def unet_kw(case):
    """oracle.unet_forward(..., **unet_kw(case))"""
    return {k: case[k] for k in ("model_channels", "channel_mult", "num_res_blocks", "attention_resolutions")}


def synth_kw(case):
    """synth.unet_param_shapes(**synth_kw(case)) / synth.synth_state_dict(seed, **synth_kw(case))"""
    return dict(unet_kw(case), num_classes=case["cond_dim"] or None)


def engine_kw(case):
    """engine.CddpmEngine(timesteps=, max_batch=, max_h=, max_w=, **engine_kw(case))"""
    return dict(unet_kw(case), cond_dim=case["cond_dim"])


def trainer_kw(case):
    """training.UNetTrainer(params, **trainer_kw(case)): the trainer has attention in the middle block only"""
    return dict(model_channels=case["model_channels"], channel_mult=case["channel_mult"], num_res_blocks=case["num_res_blocks"],
                cond_dim=case["cond_dim"] or None)


def inputs(synth, case, slice0=0):
    """(x [B,1,H,W], cond [B,cond_dim] or None) of a case, regenerated from the seeds"""
    B, H, W = case["geometry"]
    x = torch.from_numpy(synth.noise_xT(SEED_X, slice0, B, H, W))
    cond = torch.from_numpy(synth.synth_cond(SEED_COND, slice0, B, case["cond_dim"])) if case["cond_dim"] else None
    return x, cond


def timesteps(key, B):
    """the recorded timestep vectors: 't500' -> 500 for every sample, 'tmixed' -> one t per sample, spread over [0, 1000)"""
    if key == "tmixed":
        return torch.tensor([(123 + 754 * i) % 1000 for i in range(B)], dtype=torch.long)
    return torch.full((B,), int(key[1:]), dtype=torch.long)


def shapes_record(shapes):
    """an ordered {name: shape} as the two arrays a golden file holds (names, and shapes padded with zeros to rank 4)"""
    names = np.array(list(shapes), dtype="U")
    dims = np.zeros((len(shapes), 4), dtype=np.int32)
    for i, s in enumerate(shapes.values()):
        dims[i, :len(s)] = s
    return names, dims


# ---- the acceptance rule of the GPU parity tests ------------------------------------------------------------------------------------------
REL_FLOOR = 2e-5          # tests/test_gpu_unet.py::test_unet_blocks_vs_oracle: max|delta| <= 2e-5 max|ref| per block
YARD_FACTOR = 4.0         # two fp32 evaluations with different summation orders differ from EACH OTHER by about twice their distance
                          # from float64; 4 leaves a factor 2 over that


def block_ratios(got, ref64, ref32, names):
    """Per block: the engine's distance from the float64 oracle, against the yardstick (the fp32 oracle's own distance from float64 on
    that block). -> [(name, err, yardstick, max|ref|, passes)]; a block passes when err <= max(REL_FLOOR max|ref|, YARD_FACTOR yardstick).
    One dropped 32-channel chunk of a 1536-channel input moves a block by ~1/48 of its magnitude: three orders above either bound."""
    rows = []
    for n in names:
        r64, r32, g = ref64[n], ref32[n], got[n].detach().cpu()
        assert g.shape == r64.shape, (n, tuple(g.shape), tuple(r64.shape))
        err = float((g.double() - r64).abs().max())
        yard = float((r32.double() - r64).abs().max())
        mag = float(r64.abs().max())
        rows.append((n, err, yard, mag, bool(np.isfinite(err)) and err <= max(REL_FLOOR * mag, YARD_FACTOR * yard)))
    return rows


def format_ratios(rows):
    return "\n".join(f"{n:18s} max|d|={e:.3e} yardstick={y:.3e} ratio={e / max(y, 1e-30):6.2f} rel={e / (1e-30 + m):.2e} {'ok' if ok else 'FAIL'}"
                     for n, e, y, m, ok in rows)
