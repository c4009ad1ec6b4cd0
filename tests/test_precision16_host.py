"""Host side of precision-16 reconstruction (no GPU): the three new entry points in header, binding and library; the parsing of the
engine's `precision` and the mirrors' `cfg.eval_precision`; and the sanity of the AMP fixtures (tests/golden/amp/): finite, and as far
from the float64 oracle as fp16 operand rounding (2^-11, not 2^-24) puts them."""
import json
import os
import re

import pytest
import torch

import arch_cases as A
import precision16_cases as P
from conftest import GOLD, ROOT, load_pkg


def _args_of(header, name):
    m = re.search(rf"\bint {name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/cddpm.h"
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_new_entry_points_are_declared_bound_and_exported():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    for name in ("cddpm_set_precision", "cddpm_get_precision", "cddpm_op_attention_p16"):
        args = _args_of(header, name)
        assert name in lib_mod.SYMBOLS, name
        assert len(lib_mod.SYMBOLS[name][1]) == len(args), (name, args)
    # the stand-alone operator has cddpm_op_attention's argument list, whose own declaration is unchanged
    assert lib_mod.SYMBOLS["cddpm_op_attention_p16"] == lib_mod.SYMBOLS["cddpm_op_attention"]
    assert len(_args_of(header, "cddpm_op_attention")) == 7
    lib = lib_mod.load_library()                           # binds every name of SYMBOLS: raises if one is not exported
    assert lib.cddpm_get_precision(None) == -1 and lib.cddpm_set_precision(None, 16) == -1      # NULL handle: refused, no crash
    assert lib.cddpm_op_attention_p16(None, None, None, 1, 1, 64, None) == -1
    for ref in ("OpenAI_Unet.py:284-338", ":457-476"):       # the reference lines the switch stands for
        assert ref in header, ref
    assert "the handle is at precision 16" in header         # the message of cddpm_set_conv_family on such a handle


def test_engine_precision_spellings():
    eng = load_pkg("engine")
    for value, bits in ((16, 16), (32, 32), ("16", 16), ("16-mixed", 16), ("32", 32)):
        assert eng.precision_bits(value) == bits, value
    for bad in (8, "bf16", "64", None, 64, "fp16", 16.0, True, "bf16-mixed"):
        with pytest.raises(ValueError, match="precision"):
            eng.precision_bits(bad)
    assert eng.CONV_FAMILIES == {"h3": 2, "x6": 1, "f32": 0}          # precision is no fourth family


def test_engine_rejects_a_bad_precision_before_it_touches_a_device(monkeypatch):
    eng = load_pkg("engine")
    monkeypatch.setattr(eng._lib, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
    for bad in (8, "bf16", "64"):
        with pytest.raises(ValueError, match="precision"):
            eng.CddpmEngine(precision=bad)
    with pytest.raises(ValueError, match="h3"):
        eng.CddpmEngine(precision=16, conv_family="x6")
    e = object.__new__(eng.CddpmEngine)                    # set_precision parses before it calls the library
    e._h = None
    for bad in (None, 8, "bf16"):
        with pytest.raises(ValueError, match="precision"):
            e.set_precision(bad)
    with pytest.raises(ValueError, match="precision"):
        e.op_attention(torch.zeros(1, 1, 192), precision="bf16")


def _unet():
    unet_mod = load_pkg("OpenAI_Unet")
    return unet_mod.UNetModel(image_size=32, in_channels=1, model_channels=128, out_channels=1, num_res_blocks=1,
                              attention_resolutions=(3,), channel_mult=(1,), num_classes=128, num_head_channels=64,
                              use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)


def test_backend_eval_precision_is_validated_and_defaults_to_32():
    hip = _unet()._hip
    assert hip.eval_precision == 32
    hip.configure(None, None)
    assert hip.eval_precision == 32                        # absent: today's behaviour
    hip.configure(None, "x6", "16-mixed")                  # an exact FALLBACK family goes with precision 16
    assert (hip.eval_precision, hip.conv_fallback) == (16, "x6")
    hip.configure("h3", None, 16)
    assert hip.eval_precision == 16
    for fam in ("x6", "f32"):
        with pytest.raises(ValueError, match="h3"):
            hip.configure(fam, None, 16)
    with pytest.raises(ValueError, match="precision"):
        hip.configure(None, None, "bf16")
    hip.configure(None, None, 32)
    assert hip.eval_precision == 32


@pytest.mark.parametrize("mirror", ["DDPM_2D", "DDPM_2D_patched"])
def test_mirror_eval_precision_key(mirror):
    M = load_pkg(mirror)
    base = dict(imageDim=[96, 96, 4], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2], num_res_blocks=1, condition=False, patch_size=16)
    assert M.DDPM_2D(dict(base)).diffusion.model._hip.eval_precision == 32                       # absent: 32
    mod = M.DDPM_2D(dict(base, eval_precision=16))
    assert mod.diffusion.model._hip.eval_precision == 16
    assert set(mod.state_dict()) == set(M.DDPM_2D(dict(base)).state_dict())                      # a setting, never a checkpoint entry
    assert M.DDPM_2D(dict(base, eval_precision="16-mixed", conv_family="h3", conv_fallback="x6")).diffusion.model._hip.eval_precision == 16
    assert M.DDPM_2D(dict(base, eval_precision=32, conv_family="x6")).diffusion.model._hip.eval_precision == 32
    for fam in ("x6", "f32"):
        with pytest.raises(ValueError, match="h3"):
            M.DDPM_2D(dict(base, eval_precision=16, conv_family=fam))
    with pytest.raises(ValueError, match="precision"):
        M.DDPM_2D(dict(base, eval_precision="bf16"))
    # the Trainer's / cfg's TRAINING precision is not the evaluation's
    assert M.DDPM_2D(dict(base, precision=16)).diffusion.model._hip.eval_precision == 32


@pytest.mark.parametrize("experiment", ["cDDPM/DDPM_cond_spark_2D", "cDDPM/DDPM_patched"])
def test_eval_precision_is_an_ordinary_override_of_the_composed_config(experiment):
    compose = load_pkg("config").compose
    cfg_dir = os.path.join(GOLD, "configs")
    assert "eval_precision" not in compose(cfg_dir, experiment)["model"]["cfg"]                    # absent in the reference's configs: 32
    for text, value in (("16", 16), ("16-mixed", "16-mixed"), ("32", 32)):
        got = compose(cfg_dir, experiment, overrides=[f"+model.cfg.eval_precision={text}"])["model"]["cfg"]["eval_precision"]
        assert got == value and load_pkg("engine").precision_bits(got) in (16, 32)


def test_amp_manifest_lists_every_fixture_and_nothing_was_dropped():
    man = json.load(open(os.path.join(P.AMP, "MANIFEST.json")))
    assert man["dropped"] == []
    assert set(man["cases"]) == set(P.FIXTURES.values()) | {P.CHAIN["name"], P.PATCHED["name"]}
    assert sorted(f for f in os.listdir(P.AMP) if f.endswith(".npz")) == sorted(n + ".npz" for n in man["cases"])
    assert man["seeds"] == dict(weights=A.SEED_W, cond=A.SEED_COND, xT=A.SEED_X, z=P.SEED_Z)


def _sanity(label, ref):
    amp, r32, r64 = ref["amp"], ref["r32"], ref["r64"]
    assert amp.dtype == torch.float32 and amp.shape == r64.shape, label
    assert bool(torch.isfinite(amp).all()), label + ": the AMP fixture is not finite"
    d_amp, d_32 = P.rms(amp.double() - r64), P.rms(r32.double() - r64)
    print(f"{label}: AMP fixture rms distance from float64 {d_amp:.3e}, fp32 oracle {d_32:.3e}, ratio {d_amp / d_32:.0f}")
    assert d_amp >= 10 * d_32, (label, d_amp, d_32)        # operand rounding 2^-11, not 2^-24: else it was not made under autocast


@pytest.mark.parametrize("name", list(P.FIXTURES))
def test_amp_forward_fixtures_are_finite_and_fp16_far_from_float64(name):
    refs = P.forward_refs(name)
    assert set(P.amp_fixture(P.FIXTURES[name]).files) == set(A.GOLDEN_T)
    for key in A.GOLDEN_T:
        _sanity(f"{name} {key}", refs[key])


def test_amp_chain_fixture_is_finite_and_fp16_far_from_float64():
    ref = P.chain_refs()
    assert float(ref["amp"].min()) >= 0 and float(ref["amp"].max()) <= 1
    _sanity("8-step chain", ref)


def test_amp_patched_fixture_is_finite_and_fp16_far_from_float64():
    ref = P.patched_refs()
    assert P.rms(ref["r32"].double() - ref["r64"]) < 1e-5      # the float64 restatement IS the recorded fp32 test_step, rounding aside
    _sanity("patched test_step", ref)
