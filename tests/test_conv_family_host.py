"""Host side of the per-handle convolution family and the per-slice fallback (no GPU): the run grouping of flagged slices,
the validation of family names in the engine layer and the mirrors, and the three new entry points in header and binding."""
import os
import re

import pytest

from conftest import ROOT, load_pkg


def test_flagged_runs_groups_maximal_contiguous_runs():
    runs = load_pkg("engine").flagged_runs
    assert runs([0, 0, 0, 0]) == []                       # all good
    assert runs([1, 1, 1, 1]) == [(0, 4)]                 # all bad: one run
    assert runs([0, 1, 1, 0, 1]) == [(1, 3), (4, 5)]
    assert runs([1, 0, 1, 0]) == [(0, 1), (2, 3)]
    assert runs([0]) == [] and runs([1]) == [(0, 1)]      # B = 1
    assert runs([]) == []
    assert runs([False, True]) == [(1, 2)]                # any truthy flag, e.g. the bools of a torch .tolist()


def test_family_names_and_numbering():
    eng = load_pkg("engine")
    assert eng.CONV_FAMILIES == {"h3": 2, "x6": 1, "f32": 0}          # the numbering of conv_mode() / include/cddpm.h
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    for name, code in (("H3", 2), ("X6", 1), ("F32", 0)):
        assert re.search(rf"#define CDDPM_CONV_{name} {code}\b", header), name
    for name, code in eng.CONV_FAMILIES.items():
        assert eng.conv_family_code(name) == code
    for bad in ("", "H3", "fp32", "x3", None, 2):
        with pytest.raises(ValueError, match="convolution family"):
            eng.conv_family_code(bad)
    assert set(eng.EXACT_FAMILIES) == {"x6", "f32"}


def test_engine_rejects_an_unknown_family_before_it_touches_a_device():
    eng = load_pkg("engine")
    with pytest.raises(ValueError, match="convolution family"):
        eng.CddpmEngine(conv_family="bf16")


def test_backend_settings_are_validated_and_default_to_off():
    unet_mod, backend = load_pkg("OpenAI_Unet"), load_pkg("backend")
    unet = unet_mod.UNetModel(image_size=32, in_channels=1, model_channels=128, out_channels=1, num_res_blocks=1,
                              attention_resolutions=(3,), channel_mult=(1,), num_classes=128, num_head_channels=64,
                              use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True)
    hip = unet._hip
    assert isinstance(hip, backend.HipBackend)
    assert hip.conv_family is None and hip.conv_fallback is None and hip.fallback(unet) is None
    keys = set(unet.state_dict())
    hip.configure("x6", "f32")
    assert (hip.conv_family, hip.conv_fallback) == ("x6", "f32") and callable(hip.fallback(unet))
    assert set(unet.state_dict()) == keys                 # settings of the backend, never of the checkpoint
    with pytest.raises(ValueError, match="convolution family"):
        hip.configure("x7", None)
    with pytest.raises(ValueError, match="exact family"):
        hip.configure(None, "h3")                         # a fallback into the family with the range limit is none
    assert (hip.conv_family, hip.conv_fallback) == ("x6", "f32")      # a refused call changes nothing


def test_new_entry_points_are_declared_and_bound():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    for name in ("cddpm_set_conv_family", "cddpm_get_conv_family", "cddpm_slice_status"):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in lib_mod.SYMBOLS, name
    lib = lib_mod.load_library()
    assert lib.cddpm_get_conv_family(None) == -1 and lib.cddpm_set_conv_family(None, 1) == -1      # NULL handle: refused, no crash
