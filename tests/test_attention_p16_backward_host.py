"""Host side of the precision-16 attention backward (no GPU): cddpm_op_attention_backward_p16 in header, binding and library, the
trainer's `attention_precision` argument and its spellings, and the mirrors' `cfg.train_attention_precision`."""
import inspect
import os
import re

import pytest

from conftest import ROOT, load_pkg

NAME = "cddpm_op_attention_backward_p16"


def _args_of(header, name):
    m = re.search(rf"\bint {name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/cddpm.h"
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


def test_entry_point_is_declared_bound_and_exported():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    args = _args_of(header, NAME)
    assert len(args) == 8, args
    assert NAME in lib_mod.SYMBOLS and len(lib_mod.SYMBOLS[NAME][1]) == 8
    # the contract of the fp32 backward, whose own declaration is unchanged
    assert lib_mod.SYMBOLS[NAME] == lib_mod.SYMBOLS["cddpm_op_attention_backward"]
    assert [a.split()[-1] for a in args] == [a.split()[-1] for a in _args_of(header, "cddpm_op_attention_backward")]
    lib = lib_mod.load_library()                           # binds every name of SYMBOLS: raises if one is not exported
    assert hasattr(lib, NAME)
    assert getattr(lib, NAME)(None, None, None, None, 1, 1, 64, None) == -1      # NULL handle: refused, no crash
    # the training-precision comment no longer says that attention is fp32 whatever the caller asks
    assert "GroupNorm, attention, embeddings" not in header
    assert "unless the trainer asks otherwise" in header


def test_trainer_signature_and_spellings():
    tr, eng = load_pkg("training"), load_pkg("engine")
    par = inspect.signature(tr.UNetTrainer.__init__).parameters
    assert "attention_precision" in par and par["attention_precision"].default == 32
    assert par["attention_precision"].kind is inspect.Parameter.KEYWORD_ONLY
    for value, bits in ((16, 16), ("16-mixed", 16), ("16", 16), (32, 32), ("32", 32)):
        assert eng.precision_bits(value) == bits, value
    for bad in ("bf16", 8):
        with pytest.raises(ValueError, match="precision"):
            eng.precision_bits(bad)
    par = inspect.signature(eng.CddpmEngine.op_attention_backward).parameters
    assert "precision" in par and par["precision"].default == 32


def test_trainer_parses_attention_precision_before_it_touches_a_device(monkeypatch):
    tr = load_pkg("training")
    monkeypatch.setattr(tr, "CddpmEngine", lambda *a, **k: pytest.fail("an engine was created"))
    for bad in ("bf16", 8, None):
        with pytest.raises(ValueError, match="precision"):
            tr.UNetTrainer({}, device="cpu", attention_precision=bad)


def test_mirror_passes_train_attention_precision(monkeypatch):
    """HipMirror.hip_trainer (shared by DDPM_2D and the patched mirror) hands cfg.train_attention_precision to UNetTrainer; absent = 32"""
    mc, tr = load_pkg("mirror_common"), load_pkg("training")
    seen = []

    class FakeTrainer:
        def __init__(self, params, **kw):
            seen.append(kw["attention_precision"])

    monkeypatch.setattr(tr, "UNetTrainer", FakeTrainer)

    class Unet:
        model_channels, channel_mult, num_res_blocks, num_classes, dropout, attention_resolutions = 128, (1, 2, 2), 3, 128, 0.0, (3, 6, 12)

        def state_dict(self):
            return {}

    for cfg, want in (({}, 32), ({"train_attention_precision": 16}, 16), ({"train_attention_precision": "16-mixed"}, "16-mixed"),
                      ({"train_attention_precision": None}, 32)):
        m = object.__new__(mc.HipMirror)
        m.__dict__.update(cfg=cfg, diffusion=type("D", (), {"model": Unet()})(), _hip_unet_trainer=None)
        m._alias_unet = lambda: None
        m._load_pending_optimizer_state = lambda: None
        m.hip_trainer("cpu")
        assert seen[-1] == want, (cfg, seen[-1])
    for mod in ("DDPM_2D", "DDPM_2D_patched"):
        assert "train_attention_precision" in load_pkg(mod).__doc__
