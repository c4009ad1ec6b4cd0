"""Host side of the context encoder's precision 16 (no GPU): the five entry points in header, binding and library, EncoderTrainer's
`precision` argument, the mirror's `cfg.train_encoder_precision`, and the arenas: training.arena_bytes covers every p16 call."""
import inspect
import os
import re

import pytest

from conftest import ROOT, load_pkg
from test_operator_scratch_host import DESCRIPTORS, _program

OPS = ("cddpm_op_enc_pack_w_p16", "cddpm_op_enc_conv_p16", "cddpm_op_enc_conv_wgrad_p16")
QUERIES = ("cddpm_op_enc_conv_p16_scratch", "cddpm_op_enc_conv_wgrad_p16_scratch")


def _args_of(header, name, ret="int"):
    m = re.search(rf"\b{ret} {name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/cddpm.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_entry_points_are_declared_bound_and_exported():
    lib_mod = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "cddpm.h")).read()
    for name in OPS:
        args = _args_of(header, name)
        fp32 = name[:-len("_p16")]
        assert name in lib_mod.SYMBOLS and len(lib_mod.SYMBOLS[name][1]) == len(args) == len(_args_of(header, fp32))      # mirrors the fp32 entry point
    for name in QUERIES:
        args = _args_of(header, name, "size_t")
        assert name in lib_mod.SYMBOLS and len(lib_mod.SYMBOLS[name][1]) == len(args)
    lib = lib_mod.load_library()                       # binds every name of SYMBOLS: raises if one is not exported
    assert lib.cddpm_op_enc_conv_p16(None, None, None, None, 1, 1, 1, 64, 64, 1, 1, 0, None) == -1        # NULL handle: refused, no crash
    assert "wf16 [K*K][Cin / 32][Cout][32]" in header and "wd16 [K*K][Cout / 32][Cin][32]" in header       # the image layouts are documented
    src = open(os.path.join(ROOT, "conditioned-diffusion-models-uad_amd", "csrc", "encoder_train.hip")).read()
    assert "Everything NHWC fp32, plain FMA tiles" not in src and "plain fp32 FMA kernels (the encoder is" not in header


def test_trainer_precision_is_keyword_only_and_parsed_before_a_device_call():
    et = load_pkg("encoder_training")
    par = inspect.signature(et.EncoderTrainer.__init__).parameters
    assert par["precision"].default == 32 and par["precision"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(par)[:4] == ["self", "params", "ops", "drop_path_rate"]

    class NoDevice:
        def __getattr__(self, name):
            pytest.fail(f"the trainer touched ops.{name}")

    for bad in ("bf16", 8, None, "fp16"):
        with pytest.raises(ValueError, match="precision"):
            et.EncoderTrainer({}, NoDevice(), precision=bad)
    with pytest.raises(TypeError):
        et.EncoderTrainer({}, NoDevice(), 0.0, 16)


def test_mirror_passes_train_encoder_precision(monkeypatch):
    """DDPM_2D.hip_encoder_trainer hands cfg.train_encoder_precision to EncoderTrainer; absent or None = 32"""
    mod, et, de = load_pkg("DDPM_2D"), load_pkg("encoder_training"), load_pkg("DDPM_encoder")
    seen = []

    class FakeTrainer:
        def __init__(self, params, ops, drop_path_rate=0.0, *, precision=32):
            seen.append(precision)

    monkeypatch.setattr(et, "EncoderTrainer", FakeTrainer)

    class Core(de.ResNet50Encoder):
        def __init__(self):             # an instance of the native encoder's class without its weights
            pass

        def state_dict(self):
            return {}

    for cfg, want in (({}, 32), ({"train_encoder_precision": 16}, 16), ({"train_encoder_precision": "16-mixed"}, "16-mixed"),
                      ({"train_encoder_precision": None}, 32), ({"train_encoder_precision": 32, "train_attention_precision": 16}, 32)):
        m = object.__new__(mod.DDPM_2D)
        m.__dict__.update(cfg=cfg, encoder=Core(), _hip_enc_trainer=None)
        m.hip_trainer = lambda device: None
        m._alias_encoder = lambda: None
        m._load_pending_optimizer_state = lambda: None
        m.hip_encoder_trainer("cpu")
        assert seen[-1] == want, (cfg, seen[-1])
    doc = mod.__doc__
    assert "train_encoder_precision" in doc and doc.index("train_attention_precision") < doc.index("train_encoder_precision")
    assert "underflow" in doc[doc.index("train_encoder_precision"):]


@pytest.mark.parametrize("name", list(DESCRIPTORS))
def test_the_arena_holds_every_p16_call(name, monkeypatch):
    """at the descriptor's own geometry and at 64 x 128 x 128, without the floor: what UNetTrainer._fit gives each handle holds every p16
    call of the encoder, without being told the encoder's precision (encoder_training.operator_calls lists both arithmetics)"""
    tr, enc = load_pkg("training"), load_pkg("encoder_training")
    monkeypatch.setattr(tr, "ARENA_FLOOR", 0)
    case = DESCRIPTORS[name]
    prog = _program(tr, case)
    for B, H, W in (case["geometry"], (64, 128, 128)):
        main, side = tr.arena_bytes(prog, B, H, W, 8 * case["model_channels"], case["cond_dim"])
        calls = [(op, a) for op, a in enc.operator_calls(B, H, W, case["cond_dim"]) if op.endswith("_p16")]
        assert sorted({op for op, _ in calls}) == ["enc_conv_p16", "enc_conv_wgrad_p16"]
        assert len(calls) == 3 * 52 and sum(op == "enc_conv_wgrad_p16" for op, _ in calls) == 52
        for op, a in calls:
            n = tr.scratch_query(op, *a)
            assert n <= main, (op, a, n, main)
            if op == "enc_conv_wgrad_p16":
                assert n <= side, (op, a, n, side)              # 0: one pixel range of a 1x1 writes dw itself
    # the split path really takes planes: layer 4 at 16 x 128 x 128 is 4 x 4 pixels
    assert tr.scratch_query("enc_conv_p16", 16, 4, 4, 512, 2048, 1, 1, 0) > 0


def test_p16_queries_answer_zero_for_refused_shapes():
    tr = load_pkg("training")
    assert tr.scratch_query("enc_conv_wgrad_p16", 1, 8, 8, 64, 64, 3, 1) > 0
    for q, tail in (("enc_conv_p16", (0,)), ("enc_conv_p16", (1,)), ("enc_conv_wgrad_p16", ())):
        assert tr.scratch_query(q, 1, 8, 8, 32, 64, 3, 1, *tail) == 0          # Cin not a multiple of 64
        assert tr.scratch_query(q, 1, 8, 8, 64, 96, 3, 1, *tail) == 0          # Cout not a multiple of 64
        assert tr.scratch_query(q, 1, 8, 8, 64, 64, 3, 0, *tail) == 0          # stride 0
        assert tr.scratch_query(q, 1, 8, 8, 64, 64, 3, 3, *tail) == 0          # stride 3
        assert tr.scratch_query(q, 1, 8, 8, 64, 64, 5, 1, *tail) == 0          # K = 5
        assert tr.scratch_query(q, 1, 8, 8, 64, 4096, 1, 1, *tail) == 0        # beyond 2048 channels
