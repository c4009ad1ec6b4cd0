"""Host logic of training a UNet that has attention inside its resolution levels: training.unet_program with `attention_resolutions`
(reference UNetModel.__init__, OpenAI_Unet.py:604-797) -- the default is the program as it was, the `attn_levels` descriptor of
tests/arch_cases.py and a one-level descriptor visit exactly the state dict's modules, the up-ResBlock moves to sub-index 2 behind an
attention, and the skip stack balances with the attention's output on it."""
import pytest
import torch

import arch_cases as A
from conftest import load_pkg

# attention at ONE level only (ds = 2): 128 x (1, 2, 2), two ResBlocks per level
ONE_LEVEL = dict(model_channels=128, channel_mult=(1, 2, 2), num_res_blocks=2, attention_resolutions=(2,), cond_dim=128, geometry=(2, 16, 24))
DESCRIPTORS = {"attn_levels": A.CASES["attn_levels"], "one_level": ONE_LEVEL}


def _program(tr, case):
    return tr.unet_program(case["model_channels"], case["channel_mult"], case["num_res_blocks"], attention_resolutions=case["attention_resolutions"])


def _up_blocks(prog):
    return [n for kind, n, a in prog if kind == "res" and a["kind"] == "up"]


@pytest.mark.parametrize("name", list(A.CASES))
def test_default_attention_resolutions_leave_every_program_as_it_was(name):
    tr = load_pkg("training")
    c = A.CASES[name]
    args = (c["model_channels"], c["channel_mult"], c["num_res_blocks"])
    assert tr.unet_program(*args) == tr.unet_program(*args, attention_resolutions=(3, 6, 12))
    assert all(n == "middle_block.1" for kind, n, _a in tr.unet_program(*args) if kind == "attn")


@pytest.mark.parametrize("name", list(DESCRIPTORS))
def test_program_visits_exactly_the_state_dict(synth, name):
    tr = load_pkg("training")
    case = DESCRIPTORS[name]
    prog = _program(tr, case)
    shapes = synth.unet_param_shapes(**A.synth_kw(case))
    emb = {k for k in shapes if k.startswith(("time_embed.", "label_emb."))}
    assert tr.program_param_names(prog) | emb == set(shapes)
    assert tr.unsupported_blocks(shapes, prog) == []
    tab = tr.conv_table(prog)
    for k, (co, ci, ks, _folded, _grp) in tab.items():
        assert tuple(shapes[k + ".weight"][:2]) == (co, ci) and shapes[k + ".weight"][2] == ks, k
    # forward order = the state dict's registration order (the flat gradient buffer is filled from its tail by the backward pass)
    first = {}
    for i, k in enumerate(shapes):
        first.setdefault(".".join(k.split(".")[:3]), i)
    order = [first[n] for kind, n, _a in prog if kind in ("res", "attn") and not n.startswith("middle_block")]
    assert order == sorted(order)


def test_up_resblocks_sit_behind_the_attention():
    tr = load_pkg("training")
    assert _up_blocks(_program(tr, DESCRIPTORS["attn_levels"])) == ["output_blocks.1.2", "output_blocks.3.2"]
    # (1, 2, 2) x 2 ResBlocks: output blocks 0-2 at ds 4, 3-5 at ds 2 (attention), 6-8 at ds 1: the up-ResBlock of the attention's
    # level at sub-index 2, the one of the level below (ds 4: no attention) at sub-index 1
    prog = _program(tr, ONE_LEVEL)
    assert _up_blocks(prog) == ["output_blocks.2.1", "output_blocks.5.2"]
    assert [n for kind, n, _a in prog if kind == "attn"] == ["input_blocks.4.1", "input_blocks.5.1", "middle_block.1", "output_blocks.3.1",
                                                             "output_blocks.4.1", "output_blocks.5.1"]


@pytest.mark.parametrize("name", list(DESCRIPTORS) + list(A.CASES))
def test_skip_stack_balances(name):
    """the pushes and pops of UNetTrainer.forward, run on channel counts: every input block pushes once, by its last entry (the
    attention where it has one); every pop hands the concatenating ResBlock the channels its `concat` names; nothing is left"""
    tr = load_pkg("training")
    case = DESCRIPTORS.get(name) or A.CASES[name]
    prog = _program(tr, case)
    stack, ch, pops = [], None, 0
    for i, (kind, n, a) in enumerate(prog):
        if kind == "in":
            ch = case["model_channels"]
            stack.append(ch)
        elif kind == "res":
            if a.get("concat"):
                assert stack.pop() == a["concat"], n
                assert a["cin"] == ch + a["concat"], n
                pops += 1
            else:
                assert a["cin"] == ch, n
            ch = a["cout"]
            if a.get("push"):
                stack.append(ch)
        elif kind == "attn":
            assert a["c"] == ch, n
            if a.get("push"):
                assert prog[i - 1][0] == "res" and not prog[i - 1][2].get("push"), n          # one push per block: the last entry's
                stack.append(ch)
    assert stack == []
    assert pops == len(case["channel_mult"]) * (case["num_res_blocks"] + 1)
    blocks = {".".join(n.split(".")[:2]) for _k, n, _a in prog if n.startswith("input_blocks.")}
    pushes = 1 + sum(1 for kind, _n, a in prog if kind in ("res", "attn") and a.get("push"))
    assert pushes == len(blocks) == pops


def test_attention_scratch_is_the_row_statistics_of_the_largest_attention():
    """the arena share of cddpm_op_attention_backward (B x C/64 x N x 2 floats): the middle attention by default, level 0 at `attn_levels`"""
    tr = load_pkg("training")
    assert tr.attention_scratch_bytes(tr.unet_program(), 16, 128, 128) == 16 * 4 * 1024 * 2 * 4
    prog = _program(tr, DESCRIPTORS["attn_levels"])
    assert tr.attention_scratch_bytes(prog, 16, 128, 128) == 16 * 2 * 16384 * 2 * 4
    assert tr.attention_scratch_bytes(prog, 2, 16, 24) == 2 * 2 * 384 * 2 * 4
    assert tr.attention_scratch_bytes(_program(tr, ONE_LEVEL), 2, 16, 24) == 2 * 4 * 96 * 2 * 4


def test_state_dict_and_program_must_agree(synth):
    """refused before anything touches a device: a state dict with blocks the chosen program does not visit (NotImplementedError with
    their names, as before), and a program whose attention blocks the state dict does not hold (ValueError with the missing keys)"""
    tr = load_pkg("training")
    case = A.CASES["attn_levels"]
    with_att = {k: torch.zeros(s) for k, s in synth.unet_param_shapes(**A.synth_kw(case)).items()}
    without = {k: torch.zeros(s) for k, s in synth.unet_param_shapes(**dict(A.synth_kw(case), attention_resolutions=A.DEFAULT_ATT)).items()}
    with pytest.raises(NotImplementedError, match=r"input_blocks\.1\.1.*output_blocks\.1\.1.*attention_resolutions=\(3, 6, 12\)"):
        tr.UNetTrainer(with_att, device="cpu", **A.trainer_kw(case))
    with pytest.raises(NotImplementedError, match=r"output_blocks\.1\.1.*attention_resolutions=\(2,\)"):      # attention at other levels than the model's
        tr.UNetTrainer(with_att, device="cpu", attention_resolutions=(2,), **A.trainer_kw(case))
    with pytest.raises(ValueError, match=r"input_blocks\.1\.1\.norm\.bias.*input_blocks\.1\.1\.qkv\.weight") as ei:
        tr.UNetTrainer(without, device="cpu", attention_resolutions=case["attention_resolutions"], **A.trainer_kw(case))
    assert "output_blocks.5.1.proj_out.weight" in str(ei.value) and "middle_block" not in str(ei.value)


# what the rule of commit 4a2354e gave both handles at these geometries, in bytes (its UNetTrainer._fit evaluated on the host:
# max(ARENA_FLOOR, operator_scratch_bytes) + two fp16 planes of the widest ResBlock's k-images); the same for either program below
ARENA_4A2354E = {(64, 128, 128): 2348810240, (32, 96, 96): 805306368, (16, 128, 128): 738197504}


@pytest.mark.parametrize("geometry", [(64, 128, 128), (32, 96, 96), (16, 128, 128)], ids=lambda g: "x".join(map(str, g)))
def test_operator_scratch_bound_of_the_benchmarked_geometries_fits_the_arena_floor(geometry):
    """training.operator_scratch_bytes, the rule UNetTrainer._fit sizes the arenas by (arena_bytes): the library's own size queries over
    the step's calls. At the large-batch, the reference's and the benchmarked geometry, for the default program and for `attn_levels`'
    attention at every level, the arena of either handle is not larger than the one the earlier rule gave (floor + k-images: a sum,
    where the largest single call is a maximum), and it holds every term it names"""
    tr = load_pkg("training")
    B, H, W = geometry
    for att in ((3, 6, 12), (1, 2, 4)):
        prog = tr.unet_program(128, (1, 2, 2), 3, att)
        main, side = tr.operator_scratch_bytes(prog, B, H, W, 1024)
        arena = tr.arena_bytes(prog, B, H, W, 1024)
        assert arena == (max(main, tr.ARENA_FLOOR), max(side, tr.ARENA_FLOOR))       # the encoder's calls are far smaller here
        assert side <= main and max(arena) <= ARENA_4A2354E[geometry]
        assert main >= B * H * W * 9 * 4                                   # the head's partial products
        assert main >= tr.attention_scratch_bytes(prog, B, H, W)
        assert main >= 33 * B * 1024 * 4                                   # the batched embedding Linear's backward
        assert side >= 8 * 256 * 512 * 9 * 4                               # eight partial tiles of the 512 -> 256 convolution's weight gradient


def test_operator_scratch_bound_grows_past_the_floor_where_a_call_does():
    tr = load_pkg("training")
    prog = tr.unet_program()
    sizes = [tr.operator_scratch_bytes(prog, *g, 1024)[0] for g in ((2, 16, 24), (16, 128, 128), (64, 128, 128), (64, 256, 256), (64, 512, 512))]
    assert sizes == sorted(sizes)
    assert sizes[-1] >= 64 * 512 * 512 * 9 * 4 > tr.ARENA_FLOOR            # the head at 64 x 512 x 512: 604 MB
    # channels as wide as `w384_limit`'s: eight partial tiles of the 1536 -> 768 weight gradient are 340 MB, whatever the geometry
    c = A.CASES["w384_limit"]
    main, side = tr.operator_scratch_bytes(tr.unet_program(c["model_channels"], c["channel_mult"], c["num_res_blocks"]), *c["geometry"], 8 * 384)
    assert main == side and side >= 8 * 768 * 1536 * 9 * 4 > tr.ARENA_FLOOR
