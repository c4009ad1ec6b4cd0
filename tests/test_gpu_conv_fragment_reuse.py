"""GPU: the fused convolution's column-fragment mapping (csrc/conv_x6.hip: a row of taps reads each patch column once) computes what the
row mapping computed, bit for bit.

The yardstick is the library of the commit before the mapping changed: tests/golden/conv_bits_parent.json holds the md5 digests that
tools/conv_bits.py printed with CDDPM_LIB pointing at a build of that commit (recorded in the file with the seed and the shapes). The
tests recompute the digests with the product library and compare strings; the inputs are host-generated (numpy default_rng), so nothing
but the convolution decides them. Cases: tools/conv_bits.py (one tile, ragged rows, partial and narrow column tiles, two sources / two
cout blocks, identity affine, the folded upsample's classes, the 1x1 skip segment, the statistics records through the coefficients that
op_conv_gn returns), in three modes: a precision-32 handle, the 256-cout plan (CDDPM_NB2=force, read once per process: a child, as in
test_gpu_modes.py) and a precision-16 handle (as in test_gpu_precision16.py), the latter with a small UNet forward on the hi-only kernels."""
import importlib.util
import json
import os

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def _tool():
    spec = importlib.util.spec_from_file_location("conv_bits", os.path.join(ROOT, "tools", "conv_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLD, "conv_bits_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tool(parent):
    t = _tool()
    # the recorded digests are of THESE inputs
    assert parent["seed"] == t.SEED and parent["cases"] == {k: list(v) for k, v in t.CASES.items()}
    return t


def _compare(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        print(f"{name:32s} {got[name]} {'==' if got[name] == want[name] else '!='} parent {want[name]}")
    bad = [name for name in want if got[name] != want[name]]
    assert not bad, f"digests differ from the parent commit's: {bad}"


@pytest.mark.parametrize("mode", ["default", "p16"])
def test_conv_bits_equal_parent(tool, parent, mode, monkeypatch):
    monkeypatch.delenv("CDDPM_NB2", raising=False)
    _compare(tool.digests(mode), parent["modes"][mode])


def test_conv_bits_equal_parent_256_cout_plan(tool, parent):
    _compare(tool.digests_in_child("nb2"), parent["modes"]["nb2"])


def test_conv_bits_equal_parent_p16_256_cout_plan(tool, parent):
    """the hi-only 256-cout kernels <9,2,true,2> and <4,2,true,2>, which the three modes above do not reach (the operator entry points do
    not take the handle's precision): the set's 256-cout cases launched as a precision-16 handle plans them (op_conv_planned) under
    CDDPM_NB2=force. tests/golden/conv_bits_p16nb2_parent.json is `conv_bits.py --mode p16nb2` with CDDPM_LIB pointing at a build of the
    commit before conv_split_kernel took its constants and slot functions from conv_split.h. The mode asserts that the plan taken is one
    unsplit launch of 256-cout workgroups; that the operands were hi-only shows in digests that differ from the `nb2` mode's."""
    with open(os.path.join(GOLD, "conv_bits_p16nb2_parent.json")) as f:
        rec = json.load(f)
    assert rec["seed"] == tool.SEED and rec["cases"] == {k: list(tool.CASES[k]) for k in tool.P16NB2_CASES}
    want = rec["modes"]["p16nb2"]
    assert all(want[k] != parent["modes"]["nb2"][k] for k in want), "the recorded digests are those of the two-term kernels"
    _compare(tool.digests_in_child("p16nb2"), want)
