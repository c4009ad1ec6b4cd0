"""Host side of the SparK pre-training operators (no GPU): every entry point of csrc/spark_train.hip is declared in include/cddpm.h, bound in
_lib.SYMBOLS with the declaration's argument count and exported by the library; the size queries answer 0 for refused shapes and state
what a call takes for served ones."""
import os
import re
import shutil
import subprocess

from conftest import ROOT, load_pkg

OPS = ("cddpm_op_spark_bn_forward", "cddpm_op_spark_bn_backward", "cddpm_op_spark_mask_mul", "cddpm_op_spark_conv", "cddpm_op_spark_conv_wgrad",
       "cddpm_op_spark_loss", "cddpm_op_adamw_guarded")
QUERIES = ("cddpm_op_spark_bn_forward_scratch", "cddpm_op_spark_bn_backward_scratch", "cddpm_op_spark_conv_scratch",
           "cddpm_op_spark_conv_wgrad_scratch", "cddpm_op_spark_loss_scratch")


def _declared(header):
    """name -> argument count of every function include/cddpm.h declares"""
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t|size_t|void|const char\*)\s+(cddpm_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_header_declarations_equal_the_exported_symbols():
    lib_mod = load_pkg("_lib")
    declared = _declared(open(os.path.join(ROOT, "include", "cddpm.h")).read())
    for name in OPS + QUERIES:
        assert name in declared, f"{name} is not declared in include/cddpm.h"
    assert set(declared) == set(lib_mod.SYMBOLS)
    for name, nargs in declared.items():
        assert len(lib_mod.SYMBOLS[name][1]) == nargs, name
    lib_mod.load_library()                                       # binds every name of SYMBOLS: raises if one is not exported
    tool = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert tool, "no nm / llvm-nm to list the library's exports with (binutils, or ROCm's llvm)"
    nm = subprocess.run([tool, "-D", "--defined-only", lib_mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("cddpm_")}
    assert exported == set(declared), sorted(exported ^ set(declared))


def test_a_null_handle_is_refused_without_a_crash():
    lib = load_pkg("_lib").load_library()
    assert lib.cddpm_op_spark_mask_mul(None, None, None, None, 1, 2, 2, 1, 1, None) == -1
    assert lib.cddpm_op_spark_conv(None, None, None, None, None, 1, 2, 2, 4, 4, 3, 0, 0, None) == -1
    assert lib.cddpm_op_adamw_guarded(None, None, None, None, None, 4, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, None, None) == -1


def test_queries_answer_zero_for_refused_shapes_and_bytes_for_served_ones():
    q = load_pkg("_lib").scratch_query
    # BatchNorm: chunked fp64 partial sums (2 per channel forward, 3 backward) + the backward's 2 C means / the forward's status words
    assert q("spark_bn_forward", 2 * 64, 64, 64) == 2 * 64 * 8 + 256
    assert q("spark_bn_backward", 2 * 64, 64, 64) == 3 * 64 * 8 + 2 * 64 * 4
    assert q("spark_bn_forward", 32 * 96 * 96, 96 * 96, 4) > q("spark_bn_forward", 96 * 96, 96 * 96, 4) > 0
    for bad in ((128, 64, 6), (128, 64, 0), (128, 64, 2), (100, 64, 64), (0, 64, 64), (128, 0, 64)):       # C no multiple of 4 / < 4; N no multiple of HW
        assert q("spark_bn_forward", *bad) == 0 and q("spark_bn_backward", *bad) == 0
    # convolutions: nothing without a contraction split, Z planes of the result with one
    assert q("spark_conv", 4, 96, 96, 8, 4, 3, 0, 0) == 0
    planes = q("spark_conv", 1, 4, 6, 1024, 64, 3, 0, 0)
    assert planes > 0 and planes % (24 * 64 * 4) == 0
    assert q("spark_conv", 2, 3, 3, 128, 128, 4, 1, 0) % 256 == 0
    for bad in ((1, 4, 4, 8, 8, 5, 0, 0), (1, 4, 4, 8, 8, 3, 1, 0), (1, 4, 4, 8, 8, 4, 0, 1), (1, 4, 4, 0, 8, 3, 0, 0), (0, 4, 4, 8, 8, 3, 0, 0)):
        assert q("spark_conv", *bad) == 0 and q("spark_conv_wgrad", *bad[:7], 0) == 0
    assert q("spark_conv_wgrad", 4, 96, 96, 8, 4, 3, 0, 0) >= 8 * 4 * 9 * 4
    assert q("spark_conv_wgrad", 1, 2, 2, 2048, 128, 1, 0, 1) > q("spark_conv_wgrad", 1, 2, 2, 2048, 128, 1, 0, 0) > 0
    assert q("spark_conv_wgrad", 1, 2, 2, 128, 512, 1, 0, 1) == 0                  # a bias gradient beyond 256 channels
    assert q("spark_loss", 4, 96, 96, 3) > 0
    assert q("spark_loss", 4, 96, 96, 5) == 0 and q("spark_loss", 0, 96, 96, 3) == 0
