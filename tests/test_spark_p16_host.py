"""Host: precision 16 of SparK pre-training without a device -- the two scaled entry points are exported and refuse a NULL handle, the
trainer parses its precision before it touches a device, and the arena of a precision-16 trainer is sized over the fp16-MFMA convolution
calls (spark_training.operator_calls(..., precision=16)) from the library's own size queries. The mirror's precision mapping too."""
import pytest

from conftest import load_pkg

NEW = ("cddpm_op_spark_loss_scaled", "cddpm_op_adamw_scaled")
FP32_CONVS = ("enc_conv", "enc_conv_wgrad")
P16_CONVS = ("enc_conv_p16", "enc_conv_wgrad_p16")


def test_the_library_exports_the_scaled_entry_points():
    L = load_pkg("_lib")
    lib = L.load_library()
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    # a NULL handle is refused before anything is read
    assert lib.cddpm_op_spark_loss_scaled(None, None, None, None, 1, 1, 32, 32, 1.0, 0.0, None, None, None, None) == -1
    assert lib.cddpm_op_adamw_scaled(None, None, None, None, None, 4, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, None, None, None) == -1


@pytest.mark.parametrize("bad", ["bf16", 8, "bf16-mixed", None, True, 64])
def test_trainer_parses_the_precision_before_a_device(bad):
    """a device that does not exist: the ValueError is the precision's, raised before anything is created on it"""
    st = load_pkg("spark_training")
    with pytest.raises(ValueError, match="precision"):
        st.SparKTrainer({}, "cuda:99", precision=bad)


def test_precision16_names_a_gpu_device():
    """precision 16 is the fp16-MFMA kernels: a device that is no GPU is refused with a ValueError of the precision's, before anything is
    created on it (tests/test_spark_host.py pins the words it had before the step was built); the dec_dim check still comes first"""
    st = load_pkg("spark_training")
    for value in (16, "16", "16-mixed"):
        with pytest.raises(ValueError, match="precision.*not built for device 'cpu'"):
            st.SparKTrainer({}, "cpu", precision=value)
    with pytest.raises(NotImplementedError, match="dec_dim"):
        st.SparKTrainer({}, "cpu", precision=16, dec_dim=64)


def test_precision16_calls_size_the_arena():
    st, et, lib = load_pkg("spark_training"), load_pkg("encoder_training"), load_pkg("_lib")
    B, H, W = 4, 64, 64
    calls = list(st.operator_calls(B, H, W, precision=16))
    ops = [op for op, _a in calls]
    assert ops.count("enc_conv_p16") == 2 * 52 and ops.count("enc_conv_wgrad_p16") == 52
    assert not any(op in FP32_CONVS for op in ops)
    # forward and input gradient of each of the 52 convolutions: the same geometry, transposed 0 and 1
    fwd = [a[:7] for op, a in calls if op == "enc_conv_p16" and a[7] == 0]
    dx = [a[:7] for op, a in calls if op == "enc_conv_p16" and a[7] == 1]
    dw = [a for op, a in calls if op == "enc_conv_wgrad_p16"]
    assert fwd == dx == dw and len(fwd) == 52
    need = [lib.scratch_query(op, *a) for op, a in calls]
    # A size query answers 0 for a shape its operator refuses AND for a call that takes no temporaries (a convolution that is not
    # split writes its output itself: 16 of the 104 cddpm_op_enc_conv_p16 calls and 19 of the 52 weight gradients here, 13 spark_conv),
    # so "non-zero for every call" holds for the operators that always take some, as tests/test_spark_host.py asks at precision 32;
    # for the p16 convolutions "none refused" is the operator's own acceptance rule (include/cddpm.h), checked on every listed call,
    # and a listed call that answers 0 has a forward / transposed / weight-gradient sibling of the same geometry that does not.
    always = ("spark_bn_forward", "spark_bn_backward", "spark_conv_wgrad", "spark_loss", "enc_stem_wgrad")
    assert all(n > 0 for (op, _a), n in zip(calls, need) if op in always)
    assert all(a[0] == B and a[3] % 64 == 0 and a[4] % 64 == 0 and 64 <= a[3] <= 2048 and 64 <= a[4] <= 2048 and a[5] in (1, 3) and a[6] in (1, 2)
               for op, a in calls if op in P16_CONVS)
    by_geom = {}
    for (op, a), n in zip(calls, need):
        if op in P16_CONVS:
            by_geom[a[:7]] = max(by_geom.get(a[:7], 0), n)
    assert all(n > 0 for n in by_geom.values()), [g for g, n in by_geom.items() if n == 0]
    assert st.arena_bytes(B, H, W, precision=16) == max(need) > 0
    assert st.arena_bytes(B, H, W, precision="16-mixed") == max(need)
    # precision 32: today's list, which has none of the p16 calls
    today = list(st.operator_calls(B, H, W))
    assert list(st.operator_calls(B, H, W, precision=32)) == today and st.arena_bytes(B, H, W, precision=32) == st.arena_bytes(B, H, W)
    assert not any(op in P16_CONVS for op, _a in today) and sum(op == "enc_conv" for op, _a in today) == 2 * 52
    # the two lists differ in the convolutions only
    strip = lambda cs: [(op, a) for op, a in cs if op not in FP32_CONVS + P16_CONVS]
    assert strip(calls) == strip(today)
    assert list(et.pyramid_operator_calls(B, H, W)) == list(et.pyramid_operator_calls(B, H, W, 32))
    with pytest.raises(ValueError, match="precision"):
        list(st.operator_calls(B, H, W, precision="bf16"))


def test_the_mirror_maps_lightning_precisions():
    """cfg.precision in training.set_precision's spellings; the mapping needs neither library nor device"""
    S, tr = load_pkg("Spark_2D"), load_pkg("training")
    base = dict(backbone="resnet50", imageDim=[192, 192, 100], rescaleFactor=2, mask_ratio=0.65, pix_norm=False, lr=1e-4)
    assert S.Spark_2D(dict(base)).precision_bits() == 32
    for value, bits in ((32, 32), ("32-true", 32), (16, 16), ("16", 16), ("16-mixed", 16), ("bf16", 16), ("bf16-mixed", 16)):
        assert S.Spark_2D(dict(base, precision=value)).precision_bits() == bits == tr.lightning_precision_bits(value)
    with pytest.raises(ValueError, match="precision"):
        S.Spark_2D(dict(base, precision="fp8")).precision_bits()
    assert "Precision 32 only" not in S.__doc__
