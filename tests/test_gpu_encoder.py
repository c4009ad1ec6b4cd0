"""GPU: the native context encoder (csrc/encoder.hip behind DDPM_encoder.ResNet50Encoder) against the
torch restatement of timm's ResNet-50 in oracle/encoder_oracle.py. PARITY UNPINNED with respect to the reference: timm is
not installed in the build image, so the restatement itself cannot be checked against `timm.create_model('resnet50',
in_chans=1, num_classes=128)`; what is tested is that the HIP kernels compute the restated network."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "oracle"))


@pytest.fixture(scope="module")
def enc_and_weights(synth):
    E = load_pkg("DDPM_encoder")
    w = synth.synth_encoder_state_dict(0, 128)
    enc = E.ResNet50Encoder(num_classes=128)
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    yield enc, {k: torch.from_numpy(v) for k, v in w.items()}
    enc.close()


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (3, 96, 96), (1, 128, 128), (2, 80, 96),
                                   (2, 72, 88), (1, 33, 47)])          # feature maps that turn odd: 36x44 ... 9x11, 5x6, 3x3 and 17x24, 9x12, 5x6, 3x3, 2x2
def test_encoder_forward_vs_oracle(enc_and_weights, synth, B, H, W):
    import encoder_oracle as EO
    enc, sdt = enc_and_weights
    x = torch.from_numpy(synth.synth_slices(4, 0, B, H, W))
    ref = EO.resnet50_forward(x, sdt)
    out = enc(x.cuda()).cpu()
    scale = float(ref.abs().max())
    err = float((out - ref).abs().max())
    print(f"encoder {B}x{H}x{W}: max|delta| {err:.3e} (|ref| max {scale:.3e})")
    assert out.shape == (B, 128)
    assert err < 1e-4 * max(1.0, scale)
    # float64 yardstick: the fp32 oracle's own distance from a float64 run of the same network
    ref64 = EO.resnet50_forward(x.double(), {k: v.double() for k, v in sdt.items()})
    e_ref, e_hip = float((ref.double() - ref64).abs().max()), float((out.double() - ref64).abs().max())
    print(f"   vs float64: torch fp32 {e_ref:.3e}, HIP {e_hip:.3e}")
    assert e_hip < 10 * e_ref + 1e-6


def test_encoder_handle_created_for_exactly_an_odd_half_size(synth):
    """ResNet50Encoder sizes its handle for at least 64 x 128 x 128, so the module never runs a handle at its limit. Here the handle is
    created for exactly 1 x 34 x 34 through the C ABI: the stem's output is 17 x 17 x 64 = 18496 floats and layer1's 9 x 9 x 256 = 20736,
    the larger of the two because 17 is odd -- the handle's activation buffers must hold it (cddpm_encoder_create sized them for the
    stem's output alone once: 18496 floats)."""
    import ctypes as C
    import encoder_oracle as EO
    lib = load_pkg("_lib").load_library()
    w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in synth.synth_encoder_state_dict(0, 128).items() if not k.endswith("num_batches_tracked")}
    B, H, W = 1, 34, 34
    h = C.c_void_p()
    assert lib.cddpm_encoder_create(C.byref(h), 128, B, H, W, 0) == 0, lib.cddpm_encoder_last_error(None)
    try:
        names = (C.c_char_p * len(w))(*[k.encode() for k in w])
        ptrs = (C.c_void_p * len(w))(*[a.ctypes.data for a in w.values()])
        nums = (C.c_int64 * len(w))(*[a.size for a in w.values()])
        assert lib.cddpm_encoder_load_weights(h, names, ptrs, nums, len(w)) == 0, lib.cddpm_encoder_last_error(h)
        x = torch.from_numpy(synth.synth_slices(4, 0, B, H, W))
        xg, out = x.cuda().contiguous(), torch.empty(B, 128, device="cuda")
        assert lib.cddpm_encoder_forward(h, xg.data_ptr(), out.data_ptr(), B, H, W, None) == 0, lib.cddpm_encoder_last_error(h)
        assert lib.cddpm_encoder_forward(h, xg.data_ptr(), out.data_ptr(), B, H + 1, W, None) != 0          # beyond the handle's limits: refused
        torch.cuda.synchronize()
    finally:
        lib.cddpm_encoder_destroy(h)
    ref = EO.resnet50_forward(x, {k: torch.from_numpy(v) for k, v in w.items()})
    scale, err = float(ref.abs().max()), float((out.cpu() - ref).abs().max())
    print(f"encoder {B}x{H}x{W} at the handle's limit: max|delta| {err:.3e} (|ref| max {scale:.3e})")
    assert err < 1e-4 * max(1.0, scale)


def test_encoder_in_ddpm2d(enc_and_weights, synth):
    """DDPM_2D.forward(x) -> c with the SparK-wrapped native encoder (the experiment's configuration)"""
    M = load_pkg("DDPM_2D")
    cfg = dict(imageDim=[192, 192, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True,
               test_timesteps=500, backbone="Spark_Encoder_2D", version="resnet50")
    mod = M.DDPM_2D(cfg)
    _enc, sdt = enc_and_weights
    mod.encoder.encoder.load_state_dict(sdt, strict=False)
    x = torch.from_numpy(synth.synth_slices(4, 0, 2, 96, 96)).cuda()
    c = mod(x)
    assert c.shape == (2, 128) and bool(torch.isfinite(c).all())
    import encoder_oracle as EO
    assert float((c.cpu() - EO.resnet50_forward(x.cpu(), sdt)).abs().max()) < 1e-4 * max(1.0, float(c.abs().max()))
    with pytest.raises(RuntimeError):
        mod.encoder(x.cpu())
    mod.encoder.encoder.close()
