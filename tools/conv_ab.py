#!/usr/bin/env python3
"""Interleaved A/B timing of the fused convolution (default fp16-split family) across library builds, on one device with random
data. Build a side-by-side library in the container first, e.g. build.build_lib(tag="base") -> csrc/libcddpm_hip_base.so, then on
the GPU box:
    python tools/conv_ab.py --run base prod prod+nb1 prod+nb2
A variant is LIB[+OPT]: LIB = "prod" (csrc/libcddpm_hip.so) or a tag; OPT nb1 / nb2 = CDDPM_NB2=0 / force (256-cout workgroups off /
wherever the kernel can). Each variant runs in its own process (CDDPM_LIB selects the .so) through the product entry points:
cddpm_op_pack_conv once, then cddpm_op_conv_packed timed between events. Shapes are the UNet's layers at B=64 (AB_BATCH)."""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")

# name, C0, C1, Cout, k, H, W, coef, silu, up, res_mode, skipC
SHAPES = [
    ("conv1 128>128 @128", 128, 0, 128, 3, 128, 128, 1, 1, 0, 0, 0),
    ("conv2 128>128 @128 +res", 128, 0, 128, 3, 128, 128, 1, 1, 0, 1, 0),
    ("plain 128>128 @128 nocoef", 128, 0, 128, 3, 128, 128, 0, 0, 0, 0, 0),
    ("coef only 128>128 @128", 128, 0, 128, 3, 128, 128, 1, 0, 0, 0, 0),
    ("silu only 128>128 @128", 128, 0, 128, 3, 128, 128, 0, 1, 0, 0, 0),
    ("up conv1 256>256 @128", 256, 0, 256, 3, 128, 128, 1, 1, 1, 0, 0),
    ("cat conv1 512>256 @64", 256, 256, 256, 3, 64, 64, 1, 1, 0, 0, 0),
    ("conv2 256>256 @64 +skip512", 256, 0, 256, 3, 64, 64, 1, 1, 0, 0, 512),
    ("conv2 256>256 @64 noskip", 256, 0, 256, 3, 64, 64, 1, 1, 0, 0, 0),
    ("conv2 128>128 @128 +skip384", 128, 0, 128, 3, 128, 128, 1, 1, 0, 0, 384),
    ("conv 256>256 @32", 256, 0, 256, 3, 32, 32, 1, 1, 0, 0, 0),
    ("cat conv1 384>128 @128", 256, 128, 128, 3, 128, 128, 1, 1, 0, 0, 0),
]


def child(B, iters):
    import torch
    lib = importlib.import_module(PKG + "._lib").load_library()
    eng = importlib.import_module(PKG + ".engine")
    e = eng.CddpmEngine(timesteps=10, max_batch=1, max_h=32, max_w=32)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1234)
    rnd = lambda *shape, scale=1.0: torch.randn(*shape, device="cuda", generator=g) * scale
    p = lambda t: None if t is None else t.data_ptr()

    def pack(Cout, Cin, k, mode, wexp):
        w = rnd(Cout, Cin, k, k, scale=0.01)        # w * 2^wexp (and the folded class sums) stay far inside the fp16 range
        taps = 4 if mode == 2 else k * k
        img = torch.empty(lib.cddpm_packed_conv_bytes(Cout, Cin, taps) * (4 if mode == 2 else 1), dtype=torch.uint8, device="cuda")
        assert lib.cddpm_op_pack_conv(e._h, p(w), Cout, Cin, k, mode, wexp, p(img), s) == 0, lib.cddpm_last_error(e._h)
        return img

    out = []
    for (name, C0, C1, Cout, k, H, W, coef, silu, up, res, sk) in SHAPES:
        h, w = (H // 2, W // 2) if up else (H, W)
        wexp = 16
        x0, x1 = rnd(B, h, w, C0), (rnd(B, h, w, C1) if C1 else None)
        cf = rnd(3, B, C0 + C1) if coef else None
        img = pack(Cout, C0 + C1, k, 2 if up else 0, wexp)
        skip, skimg = (rnd(B, H, W, sk), pack(Cout, sk, 1, 0, wexp)) if sk else (None, None)
        bias, r = rnd(Cout), (rnd(B, H, W, Cout) if res else None)
        y = torch.empty(B, H, W, Cout, device="cuda")
        run = lambda: lib.cddpm_op_conv_packed(e._h, p(x0), C0, p(x1), C1, p(cf), silu, up, p(img), wexp, p(bias), Cout, k, p(r), 0,
                                               p(skip), sk, None, 0, p(skimg), p(y), None, B, H, W, s)
        assert run() == 0, lib.cddpm_last_error(e._h)        # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / iters
        flops = 2.0 * B * H * W * Cout * ((C0 + C1) * k * k + sk)        # nominal: the folded upsample multiplies 4/9 of it
        out.append({"shape": name, "ms": ms, "tflops": flops / ms / 1e9})
    e.close()
    print(json.dumps(out))


def main():
    if sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
        return
    assert sys.argv[1] == "--run", __doc__
    B = int(os.environ.get("AB_BATCH", "64"))
    rounds = int(os.environ.get("AB_ROUNDS", "2"))
    res = {}
    for _ in range(rounds):          # interleaved rounds
        for tag in sys.argv[2:]:
            lib, _, opt = tag.partition("+")
            env = dict(os.environ, CDDPM_LIB=os.path.join(CSRC, "libcddpm_hip.so" if lib == "prod" else f"libcddpm_hip_{lib}.so"))
            if opt:
                env["CDDPM_NB2"] = {"nb1": "0", "nb2": "force"}[opt]
            o = subprocess.run([sys.executable, __file__, "--child", str(B), "5"], env=env, capture_output=True, text=True)
            if o.returncode != 0:          # stop: nothing more is started on a device a child may have left faulted
                sys.exit(f"{tag} FAILED (exit {o.returncode}):\n{o.stderr[-2000:]}")
            res.setdefault(tag, []).append(json.loads(o.stdout.strip().splitlines()[-1]))
    for i, shp in enumerate(SHAPES):
        print(shp[0])
        for tag, runs in res.items():
            ms = [r[i]["ms"] for r in runs]
            tf = [r[i]["tflops"] for r in runs]
            print(f"   {tag:10s} ms min {min(ms):8.3f} med {sorted(ms)[len(ms) // 2]:8.3f}  TF max {max(tf):6.1f}")


if __name__ == "__main__":
    main()
