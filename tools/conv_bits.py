#!/usr/bin/env python3
"""md5 of the fused convolution's output bytes on fixed inputs, per library build (CDDPM_LIB): two builds that claim the same arithmetic
in the same order must print the same digests.

    CDDPM_LIB=<so> python tools/conv_bits.py [--set fragments|epilogue] [--mode default|nb2|p16|p16nb2|x6|all] [--json FILE] [--parent COMMIT]

Inputs come from numpy.random.default_rng(SEED) on the host (one generator per case, keyed by the case's position) and are copied to the
device: no device generator is involved. The cases are the smallest shapes at which the wave -> pixel mapping of the 16 x 16 form can go
wrong (csrc/conv_x6.hip: column fragments): one full tile, ragged rows and a partial / narrow last column tile, two sources with two cout
blocks, the identity affine, the folded upsample's patch and parity classes, the 1x1 skip segment, the statistics records (digest of the
coefficients that op_conv_gn returns), and three larger layers. Modes:
    default  a precision-32 handle
    nb2      the same under CDDPM_NB2=force (256-cout workgroups wherever the kernel can; the switch is read once per process, so this
             mode wants a process of its own: `all` starts one)
    p16      a precision-16 handle: the operators again (the operator entry points do not take the handle's precision: their
             digests are those of `default`) and a small UNet forward (plain-fp16 convolutions: the hi-only kernels)
    p16nb2   the set's 256-cout cases (P16NB2_CASES) launched as a precision-16 handle PLANS them (op_conv_planned: hi-only operands
             from the handle's precision, as in a forward) under CDDPM_NB2=force, on a handle whose maximum geometry (4 x 64 x 128)
             leaves K unsplit: the hi-only 256-cout kernels <9,2,true,2> and <4,2,true,2>, which no other mode reaches. The mode
             asserts the plan it was given (S = 1, nb2). Fragments set only; not part of `all`;
             tests/golden/conv_bits_p16nb2_parent.json
`default` and `p16` also digest that UNet forward. --json writes {parent, seed, cases, modes: {mode: {case: md5}}} (tests/golden/
conv_bits_parent.json is this file, written once with CDDPM_LIB set to a build of the parent commit).

--set epilogue: the shapes at which the epilogue's two paths occur (csrc/conv_x6.hip: a workgroup whose 8 x 32 tile lies inside the image
stores without per-lane predicates, a ragged one keeps them) -- EPILOGUE_SHAPES x EPILOGUE_OPS below, B = 2, 128 channels: 3x3 with and
without residual, the statistics records, the folded upsample with a half-resolution residual, 1x1, a 256-cout layer (256-cout workgroups
in mode nb2) and the layer as a small handle plans it (split-K: plane stores and the combine). Mode x6: an exact-bf16-family handle.
tests/golden/conv_bits_epilogue_parent.json is that output for the commit before the full-tile path."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "conditioned-diffusion-models-uad_amd"
SEED = 20261021
MODES = ("default", "nb2", "p16")
EPILOGUE_MODES = MODES + ("x6",)
NB2_MODES = ("nb2", "p16nb2")      # run under CDDPM_NB2=force

# name: (op, B, C0, C1, Cout, H, W of the SOURCE, coef, silu, res, skipC)     op: conv | up2 (folded upsample, output 2H x 2W, res_upsample)
CASES = {
    "conv 128>128 8x32": ("conv", 2, 128, 0, 128, 8, 32, 1, 1, 0, 0),
    "conv 128>128 12x40": ("conv", 2, 128, 0, 128, 12, 40, 1, 1, 0, 0),
    "conv 128>128 24x24": ("conv", 2, 128, 0, 128, 24, 24, 1, 1, 0, 0),
    "cat 256+128>256 16x40 +res": ("conv", 2, 256, 128, 256, 16, 40, 1, 1, 1, 0),
    "conv 256>128 24x24 nocoef": ("conv", 3, 256, 0, 128, 24, 24, 0, 0, 0, 0),
    "up2 256>256 9x13 +res_up": ("up2", 2, 256, 0, 256, 9, 13, 1, 1, 1, 0),
    "up2 256>256 8x16 +res_up": ("up2", 2, 256, 0, 256, 8, 16, 1, 1, 1, 0),
    "skip 128>128 +384 16x32": ("skip", 2, 128, 0, 128, 16, 32, 1, 1, 0, 384),
    "gn 128>128 12x40": ("gn", 2, 128, 0, 128, 12, 40, 0, 0, 0, 0),
    "conv 128>128 64x64": ("conv", 3, 128, 0, 128, 64, 64, 1, 1, 0, 0),
    "cat 256+128>256 32x40 +res": ("conv", 3, 256, 128, 256, 32, 40, 1, 1, 1, 0),
}
P16NB2_CASES = ("cat 256+128>256 16x40 +res", "up2 256>256 9x13 +res_up", "up2 256>256 8x16 +res_up")      # mode p16nb2: the 256-cout cases above
# epilogue set: H x W of the OUTPUT grid the tiles cover (the folded case's source; its output is 2H x 2W)
EPILOGUE_SHAPES = {"8x32": (8, 32), "16x40": (16, 40), "12x20": (12, 20), "16x64": (16, 64)}
# op: (kind, Cout, res)      kind: conv | gn | up2 | 1x1 | planned (a handle of max_batch 2 at the layer's own size: K is split)
EPILOGUE_OPS = {"3x3": ("conv", 128, 0), "3x3 +res": ("conv", 128, 1), "3x3 gn": ("gn", 128, 0), "up2 +res_up": ("up2", 128, 1),
                "1x1 +res": ("1x1", 128, 1), "3x3 >256 +res": ("conv", 256, 1), "planned +res": ("planned", 128, 1)}
UNET = dict(model_channels=128, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(3, 6, 12))      # + geometry (2, 16, 24), t = (123, 877)


def md5(t):
    return hashlib.md5(t.detach().cpu().numpy().tobytes()).hexdigest()


def run_case(e, index, spec, planned=False):
    """{suffix: md5} of one case on engine e. planned (conv / up2 cases): through op_conv_planned, the layer being the handle's whole
    image -- the handle's precision and plan apply; the plan taken must be one unsplit launch of 256-cout workgroups"""
    op, B, C0, C1, Cout, H, W, coef, silu, res, sk = spec
    rng = np.random.default_rng([SEED, index])
    n = lambda *shape, scale=1.0: torch.from_numpy((rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)))
    Cin = C0 + C1
    x0 = n(B, H, W, C0).cuda()
    x1 = n(B, H, W, C1).cuda() if C1 else None
    cf = torch.stack([n(B, Cin, scale=0.2), 1 + n(B, Cin, scale=0.2), n(B, Cin, scale=0.2)]).contiguous().cuda() if coef else None
    w = n(Cout, Cin, 3, 3, scale=1.0 / (Cin * 9) ** 0.5)
    bias = n(Cout, scale=0.1)
    if op in ("conv", "up2"):
        r = n(B, H, W, Cout).cuda() if res else None
        up, src1 = (2, None) if op == "up2" else (0, x1)
        if not planned:
            return {"": md5(e.op_conv(x0, src1, cf, silu, up, w, bias, r, bool(res) and op == "up2", 3))}
        out, _, plan = e.op_conv_planned(x0, src1, cf, silu, up, w, bias, r, bool(res) and op == "up2", 3,
                                         img_hw=(2 * H, 2 * W) if up else (H, W))
        assert plan["S"] == 1 and plan["nb2"], f"expected one unsplit launch of 256-cout workgroups, got {plan}"
        return {"": md5(out)}
    assert not planned, op
    if op == "skip":
        skip, wskip = n(B, H, W, sk).cuda(), n(Cout, sk, 1, 1, scale=1.0 / sk ** 0.5)
        return {"": md5(e.op_conv_skip(x0, cf, silu, w, bias, skip, wskip))}
    out, co = e.op_conv_gn(x0, w, bias, 1 + n(Cout, scale=0.1), n(Cout, scale=0.1))
    return {"": md5(out), " coef": md5(co)}


def run_epilogue_case(E, e, index, shape, op, mode):
    """{suffix: md5} of one (shape, op) of the epilogue set on engine e"""
    kind, Cout, res = op
    H, W = shape
    B, Cin = 2, 128
    rng = np.random.default_rng([SEED, 100 + index])
    n = lambda *shp, scale=1.0: torch.from_numpy((rng.standard_normal(shp, dtype=np.float32) * np.float32(scale)))
    k = 1 if kind == "1x1" else 3
    x0 = n(B, H, W, Cin).cuda()
    cf = torch.stack([n(B, Cin, scale=0.2), 1 + n(B, Cin, scale=0.2), n(B, Cin, scale=0.2)]).contiguous().cuda()
    w = n(Cout, Cin, k, k, scale=1.0 / (Cin * k * k) ** 0.5)
    bias = n(Cout, scale=0.1)
    r = n(B, H, W, Cout).cuda() if res else None
    if kind in ("conv", "1x1"):
        return {"": md5(e.op_conv(x0, None, cf, 1, 0, w, bias, r, False, k))}
    if kind == "up2":
        return {"": md5(e.op_conv(x0, None, cf, 1, 2, w, bias, r, True, 3))}
    if kind == "gn":
        out, co = e.op_conv_gn(x0, w, bias, 1 + n(Cout, scale=0.1), n(Cout, scale=0.1))
        return {"": md5(out), " coef": md5(co)}
    small = E.CddpmEngine(timesteps=10, max_batch=B, max_h=H, max_w=W, precision=16 if mode == "p16" else None,
                          **({"conv_family": "x6"} if mode == "x6" else {}))
    try:
        out, co, plan = small.op_conv_planned(x0, None, cf, 1, 0, w, bias, r, False, 3, img_hw=(H, W), gamma=1 + n(Cout, scale=0.1),
                                              beta=n(Cout, scale=0.1))
        return {f" S{plan['S']}": md5(out), f" S{plan['S']} coef": md5(co)}
    finally:
        small.close()


def epilogue_digests(mode):
    """{case: md5} of the epilogue set in one mode, in this process"""
    assert mode in EPILOGUE_MODES, mode
    assert (os.environ.get("CDDPM_NB2") == "force") == (mode == "nb2"), "nb2 <=> CDDPM_NB2=force, per process"
    E = importlib.import_module(PKG + ".engine")
    e = E.CddpmEngine(timesteps=10, max_batch=4, max_h=64, max_w=128, precision=16 if mode == "p16" else None,
                      **({"conv_family": "x6"} if mode == "x6" else {}))
    out = {}
    try:
        index = 0
        for sname, shape in EPILOGUE_SHAPES.items():
            for oname, op in EPILOGUE_OPS.items():
                for suffix, d in run_epilogue_case(E, e, index, shape, op, mode).items():
                    out[f"{oname} {sname}{suffix}"] = d
                index += 1
    finally:
        e.close()
    return out


def unet_digest(E, precision):
    synth = importlib.import_module(PKG + ".synth")
    B, H, W = 2, 16, 24
    e = E.CddpmEngine(timesteps=1000, max_batch=B, max_h=H, max_w=W, precision=precision, cond_dim=128, **UNET)
    try:
        e.load_weights(synth.synth_state_dict(3, num_classes=128, **UNET))
        e.set_schedule(importlib.import_module(PKG + ".schedule").schedule_buffers(1000), "pred_x0")
        rng = np.random.default_rng([SEED, 1000])
        x = torch.from_numpy(rng.standard_normal((B, 1, H, W), dtype=np.float32)).cuda()
        cond = torch.from_numpy(rng.standard_normal((B, 128), dtype=np.float32)).cuda()
        return md5(e.unet_forward(x, torch.tensor([123, 877], dtype=torch.long).cuda(), cond))
    finally:
        e.close()


def digests(mode):
    """{case: md5} of one mode, in this process (nb2: the caller has set CDDPM_NB2=force before the library's first convolution)"""
    assert mode in MODES + ("p16nb2",), mode
    assert (os.environ.get("CDDPM_NB2") == "force") == (mode in NB2_MODES), "nb2, p16nb2 <=> CDDPM_NB2=force, per process"
    E = importlib.import_module(PKG + ".engine")
    # (p16nb2: 4 x 64 x 128 is the smallest maximum geometry at which a 256-cout layer fills the chip unsplit: 256 workgroups of the 128-cout form)
    e = E.CddpmEngine(timesteps=10, max_batch=4, max_h=64, max_w=128 if mode == "p16nb2" else 64, precision=16 if mode in ("p16", "p16nb2") else None)
    out = {}
    try:
        for index, (name, spec) in enumerate(CASES.items()):      # (a case keeps its position: it keys the case's generator)
            if mode == "p16nb2" and name not in P16NB2_CASES:
                continue
            for suffix, d in run_case(e, index, spec, planned=(mode == "p16nb2")).items():
                out[name + suffix] = d
    finally:
        e.close()
    if mode not in NB2_MODES:
        out["unet forward 2x16x24"] = unet_digest(E, 16 if mode == "p16" else 32)
    return out


def digests_in_child(mode, which="fragments"):
    """the same in a process of its own (what a mode that is read once per process needs)"""
    env = dict(os.environ)
    env.pop("CDDPM_NB2", None)
    if mode in NB2_MODES:
        env["CDDPM_NB2"] = "force"
    o = subprocess.run([sys.executable, os.path.abspath(__file__), "--set", which, "--mode", mode, "--json", "-"], env=env, capture_output=True,
                       text=True, timeout=600)
    if o.returncode != 0:
        raise RuntimeError(f"conv_bits --mode {mode} failed (exit {o.returncode}):\n{o.stdout[-2000:]}\n{o.stderr[-2000:]}")
    return json.loads(o.stdout.strip().splitlines()[-1])["modes"][mode]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--set", default="fragments", choices=("fragments", "epilogue"), dest="which")
    ap.add_argument("--mode", default="default", choices=EPILOGUE_MODES + ("p16nb2", "all"))
    ap.add_argument("--json", default=None, help="write the digests to this file ('-': one line on stdout)")
    ap.add_argument("--parent", default=None, help="commit hash to record (the build CDDPM_LIB points at)")
    a = ap.parse_args()
    epi = a.which == "epilogue"
    assert not (epi and a.mode == "p16nb2"), "p16nb2 is a mode of the fragments set"
    if a.mode == "all":
        modes = {}
        for m in (EPILOGUE_MODES if epi else MODES):      # one process each; stop at the first that fails: nothing more is started on a device a child may have left faulted
            modes[m] = digests_in_child(m, a.which)
    else:
        modes = {a.mode: epilogue_digests(a.mode) if epi else digests(a.mode)}
    rec = {"parent": a.parent, "seed": SEED, "lib": os.path.basename(os.environ.get("CDDPM_LIB", "libcddpm_hip.so"))}
    if epi:
        rec.update(shapes={k: list(v) for k, v in EPILOGUE_SHAPES.items()}, ops={k: list(v) for k, v in EPILOGUE_OPS.items()}, modes=modes)
    else:
        rec.update(cases={k: list(v) for k, v in CASES.items() if a.mode != "p16nb2" or k in P16NB2_CASES}, unet={k: list(v) if isinstance(v, tuple) else v for k, v in UNET.items()},
                   modes=modes)
    if a.json == "-":
        print(json.dumps(rec))
        return
    for m, d in modes.items():
        for name, v in d.items():
            print(f"{m:8s} {name:32s} {v}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
