"""GPU: precision-16 reconstruction (cddpm_set_precision, cddpm_op_attention_p16) -- plain fp16 operands in the convolutions and the
attention of a handle's forward / reverse calls, the arithmetic the reference evaluates with under `precision: 16`.

The truth is the float64 oracle; the yardstick is the REFERENCE under fp16 autocast (tests/golden/amp/, tools/make_golden_amp.py;
for the stand-alone attention operator: QKVAttention in torch fp16 on the CPU). Acceptance (precision16_cases.acceptance): rms error <=
1.0 x the yardstick's rms distance from float64, max error <= 2 x its max distance; and the switch must be real: rms error >= 10 x
the precision-32 result's on the same input. Every test prints its ratios before it asserts.

Measured on an MI355X (rms ratio / max ratio against the yardstick; switch = p16 rms error over p32 rms error):
    attention operator   (2,15,256) 0.60 / 0.63, 1974   (2,240,128) 0.58 / 0.59, 1063   (2,384,128) 0.58 / 0.48, 901   (1,1536,256) 0.57 / 0.45, 547
    unet forward         experiment 0.47 / 0.52 and 0.48 / 0.42 (t500, tmixed), 1567   attn_levels 0.47 / 0.47, 0.45 / 0.54, ~1400
                         deep4 0.44 / 0.43, 0.45 / 0.40, ~1380   cond4 0.51 / 0.51, 0.50 / 0.50, ~1600
    8-step chain         0.56 / 0.46, 1875          patched test_step 0.50 / 0.60, 1598
    forced 256-cout plan 0.47 / 0.52, 0.48 / 0.42 (the handle's own plan at 2 x 32 x 32, bit for bit: its Cout = 256 layers are split along K);
                         on a max_batch = 40 handle 0.49 / 0.46 forced against 0.47 / 0.46 unforced, different bits
    re-run slice         max 1.96e-7 rms 4.6e-8 against the fp32 oracle's 2.03e-7 / 6.0e-8
    validation_step      loss 0.53495288 at precision 16, 0.53493118 at 32
"""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import arch_cases as A
import precision16_cases as P
from conftest import ROOT, load_pkg
from attention_cases import attention as _attention, nlc as _nlc, reference
from test_gpu_conv_family import SCALE, explicit_noise, overflowing_batch

pytestmark = pytest.mark.gpu

SWITCH = 10.0         # a precision-16 result is at least this many times as far from float64 (rms) as the precision-32 one
# (B, N, C): N below one 64-key tile; N a multiple of neither the 128-query workgroup nor the key tile; two heads; four heads x 12 query tiles
# then the tile boundaries: one short of a tile and of a workgroup, exactly one and two tiles, one and two past each, N % 4 != 0 in a
# second tile (tests/test_attention_cases_host.py admits every one: none dropped)
ATTN_SHAPES = [(2, 15, 256), (2, 240, 128), (2, 384, 128), (1, 1536, 256),
               (1, 63, 64), (1, 64, 64), (1, 127, 64), (1, 128, 64), (1, 65, 64), (2, 67, 128), (1, 129, 128), (1, 130, 64)]
_reference = functools.partial(reference, "flat")


@pytest.fixture(scope="module")
def engines(synth):
    """engine(case, precision) at the case's own geometry (one handle per pair, shared by the tests of this module)"""
    E, sched = load_pkg("engine"), load_pkg("schedule")
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            c = P.case(name)
            B, H, W = c["geometry"]
            e = E.CddpmEngine(timesteps=1000, max_batch=B, max_h=H, max_w=W, precision=precision, **A.engine_kw(c))
            e.load_weights(synth.synth_state_dict(A.SEED_W, **A.synth_kw(c)))
            e.set_schedule(sched.schedule_buffers(1000), "pred_x0")
            made[(name, precision)] = e
        return made[(name, precision)]

    yield get
    for e in made.values():
        e.close()


def _dev(v):
    return None if v is None else v.cuda()


def _check(label, got, ref, got32=None):
    """acceptance against ref = dict(r64=, amp=) and, with the precision-32 result of the same input, the switch"""
    row = P.acceptance(got, ref)
    print(P.format_acceptance(label, row))
    assert row[-1], P.format_acceptance(label, row)
    if got32 is not None:
        e32 = P.rms(got32.detach().cpu().double() - ref["r64"])
        print(f"{label}: switch p16 rms {row[0]:.3e} / p32 rms {e32:.3e} = {row[0] / e32:.0f}")
        assert row[0] >= SWITCH * e32, (label, row[0], e32)


# ---------------------------------------------------------------------------------------------- 1. the attention operator
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_p16_operator(engines, shape):
    eng = engines("experiment", 32)                        # any handle serves the operators; this one stays at precision 32
    ref = _reference(shape)
    with torch.no_grad():
        a16 = _attention(ref["qkv"].half()).double()        # the yardstick: the same forward in torch fp16 on the CPU
    qkv = _nlc(ref["qkv"])
    got = eng.op_attention(qkv, precision=16).cpu().permute(0, 2, 1)
    got32 = eng.op_attention(qkv).cpu().permute(0, 2, 1)
    assert eng.precision == 32
    _check(f"attention p16 {shape}", got, dict(r64=ref["a64"], amp=a16), got32)
    assert torch.equal(eng.op_attention(qkv, precision="16-mixed").cpu().permute(0, 2, 1), got)      # deterministic, spelling-independent


# ---------------------------------------------------------------------------------------------- 2. the UNet forward
def _forward(eng, name, key):
    c = P.case(name)
    x, cond = A.inputs(load_pkg("synth"), c)
    return eng.unet_forward(_dev(x), A.timesteps(key, c["geometry"][0]).cuda(), _dev(cond))


@pytest.mark.parametrize("key", A.GOLDEN_T)
@pytest.mark.parametrize("name", list(P.FIXTURES))
def test_unet_forward_p16_vs_amp_reference(engines, name, key):
    e16 = engines(name, 16)
    assert (e16.precision, e16.conv_family) == (16, "h3")
    got = _forward(e16, name, key)
    e16.set_precision(32)
    try:
        got32 = _forward(e16, name, key)
    finally:
        e16.set_precision(16)
    _check(f"unet forward {name} {key}", got, P.forward_refs(name)[key], got32)


# ---------------------------------------------------------------------------------------------- 3. no state leaks
def test_precision_switch_leaves_no_state(engines):
    e16, e32 = engines("experiment", 16), engines("experiment", 32)
    first = _forward(e16, "experiment", "tmixed")
    plain = _forward(e32, "experiment", "tmixed")
    assert not torch.equal(first, plain)
    e16.set_precision(32)
    try:
        assert e16.precision == 32
        assert torch.equal(_forward(e16, "experiment", "tmixed"), plain)       # bit-identical to a handle that never left precision 32
    finally:
        e16.set_precision("16-mixed")
    assert e16.precision == 16
    assert torch.equal(_forward(e16, "experiment", "tmixed"), first)
    # the family of a precision-16 handle is h3; the exact families have no precision 16
    with pytest.raises(RuntimeError, match="precision 16"):
        e16.set_conv_family("x6")
    assert (e16.conv_family, e16.precision) == ("h3", 16)
    with pytest.raises(RuntimeError, match="must be 32 or 16"):
        e16._ck(e16.lib.cddpm_set_precision(e16._h, 8), "cddpm_set_precision")
    assert torch.equal(_forward(e16, "experiment", "tmixed"), first)           # refused calls change nothing
    x6 = load_pkg("engine").CddpmEngine(timesteps=50, max_batch=1, max_h=32, max_w=32, conv_family="x6")
    try:
        with pytest.raises(RuntimeError, match="needs the h3"):
            x6.set_precision(16)
        assert x6.precision == 32
    finally:
        x6.close()


# ---------------------------------------------------------------------------------------------- 4. the reverse loop
def test_reverse_chain_p16(engines):
    e16, e32 = engines("experiment", 16), engines("experiment", 32)
    x, cond, noise = (v.cuda() for v in P.chain_inputs())
    T = P.CHAIN["start_t"]
    got = e16.reverse(x, cond, T, noise=noise)
    _check("8-step chain", got, P.chain_refs(), e32.reverse(x, cond, T, noise=noise))
    # a slice's bits do not depend on the batch it is computed in
    for b in range(2):
        one = e16.reverse(x[b:b + 1], cond[b:b + 1].contiguous(), T, noise=noise[:, b:b + 1].contiguous())
        assert torch.equal(one, got[b:b + 1]), b
    # the same chain as two reverse_range segments
    y = x.clone()
    e16.prepare_cond(cond, 2)
    e16.reverse_range_(y, T - 1, 4, noise=noise)
    e16.reverse_range_(y, 3, 0, noise=noise)
    assert torch.equal(y, got)
    # the accumulation switch has no effect at precision 16
    e16.set_accumulation_switch(0)
    try:
        assert torch.equal(e16.reverse(x, cond, T, noise=noise), got)
    finally:
        e16.set_accumulation_switch(1 << 30)


def test_precision_change_rebuilds_the_captured_step_graph(engines, monkeypatch):
    """CDDPM_GRAPH=1 replays one captured step; cddpm_set_precision bumps the handle's generation, so a graph captured at one precision
    is never replayed at the other: in place on ONE buffer (the graph's key holds its address), 16 -> 32 -> 16"""
    e16, e32 = engines("experiment", 16), engines("experiment", 32)
    x, cond, noise = (v.cuda() for v in P.chain_inputs())
    T = P.CHAIN["start_t"]
    monkeypatch.setenv("CDDPM_GRAPH", "0")
    eager = {16: e16.reverse(x, cond, T, noise=noise), 32: e32.reverse(x, cond, T, noise=noise)}
    monkeypatch.setenv("CDDPM_GRAPH", "1")
    y = torch.empty_like(x)
    e16.prepare_cond(cond, 2)
    try:
        for bits in (16, 32, 16):
            e16.set_precision(bits)
            y.copy_(x)
            e16.reverse_range_(y, T - 1, 0, noise=noise)
            assert torch.equal(y, eager[bits]), bits
    finally:
        e16.set_precision(16)


# ---------------------------------------------------------------------------------------------- 5. the 256-cout plan
CHILD = r"""
import importlib, sys, numpy as np, torch
sys.path[:0] = [%(root)r, %(root)r + "/tests"]
import arch_cases as A, precision16_cases as P
PKG = "conditioned-diffusion-models-uad_amd"
synth = importlib.import_module(PKG + ".synth"); E = importlib.import_module(PKG + ".engine"); sched = importlib.import_module(PKG + ".schedule")
c = P.EXPERIMENT
B, H, W = c["geometry"]
e = E.CddpmEngine(timesteps=1000, max_batch=B, max_h=H, max_w=W, precision=16, **A.engine_kw(c))
e.load_weights(synth.synth_state_dict(A.SEED_W)); e.set_schedule(sched.schedule_buffers(1000), "pred_x0")
x, cond = A.inputs(synth, c)
x, cond = x.cuda(), cond.cuda()
out = {}
for key in A.GOLDEN_T:
    t = A.timesteps(key, B).cuda()
    out[key] = e.unet_forward(x, t, cond).cpu().numpy()
    out[key + "_split"] = torch.cat([e.unet_forward(x[b:b + 1], t[b:b + 1], cond[b:b + 1].contiguous()) for b in range(B)]).cpu().numpy()
e.close()
# the same descriptor on a max_batch = BIG handle: there the 3x3 convolutions of level 1 are not split along K, so the forced plan
# really multiplies them on 256-cout workgroups
big = E.CddpmEngine(timesteps=1000, max_batch=%(big)d, max_h=H, max_w=W, precision=16, **A.engine_kw(c))
big.load_weights(synth.synth_state_dict(A.SEED_W)); big.set_schedule(sched.schedule_buffers(1000), "pred_x0")
t = A.timesteps("tmixed", B).cuda()
out["big"] = big.unet_forward(x, t, cond).cpu().numpy()
out["big_split"] = torch.cat([big.unet_forward(x[b:b + 1], t[b:b + 1], cond[b:b + 1].contiguous()) for b in range(B)]).cpu().numpy()
big.close()
np.savez(sys.argv[1], **out)
"""
BIG = 40              # 40 x 2 x 2 = 160 workgroups of a 16 x 16 x 256 convolution: above the 128 below which plan_ksplit splits K


def test_forced_256_cout_plan_p16(engines, synth, tmp_path):
    """one fresh process under CDDPM_NB2=force (the 256-cout workgroups at the small test geometry, where the plan alone would not take
    them): the precision-16 forward still meets the AMP reference and a batch is still the concatenation of its slices"""
    out = str(tmp_path / "nb2.npz")
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, big=BIG), out], env=dict(os.environ, CDDPM_NB2="force"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    child = np.load(out)
    refs = P.forward_refs("experiment")
    for key in A.GOLDEN_T:
        got = torch.from_numpy(child[key])
        _check(f"forced 256-cout plan, unet forward {key}", got, refs[key])
        assert np.array_equal(child[key], child[key + "_split"]), key
    same = np.array_equal(child["tmixed"], _forward(engines("experiment", 16), "experiment", "tmixed").cpu().numpy())
    print("forced plan equals this process's plan bit for bit:", same)      # recorded: split-K layers never take the 256-cout form
    # on the max_batch = BIG handle the forced plan is another accumulation order than the handle's own plan at this geometry
    _check("forced 256-cout plan, max_batch 40, unet forward tmixed", torch.from_numpy(child["big"]), refs["tmixed"])
    assert np.array_equal(child["big"], child["big_split"])
    c = P.EXPERIMENT
    own = load_pkg("engine").CddpmEngine(timesteps=1000, max_batch=BIG, max_h=32, max_w=32, precision=16, **A.engine_kw(c))
    try:
        own.load_weights(synth.synth_state_dict(A.SEED_W))
        own.set_schedule(load_pkg("schedule").schedule_buffers(1000), "pred_x0")
        unforced = _forward(own, "experiment", "tmixed").cpu().numpy()
    finally:
        own.close()
    assert not np.array_equal(child["big"], unforced)            # i.e. the 256-cout kernels DID run in the child
    _check("own plan, max_batch 40, unet forward tmixed", torch.from_numpy(unforced), refs["tmixed"])


# ---------------------------------------------------------------------------------------------- 6. the range exit
def test_range_exit_p16_falls_back_per_slice(synth, oracle, sd_np, sd_torch):
    """the batch of tests/test_gpu_conv_family.py whose slice 2 drives a 1x1-skip stream to 8e4: at precision 16 that slice is
    non-finite exactly as in h3, the existing per-slice re-run on an x6 engine handles it, and the re-run slice meets that file's bound
    (max and rms <= 2 x the fp32 oracle's own distance from float64 on the same input)"""
    E, sched = load_pkg("engine"), load_pkg("schedule")
    T, H, W, steps = 50, 32, 32, 6
    made = []
    try:
        for kw in (dict(precision=16), dict(conv_family="x6")):
            e = E.CddpmEngine(timesteps=T, max_batch=4, max_h=H, max_w=W, **kw)
            made.append(e)
            e.load_weights(sd_np)
            e.set_schedule(sched.schedule_buffers(T), "pred_x0")
        p16, x6 = made
        x, cond = overflowing_batch(synth)
        noise = explicit_noise(synth, steps, 0, 4)
        with pytest.raises(FloatingPointError, match="CDDPM_CONV"):
            p16.reverse(x, cond, steps, noise=noise.cuda())
        assert p16.slice_status(p16.reverse_unchecked(x, cond, steps, noise=noise.cuda())).cpu().tolist() == [0, 0, 1, 0]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out = p16.reverse(x, cond, steps, noise=noise.cuda(), fallback=x6)
        assert len(rec) == 1 and issubclass(rec[0].category, RuntimeWarning), [str(w.message) for w in rec]
        assert "1 of 4 slices" in str(rec[0].message) and "x6" in str(rec[0].message)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out[2], x6.reverse(x, cond, steps, noise=noise.cuda())[2])          # the re-run slice is the exact family's
        keep = p16.reverse(x[[0, 1]], cond[[0, 1]].contiguous(), steps, noise=noise[:, 0:2].contiguous().cuda())
        assert torch.equal(out[0:2], keep)                                                    # the kept slices are precision 16's
        xs, cs = x[2:3].cpu(), cond[2:3].cpu()
        buf = oracle.schedule_buffers(T)
        with torch.no_grad():
            r32 = oracle.p_sample_loop(xs, cs, sd_torch, buf, lambda t: noise[t, 2:3], start_t=steps).double()
            r64 = oracle.p_sample_loop(xs.double(), cs.double(), oracle.to_float64(sd_torch), oracle.to_float64(buf),
                                       lambda t: noise[t, 2:3].double(), start_t=steps)
        assert bool(torch.isfinite(r32).all())
        d, y = out[2:3].cpu().double() - r64, r32 - r64
        print(f"re-run slice (x {SCALE:g}) vs float64: max {float(d.abs().max()):.3e} rms {P.rms(d):.3e}; fp32 oracle (yardstick) max "
              f"{float(y.abs().max()):.3e} rms {P.rms(y):.3e}")
        assert float(d.abs().max()) <= 2 * float(y.abs().max()) and P.rms(d) <= 2 * P.rms(y)
    finally:
        for e in made:
            e.close()


# ---------------------------------------------------------------------------------------------- 7. the mirrors
class _Enc(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1)[:, :128].contiguous()


def test_ddpm2d_eval_precision_key(synth, sd_np):
    M, E, sched = load_pkg("DDPM_2D"), load_pkg("engine"), load_pkg("schedule")
    B, H, W, T = 2, 32, 32, 1000
    base = dict(imageDim=[64, 64, 100], rescaleFactor=2, unet_dim=128, dim_mults=[1, 2, 2], condition=True, test_timesteps=500, timesteps=T)

    def module(**over):
        mod = M.DDPM_2D(dict(base, **over), encoder=_Enc())
        mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        return mod.cuda()

    m16, m32 = module(eval_precision=16), module()
    fresh = E.CddpmEngine(timesteps=T, max_batch=B, max_h=H, max_w=W, precision=16)
    try:
        inp = torch.from_numpy(synth.synth_slices(2, 0, B, H, W)).cuda()
        feats = torch.from_numpy(synth.synth_cond(1, 0, B)).cuda()
        noise = torch.from_numpy(synth.noise_z(3, 0, 0, B, H, W)).cuda()
        _loss, reco = m16.reconstruct(inp, features=feats, noise=noise)
        eng = m16.diffusion.model._hip.engine
        assert (eng.precision, eng.conv_family, eng.max_batch, eng.max_h, eng.max_w) == (16, "h3", B, H, W)
        assert m32.reconstruct(inp, features=feats, noise=noise) and m32.diffusion.model._hip.engine.precision == 32
        # the single step of reconstruct (t = test_timesteps - 1) on a stand-alone precision-16 engine of the same geometry
        fresh.load_weights(sd_np)
        fresh.set_schedule(sched.schedule_buffers(T), "pred_x0")
        t = torch.full((B,), 499, device="cuda", dtype=torch.long)
        x_t = m16.diffusion.q_sample(inp * 2 - 1, t, noise)
        assert torch.equal(reco, (fresh.unet_forward(x_t, t, feats) + 1) * 0.5)
        assert not torch.equal(reco, m32.reconstruct(inp, features=feats, noise=noise)[1])
        # validation_step: a finite loss; its distance from the precision-32 loss is recorded, not bounded
        batch = {"vol": {"data": inp.unsqueeze(-1)}}
        losses = []
        for mod in (m16, m32):
            torch.manual_seed(5)
            losses.append(float(mod.validation_step(batch, 0)["loss"]))
        print(f"validation_step loss: precision 16 {losses[0]:.8f}, precision 32 {losses[1]:.8f}, |difference| {abs(losses[0] - losses[1]):.3e}")
        assert np.isfinite(losses[0]) and np.isfinite(losses[1])
    finally:
        fresh.close()
        m16.diffusion.model._hip.close()
        m32.diffusion.model._hip.close()


def test_patched_mirror_test_step_at_eval_precision_16(synth):
    """DDPM_2D_patched.test_step (grid evaluation through p_losses_grid) at the smallest geometry of tests/golden/patched -- 3 slices of
    32 x 32, four 16 x 16 boxes -- against the float64 restatement of that test_step, with the reference's own test_step under
    autocast as the yardstick"""
    Pm = load_pkg("DDPM_2D_patched")
    c = P.PATCHED
    cfg = dict(imageDim=[96, 96, c["S"]], rescaleFactor=3, unet_dim=128, dim_mults=[1, 2, 2], patch_size=c["patch_size"], inpaint=True,
               objective="pred_x0", loss="l1", test_timesteps=c["t"] + 1, lr=1e-4)
    x01, noise = P.patched_inputs()
    vol = x01[:, 0].permute(1, 2, 0)[None, None].contiguous().cuda()
    results = {}
    for bits in (16, 32):
        mod = Pm.DDPM_2D(dict(cfg, eval_precision=bits))
        mod.diffusion.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(0, num_classes=None).items()}, strict=True)
        mod = mod.cuda()
        mod._gen_noise = lambda shape, device, engine=None: noise.cuda()           # the fixture's one field for every box
        try:
            out = mod.test_step({"vol": {"data": vol}}, 0)
            assert mod.diffusion.model._hip.engine.precision == bits
            results[bits] = out["final_volume"][0, 0].permute(2, 0, 1).unsqueeze(1).cpu()
        finally:
            mod.diffusion.model._hip.close()
    _check("patched test_step", results[16], P.patched_refs(), results[32])
