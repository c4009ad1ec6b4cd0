"""GPU parity of the UNet engine at descriptors other than the experiment's 128-channel (1, 2, 2) model (tests/arch_cases.py): wider
models (256 / 384 / 512 channels: the head's dynamic LDS above 64 KB, the input convolution at 96 channel quads, Cout 768 and 1024-wide
concatenations in the split-K plan), four levels, attention inside the levels, channel_mult[0] = 2, cond_dim 0 and 4.

Every block tap and the output are compared with the float64 oracle; the yardstick of a block is the fp32 oracle's own distance from
float64 on it (arch_cases.block_ratios). Each case runs on a handle of exactly its geometry (the small-batch split-K plan) and on a
max_batch 64 / 128 x 128 handle (the large-batch plan); on each, a batch equals the concatenation of its slices bit for bit."""
import ctypes
import re

import numpy as np
import pytest
import torch

import arch_cases as A
from conftest import load_pkg

pytestmark = pytest.mark.gpu
TOL = 1e-4
PLANS = {"own": None, "large": (64, 128, 128)}
_cache = {}


def weights(synth, name):
    if ("sd", name) not in _cache:
        _cache[("sd", name)] = synth.synth_state_dict(A.SEED_W, **A.synth_kw(A.CASES[name]))
    return _cache[("sd", name)]


def references(synth, oracle, name, key):
    """(x, cond, t, float64 taps + 'out', fp32 taps + 'out') of a case at one of the timestep vectors of arch_cases.GOLDEN_T"""
    if ("ref", name, key) not in _cache:
        case = A.CASES[name]
        x, cond = A.inputs(synth, case)
        t = A.timesteps(key, case["geometry"][0])
        sd32 = oracle.to_torch_sd(weights(synth, name))
        t32, t64 = {}, {}
        with torch.no_grad():
            t32["out"] = oracle.unet_forward(x, t, cond, sd32, taps=t32, **A.unet_kw(case))
            t64["out"] = oracle.unet_forward(x.double(), t, None if cond is None else cond.double(), oracle.to_float64(sd32), taps=t64,
                                             **A.unet_kw(case))
        _cache[("ref", name, key)] = (x, cond, t, t64, t32)
    return _cache[("ref", name, key)]


def make_engine(synth, name, plan="own", timesteps=1000, conv_family=None, objective="pred_x0"):
    case = A.CASES[name]
    mb, mh, mw = PLANS[plan] or case["geometry"]
    eng = load_pkg("engine").CddpmEngine(timesteps=timesteps, max_batch=mb, max_h=mh, max_w=mw, conv_family=conv_family, **A.engine_kw(case))
    eng.load_weights(weights(synth, name))
    eng.set_schedule(load_pkg("schedule").schedule_buffers(timesteps, "cosine"), objective)
    return eng


def dev(v):
    return None if v is None else v.cuda()


def check_blocks(eng, synth, oracle, name, label):
    """every block tap and the output against the float64 oracle under the yardstick rule, at a uniform and at a mixed t; -> worst ratio"""
    worst, failed = 0.0, []
    for key in A.GOLDEN_T:
        x, cond, t, ref64, ref32 = references(synth, oracle, name, key)
        got = eng.forward_with_taps(dev(x), 500 if key == "t500" else t, dev(cond))
        rows = A.block_ratios(got, ref64, ref32, eng.block_names())
        print(f"--- {name} [{label}] {key}\n{A.format_ratios(rows)}")
        worst = max([worst] + [e / max(y, 1e-30) for _n, e, y, _m, _ok in rows])
        failed += [(key,) + r for r in rows if not r[4]]
        out_err = float((got["out"].cpu().double() - ref64["out"]).abs().max())
        assert out_err < TOL, (name, label, key, out_err)
    # one line per case and plan / family in a fixed format: `pytest -s | grep '^RATIO'` is the table of DESIGN.md section 1
    print(f"\nRATIO | {name} | {label} | {worst:.2f} |")
    assert not failed, failed
    return worst


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", list(A.CASES))
def test_blocks_vs_float64_oracle_on_both_plans(synth, oracle, name, plan):
    case = A.CASES[name]
    B = case["geometry"][0]
    eng = make_engine(synth, name, plan)
    try:
        check_blocks(eng, synth, oracle, name, plan)
        # within one handle the bits of a slice never depend on the batch it is in
        x, cond, t, _r64, _r32 = references(synth, oracle, name, "tmixed")
        full = eng.unet_forward(dev(x), t, dev(cond))
        alone = torch.cat([eng.unet_forward(dev(x[i:i + 1]), t[i:i + 1], dev(None if cond is None else cond[i:i + 1])) for i in range(B)])
        assert torch.equal(full, alone), (name, plan, float((full - alone).abs().max()))
    finally:
        eng.close()


@pytest.mark.parametrize("family", ["x6", "f32"])
@pytest.mark.parametrize("name", ["w384_limit", "attn_levels"])
def test_blocks_vs_float64_oracle_in_the_exact_families(synth, oracle, name, family):
    eng = make_engine(synth, name, "own", conv_family=family)
    try:
        assert eng.conv_family == family
        check_blocks(eng, synth, oracle, name, family)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(A.CASES))
def test_bookkeeping(synth, oracle, name):
    """weight inventory, block shapes and the workspace size of every case"""
    case = A.CASES[name]
    B, H, W = case["geometry"]
    eng = make_engine(synth, name)
    try:
        shapes = synth.unet_param_shapes(**A.synth_kw(case))
        got = dict(eng.weight_names())
        assert set(got) == set(shapes) and len(eng.weight_names()) == len(shapes), set(got) ^ set(shapes)
        assert all(got[k] == int(np.prod(s)) for k, s in shapes.items())
        _x, _c, _t, ref64, _r32 = references(synth, oracle, name, "t500")
        names = eng.block_names()
        assert set(names) == set(ref64) - {"emb"}, set(names) ^ set(ref64)
        for i, n in enumerate(names):
            c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            assert eng.lib.cddpm_block_shape(eng._h, i, H, W, ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)) == 0
            assert (B, c.value, h.value, w.value) == tuple(ref64[n].shape), (n, c.value, h.value, w.value, tuple(ref64[n].shape))
        for plan in PLANS.values():
            d = load_pkg("_lib").UnetDesc.from_buffer_copy(eng.desc)
            d.max_batch, d.max_h, d.max_w = plan or case["geometry"]
            assert eng.lib.cddpm_workspace_bytes(ctypes.byref(d)) > 0, eng.lib.cddpm_last_error(None)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["w256", "attn_levels"])
def test_sampler_steps_vs_oracle(synth, oracle, name):
    """one p_sample at a large t and a 10-step reverse loop at T = 50 against the oracle's"""
    case = A.CASES[name]
    B, H, W = case["geometry"]
    x, cond = A.inputs(synth, case)
    sd = oracle.to_torch_sd(weights(synth, name))
    z = torch.from_numpy(synth.noise_z(3, 700, 0, B, H, W))
    with torch.no_grad():
        ref = oracle.p_sample(x, 700, cond, sd, oracle.schedule_buffers(1000), z, **A.unet_kw(case))
    eng = make_engine(synth, name, timesteps=1000)
    try:
        got = eng.p_sample(dev(x), 700, dev(cond), z=z.cuda()).cpu()
    finally:
        eng.close()
    err = float((got - ref).abs().max())
    print(f"{name}: p_sample t=700 max|delta| {err:.3e}")
    assert err < TOL
    T, steps = 50, 10
    zs = {s: torch.from_numpy(synth.noise_z(3, s, 0, B, H, W)) for s in range(1, steps)}
    loop_ref = oracle.p_sample_loop(x, cond, sd, oracle.schedule_buffers(T), lambda s: zs[s], start_t=steps, **A.unet_kw(case)).numpy()
    noise = torch.zeros(steps, B, 1, H, W)
    for s, v in zs.items():
        noise[s] = v
    eng = make_engine(synth, name, timesteps=T)
    try:
        out = eng.reverse(dev(x), dev(cond), steps, noise=noise.cuda()).cpu().numpy()
    finally:
        eng.close()
    err = float(np.abs(out - loop_ref).max())
    print(f"{name}: {steps}-step reverse loop at T={T} max|delta| {err:.3e}")
    assert out.min() >= 0.0 and out.max() <= 1.0 and err < TOL


def test_reverse_graph_replay_equals_eager_with_level_attention(synth, monkeypatch):
    """tests/test_gpu_unet.py::test_reverse_graph_replay_equals_eager on `attn_levels`: the captured step has an attention (GroupNorm
    finalize, qkv, attention core, projection) in every block, so the graph has many more nodes; the bits stay those of the eager loop"""
    case = A.CASES["attn_levels"]
    B, H, W = case["geometry"]
    steps = 12
    x, cond = A.inputs(synth, case)
    noise = np.zeros((steps, B, 1, H, W), np.float32)
    for t in range(1, steps):
        noise[t] = synth.noise_z(3, t, 0, B, H, W)
    nz = torch.from_numpy(noise).cuda()
    eng = make_engine(synth, "attn_levels", timesteps=50)
    try:
        for kw in (dict(noise=nz), dict(noise=None, seed=11, slice0=5)):
            monkeypatch.setenv("CDDPM_GRAPH", "0")
            eager = eng.reverse(x.cuda(), cond.cuda(), steps, **kw)
            monkeypatch.setenv("CDDPM_GRAPH", "1")
            replay = eng.reverse(x.cuda(), cond.cuda(), steps, **kw)
            again = eng.reverse(x.cuda(), cond.cuda(), steps, **kw)
            assert torch.equal(eager, replay) and torch.equal(eager, again)
            assert float(eager.min()) >= 0.0 and float(eager.max()) <= 1.0 and float(eager.std()) > 0.01
    finally:
        eng.close()


def test_refused_descriptors_fail_create_with_their_reason(synth):
    """every descriptor of arch_cases.REFUSALS fails cddpm_create with a message naming the limit; nothing half-built is left behind:
    a valid cddpm_create in the same process works afterwards and computes"""
    E = load_pkg("engine")
    for rname, r in A.REFUSALS.items():
        kw = dict(A.REFUSAL_BASE, **r["desc"])
        with pytest.raises(RuntimeError, match=re.escape(r["message"])):
            E.CddpmEngine(timesteps=1000, **kw)
        print("refused:", rname)
    case = A.CASES["cond4"]
    eng = make_engine(synth, "cond4")
    try:
        x, cond = A.inputs(synth, case)
        out = eng.unet_forward(x.cuda(), 500, cond.cuda())
        assert bool(torch.isfinite(out).all()) and float(out.std()) > 0.01
    finally:
        eng.close()
