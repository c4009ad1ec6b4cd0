"""What the per-call tests of the context encoder's training step share (tests/test_gpu_encoder_training_p16.py,
test_gpu_encoder_training_calls.py): an EncoderTrainer whose convolution, BatchNorm and shortcut-add calls are recorded with their inputs
and outputs at their real shapes, and the check of every recorded call on its own against float64 arithmetic on its own inputs. No
end-to-end tolerance means much for this network: training-mode BatchNorm over as few as 16 samples per channel amplifies whatever one
operator adds. The convolution check takes the rounding of the operands as a parameter: fp16 at precision 16, none at precision 32."""
import torch
import torch.nn.functional as F

import encoder_op_cases as EC
from conftest import load_pkg

LIMIT = 5e-6                 # fp32 accumulation, relative to the result's maximum (tests/test_gpu_encoder_ops.py)
BN_LIMIT = 2e-5              # tests/test_gpu_encoder_ops.py


def rounded(t):
    return t.float().half().double().cpu()


def unrounded(t):
    return t.double().cpu()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def build(synth, B, H, W, **kw):
    tr, et = load_pkg("training"), load_pkg("encoder_training")
    ops = tr.UNetTrainer({"w": torch.zeros(64)}, device=torch.device("cuda", 0))
    ops._fit(B, H, W)
    ops.overlap_wgrad = False
    return et.EncoderTrainer({k: torch.from_numpy(v) for k, v in synth.synth_encoder_state_dict(0).items()}, ops, **kw)


def record(enc):
    """wraps enc.conv and enc.wgrad (the only two places convolutions are issued): each call's inputs and output are kept"""
    calls = []
    conv0, wgrad0 = enc.conv, enc.wgrad

    def conv(name, x, transposed=False, in_hw=None):
        out = conv0(name, x, transposed=transposed, in_hw=in_hw)
        calls.append(("dx" if transposed else "y", name, x.clone(), enc.p[name + ".weight"].clone(), in_hw, out.clone()))
        return out

    def wgrad(name, x, dz):
        wgrad0(name, x, dz)
        calls.append(("dw", name, x.clone(), dz.clone(), None, enc.g[name + ".weight"].clone()))

    enc.conv, enc.wgrad = conv, wgrad
    return calls


def check(enc, calls, rounding=rounded, limit=LIMIT):
    """every recorded call against float64 on its own inputs as `rounding` makes them -> {role: (count, worst error)}"""
    torch.cuda.synchronize()
    seen = {}
    for role, name, a, b, in_hw, out in calls:
        co, ci, k, st = enc.convs[name]
        if role == "y":
            ref = F.conv2d(nchw(rounding(a)), rounding(b), None, stride=st, padding=k // 2)
            got = nchw(out.double().cpu())
        elif role == "dx":
            ref = torch.nn.grad.conv2d_input((a.shape[0], ci, in_hw[0], in_hw[1]), rounding(b), nchw(rounding(a)), stride=st, padding=k // 2)
            got = nchw(out.double().cpu())
        else:
            ref = torch.nn.grad.conv2d_weight(nchw(rounding(a)), (co, ci, k, k), nchw(rounding(b)), stride=st, padding=k // 2)
            got = out.double().cpu()
        assert got.shape == ref.shape, (role, name)
        assert torch.isfinite(got).all(), (role, name)
        e = float((got - ref).abs().max() / (ref.abs().max() + 1e-300))
        assert e < limit, (role, name, e)
        n, worst = seen.get(role, (0, 0.0))
        seen[role] = (n + 1, max(worst, e))
    return seen


def record_bn(enc):
    """wraps enc.bn, enc.bn_bwd and the trainer's add_ (the shortcut's gradient joins through it) -> (forward records, backward records,
    {"add": the destination of the last add_}). The running statistics are cloned before and after each forward call (the operator updates
    them in place); everything else a call reads or writes is a tensor of its own that the step leaves alone afterwards."""
    fwd, bwd, last = [], [], {}
    bn0, bn_bwd0, add0 = enc.bn, enc.bn_bwd, enc.ops.add_
    stats = lambda name: (enc.buf[name + ".running_mean"].clone(), enc.buf[name + ".running_var"].clone())

    def bn(name, z, relu, res=None, sscale=None):
        rm0, rv0 = stats(name)
        y, mr = bn0(name, z, relu, res=res, sscale=sscale)
        rm1, rv1 = stats(name)
        fwd.append(dict(name=name, z=z, relu=relu, res=res, ss=sscale, rm0=rm0, rv0=rv0, rm1=rm1, rv1=rv1, y=y, mr=mr))
        return y, mr

    def bn_bwd(name, z, y, dy, mr, relu, sscale=None, want_dres=False):
        dz, dres = bn_bwd0(name, z, y, dy, mr, relu, sscale, want_dres=want_dres)
        bwd.append(dict(name=name, z=z, y=y, dy=dy, relu=relu, ss=sscale, dz=dz, dres=dres, dgamma=enc.g[name + ".weight"].clone(),
                        dbeta=enc.g[name + ".bias"].clone()))
        return dz, dres

    def add_(a, b):
        r = add0(a, b)
        last["add"] = a
        return r

    enc.bn, enc.bn_bwd, enc.ops.add_ = bn, bn_bwd, add_
    return fwd, bwd, last


def check_bn(enc, fwd, bwd, limit=BN_LIMIT):
    """every recorded BatchNorm call against float64 on its own inputs with its own ReLU mask
    -> {"bn " + quantity: (count, worst error relative to the quantity's maximum)}"""
    torch.cuda.synchronize()
    seen = {}
    host = lambda t: None if t is None else t.double().cpu()
    img = lambda t: None if t is None else nchw(t.double().cpu())

    def note(key, name, got, ref):
        assert got.shape == ref.shape and torch.isfinite(got).all(), (key, name)
        e = EC.rel(got, ref)
        assert e < limit, (key, name, e)
        n, worst = seen.get(key, (0, 0.0))
        seen[key] = (n + 1, max(worst, e))

    for r in fwd:
        name, y = r["name"], img(r["y"])
        ref = EC.bn_reference(img(r["z"]), host(enc.p[name + ".weight"]), host(enc.p[name + ".bias"]), None, r["relu"], mask=y > 0, res=img(r["res"]),
                              ss=host(r["ss"]), run_mean=host(r["rm0"]), run_var=host(r["rv0"]))
        mr = host(r["mr"])
        for key, got in (("y", y), ("mean", mr[0]), ("rstd", mr[1]), ("run_mean", host(r["rm1"])), ("run_var", host(r["rv1"]))):
            note("bn " + key, name, got, ref[key])
    for r in bwd:
        name = r["name"]
        mask = img(r["y"]) > 0 if r["relu"] else None
        ref = EC.bn_reference(img(r["z"]), host(enc.p[name + ".weight"]), host(enc.p[name + ".bias"]), img(r["dy"]), r["relu"], mask=mask, ss=host(r["ss"]))
        for key, got in (("dz", img(r["dz"])), ("dres", img(r["dres"])), ("dgamma", host(r["dgamma"])), ("dbeta", host(r["dbeta"]))):
            if got is not None:
                note("bn " + key, name, got, ref[key])
    return seen
