"""Training of the context encoder on the HIP operators (SURVEY.md section 8 rows f2 + f4): timm's ResNet-50 (in_chans = 1,
num_classes = cond_dim; reference src/models/modules/DDPM_encoder.py:21-23, wrapped by SparK_2D_encoder with drop_path_rate 0.05,
spark/models.py:89-109) in TRAINING mode -- BatchNorm on batch statistics with running-statistics updates, optional stochastic depth --
forward with saved activations and the backward of every operator, what `loss.backward()` does to `self.encoder` in the reference's
training_step (src/models/DDPM_2D.py:114-135; Adam over self.parameters(), :305-306).

Same construction as training.UNetTrainer: Python sequencing C-ABI operators (include/cddpm.h, "training-mode operators of the context
encoder"; csrc/encoder_train.hip, csrc/encoder_train_p16.hip, csrc/batchnorm_train.hip), one flat fp32 parameter buffer / gradient buffer / Adam state, weight images re-packed on the device
after every update. The operators run on the UNet trainer's handles; what they take from its arenas is a function of the geometry
(operator_scratch_bytes), which that trainer sizes its arenas for.

Arithmetic of the convolutions (all but the 7x7 stem): `EncoderTrainer(..., precision=32)` (default) runs the fp32 FMA kernels;
`precision=16` (the spellings of engine.precision_bits; the mirrors' `cfg.train_encoder_precision`) runs forward, input gradient and
weight gradient on plain fp16 operands with fp32 accumulation (cddpm_op_enc_*_p16), what the reference's `precision: 16` autocast computes
for self.encoder. BatchNorm, ReLU, pooling, fc, Adam and the master weights are fp32 in both. Measured: DESIGN.md section 4b. Parity: unpinned like the encoder's forward (timm is not in the image): checked against float64 autograd through
oracle/encoder_oracle.py's restatement (tests/test_gpu_encoder_training.py)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import optimizer as _optimizer
from ._lib import largest_calls
from .engine import _stream_ptr, precision_bits

STAGES = ((64, 3), (128, 4), (256, 6), (512, 3))
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def spark_bn_forward(t, name, z, act, active=None, f=1, *, res=None, sscale=None, fill=None, training=True):
    """cddpm_op_spark_bn_forward on parameter group `name` of trainer t (the owner of p, buf and the handle): sparse (active uint8
    [B,f,f]) or dense BatchNorm of z [B,H,W,C], act 0 | 1 (ReLU) | 2 (ReLU6) -> y, (mean | rstd)"""
    B, H, W, Cc = z.shape
    mr, y = t._new(2, Cc), torch.empty_like(z)
    t._ck(t.lib.cddpm_op_spark_bn_forward(t.h, _p(z), _p(t.p[name + ".weight"]), _p(t.p[name + ".bias"]), _p(sscale), _p(res), int(act),
                                          C.c_float(BN_EPS), C.c_float(BN_MOMENTUM), _p(t.buf[name + ".running_mean"]),
                                          _p(t.buf[name + ".running_var"]), _p(mr), _p(y), B * H * W, H * W, Cc, _p(active), f, H, W, _p(fill),
                                          int(training), t._s()), "op_spark_bn_forward")
    return y, mr


def spark_bn_backward(t, name, z, y, dy, mr, act, active=None, f=1, *, sscale=None, want_dres=False, dfill=None, training=True):
    """cddpm_op_spark_bn_backward of spark_bn_forward (training as there) -> dz, dres (None unless wanted); dgamma, dbeta land in t.g"""
    B, H, W, Cc = z.shape
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_dres else None
    t._ck(t.lib.cddpm_op_spark_bn_backward(t.h, _p(z), _p(y), _p(dy), _p(mr), _p(t.p[name + ".weight"]), _p(sscale), int(act), _p(dz), _p(dres),
                                           _p(t.g[name + ".weight"]), _p(t.g[name + ".bias"]), B * H * W, H * W, Cc, _p(active), f, H, W,
                                           _p(dfill), int(training), t._s()), "op_spark_bn_backward")
    return dz, dres


def plain_bn(relu, active, fill, training):
    """the one rule of EncoderTrainer.bn and bn_bwd: a BatchNorm without a mask, a fill value (forward) or its gradient (backward), ReLU6
    or evaluation mode is the dense ResNet-50's and goes through cddpm_op_enc_bn_*; every other goes through cddpm_op_spark_bn_*"""
    return active is None and fill is None and training and int(relu) != 2


def operator_calls(B, H, W, cond_dim=128):
    """the operator calls of the ResNet-50's training step (EncoderTrainer.forward / backward) on a [B, 1, H, W] batch that take
    temporaries from an arena, as (operator, arguments of its size query cddpm_op_<operator>_scratch, include/cddpm.h). The network
    is fixed, so they are a function of the geometry. Every convolution is listed in both arithmetics (enc_conv / enc_conv_p16, ...): an
    arena sized over these calls serves an EncoderTrainer of either precision."""
    def bn(c, h, w):
        yield "enc_bn_forward", (B * h * w, h * w, c)
        yield "enc_bn_backward", (B * h * w, h * w, c)

    yield "enc_stem_wgrad", (B, H, W)
    h, w = (H + 1) // 2, (W + 1) // 2              # the stem's stride
    yield from bn(64, h, w)
    h, w = (h + 1) // 2, (w + 1) // 2              # the max pool's
    cin = 64
    for s, (planes, nblocks) in enumerate(STAGES):
        for i in range(nblocks):
            st = 2 if (i == 0 and s > 0) else 1
            ho, wo = (h + st - 1) // st, (w + st - 1) // st
            convs = [(planes, cin, 1, 1, h, w), (planes, planes, 3, st, h, w), (4 * planes, planes, 1, 1, ho, wo)]
            if i == 0:
                convs.append((4 * planes, cin, 1, st, h, w))      # downsample.0
            for co, ci, kk, cs, hi, wi in convs:
                yield "enc_conv", (B, hi, wi, ci, co, kk, cs, 0)
                yield "enc_conv", (B, hi, wi, ci, co, kk, cs, 1)          # the input gradient: the transposed operator
                yield "enc_conv_wgrad", (B, hi, wi, ci, co, kk, cs)
                yield "enc_conv_p16", (B, hi, wi, ci, co, kk, cs, 0)
                yield "enc_conv_p16", (B, hi, wi, ci, co, kk, cs, 1)
                yield "enc_conv_wgrad_p16", (B, hi, wi, ci, co, kk, cs)
                yield from bn(co, (hi + cs - 1) // cs, (wi + cs - 1) // cs)
            cin, h, w = 4 * planes, ho, wo
    if cond_dim:
        yield "linear_backward", (B, cond_dim, cin, 0)                    # fc


def pyramid_operator_calls(B, H, W, precision=32):
    """the calls of EncoderTrainer.forward_pyramid / backward_pyramid (the sparse encoder of SparK pre-training) on a [B, 1, H, W] batch
    that take temporaries from an arena, in the form of operator_calls. precision (the spellings of engine.precision_bits): 32 lists
    the fp32 convolutions, 16 their _p16 forms in their place -- the arena serves an EncoderTrainer of that precision"""
    p16 = precision_bits(precision) == 16

    def bn(c, h, w):
        yield "spark_bn_forward", (B * h * w, h * w, c)
        yield "spark_bn_backward", (B * h * w, h * w, c)

    for op, args in operator_calls(B, H, W, 0):
        if op in ("enc_bn_forward", "enc_bn_backward"):
            if op == "enc_bn_forward":
                yield from bn(args[2], 1, args[1])
        elif not op.startswith("enc_conv") or op.endswith("_p16") == p16:
            yield op, args


def operator_scratch_bytes(B, H, W, cond_dim=128):
    """-> (main, side): the largest single call of operator_calls, and the largest cddpm_op_enc_conv_wgrad / _wgrad_p16 (what runs on the
    side-stream handle of the trainer whose handles the encoder uses). training.UNetTrainer._fit sizes its arenas for these too."""
    return largest_calls(operator_calls(B, H, W, cond_dim))


class EncoderTrainer(_optimizer.FlatOptimizer):
    """params: timm state_dict of the ResNet-50 (names conv1.weight, bn1.*, layerS.I.convJ.weight, layerS.I.bnJ.*, layerS.0.downsample.*,
    fc.*; running_mean / running_var included). `ops`: an object with `.lib`, `.h`, `.dev` (a training.UNetTrainer: the operators run on
    its handles and scratch arenas, which it sizes for the encoder's calls as well as its own: operator_scratch_bytes).
    precision: 32 (default) = fp32 FMA convolutions; 16 (the spellings of engine.precision_bits) = fp16 operands, fp32 accumulation."""

    LAYOUT_ERROR = "encoder optimizer state was saved for another parameter layout"

    def __init__(self, params: Dict[str, torch.Tensor], ops, drop_path_rate: float = 0.0, *, precision=32):
        self.precision = precision_bits(precision)            # parsed before a device is touched: a bad value is a ValueError here
        self.ops = ops
        # whose control block and loss scaler a guarded adam_step runs under: the trainer the encoder is trained jointly with
        self.optimizer = ops
        # called after the kernels wrote parameters or running statistics in place, which torch's version counters do not see: whoever
        # aliases these tensors (DDPM_2D: the inference encoder) sets it to drop what it derived from them
        self.on_write = None
        train_names = [k for k in params if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))]
        super().__init__(params, train_names, ops.dev)      # flat, gflat, p, g, state, and a control block for a step of its own
        self.buf = {k: params[k].detach().to(self.dev, torch.float32).clone() for k in params
                    if k.endswith("running_mean") or k.endswith("running_var")}
        self.blocks = []
        cin, nb, idx = 64, sum(n for _p2, n in STAGES), 0
        for s, (planes, nblocks) in enumerate(STAGES):
            for i in range(nblocks):
                stride = 2 if (i == 0 and s > 0) else 1
                self.blocks.append(dict(name=f"layer{s + 1}.{i}", cin=cin, planes=planes, stride=stride, down=(i == 0),
                                        drop=drop_path_rate * idx / (nb - 1)))        # timm: linearly increasing per block
                cin, idx = 4 * planes, idx + 1
        self.convs = {}
        for bk in self.blocks:
            n, pl = bk["name"], bk["planes"]
            self.convs[n + ".conv1"] = (pl, bk["cin"], 1, 1)
            self.convs[n + ".conv2"] = (pl, pl, 3, bk["stride"])
            self.convs[n + ".conv3"] = (4 * pl, pl, 1, 1)
            if bk["down"]:
                self.convs[n + ".downsample.0"] = (4 * pl, bk["cin"], 1, bk["stride"])
        # one image per role: fp32 [taps][K-dim][N-dim], or at precision 16 the fp16 images of cddpm_op_enc_pack_w_p16 (include/cddpm.h)
        img = torch.float16 if self.precision == 16 else torch.float32
        self.wf = {k: torch.empty(co * ci * kk * kk, dtype=img, device=self.dev) for k, (co, ci, kk, _s) in self.convs.items()}
        self.wd = {k: torch.empty(co * ci * kk * kk, dtype=img, device=self.dev) for k, (co, ci, kk, _s) in self.convs.items()}
        self.repack()

    # ------------------------------------------------------------------ plumbing
    @property
    def lib(self):
        return self.ops.lib

    @property
    def h(self):
        return self.ops.h

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.lib.cddpm_last_error(self.h).decode()}")

    def _s(self):
        return _stream_ptr(self.dev)

    def _new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def repack(self):
        pack = self.lib.cddpm_op_enc_pack_w_p16 if self.precision == 16 else self.lib.cddpm_op_enc_pack_w
        for k, (co, ci, kk, _s) in self.convs.items():
            self._ck(pack(self.h, _p(self.p[k + ".weight"]), co, ci, kk, _p(self.wf[k]), _p(self.wd[k]), self._s()),
                     "op_enc_pack_w")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """timm names -> current tensors (parameters are views of the flat buffer; running statistics as updated by the forward passes)"""
        out = dict(self.p)
        out.update(self.buf)
        return out

    # ------------------------------------------------------------------ operators
    def conv(self, name, x, transposed=False, in_hw=None):
        co, ci, kk, st = self.convs[name]
        B = x.shape[0]
        if not transposed:
            H, W = x.shape[1], x.shape[2]
            out = self._new(B, (H + st - 1) // st, (W + st - 1) // st, co)
            img = self.wf[name]
        else:
            H, W = in_hw
            out = self._new(B, H, W, ci)
            img = self.wd[name]
        op = self.lib.cddpm_op_enc_conv_p16 if self.precision == 16 else self.lib.cddpm_op_enc_conv
        self._ck(op(self.h, _p(x), _p(img), _p(out), B, H, W, ci, co, kk, st, int(transposed), self._s()), "op_enc_conv")
        return out

    def wgrad(self, name, x, dz):
        co, ci, kk, st = self.convs[name]
        B, H, W, _c = x.shape
        ops = self.ops
        op = self.lib.cddpm_op_enc_conv_wgrad_p16 if self.precision == 16 else self.lib.cddpm_op_enc_conv_wgrad
        if getattr(ops, "overlap_wgrad", False) and getattr(ops, "side", None) is not None:
            # as the UNet's weight gradients (training.UNetTrainer.wgrad): on the side stream and its handle, beside the main stream's chain
            # of small BatchNorm / input-gradient kernels
            ops.side.wait_stream(torch.cuda.current_stream(self.dev))
            rc = op(ops.eng_w._h, _p(x), _p(dz), _p(self.g[name + ".weight"]), B, H, W, ci, co, kk, st, ops.side.cuda_stream)
            if rc != 0:
                raise RuntimeError("op_enc_conv_wgrad failed: " + self.lib.cddpm_last_error(ops.eng_w._h).decode())
            x.record_stream(ops.side)
            dz.record_stream(ops.side)
            ops._side_busy = True
            return
        self._ck(op(self.h, _p(x), _p(dz), _p(self.g[name + ".weight"]), B, H, W, ci, co, kk, st, self._s()), "op_enc_conv_wgrad")

    def bn(self, name, z, relu, res=None, sscale=None, *, active=None, f=1, fill=None, training=True):
        """training-mode BatchNorm on parameter group `name` -> y, (mean | rstd). relu: 0 | 1 (ReLU) | 2 (ReLU6). Plain (no mask, fill,
        ReLU6 or evaluation mode: the dense ResNet-50) it is cddpm_op_enc_bn_forward; anything else is cddpm_op_spark_bn_forward, sparse
        (active uint8 [B,f,f]) or dense. Both run the one BatchNorm of the library, each on its own chunk plan (include/cddpm.h)."""
        if not plain_bn(relu, active, fill, training):
            return spark_bn_forward(self, name, z, relu, active, f, res=res, sscale=sscale, fill=fill, training=training)
        B, H, W, Cc = z.shape
        mr, y = self._new(2, Cc), torch.empty_like(z)
        self._ck(self.lib.cddpm_op_enc_bn_forward(self.h, _p(z), _p(self.p[name + ".weight"]), _p(self.p[name + ".bias"]), _p(sscale), _p(res),
                                                  int(relu), C.c_float(BN_EPS), C.c_float(BN_MOMENTUM), _p(self.buf[name + ".running_mean"]),
                                                  _p(self.buf[name + ".running_var"]), _p(mr), _p(y), B * H * W, H * W, Cc, self._s()),
                 "op_enc_bn_forward")
        return y, mr

    def bn_bwd(self, name, z, y, dy, mr, relu, sscale=None, want_dres=False, *, active=None, f=1, dfill=None, training=True):
        """the backward of bn() with the same relu, active, f and training (dfill: the gradient of its fill) -> dz, dres (None
        unless wanted); the gradients of the group's weight and bias land in g"""
        if not plain_bn(relu, active, dfill, training):
            return spark_bn_backward(self, name, z, y, dy, mr, relu, active, f, sscale=sscale, want_dres=want_dres, dfill=dfill, training=training)
        B, H, W, Cc = z.shape
        dz = torch.empty_like(z)
        dres = torch.empty_like(z) if want_dres else None
        self._ck(self.lib.cddpm_op_enc_bn_backward(self.h, _p(z), _p(y), _p(dy), _p(mr), _p(self.p[name + ".weight"]), _p(sscale), int(relu), _p(dz),
                                                   _p(dres), _p(self.g[name + ".weight"]), _p(self.g[name + ".bias"]), B * H * W, H * W, Cc,
                                                   self._s()), "op_enc_bn_backward")
        return dz, dres

    def mask_mul_(self, x, active, f):
        """x [B,H,W,C] *= the mask dilated to H x W, in place"""
        B, H, W, Cc = x.shape
        self._ck(self.lib.cddpm_op_spark_mask_mul(self.h, _p(x), _p(active), _p(x), B, H, W, Cc, f, self._s()), "op_spark_mask_mul")
        return x

    # ------------------------------------------------------------------ the ResNet-50, forward with saved activations and backward
    # One walk for the dense network (forward / backward) and for the sparse one of SparK pre-training (forward_pyramid / backward_pyramid:
    # the ResNet-50 after SparseEncoder.dense_model_to_sparse, reference spark/encoder.py:163-204). There every BatchNorm is a BatchNorm1d
    # over the ACTIVE pixels that writes zeros elsewhere (`mask` = dict(active=, f=), handed to bn / bn_bwd), and every convolution and
    # pooling output is multiplied by the mask at its resolution. A convolution is always followed by such a BatchNorm, which neither reads
    # the inactive pixels nor lets a gradient through to them, so the convolutions run unmasked (cddpm_op_enc_conv as it is); the input
    # and the max-pool output are masked by cddpm_op_spark_mask_mul.
    def _walk(self, x, drop_scales, mask=None, training=True):
        """x [B,1,H,W] fp32 contiguous: stem -> BatchNorm -> max pool -> the 16 bottleneck blocks -> (activations by name, last map).
        drop_scales: per-block [B] scales instead of fresh random draws; training False (with a mask): running statistics, no
        stochastic depth"""
        B, _c, H, W = x.shape
        kw = {} if mask is None else dict(mask, training=training)
        H1, W1 = (H + 1) // 2, (W + 1) // 2
        z0 = self._new(B, H1, W1, 64)
        self._ck(self.lib.cddpm_op_enc_stem(self.h, _p(x), _p(self.p["conv1.weight"]), _p(z0), B, H, W, self._s()), "op_enc_stem")
        a0, mr0 = self.bn("bn1", z0, True, **kw)
        cur = self._new(B, (H1 + 1) // 2, (W1 + 1) // 2, 64)
        self._ck(self.lib.cddpm_op_enc_maxpool(self.h, _p(a0), _p(cur), B, H1, W1, 64, 0, None, None, self._s()), "op_enc_maxpool")
        if mask is not None:
            self.mask_mul_(cur, **mask)
        sv: Dict[str, object] = dict(x=x, z0=z0, a0=a0, mr0=mr0)
        for bk in self.blocks:
            n = bk["name"]
            ss = None
            if training and drop_scales is not None:
                ss = drop_scales.get(n)
                ss = None if ss is None else ss.to(self.dev, torch.float32).contiguous()
            elif training and bk["drop"] > 0:
                keep = 1.0 - bk["drop"]
                ss = (torch.floor(keep + torch.rand(B, device=self.dev)) / keep).contiguous()     # timm.layers.drop_path
            z1 = self.conv(n + ".conv1", cur)
            a1, mr1 = self.bn(n + ".bn1", z1, True, **kw)
            z2 = self.conv(n + ".conv2", a1)
            a2, mr2 = self.bn(n + ".bn2", z2, True, **kw)
            z3 = self.conv(n + ".conv3", a2)
            r = dict(inp=cur, z1=z1, a1=a1, mr1=mr1, z2=z2, a2=a2, mr2=mr2, z3=z3, ss=ss)
            sc = cur
            if bk["down"]:
                zd = self.conv(n + ".downsample.0", cur)
                sc, mrd = self.bn(n + ".downsample.1", zd, False, **kw)
                r.update(zd=zd, mrd=mrd)
            out, mr3 = self.bn(n + ".bn3", z3, True, res=sc, sscale=ss, **kw)
            r.update(mr3=mr3, out=out)
            sv[n] = r
            cur = out
        if training:
            self._wrote()                   # every BatchNorm moved its running statistics
        return sv, cur

    def _wrote(self):
        if self.on_write is not None:
            self.on_write()

    def _block_backward(self, bk, r, d, mask=None):
        """d = dL/d(the block's output) -> dL/d(its input); the gradients of its parameters land in g"""
        n, inp = bk["name"], r["inp"]
        kw = mask or {}
        hw = (inp.shape[1], inp.shape[2])
        dz3, dsc = self.bn_bwd(n + ".bn3", r["z3"], r["out"], d, r["mr3"], True, r["ss"], want_dres=True, **kw)
        da2 = self.conv(n + ".conv3", dz3, transposed=True, in_hw=(r["a2"].shape[1], r["a2"].shape[2]))
        self.wgrad(n + ".conv3", r["a2"], dz3)
        dz2, _ = self.bn_bwd(n + ".bn2", r["z2"], r["a2"], da2, r["mr2"], True, **kw)
        da1 = self.conv(n + ".conv2", dz2, transposed=True, in_hw=hw)
        self.wgrad(n + ".conv2", r["a1"], dz2)
        dz1, _ = self.bn_bwd(n + ".bn1", r["z1"], r["a1"], da1, r["mr1"], True, **kw)
        dinp = self.conv(n + ".conv1", dz1, transposed=True, in_hw=hw)
        self.wgrad(n + ".conv1", inp, dz1)
        if bk["down"]:
            dzd, _ = self.bn_bwd(n + ".downsample.1", r["zd"], None, dsc, r["mrd"], False, **kw)
            self.ops.add_(dinp, self.conv(n + ".downsample.0", dzd, transposed=True, in_hw=hw))
            self.wgrad(n + ".downsample.0", inp, dzd)
        else:
            self.ops.add_(dinp, dsc)
        return dinp

    def _stem_backward(self, sv, d, mask=None):
        """d = dL/d(the max pool's output): max pool, bn1 and the stem's weight gradient (the input's gradient is never needed)"""
        a0, z0, x = sv["a0"], sv["z0"], sv["x"]
        B, H1, W1, _c = a0.shape
        da0 = torch.empty_like(a0)
        self._ck(self.lib.cddpm_op_enc_maxpool(self.h, _p(a0), None, B, H1, W1, 64, 1, _p(d), _p(da0), self._s()), "op_enc_maxpool (backward)")
        dz0, _ = self.bn_bwd("bn1", z0, a0, da0, sv["mr0"], True, **(mask or {}))
        self._ck(self.lib.cddpm_op_enc_stem_wgrad(self.h, _p(x), _p(dz0), _p(self.g["conv1.weight"]), B, x.shape[2], x.shape[3], self._s()),
                 "op_enc_stem_wgrad")
        if hasattr(self.ops, "join_side"):
            self.ops.join_side()

    # ------------------------------------------------------------------ forward (training mode), activations saved
    def forward(self, x: torch.Tensor, drop_scales: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """x [B,1,H,W] on the device -> context [B, cond_dim]. drop_scales (tests): per-block [B] scales instead of fresh random draws."""
        sv, cur = self._walk(x.float().contiguous(), drop_scales)
        B, Hc, Wc, Cc = cur.shape
        gap = self._new(B, Cc)
        self._ck(self.lib.cddpm_op_enc_avgpool(self.h, _p(cur), _p(gap), B, Hc * Wc, Cc, 0, self._s()), "op_enc_avgpool")
        wfc, bfc = self.p["fc.weight"], self.p["fc.bias"]
        out = self._new(B, wfc.shape[0])
        self._ck(self.lib.cddpm_op_linear(self.h, _p(gap), _p(wfc), _p(bfc), B, wfc.shape[0], Cc, 0, _p(out), self._s()), "op_linear")
        sv.update(gap=gap, last=cur)
        self.saved = sv
        return out

    # ------------------------------------------------------------------ backward: dL/d(context) -> gradients of every parameter
    def grad_offset(self, prefix: str) -> int:
        if not hasattr(self, "_goff"):
            base = self.gflat.data_ptr()
            self._goff = {k: (v.data_ptr() - base) // 4 for k, v in self.g.items()}
        return min((o for k, o in self._goff.items() if k.startswith(prefix)), default=self.gflat.numel())

    def backward(self, dcond: torch.Tensor, buckets=None) -> Dict[str, torch.Tensor]:
        """buckets (training.GradBuckets): told after every block how much of the flat gradient buffer's tail is final"""
        sv, g = self.saved, self.g
        gap, last = sv["gap"], sv["last"]
        B, Hc, Wc, Cc = last.shape
        wfc = self.p["fc.weight"]
        dgap = self._new(B, Cc)
        self._ck(self.lib.cddpm_op_linear_backward(self.h, _p(gap), _p(wfc), _p(dcond.float().contiguous()), B, wfc.shape[0], Cc, 0, _p(g["fc.weight"]),
                                                   _p(g["fc.bias"]), _p(dgap), self._s()), "op_linear_backward")
        d = torch.empty_like(last)
        self._ck(self.lib.cddpm_op_enc_avgpool(self.h, _p(dgap), _p(d), B, Hc * Wc, Cc, 1, self._s()), "op_enc_avgpool (backward)")
        for bk in reversed(self.blocks):
            d = self._block_backward(bk, sv[bk["name"]], d)
            if buckets is not None:
                if getattr(buckets, "on", True) and hasattr(self.ops, "join_side"):
                    self.ops.join_side()          # the side stream's weight gradients have landed before a collective reads the buffer
                buckets.mark_final(self.grad_offset(bk["name"] + "."))
        self._stem_backward(sv, d)
        self.saved = None
        return g

    # ------------------------------------------------------------------ SparK pre-training: the sparse encoder's pyramid
    def _stage_end(self):
        """name of each stage's last block -> index of its map among the four of forward_pyramid"""
        ends = [bk["name"] for i, bk in enumerate(self.blocks) if i + 1 == len(self.blocks) or self.blocks[i + 1]["down"]]
        return {n: i for i, n in enumerate(ends)}

    def forward_pyramid(self, x: torch.Tensor, active: torch.Tensor, drop_scales: Optional[Dict[str, torch.Tensor]] = None, *, training=True):
        """x [B,1,H,W] (H, W multiples of 32), active bool / uint8 [B,f,f] or [B,1,f,f] with f = H / 32, both on the device -> the masked
        outputs of layer1..4 as NHWC tensors [B,8f,8f,256], [B,4f,4f,512], [B,2f,2f,1024], [B,f,f,2048] (forward_features with pyramid = 4,
        reference spark/resnet.py:13-34) and latent [B,2048] = the layer4 map's mean over its pixels (src/models/Spark_2D.py:32).
        training False: running statistics, no stochastic depth, nothing kept for a backward. drop_scales: as forward().
        saved_pyramid keeps the keys of saved (without gap / last) plus active and f; its "x" is the masked input as [B,1,H,W], the shape
        forward() keeps (the same memory as the NHWC [B,H,W,1] the stem reads)."""
        B, _c, H, W = x.shape
        active = active.reshape(B, -1)
        f = int(round(active.shape[1] ** 0.5))
        if f * f != active.shape[1] or H != 32 * f or W != 32 * f:
            raise ValueError(f"forward_pyramid: a {H} x {W} input needs a [{B}, {H // 32}, {H // 32}] mask (side / 32), got {active.shape[1]} cells")
        mask = dict(active=active.to(self.dev, torch.uint8).contiguous(), f=f)
        xm = x.float().reshape(B, 1, H, W).clone(memory_format=torch.contiguous_format)
        self.mask_mul_(xm.view(B, H, W, 1), **mask)
        sv, cur = self._walk(xm, drop_scales, mask, training)
        sv.update(mask)
        Bc, Hc, Wc, Cc = cur.shape
        latent = self._new(B, Cc)
        self._ck(self.lib.cddpm_op_enc_avgpool(self.h, _p(cur), _p(latent), B, Hc * Wc, Cc, 0, self._s()), "op_enc_avgpool")
        self.saved_pyramid = sv if training else None
        return [sv[n]["out"] for n in self._stage_end()], latent

    def backward_pyramid(self, dfeats) -> Dict[str, torch.Tensor]:
        """dfeats: dL/d(the four maps of forward_pyramid), NHWC, layer1..4 (None: no gradient into that map) -> the gradient of every
        parameter (no gradient flows through latent: the pre-training loss does not read it)"""
        sv = self.saved_pyramid
        if sv is None:
            raise RuntimeError("backward_pyramid: no training-mode forward_pyramid to differentiate")
        mask = dict(active=sv["active"], f=sv["f"])
        stage_end = self._stage_end()
        d = None
        for bk in reversed(self.blocks):
            n = bk["name"]
            if n in stage_end and dfeats[stage_end[n]] is not None:
                df = dfeats[stage_end[n]].float().contiguous()
                d = df.clone() if d is None else self.ops.add_(d, df)
            if d is None:
                raise ValueError("backward_pyramid: the gradient of the layer4 map is needed")
            d = self._block_backward(bk, sv[n], d, mask)
        self.mask_mul_(d, **mask)                                      # the masked max-pool output (SparseMaxPooling, encoder.py:42-43)
        self._stem_backward(sv, d, mask)
        self.saved_pyramid = None
        return self.g

    def adam_step(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=None, guarded=False, extra_unscale=None):
        """Adam over the flat buffer under the guard of the trainer it is trained with (`optimizer`: training.UNetTrainer): the encoder and
        the UNet are ONE optimizer in the reference (`optim.Adam(self.parameters())`, DDPM_2D.py:305-306), so the step count and the skip
        decision are that trainer's control block. guarded: its `guard(others=(self,))` was called for this step; else the encoder is
        stepped alone, under its own control block. grad_scale None: 1, or -- guarded, with the trainer's dynamic loss scaling on -- its
        device scale, the loss scale too is shared (gradient = gflat * extra_unscale (default 1) / scale; the trainer updates the scale
        after this)."""
        if not guarded:
            _optimizer.guard(self, (self,), betas)
        opt = self.optimizer if guarded else self
        scaler = opt.step_scaler(grad_scale)
        if scaler is not None:
            _optimizer.update(opt, self, lr, betas, eps, unscale=1.0 if extra_unscale is None else extra_unscale, scaler=scaler)
        else:
            _optimizer.update(opt, self, lr, betas, eps, unscale=1.0 / (grad_scale if grad_scale is not None else 1.0))
        self.repack()
        self._wrote()

    def optimizer_state(self) -> Dict[str, torch.Tensor]:
        m, v = _optimizer.moments(self)
        return {"m": m.detach().clone(), "v": v.detach().clone(), "layout": self.layout()}

    def load_optimizer_state(self, state) -> None:
        self.check_layout(state["layout"])
        self.load_moments(state["m"], state["v"])

    def parameters_changed(self) -> None:
        """parameters were written from outside (load_state_dict into the aliased module): rebuild the operators' weight images"""
        self.repack()
