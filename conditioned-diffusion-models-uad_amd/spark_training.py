"""SparK masked pre-training of the context encoder on the HIP operators: one training step of the reference's
`experiment=cDDPM/Spark_2D_pretrain` (src/models/Spark_2D.py; src/models/modules/spark/Spark_2D.py:143-199): the sparse ResNet-50
(encoder_training.EncoderTrainer.forward_pyramid), densify (sparse BatchNorm, mask tokens, en_de_lins), the LightDecoder
(spark/decoder.py), the masked L2 loss [+ the L1 mean], the backward of all of it and AdamW (src/models/Spark_2D.py:123-124).

Same construction as the other trainers: Python sequencing C-ABI operators (include/cddpm.h, "operators of SparK masked pre-training";
csrc/spark_train.hip, csrc/batchnorm_train.hip) on NHWC fp32 device tensors. The densify and decoder parameters live in ONE flat fp32 buffer (`flat`, views `p[name]`
under the reference's names without the `model.` prefix), their gradients in a second (`gflat`), Adam's moments in two more; the ResNet-50's
are the EncoderTrainer's (`enc.flat`, ...). The operators run on a handle of this trainer's own, whose arena it sizes for its calls from
the library's size queries (operator_calls).

Built: the configuration of the reference experiment -- resnet50, four pyramid levels, BatchNorm densify norms, double = True (ConvTranspose2d
4/2/1), heavy [0, 1], cmid 0, no positional embedding, pix_norm 0, loss on the masked cells. dec_dim must be a multiple of 128 (the last
decoder BatchNorm then has 4 channels, the least cddpm_op_spark_bn_forward takes).

Precision (the trainer's own: `SparKTrainer(..., precision=16)`, the spellings of engine.precision_bits; the process-wide
cddpm_set_train_precision is neither read nor set): at 16 -- what the reference's `precision: 16` (configs/trainer/default.yaml:7, which
Spark_2D_pretrain inherits) computes under autocast -- every convolution of the sparse ResNet-50 but the 7x7 stem runs forward, input
gradient and weight gradient on the fp16-MFMA operators (EncoderTrainer(precision=16): fp16 operands, fp32 accumulation), in training and
in evaluation forwards. The sparse and dense BatchNorms, mask multiply, max pool, stem, en_de_lins, the LightDecoder, the loss, AdamW and
the master weights are fp32 at either precision (launch- and memory-bound at 4 to 128 channels: DESIGN.md section 4b-g). Precision 16
trains under a dynamic loss scale on the device (enable_loss_scaling; torch GradScaler's rule and default start 65536), as Lightning's
native AMP does for the reference: unscaled, most of the gradient inside layer3 / layer4 lies below fp16's smallest normal."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import optimizer as _optimizer
from ._lib import largest_calls
from .encoder_training import EncoderTrainer, pyramid_operator_calls, spark_bn_backward, spark_bn_forward, _p
from .engine import _stream_ptr, precision_bits

ENC_PREFIX = "sparse_encoder.sp_cnn."
ENC_DIMS = (2048, 1024, 512, 256)            # channels of the maps densify reads, smallest map first


def decoder_layers(dec_dim=128):
    """-> [(name, kind, Cin, Cout, K)] of every convolution outside the ResNet, with the reference's module names"""
    out = []
    for i, c in enumerate(ENC_DIMS):
        out.append((f"en_de_lins.{i}", "conv", c, dec_dim >> i, 1 if i == 0 else 3))
    for i in range(5):
        c = dec_dim >> i
        out += [(f"dense_decoder.dec.{i}.up", "convT", c, c, 4), (f"dense_decoder.dec.{i}.conv.0.b.0", "conv", c, c, 3),
                (f"dense_decoder.dec.{i}.conv.0.b.3", "conv", c, c // 2, 3)]
    out.append(("dense_decoder.proj", "conv", dec_dim >> 5, 1, 1))
    return out


def operator_calls(B, H, W, dec_dim=128, precision=32):
    """the calls of SparKTrainer.forward / backward on a [B, 1, H, W] batch that take temporaries from the arena, as (operator, arguments of
    its size query): the sparse encoder's at `precision` (encoder_training.pyramid_operator_calls) and those of densify, decoder and loss
    (cddpm_op_spark_loss_scaled takes what cddpm_op_spark_loss takes)"""
    yield from pyramid_operator_calls(B, H, W, precision)
    f = H // 32
    res = {}
    for i in range(4):
        res[f"en_de_lins.{i}"] = f << i
        yield "spark_bn_forward", (B * (f << i) ** 2, (f << i) ** 2, ENC_DIMS[i])
        yield "spark_bn_backward", (B * (f << i) ** 2, (f << i) ** 2, ENC_DIMS[i])
    for i in range(5):
        res[f"dense_decoder.dec.{i}.up"] = f << i
        res[f"dense_decoder.dec.{i}.conv.0.b.0"] = res[f"dense_decoder.dec.{i}.conv.0.b.3"] = f << (i + 1)
        for c in (dec_dim >> i, dec_dim >> (i + 1)):
            yield "spark_bn_forward", (B * (f << (i + 1)) ** 2, (f << (i + 1)) ** 2, c)
            yield "spark_bn_backward", (B * (f << (i + 1)) ** 2, (f << (i + 1)) ** 2, c)
    res["dense_decoder.proj"] = H
    for name, kind, ci, co, k in decoder_layers(dec_dim):
        t, r = int(kind == "convT"), res[name]
        yield "spark_conv", (B, r, r, ci, co, k, t, 0)
        yield "spark_conv", (B, r, r, ci, co, k, t, 1)
        yield "spark_conv_wgrad", (B, r, r, ci, co, k, t, int(kind == "convT" or name.startswith("en_de_lins") or name.endswith("proj")))
    yield "spark_loss", (B, H, W, f)


def arena_bytes(B, H, W, dec_dim=128, precision=32):
    return largest_calls(operator_calls(B, H, W, dec_dim, precision))[0]


class SparKTrainer(_optimizer.FlatOptimizer):
    """params: the reference's state dict of SparK_2D without the `model.` prefix (sparse_encoder.sp_cnn.*, en_de_norms.*, en_de_lins.*,
    mask_tokens.*, dense_decoder.*; running statistics included, num_batches_tracked and the image-norm buffers ignored).
    loss_weights (w_mask, w_l1): loss = w_mask * masked L2 + w_l1 * mean |reco - x| -- (1, 0) is `loss_on_mask: True`, (delta_mask, 1) the
    other branch of Spark_2D.forward (src/models/Spark_2D.py:28-31).
    precision: 32 (default) | 16, the spellings of engine.precision_bits ("bf16" and anything else: ValueError) -- the arithmetic of the
    sparse ResNet-50's convolutions (module docstring). 16 turns dynamic loss scaling on (enable_loss_scaling's defaults) and needs a
    GPU device: with any other it is a ValueError, raised like a bad precision before a device is touched."""

    # torch.cuda.amp.GradScaler()'s own init_scale and so the reference Trainer's start (measured inside the
    # stages: at most 0.001 % of the dz operands stay below fp16's smallest normal, the largest is 1.3e4 at 3x96x96 and falls with the
    # batch; a batch that overflows there backs off in its first steps). A default start: enable_loss_scaling makes the block at once.
    DEFAULT_INIT_SCALE = 65536.0
    LAYOUT_ERROR = "SparK optimizer state was saved for another parameter layout"

    def __init__(self, params: Dict[str, torch.Tensor], device=None, *, dec_dim=128, drop_path_rate=0.05, loss_weights=(1.0, 0.0), precision=32):
        self.precision = precision_bits(precision)            # parsed before a device is touched: a bad value is a ValueError here
        if dec_dim < 128 or dec_dim % 128:
            raise NotImplementedError(f"SparKTrainer: dec_dim {dec_dim} must be a multiple of 128")
        from .training import UNetTrainer
        self.dev = torch.device(device) if device is not None else next(iter(params.values())).device
        if self.precision == 16 and self.dev.type != "cuda":
            # checked like the precision itself, before a device is touched: a precision-16 request that names no GPU keeps the answer it
            # had before the fp16-MFMA step was built (a ValueError that says "precision 32 only"), not the handle's "no HIP device"
            raise ValueError(f"SparKTrainer: precision {precision!r} is not built for device '{self.dev}': its convolutions are the fp16-MFMA "
                             "kernels of a GPU; off a GPU the request is refused as before (precision 32 only)")
        self.dec_dim, self.loss_weights = int(dec_dim), (float(loss_weights[0]), float(loss_weights[1]))
        # the handle the operators run on (no UNet is trained on it; overlap off: every call of this step runs on the one stream)
        self.ops = UNetTrainer({"w": torch.zeros(64)}, device=self.dev, overlap_wgrad=False)
        self.enc = EncoderTrainer({k[len(ENC_PREFIX):]: v for k, v in params.items() if k.startswith(ENC_PREFIX)}, self.ops, drop_path_rate,
                                  precision=self.precision)
        self.enc.optimizer = self           # one AdamW over both buffers: this trainer's control block and scaler
        skip = ("num_batches_tracked", "running_mean", "running_var")
        own = {k: v for k, v in params.items() if not k.startswith(ENC_PREFIX) and k.split(".")[0] in ("en_de_norms", "en_de_lins", "mask_tokens", "dense_decoder")}
        super().__init__(own, [k for k in own if not k.endswith(skip)], self.dev)      # flat, gflat, p, g, state, ctrl, the loss scaler (off)
        self.buf = {k: own[k].detach().to(self.dev, torch.float32).clone() for k in own if k.endswith(("running_mean", "running_var"))}
        want = {n + ".weight" for n, *_ in decoder_layers(self.dec_dim)} | {f"mask_tokens.{i}" for i in range(4)}
        missing = sorted(want - set(self.p))
        if missing:
            raise ValueError(f"SparKTrainer: the state dict lacks {', '.join(missing[:4])}{' ...' if len(missing) > 4 else ''}")
        self.layers = {n: (kind, ci, co, k) for n, kind, ci, co, k in decoder_layers(self.dec_dim)}
        self._arena = (0, 0, 0)
        self.saved = None
        if self.precision == 16:            # dynamic loss scaling: on by default at precision 16, available at 32
            self.enable_loss_scaling()

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

    def _fit(self, B, H, W):
        """the handle's arena holds the largest call of this step at the largest geometry seen (operator_calls: the library's own size queries)"""
        if B <= self._arena[0] and H <= self._arena[1] and W <= self._arena[2]:
            return
        B, H, W = max(B, self._arena[0]), max(H, self._arena[1]), max(W, self._arena[2])
        torch.cuda.synchronize(self.dev)
        self._ck(self.lib.cddpm_op_set_scratch(self.h, arena_bytes(B, H, W, self.dec_dim, self.precision)), "op_set_scratch")
        self._arena = (B, H, W)

    def close(self):
        self.ops.close()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """the reference's names without `model.` -> current tensors (views of the flat buffers; running statistics as the forwards left them)"""
        out = {ENC_PREFIX + k: v for k, v in self.enc.state_dict().items()}
        out.update(self.p)
        out.update(self.buf)
        return out

    # ------------------------------------------------------------------ operators
    def conv(self, name, x, backward=False):
        """layer `name` forward on its input x, or (backward) its input gradient from x = dL/d(output)"""
        kind, ci, co, k = self.layers[name]
        t = int(kind == "convT")
        B = x.shape[0]
        if not backward:
            H, W = x.shape[1], x.shape[2]
            out = self._new(B, H << t, W << t, co)
        else:
            H, W = x.shape[1] >> t, x.shape[2] >> t
            out = self._new(B, H, W, ci)
        bias = self.p.get(name + ".bias") if not backward else None
        self._ck(self.lib.cddpm_op_spark_conv(self.h, _p(x), _p(self.p[name + ".weight"]), _p(bias), _p(out), B, H, W, ci, co, k, t, int(backward), self._s()),
                 "op_spark_conv")
        return out

    def wgrad(self, name, x, dy):
        kind, ci, co, k = self.layers[name]
        B, H, W, _c = x.shape
        self._ck(self.lib.cddpm_op_spark_conv_wgrad(self.h, _p(x), _p(dy), _p(self.g[name + ".weight"]), _p(self.g.get(name + ".bias")), B, H, W, ci, co, k,
                                                    int(kind == "convT"), self._s()), "op_spark_conv_wgrad")

    def bn(self, name, z, act, active=None, f=1, res=None, fill=None, training=True):
        return spark_bn_forward(self, name, z, act, active, f, res=res, fill=fill, training=training)

    def bn_bwd(self, name, z, y, dy, mr, act, active=None, f=1, dfill=None):
        return spark_bn_backward(self, name, z, y, dy, mr, act, active, f, dfill=dfill)[0]

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, active: torch.Tensor, training=True, drop_scales: Optional[Dict[str, torch.Tensor]] = None):
        """x [B,1,H,W] (H = W a multiple of 32), active bool [B,1,f,f] / [B,f,f] (f = H / 32; True = kept) -> loss (0-d), reco [B,1,H,W],
        latent [B,2048], all on the device. training: batch statistics and stochastic depth, activations kept for backward(); else running
        statistics. `terms` holds (masked L2, L1 mean) of the call."""
        x = x.to(self.dev, torch.float32).contiguous()
        B, _c, H, W = x.shape
        if H != W or H % 32:
            raise ValueError(f"SparKTrainer: the input must be square with a side that is a multiple of 32, got {H} x {W}")
        self._fit(B, H, W)
        f = H // 32
        active = active.reshape(B, f, f).to(self.dev, torch.uint8).contiguous()
        feats, latent = self.enc.forward_pyramid(x, active, drop_scales, training=training)
        sv = dict(x=x, active=active, f=f, dens=[], dec=[])
        cur_f, to_dec = f, []
        for i, fea in enumerate(reversed(feats)):                  # from the smallest map up (spark/Spark_2D.py:157-171)
            t, mr = self.bn(f"en_de_norms.{i}", fea, 0, active, f, fill=self.p[f"mask_tokens.{i}"], training=training)
            to_dec.append(self.conv(f"en_de_lins.{i}", t))
            sv["dens"].append(dict(fea=fea, t=t, mr=mr))
        h = to_dec[0]
        for i in range(5):                                         # LightDecoder.forward (spark/decoder.py:70-76)
            n = f"dense_decoder.dec.{i}"
            up = self.conv(n + ".up", h)
            z1 = self.conv(n + ".conv.0.b.0", up)
            a1, mr1 = self.bn(n + ".conv.0.b.1", z1, 2, training=training)
            z2 = self.conv(n + ".conv.0.b.3", a1)
            # the next level's `x + to_dec[i + 1]` rides on this BatchNorm's shortcut operand
            out, mr2 = self.bn(n + ".conv.0.b.4", z2, 0, res=to_dec[i + 1] if i < 3 else None, training=training)
            sv["dec"].append(dict(inp=h, up=up, z1=z1, a1=a1, mr1=mr1, z2=z2, mr2=mr2))
            h = out
        rec = self.conv("dense_decoder.proj", h)
        sv["last"] = h
        terms, drec = self._new(2), (torch.empty_like(rec) if training else None)
        wm, wl = self.loss_weights
        if self.loss_scaling:               # drec carries the device scale; the terms, and so the loss returned, do not
            self._ck(self.lib.cddpm_op_spark_loss_scaled(self.h, _p(rec), _p(x), _p(active), f, B, H, W, C.c_float(wm), C.c_float(wl), _p(self.scaler),
                                                         _p(terms), _p(drec), self._s()), "op_spark_loss_scaled")
        else:
            self._ck(self.lib.cddpm_op_spark_loss(self.h, _p(rec), _p(x), _p(active), f, B, H, W, C.c_float(wm), C.c_float(wl), _p(terms), _p(drec),
                                                  self._s()), "op_spark_loss")
        sv["drec"] = drec
        self.saved = sv if training else None
        self.terms = terms
        loss = terms[0] * wm + terms[1] * wl
        return loss, rec.view(B, 1, H, W), latent

    # ------------------------------------------------------------------ backward: the gradient of `loss` w.r.t. every parameter
    # (with dynamic loss scaling on: times the device scale the forward's loss gradient was formed with; adamw_step divides it out)
    def backward(self):
        sv = self.saved
        if sv is None:
            raise RuntimeError("SparKTrainer.backward: no training-mode forward to differentiate")
        active, f = sv["active"], sv["f"]
        self.wgrad("dense_decoder.proj", sv["last"], sv["drec"])
        d = self.conv("dense_decoder.proj", sv["drec"], backward=True)
        dto = [None] * 4
        for i in reversed(range(5)):
            n, r = f"dense_decoder.dec.{i}", sv["dec"][i]
            dz2 = self.bn_bwd(n + ".conv.0.b.4", r["z2"], None, d, r["mr2"], 0)
            self.wgrad(n + ".conv.0.b.3", r["a1"], dz2)
            da1 = self.conv(n + ".conv.0.b.3", dz2, backward=True)
            dz1 = self.bn_bwd(n + ".conv.0.b.1", r["z1"], r["a1"], da1, r["mr1"], 2)
            self.wgrad(n + ".conv.0.b.0", r["up"], dz1)
            dup = self.conv(n + ".conv.0.b.0", dz1, backward=True)
            self.wgrad(n + ".up", r["inp"], dup)
            d = self.conv(n + ".up", dup, backward=True)           # dL/d(this level's input) = dL/d(previous output) = dL/d(to_dec[i])
            if i < 4:
                dto[i] = d
        dfeats = []
        for i in range(4):
            r = sv["dens"][i]
            self.wgrad(f"en_de_lins.{i}", r["t"], dto[i])
            dt = self.conv(f"en_de_lins.{i}", dto[i], backward=True)
            dfeats.append(self.bn_bwd(f"en_de_norms.{i}", r["fea"], None, dt, r["mr"], 0, active, f, dfill=self.g[f"mask_tokens.{i}"]))
        self.enc.backward_pyramid(list(reversed(dfeats)))
        self.saved = None
        return self.g

    # ------------------------------------------------------------------ AdamW over every parameter, one decision for both buffers
    def adamw_step(self, lr=1e-4, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-8):
        """torch.optim.AdamW(self.parameters(), lr, weight_decay, betas) of Spark_2D.configure_optimizers: decoupled decay, then Adam, on
        the encoder's and on this trainer's flat buffers under one control block -- a step with a non-finite gradient anywhere moves and
        decays nothing and does not count. With dynamic loss scaling on, the order of include/cddpm.h: the checks, one commit,
        cddpm_op_adamw_scaled on both buffers (the gradient buffers hold scale x the gradient; the scale of this step's loss is divided
        out on the device), one cddpm_op_scaler_update."""
        owners = (self, self.enc)
        _optimizer.guard(self, owners, betas)
        scaler = self.step_scaler()
        for t in owners:
            _optimizer.update(self, t, lr, betas, eps, weight_decay=weight_decay, scaler=scaler)
        if scaler is not None:
            self.update_loss_scale()
        self.enc.repack()

    def layout(self):
        """of both buffers, the encoder's first under an "enc:" prefix: the order of optimizer_state's m and v"""
        return [("enc:" + k, n) for k, n in self.enc.layout()] + super().layout()

    def optimizer_state(self) -> Dict[str, object]:
        """Adam's moments of both buffers (encoder first) with the layout they belong to and the step count: what mirror_common checkpoints"""
        (em, ev), (m, v) = _optimizer.moments(self.enc), _optimizer.moments(self)
        out = {"m": torch.cat([em, m]).detach().clone(), "v": torch.cat([ev, v]).detach().clone(), "layout": self.layout(),
               "step": self.step_count, "skipped": self.skipped_steps}
        if self.loss_scaling:               # UNetTrainer.optimizer_state's entry: the settings and the device block
            out["scaler"] = self.scaler_state()
        return out

    def load_optimizer_state(self, state) -> None:
        self.check_layout(state["layout"])
        n = self.enc.flat.numel()
        self.enc.load_moments(state["m"][:n], state["v"][:n])
        self.load_moments(state["m"][n:], state["v"][n:])
        self.ctrl.zero_()
        self.ctrl[1], self.ctrl[3] = int(state.get("step", 0)), int(state.get("skipped", 0))
        # the bias corrections of the control block are rewritten by the next cddpm_op_guard_commit before any update reads them
        self.load_scaler_state(state.get("scaler"))      # absent: saved without dynamic loss scaling -- the scaler is left as it is

    def parameters_changed(self) -> None:
        self.enc.repack()
