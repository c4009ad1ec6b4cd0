"""Mirror of the reference's SparK pre-training LightningModule (src/models/Spark_2D.py: `Spark_2D`, the `_target_` of
`experiment=cDDPM/Spark_2D_pretrain`), on the HIP operators: masked pre-training of the ResNet-50 context encoder whose checkpoint the
headline experiment starts from (configs/experiment/cDDPM/DDPM_cond_spark_2D.yaml:44-45 `pretrained_encoder: True`; DDPM_2D.py ingests it).

Same `cfg` keys, same state_dict names and shapes (`model.sparse_encoder.sp_cnn.*` with num_batches_tracked, `model.en_de_norms.*`,
`model.en_de_lins.*`, `model.mask_tokens.*`, `model.dense_decoder.*`, the buffers `model.imn_m`, `model.imn_s`, `model.norm_black`), same
`forward(x) -> (loss, reco, latent)`, `training_step` / `validation_step` logging `train/Loss_comb` / `val/Loss_comb`,
`configure_optimizers` (AdamW, weight_decay cfg.weight_decay or 0.05, betas (0.9, 0.95)), `update_prefix`. The arithmetic is
spark_training.SparKTrainer's (csrc/spark_train.hip + the encoder's training operators); the step is optimised manually, so the
torch.optim.AdamW that configure_optimizers returns is never stepped and AdamW's state travels in the checkpoint under
`hip_optimizer_state`, as the other mirrors' does. The cell mask is drawn on the host from torch's default generator exactly as
SparK_2D.mask draws it (spark/Spark_2D.py:139-141): under torch.manual_seed the mirror picks the reference's cells.

Built: the experiment's configuration. Refused with NotImplementedError (the convention of DDPM_encoder.py): a missing `backbone` or one
other than resnet50, mask_ratio != mask_ratio2, uniform, pe, pix_norm other than 0, dense_loss, loss_l2 False, pyramid != 4, double
False, hea != [0, 1], cmid != 0, a dec_dim that is no multiple of 128, an input side that is no multiple of 32. `en_de_norm` and `sbn`
are ignored, as SparK_2D.__init__ hard-codes 'bn' and False over them (spark/Spark_2D.py:31-33).
Precision: `cfg.precision`, or the attached Lightning trainer's `precision` (the experiment inherits `precision: 16` from
configs/trainer/default.yaml:7), in the spellings and with the mapping of training.set_precision (unset: 32). It is
the SparKTrainer's own precision, read when the trainer is created; the process-wide training precision is not touched. At 16 the sparse
ResNet-50's convolutions run on the fp16-MFMA operators under a dynamic loss scale on the device, as Lightning's native AMP trains the
reference: `train/loss_scale` and `train/skipped_steps` are logged from device tensors, the consecutive skips are read once every 50
steps (30 or more: one RuntimeWarning), the scaler travels in the checkpoint with AdamW's state, and a reference checkpoint's
`native_amp_scaling_state` seeds scale and growth tracker.
Initialisation follows the reference's distributions (timm's ResNet init with zero_init_last, PyTorch's Conv2d default for en_de_lins,
LightDecoder.initialize, trunc_normal_ tokens) drawn from torch's generator; it is not the reference's random stream (timm is not here to
consume it in its order). `test_step`: not built -- the experiment sets `test_after_training: False`."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .mirror_common import AttrDict, HipMirror, _Base, _cfg_get, _to_cpu
from .synth import SPARK_ENC_PREFIX, spark_param_shapes

BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked")
ROOT_BUFFERS = ("model.imn_m", "model.imn_s", "model.norm_black")


def draw_mask(B: int, f: int, len_keep: int, generator=None) -> torch.Tensor:
    """SparK_2D.mask for mask_ratio == mask_ratio2 (spark/Spark_2D.py:139-141): bool [B,1,f,f] on the host, True = kept"""
    idx = torch.rand(B, f * f, generator=generator).argsort(dim=1)[:, :len_keep]
    return torch.zeros(B, f * f, dtype=torch.bool).scatter_(dim=1, index=idx, value=True).view(B, 1, f, f)


def check_cfg(cfg):
    """-> (input_size, dec_dim, mask_ratio, drop_path_rate) of a cfg this package builds; NotImplementedError for anything else"""
    def refuse(what):
        raise NotImplementedError(f"Spark_2D: {what} is not built natively (the configuration of experiment=cDDPM/Spark_2D_pretrain is)")
    backbone = cfg.get("backbone", None)
    if backbone != "resnet50":
        refuse(f"backbone={backbone!r} (only resnet50)")
    mask_ratio = cfg.get("mask_ratio", 0.6)
    if cfg.get("mask_ratio2", mask_ratio) != mask_ratio:
        refuse("mask_ratio != mask_ratio2")
    for key, want in (("uniform", False), ("pe", False), ("dense_loss", False), ("loss_l2", True), ("pyramid", 4), ("double", True), ("cmid", 0)):
        if cfg.get(key, want) != want:
            refuse(f"{key}={cfg.get(key)!r}")
    if int(cfg.get("pix_norm", 1)) != 0:           # the reference's default is 1; the experiment's yaml sets False
        refuse(f"pix_norm={cfg.get('pix_norm', 1)!r} (only 0 / False)")
    if list(cfg.get("hea", [0, 1])) != [0, 1]:
        refuse(f"hea={cfg.get('hea')!r}")
    dec_dim = int(cfg.get("dec_dim", 128))
    if dec_dim < 128 or dec_dim % 128:
        refuse(f"dec_dim={dec_dim} (a multiple of 128)")
    size = int(cfg["imageDim"][1] / cfg["rescaleFactor"])
    if size < 32 or size % 32:
        refuse(f"an input side of {size} (a multiple of 32)")
    dp = cfg.get("dp", 0)
    return size, dec_dim, float(mask_ratio), float(dp if dp != 0 else 0.05)          # spark/models.py:50, :68-69


def _init_tensor(name, t):
    """the reference's initial distribution of tensor `name` (see the module docstring)"""
    leaf = name.rsplit(".", 1)[1]
    if name in ROOT_BUFFERS:
        vals = {"model.imn_m": (0.485, 0.456, 0.406), "model.imn_s": (0.229, 0.224, 0.225)}.get(name)       # timm.data IMAGENET_DEFAULT_*
        return t.zero_() if vals is None else t.copy_(torch.tensor(vals).view(1, 3, 1, 1))
    if leaf in ("running_mean", "num_batches_tracked"):
        return t.zero_()
    if leaf == "running_var":
        return t.fill_(1.0)
    if "mask_tokens" in name:
        return nn.init.trunc_normal_(t, mean=0, std=.02, a=-.02, b=.02)
    if t.dim() == 1:                                # BatchNorm weight / bias, convolution bias
        is_gamma = leaf == "weight"
        if name.startswith("model.en_de_lins") and leaf == "bias":
            fan_in = (2048 >> int(name.split(".")[2])) * (1 if name.split(".")[2] == "0" else 9)
            return nn.init.uniform_(t, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
        if is_gamma and name.startswith(SPARK_ENC_PREFIX) and name.endswith("bn3.weight"):
            return t.zero_()                        # timm's zero_init_last
        return t.fill_(1.0) if is_gamma else t.zero_()
    if name.startswith(SPARK_ENC_PREFIX) or name.endswith(".up.weight"):
        return nn.init.kaiming_normal_(t, mode="fan_out", nonlinearity="relu")
    if name.startswith("model.en_de_lins"):
        return nn.init.kaiming_uniform_(t, a=math.sqrt(5))
    return nn.init.trunc_normal_(t, std=.02)        # LightDecoder.initialize: every Conv2d of the decoder


class _Tree(nn.Module):
    """a module tree that holds tensors at dotted paths (`a.b.0.weight`): containers for the path, a parameter or buffer at the leaf"""

    def put(self, path, tensor, buffer):
        node = self
        *parts, leaf = path.split(".")
        for part in parts:
            if part not in node._modules:
                node.add_module(part, _Tree())
            node = node._modules[part]
        if buffer:
            node.register_buffer(leaf, tensor)
        else:
            node.register_parameter(leaf, nn.Parameter(tensor))


class Spark_2D(_Base):
    SCALER_CHECK_EVERY, SCALER_STALL_SKIPS = HipMirror.SCALER_CHECK_EVERY, HipMirror.SCALER_STALL_SKIPS      # of HipMirror._watch_loss_scale

    def __init__(self, cfg, prefix=None):
        super().__init__()
        if isinstance(cfg, dict) and not isinstance(cfg, AttrDict):
            cfg = AttrDict(cfg)
        self.cfg = cfg
        self.input_size, self.dec_dim, self.mask_ratio, self.drop_path_rate = check_cfg(cfg)
        self.downsample_raito = 32
        self.fmap_size = self.input_size // 32
        self.len_keep = round(self.fmap_size * self.fmap_size * (1 - self.mask_ratio))
        self.model = _Tree()
        for name, shape in spark_param_shapes(self.dec_dim, self.input_size).items():
            leaf = name.rsplit(".", 1)[1]
            t = torch.zeros(shape, dtype=torch.int64 if leaf == "num_batches_tracked" else torch.float32)
            with torch.no_grad():
                _init_tensor(name, t)
            self.model.put(name[len("model."):], t, buffer=leaf in BUFFER_LEAVES or name in ROOT_BUFFERS)
        self.prefix = prefix
        self.logged = {}
        self._hip_spark_trainer = None
        if hasattr(self, "save_hyperparameters") and _Base is not nn.Module:
            try:
                self.save_hyperparameters()
            except Exception:
                pass

    # ------------------------------------------------------------------ the training state on the HIP operators
    def loss_weights(self):
        """(w_mask, w_l1) of Spark_2D.forward (src/models/Spark_2D.py:28-31; L1_AE's lossStrategy, src/models/losses.py:13-18)"""
        if _cfg_get(self.cfg, "loss_on_mask", False):
            return 1.0, 0.0
        strat = _cfg_get(self.cfg, "lossStrategy", "mean")
        if strat not in ("mean", "sum"):
            raise ValueError(f"lossStrategy {strat!r}: 'mean' or 'sum'")
        return float(_cfg_get(self.cfg, "delta_mask", 0)), (1.0 if strat == "mean" else float(self.input_size * self.input_size))

    def precision_bits(self) -> int:
        """16 | 32 from cfg.precision or the attached Lightning trainer's precision (HipMirror._train_precision), through
        training.set_precision's mapping; neither given: 32"""
        from .training import lightning_precision_bits
        return lightning_precision_bits(HipMirror._train_precision(self))

    def hip_trainer(self, device):
        """spark_training.SparKTrainer with this module's tensors; from here on the module's parameters and running statistics ARE the
        trainer's buffers (state_dict() / checkpoints see the trained values)"""
        if self._hip_spark_trainer is None:
            from .spark_training import SparKTrainer
            sd = {k[len("model."):]: v for k, v in self.state_dict().items()}
            self._hip_spark_trainer = SparKTrainer(sd, device, dec_dim=self.dec_dim, drop_path_rate=self.drop_path_rate, loss_weights=self.loss_weights(),
                                                   precision=self.precision_bits())
            st = getattr(self, "_pending_opt_state", None)
            if st:
                self._hip_spark_trainer.load_optimizer_state(st)
                self._pending_opt_state = None
            self._seed_loss_scaling()
        self._alias()
        return self._hip_spark_trainer

    def _alias(self):
        """parameters and float buffers of the module are views of / the very tensors of the trainer. `.to()` / `.cpu()` replace `.data`
        silently: a broken alias is repaired in the direction that loses nothing (the module's values are copied into the trainer first)."""
        tr_ = self._hip_spark_trainer
        live = tr_.state_dict()
        was, changed = getattr(self, "_aliased", False), False
        for k, prm in self.model.named_parameters():
            view = live[k]
            if prm.data_ptr() != view.data_ptr():
                if was:
                    view.copy_(prm.data.detach().to(view.device, view.dtype))
                    changed = True
                prm.data = view
        for k, buf in list(self.model.named_buffers()):
            if k not in live:
                continue
            view = live[k]
            if buf.data_ptr() != view.data_ptr():
                if was:
                    view.copy_(buf.detach().to(view.device, view.dtype))
                node, leaf = self.model, k
                *parts, leaf = k.split(".")
                for part in parts:
                    node = node._modules[part]
                node._buffers[leaf] = view
        versions = tuple(p._version for p in self.model.parameters())
        if was and (changed or versions != self._param_versions):
            tr_.parameters_changed()                # load_state_dict / a repaired alias wrote the flat buffers: the weight images follow
        self._aliased, self._param_versions = True, versions

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict=strict)
        if self._hip_spark_trainer is not None:
            self._alias()
        return out

    # ------------------------------------------------------------------ reference src/models/Spark_2D.py
    def _run(self, x, training):
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.input_size or x.shape[3] != self.input_size:
            raise ValueError(f"Spark_2D: expected [B, 1, {self.input_size}, {self.input_size}] slices, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("Spark_2D runs on the HIP operators: the input must be on the GPU (there is no CPU path)")
        tr_ = self.hip_trainer(x.device)
        active = draw_mask(x.shape[0], self.fmap_size, self.len_keep)              # host, default generator: SparK_2D.mask
        self.last_active = active
        with torch.autocast("cuda", enabled=False):
            out = tr_.forward(x, active, training=training)
        if training:
            for k, buf in self.model.named_buffers():
                if k.endswith("num_batches_tracked"):
                    buf += 1
            self._param_versions = tuple(p._version for p in self.model.parameters())
        return out

    def forward(self, x):
        """-> loss, reco [B,1,H,W], latent [B,2048] (reference :26-32); batch statistics in train() mode, running statistics in eval()"""
        return self._run(x, self.training)

    def _log(self, name, value, batch_size):
        self.logged[name] = value.detach()
        if hasattr(self, "log") and _Base is not nn.Module:
            try:
                self.log(name, value, prog_bar=False, on_step=False, on_epoch=True, batch_size=batch_size, sync_dist=True)
            except Exception:
                pass

    @staticmethod
    def _input(batch):
        v = batch["vol"]
        v = v["data"] if isinstance(v, dict) else v          # torchio's DATA key
        return v.squeeze(-1)

    def training_step(self, batch, batch_idx: int):
        """reference :34-41, with the backward pass and the AdamW update that Lightning's automatic optimisation does there"""
        input = self._input(batch)
        loss, _reco, _latent = self._run(input, True)
        tr_ = self._hip_spark_trainer
        tr_.backward()
        tr_.adamw_step(lr=float(self.cfg.lr), weight_decay=float(_cfg_get(self.cfg, "weight_decay", 0.05)), betas=(0.9, 0.95))
        self._param_versions = tuple(p._version for p in self.model.parameters())
        self._log(f"{self.prefix}train/Loss_comb", loss, input.shape[0])
        if tr_.loss_scaling:
            HipMirror._watch_loss_scale(self, tr_, record=self.logged)
        return {"loss": loss}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int):
        """reference :45-50; Lightning validates in eval() mode: running statistics, no stochastic depth, a fresh mask"""
        input = self._input(batch)
        loss, _reco, _latent = self._run(input, False)
        self._log(f"{self.prefix}val/Loss_comb", loss, input.shape[0])
        return {"loss": loss}

    def test_step(self, batch, batch_idx: int):
        raise NotImplementedError("Spark_2D.test_step is not built: experiment=cDDPM/Spark_2D_pretrain sets test_after_training: False; "
                                  "evaluate the encoder through the DDPM_2D mirror that ingests this model's checkpoint")

    @property
    def automatic_optimization(self):        # training_step above steps the optimizer itself
        return False

    def configure_optimizers(self):
        return torch.optim.AdamW(self.parameters(), lr=self.cfg.lr, weight_decay=_cfg_get(self.cfg, "weight_decay", 0.05), betas=[0.9, 0.95])

    def update_prefix(self, prefix):
        self.prefix = prefix

    # ------------------------------------------------------------------ checkpoints: AdamW's state lives in the trainer
    def hip_optimizer_state(self):
        return None if self._hip_spark_trainer is None else {"spark": self._hip_spark_trainer.optimizer_state()}

    def load_hip_optimizer_state(self, state):
        st = dict(state["spark"])
        if self._hip_spark_trainer is not None:
            self._hip_spark_trainer.load_optimizer_state(st)
        else:
            self._pending_opt_state = st

    def on_save_checkpoint(self, checkpoint):
        st = self.hip_optimizer_state()
        if st is not None:
            checkpoint["hip_optimizer_state"] = {k: _to_cpu(v) for k, v in st.items()}

    def on_load_checkpoint(self, checkpoint):
        """restores hip_optimizer_state (AdamW's moments, the step count, the loss scaler); a checkpoint without it but with Lightning 1.5's
        `native_amp_scaling_state` (a reference checkpoint trained at precision 16: GradScaler.state_dict()) seeds the scale and growth
        tracker of a precision-16 trainer"""
        st = checkpoint.get("hip_optimizer_state")
        if st is not None:
            self.load_hip_optimizer_state(st)
        elif checkpoint.get("native_amp_scaling_state"):
            from .training import loss_scaling_from_grad_scaler
            self._pending_amp_scaler = loss_scaling_from_grad_scaler(checkpoint["native_amp_scaling_state"])
            self._seed_loss_scaling()

    def _seed_loss_scaling(self):
        """a seed from a reference checkpoint restarts the scaler of a precision-16 trainer (now, or once the trainer exists); at 32 it
        is dropped: there the scaler is off, as a precision-32 Lightning run has none"""
        tr_, seed = self._hip_spark_trainer, getattr(self, "_pending_amp_scaler", None)
        if tr_ is None or seed is None:
            return
        self._pending_amp_scaler = None
        if tr_.precision == 16:
            tr_.enable_loss_scaling(**seed)
