"""What the LightningModule mirrors of this package share (DDPM_2D.py, DDPM_2D_patched.py): the cfg stand-in, the Lightning base class
when it is installed, and `HipMirror` -- the UNet's training state on the HIP operators with its parameter aliasing, the checkpoint
hooks that carry Adam's state, precision selection, loss-scale logging, the evaluation bookkeeping and the optimizer stub of manual
optimisation. A mirror derives from (HipMirror, _Base) and sets `self.cfg`, `self.diffusion`, `self.prefix`."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

try:  # Lightning 1.5 path first (what the reference pins), then 2.x, then a plain Module
    from pytorch_lightning.core.lightning import LightningModule as _Base  # type: ignore
except Exception:  # pragma: no cover - depends on the environment
    try:
        from pytorch_lightning import LightningModule as _Base  # type: ignore
    except Exception:
        _Base = nn.Module


class AttrDict(dict):
    """cfg stand-in when omegaconf is absent: cfg.key, cfg['key'], cfg.get(key, default)"""
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


def _cfg_get(cfg, key, default=None):
    try:
        v = cfg.get(key, default)
    except AttributeError:
        v = getattr(cfg, key, default)
    return default if v is None else v


def _to_cpu(state):
    """a checkpoint entry with its tensors on the host (nested dicts included)"""
    if torch.is_tensor(state):
        return state.cpu()
    if isinstance(state, dict):
        return {k: _to_cpu(v) for k, v in state.items()}
    return state


class HipMirror:
    SCALER_CHECK_EVERY = 50      # training steps between two read-backs of the loss scaler's consecutive skips
    SCALER_STALL_SKIPS = 30      # that many skips in a row: warn once

    def _record_volume_scores(self, features, input, loss_diff):
        """the per-volume bookkeeping the reference's test_step does before `_test_step` (:216-220, :249-254, :258-271): the mean context
        vector of the volume, the L1 reconstruction loss as the three anomaly scores; `_test_end` / `calc_thresh` read these lists"""
        import numpy as np
        ed = self.eval_dict
        if _cfg_get(self.cfg, "condition", True) and features is not None:
            latent = [features.mean(0).squeeze().detach().cpu()]
        else:
            latent = [torch.tensor([0], dtype=float).repeat(input.shape[0])]
        self.latentSpace_slice.extend(latent)
        ed.setdefault("latentSpace", []).append(torch.mean(torch.stack(latent), 0))
        score = float(np.mean([loss_diff.detach().cpu()]))          # AnomalyScoreReg = AnomalyScoreReco = AnomalyScoreComb = loss_diff
        ed.setdefault("AnomalyScoreRegPerVol", []).append(score)
        if not _cfg_get(self.cfg, "use_postprocessed_score", True):
            ed.setdefault("AnomalyScoreRecoPerVol", []).append(score)
            ed.setdefault("AnomalyScoreCombPerVol", []).append(score)
            ed.setdefault("AnomalyScoreCombiPerVol", []).append(score * score)
            ed.setdefault("AnomalyScoreCombPriorPerVol", []).append(score + _cfg_get(self.cfg, "beta", 0) * 0)
            ed.setdefault("AnomalyScoreCombiPriorPerVol", []).append(score * 0)

    def on_test_start(self):
        """reference :156-170: the bookkeeping `_test_step` / `_test_end` of the reference's evaluation write into. Inside the reference
        tree its own metric code (src/utils/utils_eval.py: sklearn / monai / skimage) is used; standalone, the package's device metric
        pass (utils_eval.py) with the same eval_dict keys."""
        try:
            from src.utils.utils_eval import get_eval_dictionary  # type: ignore  (reference tree on sys.path)
        except ImportError:       # standalone: the package's native metric pass (utils_eval.py); a BROKEN reference install still raises
            from .utils_eval import get_eval_dictionary
        self.eval_dict = get_eval_dictionary()
        self.inds, self.latentSpace_slice, self.diffs_list, self.seg_list = [], [], [], []
        self.new_size = [160, 190, 160]
        if not hasattr(self, "threshold"):
            self.threshold = {}

    def on_test_end(self):
        """reference :288-291: `_test_end(self)` of the reference's utils_eval when it is importable, the package's native one otherwise"""
        try:
            from src.utils.utils_eval import _test_end  # type: ignore
        except ImportError:
            from .utils_eval import _test_end
        _test_end(self)

    def hip_trainer(self, device):
        """the UNet's training state on the HIP operators (training.UNetTrainer). From here on the UNet module's parameters ARE views of
        the trainer's flat buffer: state_dict() / checkpoints see the trained values, and the evaluation path re-packs them on its next call."""
        if getattr(self, "_hip_unet_trainer", None) is None:
            from .training import UNetTrainer
            unet = self.diffusion.model
            self._hip_unet_trainer = UNetTrainer({k: v for k, v in unet.state_dict().items()}, model_channels=unet.model_channels,
                                        channel_mult=tuple(unet.channel_mult), num_res_blocks=unet.num_res_blocks,
                                        cond_dim=unet.num_classes, device=device, dropout=float(unet.dropout or 0),       # cfg.dropout_unet
                                        attention_resolutions=tuple(unet.attention_resolutions),                         # cfg.att_res
                                        attention_precision=_cfg_get(self.cfg, "train_attention_precision", 32),
                                        attention_family=_cfg_get(self.cfg, "train_attention_family", "f32"))
            self._alias_unet()
            self._load_pending_optimizer_state()
        return self._hip_unet_trainer

    def _alias_unet(self):
        """the UNet module's parameters become (again) views of the trainer's flat buffer. `module.to()` / `.cpu()` / `.float()` /
        `.half()` silently replace `param.data` (Lightning's teardown calls `.cpu()`): before every step the alias is verified, and a broken
        one is repaired in the direction that loses nothing -- the module's current values are copied into the flat buffer first."""
        tr_, changed = self._hip_unet_trainer, False
        for k, prm in self.diffusion.model.named_parameters():
            view = tr_.p[k]
            if prm.data_ptr() != view.data_ptr() or prm.device != view.device or prm.dtype != view.dtype:
                if getattr(self, "_aliased", False):            # was aliased before: the module holds the values the user sees
                    view.copy_(prm.data.detach().to(view.device, view.dtype))
                    changed = True
                prm.data = view
        versions = tuple(prm._version for prm in self.diffusion.model.parameters())
        if getattr(self, "_aliased", False) and (changed or versions != self._param_versions):
            tr_.parameters_changed()          # load_state_dict / a repaired alias wrote the flat buffer: exponents + packed images follow
        self._aliased, self._param_versions = True, versions

    # ------------------------------------------------------------------ checkpoints: Adam's state lives in the trainers, not in torch.optim
    def hip_optimizer_state(self):
        """Adam moments + step count of the HIP trainers (None before the first training step)"""
        out = {}
        if getattr(self, "_hip_unet_trainer", None) is not None:
            out["unet"] = self._hip_unet_trainer.optimizer_state()
        if getattr(self, "_hip_enc_trainer", None) is not None:
            out["encoder"] = self._hip_enc_trainer.optimizer_state()
        return out or None

    def load_hip_optimizer_state(self, state):
        """restores what hip_optimizer_state returned; before the trainers exist it is kept and applied when they are created"""
        self._pending_opt_state = state
        self._load_pending_optimizer_state()

    def _load_pending_optimizer_state(self):
        st = getattr(self, "_pending_opt_state", None)
        if not st:
            return
        if "unet" in st and getattr(self, "_hip_unet_trainer", None) is not None:
            self._hip_unet_trainer.load_optimizer_state(st.pop("unet"))
        if "encoder" in st and getattr(self, "_hip_enc_trainer", None) is not None:
            self._hip_enc_trainer.load_optimizer_state(st.pop("encoder"))

    def on_save_checkpoint(self, checkpoint):
        """Lightning hook: `configure_optimizers` returns a torch Adam that is never stepped (manual optimisation on the HIP operators), so
        the checkpoint's `optimizer_states` is empty; the real Adam state (m, v, step count, the dynamic loss scaler -- what the
        reference's checkpoints carry in `optimizer_states` and `native_amp_scaling_state`) goes under its own key"""
        st = self.hip_optimizer_state()
        if st is not None:
            checkpoint["hip_optimizer_state"] = {k: _to_cpu(v) for k, v in st.items()}

    def on_load_checkpoint(self, checkpoint):
        """restores hip_optimizer_state; a checkpoint without it but with Lightning 1.5's native AMP scaler state (a reference checkpoint
        trained at precision 16: `native_amp_scaling_state` = GradScaler.state_dict()) seeds the loss scale and growth tracker of the
        dynamic loss scaling, applied when a precision-16 step turns it on"""
        st = checkpoint.get("hip_optimizer_state")
        if st is not None:
            self.load_hip_optimizer_state({k: dict(v) for k, v in st.items()})
        elif checkpoint.get("native_amp_scaling_state"):
            from .training import loss_scaling_from_grad_scaler
            self._pending_amp_scaler = loss_scaling_from_grad_scaler(checkpoint["native_amp_scaling_state"])

    def _loss_scaling(self, trainer, bits):
        """precision 16 (plain fp16 operands) trains under a dynamic loss scale, as Lightning's native AMP does with a GradScaler; at 32
        nothing changes. A seed from a reference checkpoint (on_load_checkpoint) restarts the scaler from its scale and growth tracker."""
        if bits != 16:
            return
        seed = getattr(self, "_pending_amp_scaler", None)
        self._pending_amp_scaler = None
        if seed is not None or not trainer.loss_scaling:
            trainer.enable_loss_scaling(**(seed or {}))

    def _watch_loss_scale(self, trainer, record=None):
        """logs the loss scale and the skipped steps (device tensors: no read-back here; `record`: a dict that takes the two values as
        well, whether or not there is a logger) and, every SCALER_CHECK_EVERY steps, reads the consecutive skips once:
        SCALER_STALL_SKIPS of them in a row mean the gradients are non-finite whatever the scale (a NaN input, a diverged run) -- one
        RuntimeWarning instead of a run that silently stops learning. Spark_2D, no HipMirror itself, calls it too (with `record`)."""
        log = self.log if hasattr(self, "log") and _Base is not nn.Module else None
        if log is not None or record is not None:
            try:
                values = {"train/loss_scale": trainer.loss_scale_tensor().clone(), "train/skipped_steps": trainer.ctrl[3].float()}
            except (AttributeError, TypeError):         # a trainer without the device blocks: nothing to log
                values = {}
            for name, value in values.items():
                if record is not None:
                    record[name] = value
                if log is not None:
                    try:
                        log(f"{self.prefix}{name}", value, on_step=True, on_epoch=False)
                    except Exception:
                        pass
        self._scaler_steps = getattr(self, "_scaler_steps", 0) + 1
        if self._scaler_steps % self.SCALER_CHECK_EVERY:
            return
        skips = trainer.consecutive_skips
        if skips < self.SCALER_STALL_SKIPS:
            self._scaler_warned = False
        elif not getattr(self, "_scaler_warned", False):
            self._scaler_warned = True
            warnings.warn(f"{skips} training steps in a row were skipped for non-finite gradients (loss scale now "
                          f"{trainer.loss_scale:g}): the gradients are not finite at any scale -- a NaN / inf input or a diverged run?",
                          RuntimeWarning, stacklevel=2)

    def _train_precision(self):
        """the Trainer's `precision` (the reference trains with 16: configs/trainer/default.yaml:7) or cfg.precision; None = leave the
        process default (CDDPM_TRAIN_PRECISION or fp32-grade)"""
        prec = _cfg_get(self.cfg, "precision", None)
        if prec is None:
            try:
                tr_ = getattr(self, "trainer", None)        # Lightning attaches it; a bare nn.Module base has none
            except Exception:
                tr_ = None
            prec = getattr(tr_, "precision", None) if tr_ is not None else None
        return prec

    def update_prefix(self, prefix):
        """reference :308"""
        self.prefix = prefix

    @property
    def automatic_optimization(self):        # Lightning: training_step above steps the optimizer itself
        return False

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=_cfg_get(self.cfg, "lr", 1e-4))
