"""Host-side mirror of the reference LightningModule of the patched DDPM (reference src/models/DDPM_2D_patched.py): the Hydra target
`src.models.DDPM_2D_patched.DDPM_2D` of `experiment=cDDPM/DDPM_patched`, the pDDPM baseline.

An unconditioned UNet (num_classes=None) is trained to denoise ONE box per slice -- the rest of the slice stays clean context --
and evaluated by reconstructing every box of a grid and stitching the reconstructions. Kept from the reference: the constructor
`DDPM_2D(cfg, prefix=None)` with its cfg keys and defaults (:22-65; `attention_resolutions` is its formula imageDim[0] / 32, / 16,
/ 8, floats that name a level only at small imageDim; `use_checkpoint=True` is accepted and ignored), `.diffusion`, `.boxes`,
`forward() -> None`, the box choice of training_step / validation_step (:83-91: a random cell of the grid under `grid_boxes`, else
sample_single_box), test_step's slice selection, bookkeeping and volume re-assembly, `configure_optimizers`, `update_prefix`.

On the HIP path: training_step runs `training.training_step(..., box=, inpaint=)` under manual optimisation (the box is noised by
cddpm_box_q_sample, the loss is cddpm_op_loss_box); test_step does the reference's K-box loop (:185-215) as ONE
`GaussianDiffusion.p_losses_grid` call: batched UNet forwards over all K D (box, slice) pairs and one stitching launch. What the two
mirrors share (trainer aliasing, checkpoint hooks, precision, loss-scale logging, evaluation bookkeeping) is mirror_common.HipMirror.
The cfg keys `conv_family`, `conv_fallback`, `eval_precision`, `train_attention_precision`, `attention_family` and
`train_attention_family` (absent in the reference; unset = nothing changes) mean what they mean in DDPM_2D.py: `eval_precision: 16` evaluates (test_step, validation_step) with plain fp16 operands in the
UNet's engine; `train_attention_precision: 16` trains the attention cores on the fp16-MFMA kernels. `evalHausdorff: true` reaches the
standalone metric pass with the rest of the cfg, like `evalSeg`: HausPerVol gets the device Hausdorff distance instead of NaN.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .DDPM_2D import DDPM_2D as _CondMirror
from .OpenAI_Unet import UNetModel as OpenAI_UNet
from .cond_DDPM import GaussianDiffusion
from .engine import attention_family_code
from .mirror_common import AttrDict, HipMirror, _Base, _cfg_get
from .patch_sampling import BoxSampler


class DDPM_2D(HipMirror, _Base):
    def __init__(self, cfg, prefix=None):
        super().__init__()
        if isinstance(cfg, dict) and not isinstance(cfg, AttrDict):
            cfg = AttrDict(cfg)
        self.cfg = cfg
        size = (int(cfg["imageDim"][0] / cfg["rescaleFactor"]), int(cfg["imageDim"][1] / cfg["rescaleFactor"]))
        # the reference's formula (:28): floats. One that is no integer (imageDim[0] = 100 -> 3.125) matches no level (`ds in
        # attention_resolutions`); the engine and the trainer take integers, so it becomes 0, which no level has either
        dim0 = int(cfg["imageDim"][0])
        att = tuple(int(a) if float(a).is_integer() else 0 for a in (dim0 / 32, dim0 / 16, dim0 / 8))
        model = OpenAI_UNet(
            image_size=size, in_channels=1, model_channels=_cfg_get(cfg, "unet_dim", 64), out_channels=1,
            num_res_blocks=_cfg_get(cfg, "num_res_blocks", 3), attention_resolutions=att,
            dropout=_cfg_get(cfg, "dropout_unet", 0), channel_mult=_cfg_get(cfg, "dim_mults", [1, 2, 4, 8]),
            conv_resample=True, dims=2, num_classes=None, use_checkpoint=True, use_fp16=True, num_heads=_cfg_get(cfg, "num_heads", 1),
            num_head_channels=64, num_heads_upsample=-1, use_scale_shift_norm=True, resblock_updown=True,
            use_new_attention_order=True, use_spatial_transformer=False, transformer_depth=1)
        model.convert_to_fp16()
        model._hip.configure(_cfg_get(cfg, "conv_family", None), _cfg_get(cfg, "conv_fallback", None), _cfg_get(cfg, "eval_precision", None),
                             _cfg_get(cfg, "attention_family", None))
        attention_family_code(_cfg_get(cfg, "train_attention_family", "f32"))      # a bad value: ValueError here, before any device
        timesteps = _cfg_get(cfg, "timesteps", 1000)
        self.test_timesteps = _cfg_get(cfg, "test_timesteps", 150)
        self.diffusion = GaussianDiffusion(
            model, image_size=size, timesteps=timesteps, sampling_timesteps=_cfg_get(cfg, "sampling_timesteps", self.test_timesteps),
            objective=_cfg_get(cfg, "objective", "pred_x0"), channels=1, loss_type=_cfg_get(cfg, "loss", "l1"),
            p2_loss_weight_gamma=_cfg_get(cfg, "p2_gamma", 0), inpaint=bool(_cfg_get(cfg, "inpaint", False)), cfg=cfg)
        self.boxes = BoxSampler(cfg)
        self.prefix = prefix
        if hasattr(self, "save_hyperparameters") and _Base is not nn.Module:
            try:
                self.save_hyperparameters()
            except Exception:
                pass

    def forward(self):
        return None

    _gen_noise = _CondMirror._gen_noise          # gen_noise(cfg) as a device simplex field, or None when cfg.noisetype is unset

    def _pick_boxes(self, input):
        """reference :83-91: under `grid_boxes` one cell of the grid per slice (sample_grid, then ONE randint call over the cells),
        else sample_single_box; [B,4,1] either way"""
        if _cfg_get(self.cfg, "grid_boxes", False):
            grid = self.boxes.sample_grid(input)
            ind = torch.randint(0, grid.shape[1], (input.shape[0],))
            return grid[torch.arange(input.shape[0]), ind].unsqueeze(-1)
        return self.boxes.sample_single_box(input)

    def training_step(self, batch, batch_idx: int):
        """One optimisation step of the reference's training_step (:76-102): a box per slice, `gen_noise` or Gaussian noise, the box
        loss at a random t per slice -- gradient, data-parallel all-reduce and Adam(lr = cfg.lr) on the HIP operators, as the cDDPM
        mirror does (manual optimisation: there is no autograd graph to hand back)."""
        from . import training as _training
        prec = self._train_precision()
        bits = _training.set_precision(prec) if prec is not None else _training.get_precision()
        input = batch["vol"]["data"].squeeze(-1).float()
        dev = input.device
        trainer = self.hip_trainer(dev)
        self._alias_unet()
        self._loss_scaling(trainer, bits)
        bbox = self._pick_boxes(input)
        noise = self._gen_noise(input.shape, dev, engine=trainer.eng)
        if noise is None:
            noise = torch.randn_like(input)
        d = self.diffusion
        t = torch.randint(0, d.num_timesteps, (input.shape[0],), device=dev).long()
        ddp = torch.distributed.is_available() and torch.distributed.is_initialized()
        slice0 = torch.distributed.get_rank() * input.shape[0] if ddp else 0
        loss = _training.training_step(trainer, input, None, t=t, noise=noise.float(), timesteps=d.num_timesteps, slice0=slice0,
                                       objective=d.objective, loss_type=d.loss_type, all_reduce=ddp, lr=_cfg_get(self.cfg, "lr", 1e-4),
                                       buffers={k: getattr(d, k) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                                                                           "p2_loss_weight")},
                                       box=bbox, inpaint=d.inpaint)
        d.model._hip.invalidate()
        if trainer.loss_scaling:
            self._watch_loss_scale(trainer)
        if hasattr(self, "log") and _Base is not nn.Module:
            try:
                self.log(f"{self.prefix}train/Loss", loss, prog_bar=False, on_step=False, on_epoch=True, batch_size=input.shape[0], sync_dist=True)
            except Exception:
                pass
        return {"loss": loss.detach()}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int):
        """reference :104-127: the training loss on a validation batch, forward only"""
        input = batch["vol"]["data"].squeeze(-1).float()
        bbox = self._pick_boxes(input)
        noise = self._gen_noise(input.shape, input.device)
        with torch.autocast("cuda", enabled=False):
            loss, _reco = self.diffusion(input, box=bbox, noise=noise)
        if hasattr(self, "log") and _Base is not nn.Module:
            try:
                self.log(f"{self.prefix}val/Loss_comb", loss, prog_bar=False, on_step=False, on_epoch=True, batch_size=input.shape[0], sync_dist=True)
            except Exception:
                pass
        return {"loss": loss}

    @torch.no_grad()
    def test_step(self, batch, batch_idx: int):
        """The evaluation call of the reference (:139-248): the `num_eval_slices` centre slices when that key is set (:154-163), depth to
        the batch axis, the grid of boxes, ONE noise field for all boxes, then every box reconstructed at t = test_timesteps - 1 and
        stitched (`overlap` / `agg_overlap` = 'cut' | 'avg') -- here one p_losses_grid call --, the volume re-assembled as
        [1,1,H,W,D], the bookkeeping of :219-241 and `_test_step` (the reference's when its tree is importable, else the package's
        device metric pass) when the batch carries its inputs and on_test_start ran. Returns the tensors either way."""
        def data_of(key):
            v = batch.get(key) if hasattr(batch, "get") else None
            if v is None:
                return None
            return v["data"] if isinstance(v, dict) else v

        def field(key, default=None):
            return batch.get(key, default) if hasattr(batch, "get") else default

        self.dataset = field("Dataset")
        self.stage = field("stage")
        input = data_of("vol")                                              # [1,1,H,W,D]
        data_orig, data_seg, data_mask = data_of("vol_orig"), data_of("seg_orig"), data_of("mask_orig")
        if data_orig is not None and (data_seg is None or not field("seg_available", data_seg is not None)):
            data_seg = torch.zeros_like(data_orig)
        D = input.size(4)
        num_slices = _cfg_get(self.cfg, "num_eval_slices", D)
        ind_offset = 0
        if num_slices != D:
            start_slice = int((D - num_slices) / 2)
            sl = slice(start_slice, start_slice + num_slices)
            input = input[..., sl]
            data_orig = data_orig[..., sl] if data_orig is not None else None
            data_seg = data_seg[..., sl] if data_seg is not None else None
            data_mask = data_mask[..., sl] if data_mask is not None else None
            ind_offset = start_slice
        assert input.shape[0] == 1, "Batch size must be 1"
        input = input.squeeze(0).permute(3, 0, 1, 2).contiguous().float()   # [D,1,H,W]
        bbox = self.boxes.sample_grid(input)
        overlap = bool(_cfg_get(self.cfg, "overlap", False))
        agg = _cfg_get(self.cfg, "agg_overlap", "cut")
        stitch = "paste" if not overlap else agg
        if stitch not in ("paste", "cut", "avg"):
            # the reference pastes nothing for any other value and returns zeros: an error here
            raise ValueError(f"agg_overlap must be 'cut' or 'avg', got {agg!r}")
        noise = self._gen_noise(input.shape, input.device)
        d = self.diffusion
        t = torch.full((input.shape[0],), int(self.test_timesteps) - 1, device=input.device, dtype=torch.long)
        with torch.autocast("cuda", enabled=False):
            loss_diff, reco = d.p_losses_grid(input * 2 - 1, t, bbox, None if noise is None else noise.float(), stitch=stitch,
                                              cut=self.boxes.sample_grid_cut(input) if stitch == "cut" else None,
                                              chunk=int(_cfg_get(self.cfg, "eval_chunk", 64)))
        final_volume = reco.clone().squeeze().permute(1, 2, 0).unsqueeze(0).unsqueeze(0)
        out = {"loss": loss_diff, "final_volume": final_volume, "input": input, "boxes": bbox, "ind_offset": ind_offset}
        if hasattr(self, "eval_dict"):
            self._record_volume_scores(None, input, loss_diff)
        if data_orig is not None and data_mask is not None and hasattr(self, "eval_dict"):
            try:
                from src.utils.utils_eval import _test_step  # type: ignore  (reference tree on sys.path)
            except ImportError:
                from .utils_eval import _test_step
            _test_step(self, final_volume, data_orig, data_seg, data_mask, batch_idx, field("ID"), field("label"))
        return out
