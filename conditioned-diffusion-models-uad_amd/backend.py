"""Glue between the host-side mirrors (OpenAI_Unet.UNetModel, cond_DDPM.GaussianDiffusion) and the HIP engine.

A UNetModel owns one HipBackend. The backend (re)creates the CddpmEngine when the device, the capacity
(batch / image size), the weights (load_state_dict, .to()) or the schedule change, so user code keeps the
reference's workflow: build modules, load a checkpoint, move to the GPU, call forward / p_sample_loop.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import schedule as _schedule
from .engine import EXACT_FAMILIES, CddpmEngine, attention_family_code, conv_family_code, precision_bits


class HipBackend:
    def __init__(self, unet):
        self._unet_desc = dict(
            model_channels=unet.model_channels, channel_mult=tuple(unet.channel_mult),
            num_res_blocks=unet.num_res_blocks, attention_resolutions=tuple(unet.attention_resolutions),
            head_channels=unet.num_head_channels, cond_dim=unet.num_classes or 0,
            in_channels=unet.in_channels, out_channels=unet.out_channels)
        self.timesteps = 1000
        self.objective = "pred_x0"
        self.buffers: Optional[Dict[str, torch.Tensor]] = None
        self.engine: Optional[CddpmEngine] = None
        self._key = None
        self._sched_key = None
        self.conv_family: Optional[str] = None       # None: the process default (CDDPM_CONV, else h3)
        self.conv_fallback: Optional[str] = None     # None: off; 'x6' / 'f32': re-run slices that left the fp16 range there
        self._fallback_engine: Optional[CddpmEngine] = None
        self.eval_precision: int = 32                # 16: the engine evaluates in the reference's `precision: 16` arithmetic
        self.attention_family: Optional[str] = None  # None: exact fp32 attention; 'h3': fp32-grade fp16 splits (at eval_precision 32)

    def configure(self, conv_family: Optional[str] = None, conv_fallback: Optional[str] = None, eval_precision=None,
                  attention_family: Optional[str] = None):
        """the engine's convolution family, the exact family non-finite slices are re-run in, the engine's precision and its
        attention family (DDPM_2D: cfg.conv_family, cfg.conv_fallback, cfg.eval_precision, cfg.attention_family); all default to unset
        = the behaviour without them. eval_precision 16 with an exact conv_family is a ValueError: only the h3 family has it. A
        fallback engine keeps exact fp32 attention."""
        bits = 32 if eval_precision is None else precision_bits(eval_precision)
        if attention_family is not None:
            attention_family_code(attention_family)
        if attention_family != self.attention_family:
            self.attention_family = attention_family
            self.close()
        if bits == 16 and conv_family is not None and conv_family_code(conv_family) != conv_family_code("h3"):
            raise ValueError(f"eval_precision 16 needs the h3 convolution family, got conv_family={conv_family!r}")
        if bits != self.eval_precision:
            self.eval_precision = bits
            self.close()
        if conv_family is not None:
            conv_family_code(conv_family)
        if conv_fallback is not None:
            conv_family_code(conv_fallback)
            if conv_fallback not in EXACT_FAMILIES:
                raise ValueError(f"conv_fallback must be an exact family ({' or '.join(EXACT_FAMILIES)}), got {conv_fallback!r}")
        if (conv_family, conv_fallback) != (self.conv_family, self.conv_fallback):
            self.conv_family, self.conv_fallback = conv_family, conv_fallback
            self.close()

    # the diffusion wrapper registers its schedule here; a bare UNetModel uses the default cosine one
    def set_schedule(self, buffers: Dict[str, torch.Tensor], objective: str):
        self.buffers = {k: v.detach().cpu() for k, v in buffers.items()}
        self.timesteps = int(self.buffers["betas"].shape[0])
        self.objective = objective
        self._sched_key = None

    @staticmethod
    def _weights_key(unet):
        return tuple((p.data_ptr(), p._version) for p in unet.parameters())

    def get(self, unet, B: int, H: int, W: int, device: torch.device) -> CddpmEngine:
        if device.type != "cuda":
            raise RuntimeError(f"the cDDPM HIP path runs on an MI355X only; tensors are on {device}. "
                               "There is no CPU fallback (use the reference, or oracle/ in tests).")
        wkey = self._weights_key(unet)
        e = self.engine
        need = (e is None or e.device != device or e.timesteps != self.timesteps or B > e.max_batch
                or H * W > e.max_h * e.max_w or H > e.max_h or W > e.max_w or wkey != self._key)
        if need:
            if e is not None:
                e.close()
            self._close_fallback()                   # same geometry, weights and schedule as the main engine, or none
            max_b = max(B, e.max_batch if e is not None else 1)
            max_h = max(H, e.max_h if e is not None else 0)
            max_w = max(W, e.max_w if e is not None else 0)
            e = CddpmEngine(timesteps=self.timesteps, max_batch=max_b, max_h=max_h, max_w=max_w, device=device,
                            conv_family=self.conv_family, precision=self.eval_precision, attention_family=self.attention_family,
                            **self._unet_desc)
            e.load_weights(unet.state_dict())
            self.engine, self._key, self._sched_key = e, wkey, None
        skey = (id(self.buffers), self.objective)
        if self._sched_key != skey:
            bufs = self.buffers if self.buffers is not None else _schedule.schedule_buffers(self.timesteps)
            e.set_schedule(bufs, self.objective)
            self._sched_key = skey
            self._close_fallback()
        return e

    def fallback(self, unet):
        """what the engine's `fallback=` argument takes: None when cfg.conv_fallback is unset, else a callable that creates the
        fallback engine on the first flagged slice -- the main engine's geometry, weights and schedule in the exact family --
        and returns the same one until the main engine is rebuilt"""
        if self.conv_fallback is None:
            return None

        def make() -> CddpmEngine:
            e = self.engine
            if e is None:
                raise RuntimeError("no main engine yet: the fallback engine mirrors it")
            if self._fallback_engine is None:
                fb = CddpmEngine(timesteps=e.timesteps, max_batch=e.max_batch, max_h=e.max_h, max_w=e.max_w, device=e.device,
                                 conv_family=self.conv_fallback, **self._unet_desc)
                fb.load_weights(unet.state_dict())
                fb.set_schedule(self.buffers if self.buffers is not None else _schedule.schedule_buffers(self.timesteps), self.objective)
                self._fallback_engine = fb
            return self._fallback_engine
        return make

    def _close_fallback(self):
        if self._fallback_engine is not None:
            self._fallback_engine.close()
            self._fallback_engine = None

    def invalidate(self):
        """the parameters were updated outside torch's version counters (the training step's Adam kernel writes them in place): the next
        `get` re-packs the inference engine's weights"""
        self._key = None

    def close(self):
        self._close_fallback()
        if self.engine is not None:
            self.engine.close()
            self.engine = None
