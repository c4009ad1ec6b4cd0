"""Thin Python owner of one libcddpm_hip handle: PyTorch-ROCm tensors in, raw pointers out.

PyTorch is used for device memory, the current HIP stream and (elsewhere) torch.distributed only;
every FLOP of the path runs in csrc/*.hip through the C ABI of include/cddpm.h.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

OBJECTIVES = {"pred_x0": 0, "pred_noise": 1}
# convolution families of a handle, in the numbering of include/cddpm.h (cddpm_set_conv_family)
CONV_FAMILIES = {"h3": 2, "x6": 1, "f32": 0}
EXACT_FAMILIES = ("x6", "f32")      # no range limit on the activations: what a fallback engine must be


def conv_family_code(name: str) -> int:
    """'h3' / 'x6' / 'f32' -> the library's family number; anything else is a ValueError (no GPU needed)"""
    if not isinstance(name, str) or name not in CONV_FAMILIES:
        raise ValueError(f"unknown convolution family {name!r}: expected one of {', '.join(CONV_FAMILIES)}")
    return CONV_FAMILIES[name]


# attention families of a handle (cddpm_set_attention_family), in the same numbering: exact fp32 MFMA (what a handle starts with) or the
# fp32-grade three-term fp16 split. There is no x6 attention: 'x6' is refused, not mapped.
ATTENTION_FAMILIES = {"f32": 0, "h3": 2}


def attention_family_code(name) -> int:
    """'f32' / 'h3' -> the library's family number; anything else ('x6', None, 2) is a ValueError (no GPU needed)"""
    if not isinstance(name, str) or name not in ATTENTION_FAMILIES:
        raise ValueError(f"unknown attention family {name!r}: expected one of {', '.join(ATTENTION_FAMILIES)} (there is no x6 attention)")
    return ATTENTION_FAMILIES[name]


def _attention_symbol(stem: str, precision, family) -> str:
    """the C ABI symbol of an attention operator: precision 16 selects the p16 kernels whatever the family, as on a handle"""
    code = attention_family_code(family)
    return stem + ("_p16" if precision_bits(precision) == 16 else "_h3" if code == 2 else "")


# precision of a handle's reconstruction path (cddpm_set_precision): the spellings of Lightning's Trainer(precision=...) that mean
# fp16 autocast or full precision. There is no bf16 reconstruction: 'bf16' is refused, not mapped.
PRECISIONS = {16: 16, 32: 32, "16": 16, "16-mixed": 16, "32": 32}


def precision_bits(value) -> int:
    """16 / 32 / '16' / '16-mixed' / '32' -> 16 or 32; anything else (None, 8, 'bf16', '64', True) is a ValueError (no GPU needed)"""
    if isinstance(value, bool) or not isinstance(value, (int, str)) or value not in PRECISIONS:
        raise ValueError(f"unknown precision {value!r}: expected 32, 16, '32', '16' or '16-mixed' (there is no bf16 reconstruction)")
    return PRECISIONS[value]


def flagged_runs(flags: Sequence) -> List[Tuple[int, int]]:
    """Maximal contiguous runs [i, j) of truthy entries of a per-slice flag sequence: [0,1,1,0,1] -> [(1,3),(4,5)].
    Runs, not single slices, because the device Philox keys a slice's noise by slice0 + its position in the batch: a run
    re-submitted with slice0 + i draws what its slices drew in the whole batch."""
    runs, start = [], None
    for k, f in enumerate(flags):
        if f and start is None:
            start = k
        elif not f and start is not None:
            runs.append((start, k))
            start = None
    if start is not None:
        runs.append((start, len(flags)))
    return runs


def _stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def _check_dev(t: torch.Tensor, name: str, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on a HIP device (got {type(t).__name__} on "
                           f"{getattr(t, 'device', None)}); the HIP path has no CPU fallback")
    if t.device != device:
        raise RuntimeError(f"{name} lives on {t.device}, the engine on {device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype}); the path computes in fp32 only")
    return t.contiguous()


def box_rows(boxes, rows: Optional[int] = None) -> torch.Tensor:
    """The patched DDPM's boxes as an integer [rows, 4] tensor of (x0, y1, x2, y3), where they lie: accepts [rows,4], the reference's
    [rows,4,1] (sample_single_box) and [K,S,4] (flattened box-major), tensors or nested lists. A host tensor is checked for negative
    coordinates (Python slicing would wrap them around; the kernels clip at 0); a device tensor is taken as it is. No GPU needed."""
    b = boxes if isinstance(boxes, torch.Tensor) else torch.as_tensor(boxes)
    if b.dtype.is_floating_point or b.dtype == torch.bool:
        raise RuntimeError(f"boxes must be integers, got {b.dtype}")
    if b.dim() == 3 and b.shape[-1] == 1:
        b = b[..., 0]
    if b.dim() == 3 and b.shape[-1] == 4:
        b = b.reshape(-1, 4)
    if b.dim() != 2 or b.shape[1] != 4 or b.shape[0] < 1 or (rows is not None and b.shape[0] != rows):
        raise RuntimeError(f"boxes must be [{'N' if rows is None else rows}, 4] rows (x0, y1, x2, y3), got {tuple(boxes.shape) if hasattr(boxes, 'shape') else type(boxes).__name__}")
    if not b.is_cuda and int(b.min()) < 0:
        raise ValueError("box coordinates must not be negative")
    return b


def check_boxes(boxes, rows: Optional[int], device) -> torch.Tensor:
    """box_rows on the device as contiguous int32 (what the kernels read)"""
    return box_rows(boxes, rows).to(device, torch.int32).contiguous()


class CddpmEngine:
    """One device's packed UNet + schedule tables + workspace (cddpm_create .. cddpm_destroy)."""

    def __init__(self, *, model_channels=128, channel_mult=(1, 2, 2), num_res_blocks=3,
                 attention_resolutions=(3, 6, 12), head_channels=64, cond_dim=128, timesteps=1000,
                 max_batch=1, max_h=128, max_w=128, device=None, in_channels=1, out_channels=1, conv_family=None,
                 precision=None, attention_family=None):
        """conv_family: None (the process default: CDDPM_CONV, else h3), 'h3', 'x6' or 'f32' -- set on the handle before any
        weights are loaded. precision: None (32), 32, 16, '32', '16' or '16-mixed' -- see set_precision; 16 needs the h3 family.
        attention_family: None ('f32'), 'f32' or 'h3' -- see set_attention_family."""
        family = None if conv_family is None else conv_family_code(conv_family)
        attn_family = None if attention_family is None else attention_family_code(attention_family)
        bits = None if precision is None else precision_bits(precision)
        if bits == 16 and conv_family is not None and conv_family != "h3":
            raise ValueError(f"precision 16 needs the h3 convolution family, got conv_family={conv_family!r}")
        self.lib = _lib.load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the cDDPM HIP path needs an MI355X (gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        d = _lib.UnetDesc()
        d.in_channels, d.out_channels, d.model_channels = in_channels, out_channels, model_channels
        d.num_levels = len(channel_mult)
        for i, m in enumerate(channel_mult):
            d.channel_mult[i] = int(m)
        d.num_res_blocks = num_res_blocks
        d.num_attention_resolutions = len(attention_resolutions)
        for i, a in enumerate(attention_resolutions):
            d.attention_resolutions[i] = int(a)
        d.head_channels, d.cond_dim, d.timesteps = head_channels, int(cond_dim or 0), timesteps
        d.max_batch, d.max_h, d.max_w = max_batch, max_h, max_w
        self.desc = d
        self.timesteps = timesteps
        self.cond_dim = int(cond_dim or 0)
        self.max_batch, self.max_h, self.max_w = max_batch, max_h, max_w
        self._h = C.c_void_p()
        rc = self.lib.cddpm_create(C.byref(self._h), C.byref(d), self.device.index)
        if rc != 0:
            msg = self.lib.cddpm_last_error(None).decode()
            self._h = None
            raise RuntimeError(f"cddpm_create failed: {msg}")
        self._keep = []   # tensors whose pointers the library may still read (taps)
        if family is not None:
            self._ck(self.lib.cddpm_set_conv_family(self._h, family), "cddpm_set_conv_family")
        if bits is not None:
            self._ck(self.lib.cddpm_set_precision(self._h, bits), "cddpm_set_precision")
        if attn_family is not None:
            self._ck(self.lib.cddpm_set_attention_family(self._h, attn_family), "cddpm_set_attention_family")

    # ------------------------------------------------------------------ lifetime / errors
    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self.lib.cddpm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.lib.cddpm_last_error(self._h).decode()}")

    # ------------------------------------------------------------------ setup
    @property
    def conv_family(self) -> str:
        code = self.lib.cddpm_get_conv_family(self._h)
        return {v: k for k, v in CONV_FAMILIES.items()}[code]

    def set_conv_family(self, name: str):
        """Change the handle's convolution family. Packed weights belong to a family: after a change to a DIFFERENT family the
        caller must call load_weights (and set_schedule) again -- until then every forward / reverse call raises."""
        self._ck(self.lib.cddpm_set_conv_family(self._h, conv_family_code(name)), "cddpm_set_conv_family")

    @property
    def attention_family(self) -> str:
        code = self.lib.cddpm_get_attention_family(self._h)
        return {v: k for k, v in ATTENTION_FAMILIES.items()}[code]

    def set_attention_family(self, name: str):
        """Arithmetic of the attention blocks of this engine's forward / reverse calls at precision 32 (cddpm_set_attention_family).
        'f32': exact fp32 MFMA (the default). 'h3': fp32-grade products from two-term fp16 splits on the fp16 matrix pipe, with the
        h3 range contract (|q / 8|, |k|, |v| < 65504, else a non-finite slice). At precision 16 the engine runs the fp16 kernel
        whatever the family is. No weights are reloaded. Any other value raises ValueError before the library is called."""
        self._ck(self.lib.cddpm_set_attention_family(self._h, attention_family_code(name)), "cddpm_set_attention_family")

    @property
    def precision(self) -> int:
        return int(self.lib.cddpm_get_precision(self._h))

    def set_precision(self, value):
        """Arithmetic of this engine's forward / reverse calls (cddpm_set_precision). 32: fp32-grade products (the default). 16 (also
        '16', '16-mixed'; h3 engines only): what the reference evaluates with under `precision: 16` -- plain fp16 operands with fp32
        accumulation in the convolutions and the attention, everything else fp32; about the accuracy of fp16 autocast, the h3
        family's range limit (|activation| < 65504: `fallback=` re-runs the slices that leave it). No weights are reloaded. Any
        other value raises ValueError before the library is called."""
        bits = precision_bits(value)
        self._ck(self.lib.cddpm_set_precision(self._h, bits), "cddpm_set_precision")

    def weight_names(self):
        n = self.lib.cddpm_num_weights(self._h)
        return [(self.lib.cddpm_weight_name(self._h, i).decode(), int(self.lib.cddpm_weight_numel(self._h, i)))
                for i in range(n)]

    def load_weights(self, state_dict: Mapping[str, object], prefix: str = ""):
        """state_dict: reference names (optionally under `prefix`, e.g. 'diffusion.model.') -> tensor/ndarray."""
        names, arrs = [], []
        for name, _numel in self.weight_names():
            key = prefix + name
            if key not in state_dict:
                raise KeyError(f"state_dict has no '{key}'")
            v = state_dict[key]
            if isinstance(v, torch.Tensor):
                v = v.detach().to("cpu", torch.float32).contiguous().numpy()
            v = np.ascontiguousarray(v, dtype=np.float32)
            names.append(name.encode())
            arrs.append(v)
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        c_numels = (C.c_int64 * n)(*[a.size for a in arrs])
        self._ck(self.lib.cddpm_load_weights(self._h, c_names, c_ptrs, c_numels, n), "cddpm_load_weights")

    def set_schedule(self, buffers: Mapping[str, object], objective: str = "pred_x0"):
        """buffers: the GaussianDiffusion schedule buffers (host tensors/arrays of length T)."""
        def host(name):
            v = buffers[name]
            if isinstance(v, torch.Tensor):
                v = v.detach().to("cpu", torch.float32).numpy()
            return np.ascontiguousarray(v, dtype=np.float32)
        arrs = [host(k) for k in ("posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped",
                                  "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")]
        self._qs = (host("sqrt_alphas_cumprod"), host("sqrt_one_minus_alphas_cumprod"))
        T = arrs[0].shape[0]
        self._ck(self.lib.cddpm_set_schedule(self._h, *[a.ctypes.data for a in arrs], T, OBJECTIVES[objective]),
                 "cddpm_set_schedule")

    def prepare_cond(self, cond: Optional[torch.Tensor], B: int):
        if self.cond_dim > 0:
            cond = _check_dev(cond, "cond", self.device)
            if tuple(cond.shape) != (B, self.cond_dim):
                raise RuntimeError(f"cond must be [{B}, {self.cond_dim}], got {tuple(cond.shape)}")
            ptr = cond.data_ptr()
        else:
            ptr = None
        self._ck(self.lib.cddpm_prepare_cond(self._h, ptr, B, _stream_ptr(self.device)), "cddpm_prepare_cond")
        self._cond_keep = cond

    # ------------------------------------------------------------------ the path
    def unet_forward(self, x: torch.Tensor, t, cond: Optional[torch.Tensor] = None, *, fallback=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """UNetModel.forward: x [B,1,H,W] fp32 on device, t int or int tensor [B]; cond [B,cond_dim] or None
        to reuse the context of the previous prepare_cond. fallback: as in `reverse` (needs `cond` when the model is conditional:
        the fallback engine prepares the flagged slices' context itself). out: a contiguous fp32 tensor of x's shape on the device
        that receives the result (e.g. a slice of a larger buffer) instead of a new one."""
        if out is not None:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == self.device and out.dtype == torch.float32
                    and out.is_contiguous() and out.shape == x.shape):
                raise RuntimeError(f"out must be a contiguous float32 tensor of shape {tuple(x.shape)} on {self.device}")
        if fallback is not None:
            res = self._unet_forward_with_fallback(x, t, cond, fallback)
            return res if out is None else out.copy_(res)
        x = _check_dev(x, "x", self.device)
        B, c, H, W = x.shape
        if c != 1:
            raise RuntimeError("x must be [B,1,H,W]")
        if cond is not None or self.cond_dim == 0:
            self.prepare_cond(cond, B)
        if out is None:
            out = torch.empty_like(x)
        if isinstance(t, torch.Tensor):
            tt = self._t_tensor(t, B)
            rc = self.lib.cddpm_unet_forward(self._h, x.data_ptr(), tt.data_ptr(), 0, out.data_ptr(), B, H, W,
                                             _stream_ptr(self.device))
        else:
            rc = self.lib.cddpm_unet_forward(self._h, x.data_ptr(), None, int(t), out.data_ptr(), B, H, W,
                                             _stream_ptr(self.device))
        self._ck(rc, "cddpm_unet_forward")
        return out

    def _t_tensor(self, t: torch.Tensor, B: int) -> torch.Tensor:
        """per-sample timesteps index the device tables (time-embedding table, schedule buffers): range-checked here
        like the reference's `extract` would fail on an out-of-range gather (cond_DDPM.py:266-269)"""
        if t.numel() != B:
            raise RuntimeError("t must have B elements")
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= self.timesteps:
            raise IndexError(f"timestep indices must lie in [0, {self.timesteps}), got [{lo}, {hi}]")
        return t.to(self.device, torch.int32).contiguous()

    def reverse(self, x_T: torch.Tensor, cond: Optional[torch.Tensor], t_start: int, *, noise: Optional[torch.Tensor] = None,
                seed: int = 0, slice0: int = 0, fallback=None) -> torch.Tensor:
        """p_sample_loop from x_T: steps t_start-1 .. 0, returns the reconstruction in [0,1] (new tensor).
        noise: [t_start, B, 1, H, W] with z_t at index t (index 0 unused), or None for the device Philox.
        fallback: None, or an engine of an exact family ('x6' / 'f32') with this engine's geometry, weights and schedule (or a
        callable returning one, called on the first flagged slice): slices whose result is not finite -- an activation left the
        fp16 range of the h3 family -- are run again on it from their x_T, in contiguous runs, and scattered back; every other
        slice keeps the bits of the plain call. One warning names the count; a slice still not finite afterwards (a NaN in the
        input) raises FloatingPointError."""
        if fallback is not None:
            return self._reverse_with_fallback(x_T, cond, t_start, noise, seed, slice0, fallback)
        x = self.reverse_unchecked(x_T, cond, t_start, noise=noise, seed=seed, slice0=slice0)
        self._check_finite(x, "cddpm_reverse")
        return x

    # ------------------------------------------------------------------ per-slice fallback out of the fp16 range
    def slice_status(self, x: torch.Tensor) -> torch.Tensor:
        """int32 [B] on the device: 1 where slice b of x [B,1,H,W] holds an inf or a NaN, else 0 (cddpm_slice_status: one launch,
        no host synchronisation)"""
        x = _check_dev(x, "x", self.device)
        if x.dim() != 4 or x.shape[1] != 1:
            raise RuntimeError("x must be [B,1,H,W]")
        B, _c, H, W = x.shape
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        self._ck(self.lib.cddpm_slice_status(self._h, x.data_ptr(), B, H, W, status.data_ptr(), _stream_ptr(self.device)),
                 "cddpm_slice_status")
        return status

    def _fallback_engine(self, fallback) -> "CddpmEngine":
        fb = fallback() if callable(fallback) and not isinstance(fallback, CddpmEngine) else fallback
        if not isinstance(fb, CddpmEngine):
            raise RuntimeError(f"fallback must be a CddpmEngine (or a callable returning one), got {type(fb).__name__}")
        if fb.conv_family not in EXACT_FAMILIES:
            raise RuntimeError(f"the fallback engine must be of an exact convolution family ({' or '.join(EXACT_FAMILIES)}), "
                               f"got {fb.conv_family}")
        if (fb.max_batch, fb.max_h, fb.max_w, fb.timesteps) != (self.max_batch, self.max_h, self.max_w, self.timesteps):
            raise RuntimeError("the fallback engine must be created with the same geometry (the kernel plan is part of a slice's bits)")
        if fb.device != self.device:
            raise RuntimeError(f"the fallback engine lives on {fb.device}, this engine on {self.device}")
        return fb

    def _rerun_flagged(self, out: torch.Tensor, fallback, what: str, rerun: Callable[["CddpmEngine", int, int], torch.Tensor]):
        """the shared tail of the fallback paths: flags of `out` (B ints to the host), `rerun(engine, i, j)` for every flagged run,
        results scattered into `out`, one warning, and the existing error when a re-run slice is still not finite"""
        flags = self.slice_status(out).cpu().tolist()
        runs = flagged_runs(flags)
        if not runs:
            return out
        fb = self._fallback_engine(fallback)
        for i, j in runs:
            out[i:j] = rerun(fb, i, j)
        n = sum(j - i for i, j in runs)
        warnings.warn(f"{what}: {n} of {len(flags)} slices left the fp16 range of the {self.conv_family} convolution family and were "
                      f"run again in the {fb.conv_family} family (slices {', '.join(f'[{i}, {j})' for i, j in runs)})", RuntimeWarning,
                      stacklevel=4)
        still = [k for i, j in runs for k, f in zip(range(i, j), self.slice_status(out[i:j]).cpu().tolist()) if f]
        if still:
            raise FloatingPointError(f"{what}: slices {still} are still non-finite after the re-run in the exact {fb.conv_family} "
                                     "convolution family: the input or the weights hold non-finite values, not an fp16 overflow.")
        return out

    def _reverse_with_fallback(self, x_T, cond, t_start, noise, seed, slice0, fallback):
        x_T = _check_dev(x_T, "x_T", self.device)
        out = self.reverse_unchecked(x_T, cond, t_start, noise=noise, seed=seed, slice0=slice0)
        B, _c, H, W = x_T.shape
        nz = None if noise is None else _check_dev(noise, "noise", self.device).reshape(t_start, B, 1, H, W)

        def rerun(fb, i, j):
            return fb.reverse_unchecked(x_T[i:j], None if cond is None else cond[i:j].contiguous(), t_start,
                                        noise=None if nz is None else nz[:, i:j].contiguous(), seed=seed, slice0=slice0 + i)
        return self._rerun_flagged(out, fallback, "cddpm_reverse", rerun)

    def _unet_forward_with_fallback(self, x, t, cond, fallback):
        if cond is None and self.cond_dim > 0:
            raise RuntimeError("unet_forward(fallback=...) needs cond: the fallback engine prepares the flagged slices' context itself")
        x = _check_dev(x, "x", self.device)
        out = self.unet_forward(x, t, cond)

        def rerun(fb, i, j):
            return fb.unet_forward(x[i:j], t[i:j] if isinstance(t, torch.Tensor) else t, None if cond is None else cond[i:j].contiguous())
        return self._rerun_flagged(out, fallback, "cddpm_unet_forward", rerun)

    def reverse_unchecked(self, x_T: torch.Tensor, cond: Optional[torch.Tensor], t_start: int, *, noise: Optional[torch.Tensor] = None,
                          seed: int = 0, slice0: int = 0) -> torch.Tensor:
        """`reverse` without the final finiteness check (the fallback path reads per-slice flags instead)"""
        x = _check_dev(x_T, "x_T", self.device).clone()
        B, c, H, W = x.shape
        if c != 1:
            raise RuntimeError("x_T must be [B,1,H,W]")
        self.prepare_cond(cond, B)
        nptr = None
        if noise is not None:
            noise = _check_dev(noise, "noise", self.device)
            if noise.numel() != t_start * B * H * W:
                raise RuntimeError(f"noise must hold t_start*B*H*W = {t_start * B * H * W} values, got {noise.numel()}")
            nptr = noise.data_ptr()
        self._ck(self.lib.cddpm_reverse(self._h, x.data_ptr(), nptr, seed, slice0, t_start, B, H, W,
                                        _stream_ptr(self.device)), "cddpm_reverse")
        return x

    def reverse_two_streams(self, twin: "CddpmEngine", x_T: torch.Tensor, cond: Optional[torch.Tensor], t_start: int, *, seed: int = 0,
                            slice0: int = 0) -> torch.Tensor:
        """`reverse` for a SMALL batch as two half-batches on two streams: this engine runs the first half, `twin` (an engine created
        with the same geometry and loaded with the same weights and schedule: the same kernel plan, hence the same bits) the second,
        enqueued step by step in alternation, so that one half's small launches (GroupNorm finalizes, split-K combines, attention, the
        posterior step) run behind the other half's convolutions. Same result as `reverse`, bit for bit (slices are independent; noise is
        keyed by the global slice index); measured +4.3 % at B = 4, +2.4 % at B = 2, nothing from B = 8 on (tools/dual_stream_reverse.py).
        Device Philox noise only."""
        x = _check_dev(x_T, "x_T", self.device).clone()
        B, c, H, W = x.shape
        if c != 1 or B < 2:
            raise RuntimeError("reverse_two_streams needs x_T [B,1,H,W] with B >= 2")
        if (twin.max_batch, twin.max_h, twin.max_w, twin.timesteps) != (self.max_batch, self.max_h, self.max_w, self.timesteps):
            raise RuntimeError("the twin engine must be created with the same geometry (the kernel plan is part of a slice's bits)")
        h = (B + 1) // 2
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_two_streams", None) is None:
            self._two_streams = (torch.cuda.Stream(self.device), torch.cuda.Stream(self.device))
        halves = [(self, self._two_streams[0], x[:h], None if cond is None else cond[:h].contiguous(), slice0),
                  (twin, self._two_streams[1], x[h:], None if cond is None else cond[h:].contiguous(), slice0 + h)]
        for e, s, xs, cs, _s0 in halves:
            s.wait_stream(main)
            with torch.cuda.stream(s):
                e.prepare_cond(cs, xs.shape[0])
        for t in range(t_start - 1, -1, -1):
            for e, s, xs, _cs, s0 in halves:
                with torch.cuda.stream(s):
                    e.reverse_range_(xs, t, t, seed=seed, slice0=s0)
        for _e, s, _xs, _cs, _s0 in halves:
            main.wait_stream(s)
        self._check_finite(x, "reverse_two_streams")
        return x

    def reverse_range_(self, x: torch.Tensor, t_hi: int, t_lo: int, *, noise: Optional[torch.Tensor] = None, seed: int = 0,
                       slice0: int = 0) -> torch.Tensor:
        """steps t_hi .. t_lo of the chain IN PLACE on a device tensor (context from the last prepare_cond); the result is
        mapped to [0,1] exactly when t_lo == 0 (cddpm_reverse_range). No host synchronisation: the caller checks the
        final reconstruction (`check_finite`)."""
        x = _check_dev(x, "x", self.device)
        B, _c, H, W = x.shape
        nptr = _check_dev(noise, "noise", self.device).data_ptr() if noise is not None else None
        self._ck(self.lib.cddpm_reverse_range(self._h, x.data_ptr(), nptr, seed, slice0, int(t_hi), int(t_lo), B, H, W,
                                              _stream_ptr(self.device)), "cddpm_reverse_range")
        return x

    def check_finite(self, x: torch.Tensor, what: str = "reconstruction"):
        self._check_finite(x, what)

    @staticmethod
    def _check_finite(x: torch.Tensor, what: str):
        """A non-finite reconstruction is an error, not a result. The default convolution family carries fp32 products on
        the fp16 matrix pipe and needs |activation| < 65504; a model that exceeds it overflows to
        inf/NaN, which the posterior step propagates like torch.clamp does. One reduction + sync per reconstruction."""
        if not bool(torch.isfinite(x).all().item()):
            raise FloatingPointError(f"{what}: non-finite values in the result. If the weights are sane, an activation left the "
                                     "fp16 range of the default convolution family: rerun with CDDPM_CONV=x6 (exact bf16 split, "
                                     "no range limit) or CDDPM_CONV=f32.")

    def p_sample(self, x: torch.Tensor, t: int, cond: Optional[torch.Tensor] = None, *, z: Optional[torch.Tensor] = None,
                 seed: int = 0, slice0: int = 0) -> torch.Tensor:
        """one reverse step x_t -> x_{t-1} (values stay in [-1,1]); cond None reuses the prepared context."""
        x = _check_dev(x, "x", self.device).clone()
        B, _c, H, W = x.shape
        if cond is not None or self.cond_dim == 0:
            self.prepare_cond(cond, B)
        zp = _check_dev(z, "z", self.device).data_ptr() if z is not None else None
        self._ck(self.lib.cddpm_p_sample(self._h, x.data_ptr(), zp, seed, slice0, int(t), B, H, W,
                                         _stream_ptr(self.device)), "cddpm_p_sample")
        return x

    def ddim_step(self, x: torch.Tensor, t: int, coef_x0: float, coef_eps: float, sigma: float, *, add_noise: bool,
                  finalize: bool = False, z: Optional[torch.Tensor] = None, seed: int = 0, slice0: int = 0) -> torch.Tensor:
        """one DDIM update in place on a device tensor (context from the last prepare_cond); see cddpm_ddim_step"""
        x = _check_dev(x, "x", self.device)
        B, _c, H, W = x.shape
        zp = _check_dev(z, "z", self.device).data_ptr() if z is not None else None
        self._ck(self.lib.cddpm_ddim_step(self._h, x.data_ptr(), zp, seed, slice0, int(t), float(coef_x0), float(coef_eps),
                                          float(sigma), int(bool(add_noise)), int(bool(finalize)), B, H, W,
                                          _stream_ptr(self.device)), "cddpm_ddim_step")
        return x

    def p_sample_(self, x: torch.Tensor, t: int, *, seed: int = 0, slice0: int = 0) -> torch.Tensor:
        """in-place reverse step on a device tensor, context from the last prepare_cond (bench loop)"""
        x = _check_dev(x, "x", self.device)
        B, _c, H, W = x.shape
        self._ck(self.lib.cddpm_p_sample(self._h, x.data_ptr(), None, seed, slice0, int(t), B, H, W,
                                         _stream_ptr(self.device)), "cddpm_p_sample")
        return x

    def set_accumulation_switch(self, t_switch: int):
        """reverse steps t >= t_switch use the faster two-level-accumulation convolution plan (include/cddpm.h); default off (2^30).
        No effect at precision 16, which takes that plan on every step."""
        self._ck(self.lib.cddpm_set_accumulation_switch(self._h, int(t_switch)), "cddpm_set_accumulation_switch")

    def set_clip_denoised(self, on: bool):
        """clip_denoised of p_sample / ddim_sample (cond_DDPM.py:433, :467) for every later step on this engine"""
        self._ck(self.lib.cddpm_set_clip_denoised(self._h, int(bool(on))), "cddpm_set_clip_denoised")

    # 0-4: the reconstruction path; 5-8: the training operators (weight gradients, GroupNorm backward, the context encoder, Adam + re-packing)
    PROF_CLASSES = ("conv3x3_mfma", "conv1x1_mfma", "attention", "groupnorm", "other", "wgrad", "groupnorm_backward", "encoder", "optimizer")

    def set_profiling(self, on: bool):
        self._ck(self.lib.cddpm_set_profiling(self._h, int(on)), "cddpm_set_profiling")

    def get_profile(self):
        n = len(self.PROF_CLASSES)
        ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        ln = (C.c_int64 * n)()
        self._ck(self.lib.cddpm_get_profile(self._h, n, ms, fl, by, ln), "cddpm_get_profile")
        return {name: dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=int(ln[i])) for i, name in enumerate(self.PROF_CLASSES)}

    def noise_fill(self, B: int, H: int, W: int, *, seed: int, stream_id: int, t: int = 0, slice0: int = 0) -> torch.Tensor:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_noise_fill(self._h, out.data_ptr(), seed, stream_id, t, slice0, B, H, W,
                                           _stream_ptr(self.device)), "cddpm_noise_fill")
        return out

    def residual_postprocess(self, orig: torch.Tensor, recon: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None, *,
                             squared: bool = False, erode_iterations: int = 0, median_k: int = 0) -> torch.Tensor:
        """Residual map of a volume [S,H,W] on the device: |orig - recon| (or squared; recon=None: `orig` as it is), times
        the eroded brain mask, 3-D median filtered -- the CPU/scipy part of the reference's _test_step
        (utils_eval.py:29-33, :64-71), bit-exact."""
        orig = _check_dev(orig, "orig", self.device)
        if recon is not None:
            recon = _check_dev(recon, "recon", self.device)
        if orig.dim() != 3 or (recon is not None and recon.shape != orig.shape):
            raise RuntimeError("orig / recon must be [S,H,W] volumes of the same shape")
        mptr = None
        if mask is not None:
            mask = _check_dev(mask, "mask", self.device)
            if mask.shape != orig.shape:
                raise RuntimeError("mask must have the shape of the volume")
            mptr = mask.data_ptr()
        S, H, W = orig.shape
        out = torch.empty_like(orig)
        tmp = torch.empty_like(orig) if median_k else None
        self._ck(self.lib.cddpm_residual_postprocess(self._h, orig.data_ptr(), recon.data_ptr() if recon is not None else None,
                                                     mptr, S, H, W, int(squared),
                                                     int(erode_iterations), int(median_k),
                                                     tmp.data_ptr() if tmp is not None else None, out.data_ptr(),
                                                     _stream_ptr(self.device)), "cddpm_residual_postprocess")
        return out

    # ------------------------------------------------------------------ evaluation metrics (eval_metrics.hip)
    EVAL_FLAGS = {"voxel_metrics": 1, "component_filter": 2, "row_curve": 4, "threshold_override": 8}   # include/cddpm.h
    EVAL_RECORD, EVAL_SET_RESULT = 24, 8

    def _eval_workspace(self, n: int, rows: int) -> torch.Tensor:
        """caller-side workspace of the metric entry points: sized once per (n, rows) by cddpm_eval_workspace_bytes, grown on demand"""
        sizes = self.__dict__.setdefault("_eval_ws_sizes", {})
        if (n, rows) not in sizes:
            b = int(self.lib.cddpm_eval_workspace_bytes(int(n), int(rows)))
            if b == 0:
                raise RuntimeError(f"cddpm_eval_workspace_bytes: {n} voxels in {rows} rows is outside the supported range")
            sizes[(n, rows)] = b
        need = sizes[(n, rows)]
        ws = getattr(self, "_eval_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._eval_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def eval_volume(self, recon: torch.Tensor, orig: torch.Tensor, seg: torch.Tensor, mask: torch.Tensor, diff: torch.Tensor, *,
                    voxel_metrics: bool, component_filter: bool, row_curve: bool, threshold: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """One volume's metric record on the device (cddpm_eval_volume; _test_step, utils_eval.py:36-178). All five volumes are
        [R, D1, D2] fp32 with R = axis 0 of the reference's [H, W, D] volume; `diff` is the post-processed residual. threshold:
        the test stage's override (None: the volume's own find_best_val). Returns device tensors: record [EVAL_RECORD] float64,
        row_score [R] fp32, row_label [R] int32, row_counts [R, 3] int32 (#pred, #pred & seg, #seg, unfiltered), pred [R, D1, D2]
        uint8 (the filtered prediction)."""
        vols = {}
        for name, t in (("recon", recon), ("orig", orig), ("seg", seg), ("mask", mask), ("diff", diff)):
            vols[name] = _check_dev(t, name, self.device)
            if t.dim() != 3 or t.shape != diff.shape:
                raise RuntimeError(f"{name} must be an [R, D1, D2] volume of the residual's shape {tuple(diff.shape)}, got {tuple(t.shape)}")
        R, D1, D2 = diff.shape
        flags = ((self.EVAL_FLAGS["voxel_metrics"] if voxel_metrics else 0) | (self.EVAL_FLAGS["component_filter"] if component_filter else 0)
                 | (self.EVAL_FLAGS["row_curve"] if row_curve else 0) | (self.EVAL_FLAGS["threshold_override"] if threshold is not None else 0))
        ws = self._eval_workspace(R * D1 * D2, R)
        out = dict(record=torch.empty(self.EVAL_RECORD, dtype=torch.float64, device=self.device),
                   row_score=torch.empty(R, dtype=torch.float32, device=self.device),
                   row_label=torch.empty(R, dtype=torch.int32, device=self.device),
                   row_counts=torch.zeros(R, 3, dtype=torch.int32, device=self.device),
                   pred=torch.zeros(R, D1, D2, dtype=torch.uint8, device=self.device))
        self._ck(self.lib.cddpm_eval_volume(self._h, vols["recon"].data_ptr(), vols["orig"].data_ptr(), vols["seg"].data_ptr(),
                                            vols["mask"].data_ptr(), vols["diff"].data_ptr(), R, D1, D2, flags,
                                            float(threshold) if threshold is not None else 0.0, ws.data_ptr(), ws.numel(),
                                            out["record"].data_ptr(), out["row_score"].data_ptr(), out["row_label"].data_ptr(),
                                            out["row_counts"].data_ptr(), out["pred"].data_ptr(), _stream_ptr(self.device)),
                 "cddpm_eval_volume")
        return out

    def eval_set(self, x: torch.Tensor, y: torch.Tensor, *, healthy: bool) -> torch.Tensor:
        """Over an accumulated validation set (cddpm_eval_set; _test_end, utils_eval.py:247-286): x [n] fp32 residuals, y [n] int8
        labels. Returns [EVAL_SET_RESULT] float64 on the device: AUROC, AUPRC, t_1p, t_5p, t_10p (healthy: labels read as zero),
        best dice, its threshold (threshold['total']), max."""
        x = _check_dev(x, "x", self.device)
        if not isinstance(y, torch.Tensor) or not y.is_cuda or y.device != self.device or y.dtype != torch.int8:
            raise RuntimeError(f"y must be an int8 tensor on {self.device}")
        if x.dim() != 1 or y.shape != x.shape or x.numel() < 1:
            raise RuntimeError(f"x and y must be non-empty 1-D tensors of one length, got {tuple(x.shape)} and {tuple(y.shape)}")
        y = y.contiguous()
        ws = self._eval_workspace(x.numel(), 0)
        out = torch.empty(self.EVAL_SET_RESULT, dtype=torch.float64, device=self.device)
        self._ck(self.lib.cddpm_eval_set(self._h, x.data_ptr(), y.data_ptr(), x.numel(), int(bool(healthy)), ws.data_ptr(), ws.numel(),
                                         out.data_ptr(), _stream_ptr(self.device)), "cddpm_eval_set")
        return out

    # ------------------------------------------------------------------ Hausdorff distance (eval_hausdorff.hip)
    HAUSDORFF_SQUEEZE, HAUSDORFF_RESULT, HAUSDORFF_FAR = 1, 8, 1 << 28     # include/cddpm.h

    def _hausdorff_workspace(self, R: int, D1: int, D2: int) -> torch.Tensor:
        """caller-side workspace of cddpm_eval_hausdorff: sized by cddpm_hausdorff_workspace_bytes, grown on demand, its own buffer"""
        need = int(self.lib.cddpm_hausdorff_workspace_bytes(int(R), int(D1), int(D2)))
        if need == 0:
            raise RuntimeError(f"cddpm_hausdorff_workspace_bytes: {self.lib.cddpm_last_error(None).decode()}")
        ws = getattr(self, "_hausdorff_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._hausdorff_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def hausdorff(self, pred: torch.Tensor, seg: torch.Tensor, *, squeeze: bool = True, fields: bool = False) -> Dict[str, torch.Tensor]:
        """The undirected Hausdorff distance between the surfaces of pred != 0 and seg != 0 (cddpm_eval_hausdorff; HausPerVol of
        _test_step, utils_eval.py:131-135). pred: [R, D1, D2] uint8, the `pred` of eval_volume; seg: [R, D1, D2] fp32, raw data_seg.
        squeeze: erode along the axes where the union's bounding box is wider than one voxel only (monai's crop + np.squeeze).
        Returns device tensors: record [HAUSDORFF_RESULT] float64 (distance, the two directed squared distances, the two edge counts,
        the three active-axis flags); with fields=True also edges [R, D1, D2] uint8 (bit 0: pred's edge, bit 1: seg's) and dist2
        [2, R, D1, D2] int32 (squared distance of every voxel to pred's edge, to seg's edge; HAUSDORFF_FAR for an empty edge set)."""
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.device != self.device or pred.dtype != torch.uint8:
            raise RuntimeError(f"pred must be a uint8 tensor on {self.device} (got {getattr(pred, 'dtype', type(pred).__name__)})")
        seg = _check_dev(seg, "seg", self.device)
        if pred.dim() != 3 or seg.shape != pred.shape:
            raise RuntimeError(f"pred and seg must be [R, D1, D2] volumes of one shape, got {tuple(pred.shape)} and {tuple(seg.shape)}")
        pred = pred.contiguous()
        R, D1, D2 = pred.shape
        ws = self._hausdorff_workspace(R, D1, D2)
        out = dict(record=torch.empty(self.HAUSDORFF_RESULT, dtype=torch.float64, device=self.device))
        if fields:
            out["edges"] = torch.empty(R, D1, D2, dtype=torch.uint8, device=self.device)
            out["dist2"] = torch.empty(2, R, D1, D2, dtype=torch.int32, device=self.device)
        self._ck(self.lib.cddpm_eval_hausdorff(self._h, pred.data_ptr(), seg.data_ptr(), R, D1, D2,
                                               self.HAUSDORFF_SQUEEZE if squeeze else 0, ws.data_ptr(), ws.numel(),
                                               out["record"].data_ptr(), out["edges"].data_ptr() if fields else None,
                                               out["dist2"].data_ptr() if fields else None, _stream_ptr(self.device)),
                 "cddpm_eval_hausdorff")
        return out

    # ------------------------------------------------------------------ augmented training slices (augment.hip)
    AUG_META, AUG_PAR, AUG_ALL, AUG_MAX_SIGMA = 4, 28, 15, 8.0                # include/cddpm.h

    @classmethod
    def check_augment_tables(cls, meta: np.ndarray, par: np.ndarray, N: int, D: int) -> None:
        """what cddpm_aug_slices' first kernel refuses per sample, checked on the host tables before they are copied: a RuntimeError names
        the first bad row. meta [B, 4] int32 {volume, z, flags, g | axis << 8}, par [B, 28] fp32 {gamma, sigma0..2, I, c[20], unused}."""
        if meta.ndim != 2 or meta.shape[1] != cls.AUG_META or meta.dtype != np.int32:
            raise RuntimeError(f"meta must be [B, {cls.AUG_META}] int32, got {meta.shape} {meta.dtype}")
        if par.shape != (meta.shape[0], cls.AUG_PAR) or par.dtype != np.float32:
            raise RuntimeError(f"par must be [{meta.shape[0]}, {cls.AUG_PAR}] float32, got {par.shape} {par.dtype}")
        if meta.shape[0] < 1:
            raise RuntimeError("an empty batch")
        axis, sig = meta[:, 3] >> 8, par[:, 1:4]
        for what, bad in ((f"volume outside [0, {N})", (meta[:, 0] < 0) | (meta[:, 0] >= N)),
                          (f"z outside [0, {D})", (meta[:, 1] < 0) | (meta[:, 1] >= D)),
                          ("ghosting axis outside 0 ... 2", (axis < 0) | (axis > 2)),
                          ("unknown flag bits", (meta[:, 2] & ~cls.AUG_ALL) != 0),
                          (f"sigma_voxel outside [0, {cls.AUG_MAX_SIGMA:g}]", ~((sig >= 0) & (sig <= cls.AUG_MAX_SIGMA)).all(axis=1)),
                          ("a non-finite parameter", ~np.isfinite(par[:, [0] + list(range(4, 25))]).all(axis=1))):
            if bad.any():
                b = int(np.argmax(bad))
                raise RuntimeError(f"cddpm_aug_slices: sample {b}: {what} (meta {meta[b].tolist()}, sigma {sig[b].tolist()})")

    def _augment_buffers(self, entry: str, B: int, H: int, W: int, D: int):
        """the workspace of `entry` (cddpm_aug_slices or cddpm_aug_pipeline), asked for once per geometry and largest batch through the
        library's own size query (cddpm_aug_workspace_bytes / cddpm_aug_pipeline_workspace_bytes, the operator-scratch convention), and two
        pinned staging rows for the tables, so that one copy can be in flight while the next is filled. A smaller batch of the same
        geometry runs in the same buffers."""
        query, meta_n, par_n = self._AUG_ENTRIES[entry]
        key = (H, W, D)
        cache = self.__dict__.setdefault("_aug", {})
        st = cache.get(entry)
        if st is None or st["key"] != key or B > st["cap"]:
            need = int(getattr(self.lib, query)(B, H, W, D))
            if need == 0:
                raise RuntimeError(f"{query}: {self.lib.cddpm_last_error(None).decode()}")
            row = 4 * (meta_n + par_n)
            st = cache[entry] = dict(key=key, cap=B, ws=torch.empty(need, dtype=torch.uint8, device=self.device),
                                     host=[torch.empty(B * row, dtype=torch.uint8).pin_memory() for _ in range(2)],
                                     dev=[torch.empty(B * row, dtype=torch.uint8, device=self.device) for _ in range(2)],
                                     done=[None, None], turn=0)
        return st

    def _augment_call(self, entry: str, check, bank, meta, par, out: Optional[torch.Tensor]) -> torch.Tensor:
        """what augment_slices and augment_pipeline share: the host check of the two tables, their staging through pinned memory with ONE
        asynchronous host-to-device copy, and the library call on the current stream"""
        _query, meta_n, par_n = self._AUG_ENTRIES[entry]
        meta = np.ascontiguousarray(meta.numpy() if isinstance(meta, torch.Tensor) else meta)
        par = np.ascontiguousarray(par.numpy() if isinstance(par, torch.Tensor) else par)
        data = _check_dev(bank.data, "bank.data", self.device)
        N, D, H, W = data.shape
        check(meta, par, N, D)
        B = meta.shape[0]
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (B, H, W)
              or not out.is_contiguous()):
            raise RuntimeError(f"out must be a contiguous [{B}, {H}, {W}] float32 tensor on {self.device}")
        st = self._augment_buffers(entry, B, H, W, D)
        i = st["turn"]
        st["turn"] = 1 - i
        if st["done"][i] is not None:
            st["done"][i].synchronize()                # the copy that last read this staging row (two calls ago) has long finished
        host, dev, nm, tot = st["host"][i], st["dev"][i], B * 4 * meta_n, B * 4 * (meta_n + par_n)
        host[:nm].view(torch.int32).view(B, meta_n).copy_(torch.from_numpy(meta))
        host[nm:tot].view(torch.float32).view(B, par_n).copy_(torch.from_numpy(par))
        dev[:tot].copy_(host[:tot], non_blocking=True)
        st["done"][i] = torch.cuda.Event()
        st["done"][i].record(torch.cuda.current_stream(self.device))
        self._ck(getattr(self.lib, entry)(self._h, data.data_ptr(), N, H, W, D, dev.data_ptr(), dev.data_ptr() + nm, B,
                                          st["ws"].data_ptr(), st["ws"].numel(), out.data_ptr(), _stream_ptr(self.device)), entry)
        return out

    def augment_slices(self, bank, meta, par, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One batch of augmented training slices from a resident bank (cddpm_aug_slices; get_augment + vol2slice of the reference's
        create_dataset.py:220-250, :143-193). bank: an augment.VolumeBank on this engine's device; meta [B, 4] int32 and par [B, 28] fp32:
        HOST tables (numpy or CPU tensors), one row per output slice, as IntensityAugment.draw returns them. They are checked here
        (check_augment_tables: a bad row raises before anything is copied or enqueued and `out` stays untouched), staged through pinned
        memory with ONE asynchronous host-to-device copy, and applied by one library call on the current stream. Returns out [B, H, W]
        fp32 on the device (`out=`: written in place)."""
        return self._augment_call("cddpm_aug_slices", self.check_augment_tables, bank, meta, par, out)

    # the eleven-slot pipeline (include/cddpm.h, "The augmentation pipeline")
    PIPE_META, PIPE_PAR, PIPE_ALL = 8, 64, 2047
    PIPE_META_GHOST, PIPE_META_POLICY_GHOST, PIPE_PAR_SLOT, PIPE_PAR_POLICY, PIPE_PAR_NOISE_STD, PIPE_PAR_MATRIX = 3, 4, 0, 25, 50, 51
    _AUG_ENTRIES = {"cddpm_aug_slices": ("cddpm_aug_workspace_bytes", AUG_META, AUG_PAR),
                    "cddpm_aug_pipeline": ("cddpm_aug_pipeline_workspace_bytes", PIPE_META, PIPE_PAR)}

    @classmethod
    def check_pipeline_tables(cls, meta: np.ndarray, par: np.ndarray, N: int, D: int) -> None:
        """check_augment_tables for cddpm_aug_pipeline's tables: meta [B, 8] int32 {volume, z, flags, g | axis << 8 of the ghosting slot
        and of the policy ghosting, key0, key1, unused}, par [B, 64] fp32 {slot set [25], policy set [25], noise std, M[9], unused}.
        g is the word's low byte, so every g a word can hold is in range; a negative word or an axis above 2 is refused per slot."""
        if meta.ndim != 2 or meta.shape[1] != cls.PIPE_META or meta.dtype != np.int32:
            raise RuntimeError(f"meta must be [B, {cls.PIPE_META}] int32, got {meta.shape} {meta.dtype}")
        if par.shape != (meta.shape[0], cls.PIPE_PAR) or par.dtype != np.float32:
            raise RuntimeError(f"par must be [{meta.shape[0]}, {cls.PIPE_PAR}] float32, got {par.shape} {par.dtype}")
        if meta.shape[0] < 1:
            raise RuntimeError("an empty batch")
        checks = [(f"volume outside [0, {N})", (meta[:, 0] < 0) | (meta[:, 0] >= N)),
                  (f"z outside [0, {D})", (meta[:, 1] < 0) | (meta[:, 1] >= D)),
                  ("unknown flag bits", (meta[:, 2] & ~cls.PIPE_ALL) != 0)]
        for name, col, par0 in (("slot", cls.PIPE_META_GHOST, cls.PIPE_PAR_SLOT), ("policy", cls.PIPE_META_POLICY_GHOST, cls.PIPE_PAR_POLICY)):
            word, sig = meta[:, col], par[:, par0 + 1:par0 + 4]
            checks += [(f"{name} ghosting word: g | axis << 8 with axis outside 0 ... 2", (word < 0) | ((word >> 8) > 2)),
                       (f"{name} sigma_voxel outside [0, {cls.AUG_MAX_SIGMA:g}]", ~((sig >= 0) & (sig <= cls.AUG_MAX_SIGMA)).all(axis=1)),
                       (f"a non-finite {name} parameter", ~np.isfinite(par[:, [par0] + list(range(par0 + 4, par0 + 25))]).all(axis=1))]
        checks += [("a non-finite noise std", ~np.isfinite(par[:, cls.PIPE_PAR_NOISE_STD])),
                   ("a non-finite affine matrix entry", ~np.isfinite(par[:, cls.PIPE_PAR_MATRIX:cls.PIPE_PAR_MATRIX + 9]).all(axis=1))]
        for what, bad in checks:
            if bad.any():
                b = int(np.argmax(bad))
                raise RuntimeError(f"cddpm_aug_pipeline: sample {b}: {what} (meta {meta[b].tolist()})")

    def augment_pipeline(self, bank, meta, par, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One batch of training slices through get_augment's whole order (cddpm_aug_pipeline: the individual bias, noise, ghosting, blur
        and gamma, the affine and the flip, then the policy group, then vol2slice). meta [B, 8] int32 and par [B, 64] fp32: HOST tables
        as augment.SliceAugment.draw returns them. Checked (check_pipeline_tables), staged and applied exactly as augment_slices does.
        Returns out [B, H, W] fp32 on the device (`out=`: written in place)."""
        return self._augment_call("cddpm_aug_pipeline", self.check_pipeline_tables, bank, meta, par, out)

    # ------------------------------------------------------------------ preprocessed volumes (preprocess.hip)
    PREP_SMOOTH, PREP_CROPPAD, PREP_RESCALE, PREP_RESAMPLE, PREP_ALL, PREP_RECORD = 1, 2, 4, 8, 15, 16      # include/cddpm.h

    @classmethod
    def prep_output_shape(cls, shape: Sequence[int], stages: int, target: Optional[Sequence[int]], f: float) -> Tuple[int, int, int]:
        """(H', W', D') of a preprocessed (H, W, D) volume: the target under CROPPAD, then ceil(N / f) per axis under RESAMPLE"""
        out = tuple(int(t) for t in target) if stages & cls.PREP_CROPPAD else tuple(int(n) for n in shape)
        if stages & cls.PREP_RESAMPLE and float(f) != 1.0:
            out = tuple(int(np.ceil(n / float(f))) for n in out)
        return out

    def _prep_workspace(self, key) -> torch.Tensor:
        """cddpm_prep_volume's workspace, asked for once per geometry (H, W, D, stages, th, tw, td, f) through the library's own size
        query (the operator-scratch convention); a call of another geometry replaces it"""
        st = getattr(self, "_prep", None)
        if st is None or st[0] != key:
            need = int(self.lib.cddpm_prep_workspace_bytes(*key))
            if need == 0:
                raise RuntimeError(f"cddpm_prep_workspace_bytes: {self.lib.cddpm_last_error(None).decode()}")
            st = self._prep = (key, torch.empty(need, dtype=torch.uint8, device=self.device))
        return st[1]

    def _check_labels(self, t, name: str, shape) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.device or t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must be a uint8 tensor of shape {tuple(shape)} on {self.device}")
        return t.contiguous()

    def preprocess_volume(self, vol: torch.Tensor, mask: Optional[torch.Tensor] = None, *, stages: int, target: Optional[Sequence[int]] = None,
                          perc: Sequence[float] = (1.0, 99.0), f: float = 1.0, dt: float = 0.125, iterations: int = 3,
                          spacing: Sequence[float] = (1.0, 1.0, 1.0), out: Optional[torch.Tensor] = None,
                          mask_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One raw volume through the stages of cddpm_prep_volume (sitk_reader's CurvatureFlow and get_transform's CropOrPad,
        RescaleIntensity, Resample; create_dataset.py:252-258, :196-218). vol [H, W, D] fp32 and mask [H, W, D] uint8 (None: vol > 0) on
        this engine's device, torchio's layout. Returns device tensors: vol [D', H', W'] fp32 and mask [D', H', W'] uint8, slice-major
        (`out=`, `mask_out=`: written in place, e.g. a slot of a VolumeBank), and record [PREP_RECORD] float64."""
        vol = _check_dev(vol, "vol", self.device)
        if vol.dim() != 3:
            raise RuntimeError(f"vol must be [H, W, D], got {tuple(vol.shape)}")
        H, W, D = vol.shape
        if mask is not None:
            mask = self._check_labels(mask, "mask", vol.shape)
        stages, f = int(stages), float(f)
        th, tw, td = (int(t) for t in target) if stages & self.PREP_CROPPAD else (0, 0, 0)
        ws = self._prep_workspace((H, W, D, stages, th, tw, td, f))
        h2, w2, d2 = self.prep_output_shape(vol.shape, stages, target, f)
        if out is None:
            out = torch.empty(d2, h2, w2, dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (d2, h2, w2)
              or not out.is_contiguous()):
            raise RuntimeError(f"out must be a contiguous [{d2}, {h2}, {w2}] float32 tensor on {self.device}")
        if mask_out is None:
            mask_out = torch.empty(d2, h2, w2, dtype=torch.uint8, device=self.device)
        elif (not isinstance(mask_out, torch.Tensor) or mask_out.device != self.device or mask_out.dtype != torch.uint8
              or tuple(mask_out.shape) != (d2, h2, w2) or not mask_out.is_contiguous()):
            raise RuntimeError(f"mask_out must be a contiguous [{d2}, {h2}, {w2}] uint8 tensor on {self.device}")
        record = torch.empty(self.PREP_RECORD, dtype=torch.float64, device=self.device)
        par = (C.c_double * 8)(float(dt), *(float(s) for s in spacing), float(perc[0]), float(perc[1]), f, 0.0)
        self._ck(self.lib.cddpm_prep_volume(self._h, vol.data_ptr(), mask.data_ptr() if mask is not None else None, H, W, D, stages,
                                            int(iterations), th, tw, td, C.addressof(par), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                            mask_out.data_ptr(), record.data_ptr(), _stream_ptr(self.device)), "cddpm_prep_volume")
        return dict(vol=out, mask=mask_out, record=record)

    def preprocess_labels(self, lab: torch.Tensor, *, stages: int, target: Optional[Sequence[int]] = None, f: float = 1.0,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A label volume [H, W, D] uint8 through CROPPAD and RESAMPLE alone (cddpm_prep_labels; the other stage bits of `stages` are
        dropped: images only). Returns [D', H', W'] uint8 on the device."""
        if not isinstance(lab, torch.Tensor) or lab.dim() != 3:
            raise RuntimeError("lab must be a [H, W, D] uint8 tensor")
        lab = self._check_labels(lab, "lab", lab.shape)
        H, W, D = lab.shape
        stages, f = int(stages) & (self.PREP_CROPPAD | self.PREP_RESAMPLE), float(f)
        th, tw, td = (int(t) for t in target) if stages & self.PREP_CROPPAD else (0, 0, 0)
        h2, w2, d2 = self.prep_output_shape(lab.shape, stages, target, f)
        if out is None:
            out = torch.empty(d2, h2, w2, dtype=torch.uint8, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.uint8 or tuple(out.shape) != (d2, h2, w2)
              or not out.is_contiguous()):
            raise RuntimeError(f"out must be a contiguous [{d2}, {h2}, {w2}] uint8 tensor on {self.device}")
        self._ck(self.lib.cddpm_prep_labels(self._h, lab.data_ptr(), H, W, D, stages, th, tw, td, f, out.data_ptr(),
                                            _stream_ptr(self.device)), "cddpm_prep_labels")
        return out

    def simplex_noise(self, B: int, H: int, W: int, *, seed: int, octaves: int = 6, persistence: float = 0.8,
                      frequency: float = 64.0) -> torch.Tensor:
        """gen_noise for noisetype 'simplex': float16 [B,1,H,W], the same field for every batch item, bit-exact
        with the reference's CPU generator for the given newSeed value."""
        out = torch.empty((B, 1, H, W), dtype=torch.float16, device=self.device)
        self._ck(self.lib.cddpm_simplex_fill(self._h, out.data_ptr(), int(seed), B, H, W, octaves, float(persistence),
                                             float(frequency), _stream_ptr(self.device)), "cddpm_simplex_fill")
        return out

    def q_sample(self, x01: torch.Tensor, t, noise: torch.Tensor) -> torch.Tensor:
        x01 = _check_dev(x01, "x01", self.device)
        noise = _check_dev(noise, "noise", self.device)
        B, _c, H, W = x01.shape
        out = torch.empty_like(x01)
        sa, s1 = self._qs
        if isinstance(t, torch.Tensor):
            tt = self._t_tensor(t, B)
            tp, tu = tt.data_ptr(), 0
        else:
            tt, tp, tu = None, None, int(t)
        self._ck(self.lib.cddpm_q_sample(self._h, x01.data_ptr(), noise.data_ptr(), tp, tu, sa.ctypes.data, s1.ctypes.data,
                                         sa.shape[0], out.data_ptr(), B, H, W, _stream_ptr(self.device)), "cddpm_q_sample")
        torch.cuda.current_stream(self.device).synchronize()   # host tables were read asynchronously
        return out

    # ------------------------------------------------------------------ the patched DDPM: box noising, stitching, box loss
    STITCH_MODES = {"paste": 0, "cut": 1, "avg": 2}        # CDDPM_STITCH_* of include/cddpm.h

    def _q_tables(self):
        """the q_sample coefficient tables of set_schedule on the device (uploaded once per schedule)"""
        if getattr(self, "_qs", None) is None:
            raise RuntimeError("no schedule installed: call set_schedule first")
        if getattr(self, "_qs_dev_of", None) is not self._qs:
            self._qs_dev = tuple(torch.from_numpy(a).to(self.device) for a in self._qs)
            self._qs_dev_of = self._qs
        return self._qs_dev

    def box_q_sample(self, x01: torch.Tensor, t, noise: torch.Tensor, boxes: torch.Tensor, *, tables=None) -> torch.Tensor:
        """cddpm_box_q_sample: x01, noise [S,1,H,W]; boxes [N,4] rows (x0, y1, x2, y3), N a multiple of S -> [N,1,H,W], slice n made
        from slice n % S: 2 x01 - 1 outside its box, q_sample inside. t: int, or an int tensor [S]. tables: (sqrt_alphas_cumprod,
        sqrt_one_minus_alphas_cumprod) as float32 device tensors [T] (default: the installed schedule's)."""
        x01 = _check_dev(x01, "x01", self.device)
        noise = _check_dev(noise, "noise", self.device)
        if x01.dim() != 4 or x01.shape[1] != 1 or noise.shape != x01.shape:
            raise RuntimeError(f"x01 and noise must both be [S,1,H,W], got {tuple(x01.shape)} and {tuple(noise.shape)}")
        S, _c, H, W = x01.shape
        boxes = check_boxes(boxes, None, self.device)
        N = boxes.shape[0]
        if N < S or N % S:
            raise RuntimeError(f"{N} boxes for {S} slices: the number of boxes must be a multiple of the number of slices")
        sa, s1 = tables if tables is not None else self._q_tables()
        sa, s1 = _check_dev(sa, "sqrt_alphas_cumprod", self.device), _check_dev(s1, "sqrt_one_minus_alphas_cumprod", self.device)
        T = sa.numel()
        if s1.numel() != T:
            raise RuntimeError("the two coefficient tables differ in length")
        if isinstance(t, torch.Tensor):
            if t.numel() != S:
                raise RuntimeError("t must have one element per source slice")
            if not t.is_cuda:                               # a host tensor is range-checked for free; a device one is clamped by the kernel
                lo, hi = int(t.min()), int(t.max())
                if lo < 0 or hi >= T:
                    raise IndexError(f"timestep indices must lie in [0, {T}), got [{lo}, {hi}]")
            tt = t.to(self.device, torch.int32).contiguous()
            tp, tu = tt.data_ptr(), 0
        else:
            tt, tp, tu = None, None, int(t)
        out = torch.empty((N, 1, H, W), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_box_q_sample(self._h, x01.data_ptr(), noise.data_ptr(), tp, tu, sa.data_ptr(), s1.data_ptr(), T,
                                             boxes.data_ptr(), out.data_ptr(), S, N, H, W, _stream_ptr(self.device)), "cddpm_box_q_sample")
        return out

    def box_stitch(self, reco: torch.Tensor, boxes: torch.Tensor, cut: Optional[torch.Tensor] = None, mode: str = "paste", *,
                   slices: Optional[int] = None) -> torch.Tensor:
        """cddpm_box_stitch: reco [K*S,1,H,W] box-major (n = k S + s), boxes / cut [K*S,4] in the same order -> [S,1,H,W], the
        reference's `reco_patched` after its last box. mode 'paste' | 'cut' (pastes the `cut` rows) | 'avg'. slices: S (default:
        taken from a [K,S,4] boxes tensor)."""
        if mode not in self.STITCH_MODES:
            raise ValueError(f"unknown stitch mode {mode!r}: expected one of {', '.join(self.STITCH_MODES)}")
        reco = _check_dev(reco, "reco", self.device)
        if reco.dim() != 4 or reco.shape[1] != 1:
            raise RuntimeError(f"reco must be [K*S,1,H,W], got {tuple(reco.shape)}")
        N, _c, H, W = reco.shape
        if slices is None:
            if not (isinstance(boxes, torch.Tensor) and boxes.dim() == 3 and boxes.shape[-1] == 4):
                raise RuntimeError("box_stitch: pass slices=S, or boxes as a [K,S,4] tensor")
            slices = boxes.shape[1]
        S = int(slices)
        if S < 1 or N % S:
            raise RuntimeError(f"{N} reconstructions are not a multiple of {S} slices")
        boxes = check_boxes(boxes, N, self.device)
        if mode == "cut":
            if cut is None:
                raise RuntimeError("stitch mode 'cut' needs the sample_grid_cut boxes")
            cut = check_boxes(cut, N, self.device)
        else:
            cut = None
        out = torch.empty((S, 1, H, W), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_box_stitch(self._h, reco.data_ptr(), boxes.data_ptr(), cut.data_ptr() if cut is not None else None,
                                           self.STITCH_MODES[mode], out.data_ptr(), S, N // S, H, W, _stream_ptr(self.device)), "cddpm_box_stitch")
        return out

    def loss_box(self, out: torch.Tensor, x0: torch.Tensor, noise: Optional[torch.Tensor], boxes: torch.Tensor, *, objective="pred_x0",
                 loss_type="l1", inpaint=False, w_b: Optional[torch.Tensor] = None, grad_scale: float = 1.0,
                 scaler: Optional[torch.Tensor] = None, want_grad: bool = True):
        """cddpm_op_loss_box: the loss of p_losses with one box per slice -> (loss_b [B], dout or None). out, x0 (the image in [-1,1]),
        noise: [B,1,H,W]; dout = scale * dL/d(out) with scale = grad_scale, or the device loss scale of `scaler` (int32[4])."""
        if objective not in OBJECTIVES:
            raise ValueError(f"unknown objective {objective!r}")
        if loss_type not in ("l1", "l2"):
            raise ValueError(f"invalid loss type {loss_type}")
        out = _check_dev(out, "out", self.device)
        x0 = _check_dev(x0, "x0", self.device)
        if out.dim() != 4 or out.shape[1] != 1 or x0.shape != out.shape:
            raise RuntimeError(f"out and x0 must both be [B,1,H,W], got {tuple(out.shape)} and {tuple(x0.shape)}")
        B, _c, H, W = out.shape
        pn = objective == "pred_noise"
        if pn:
            if noise is None:
                raise RuntimeError("the pred_noise loss needs the noise")
            noise = _check_dev(noise, "noise", self.device)
            if noise.shape != out.shape:
                raise RuntimeError(f"noise must be {tuple(out.shape)}, got {tuple(noise.shape)}")
        boxes = check_boxes(boxes, B, self.device)
        if w_b is not None:
            w_b = _check_dev(w_b, "w_b", self.device)
            if w_b.numel() != B:
                raise RuntimeError("w_b must have one weight per slice")
        if scaler is not None and not (scaler.is_cuda and scaler.dtype == torch.int32 and scaler.numel() >= 4):
            raise RuntimeError("scaler must be the int32[4] device block of the dynamic loss scaling")
        dout = torch.empty_like(out) if want_grad else None
        loss_b = torch.empty(B, dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_loss_box(self._h, out.data_ptr(), x0.data_ptr(), noise.data_ptr() if pn else None, boxes.data_ptr(),
                                            w_b.data_ptr() if w_b is not None else None, int(pn), int(bool(inpaint)), int(loss_type == "l2"),
                                            B, H, W, C.c_float(float(grad_scale)), scaler.data_ptr() if scaler is not None else None,
                                            dout.data_ptr() if dout is not None else None, loss_b.data_ptr(), _stream_ptr(self.device)),
                 "cddpm_op_loss_box")
        return loss_b, dout

    # ------------------------------------------------------------------ test surface
    def block_names(self):
        return [self.lib.cddpm_block_name(self._h, i).decode() for i in range(self.lib.cddpm_num_blocks(self._h))]

    def forward_with_taps(self, x: torch.Tensor, t, cond) -> Dict[str, torch.Tensor]:
        """forward that also returns every block output as NCHW tensors (tests only)."""
        x = _check_dev(x, "x", self.device)
        B, _c, H, W = x.shape
        names = self.block_names()
        bufs = {}
        for i, n in enumerate(names):
            if n == "out":
                continue
            cc, hh, ww = C.c_int(), C.c_int(), C.c_int()
            self._ck(self.lib.cddpm_block_shape(self._h, i, H, W, C.byref(cc), C.byref(hh), C.byref(ww)), "cddpm_block_shape")
            t_ = torch.empty((B, hh.value, ww.value, cc.value), dtype=torch.float32, device=self.device)
            self._ck(self.lib.cddpm_set_tap(self._h, i, t_.data_ptr()), "cddpm_set_tap")
            bufs[n] = t_
        try:
            out = self.unet_forward(x, t, cond)
            torch.cuda.synchronize(self.device)
        finally:
            for i in range(len(names)):
                self.lib.cddpm_set_tap(self._h, i, None)
        res = {n: v.permute(0, 3, 1, 2).contiguous() for n, v in bufs.items()}
        res["out"] = out
        return res

    def op_conv(self, src0, src1, coef, silu, upsample, weight, bias, res, res_upsample, ksize):
        """fused conv on NHWC device tensors (see cddpm_op_conv); weight [Cout,Cin,k,k] host/any tensor."""
        B, h, w, C0 = src0.shape
        H, W = (2 * h, 2 * w) if upsample else (h, w)     # upsample: 0 none, 1 gather form, 2 folded form
        C1 = src1.shape[-1] if src1 is not None else 0
        wt = np.ascontiguousarray(weight.detach().cpu().numpy(), dtype=np.float32)
        bs = np.ascontiguousarray(bias.detach().cpu().numpy(), dtype=np.float32)
        Cout = wt.shape[0]
        out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_conv(
            self._h, src0.data_ptr(), C0, src1.data_ptr() if src1 is not None else None, C1,
            coef.data_ptr() if coef is not None else None, int(silu), int(upsample), wt.ctypes.data, bs.ctypes.data,
            Cout, ksize, res.data_ptr() if res is not None else None, int(res_upsample), out.data_ptr(), B, H, W,
            _stream_ptr(self.device)), "cddpm_op_conv")
        return out

    def op_conv_planned(self, src0, src1, coef, silu, upsample, weight, bias, res, res_upsample, ksize, *, img_hw, t=-1, skip0=None,
                        skip1=None, wskip=None, gamma=None, beta=None, out=None):
        """one fused conv on NHWC device tensors launched as this engine's HANDLE plans it (cddpm_op_conv_planned): the layer of a
        forward at img_hw = (H, W) on reverse step t (t < 0: a single forward). upsample: 0 or 2 (the folded form). skip0 / skip1 / wskip:
        the two-source 1x1 skip segment; gamma / beta: also return the output's GroupNorm coefficients [3,B,Cout]. out: a contiguous
        [B,H,W,Cout] view to write into. -> (out, coef_out or None, plan) with plan = {'S', 'kbound' (S + 1 chunk bounds), 'nb2',
        'scale_exp'}, what the library reports it took."""
        if upsample not in (0, 2, False):
            raise ValueError("op_conv_planned: upsample is 0 or 2 (the folded form the UNet uses)")
        B, h, w, C0 = src0.shape
        H, W = (2 * h, 2 * w) if upsample else (h, w)
        f = lambda x: None if x is None else np.ascontiguousarray(x.detach().cpu().numpy(), dtype=np.float32)
        hp = lambda a: None if a is None else a.ctypes.data
        dp = lambda x: None if x is None else x.data_ptr()
        wt, bs, ws, g, b = f(weight), f(bias), f(wskip), f(gamma), f(beta)
        Cout = wt.shape[0]
        if out is None:
            out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=self.device)
        if tuple(out.shape) != (B, H, W, Cout) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("op_conv_planned: out must be a contiguous float32 [B,H,W,Cout] tensor")
        coef_out = torch.empty((3, B, Cout), dtype=torch.float32, device=self.device) if g is not None else None
        S, nb2, e = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        kb = (C.c_int * 9)()
        self._ck(self.lib.cddpm_op_conv_planned(
            self._h, src0.data_ptr(), C0, dp(src1), src1.shape[-1] if src1 is not None else 0, dp(coef), int(silu), 1 if upsample else 0,
            hp(wt), hp(bs), Cout, ksize, dp(res), int(res_upsample), dp(skip0), skip0.shape[-1] if skip0 is not None else 0, dp(skip1),
            skip1.shape[-1] if skip1 is not None else 0, hp(ws), hp(g), hp(b), dp(coef_out), out.data_ptr(), B, H, W, int(img_hw[0]),
            int(img_hw[1]), int(t), C.byref(S), kb, C.byref(nb2), C.byref(e), _stream_ptr(self.device)), "cddpm_op_conv_planned")
        plan = {"S": S.value, "kbound": [int(kb[j]) for j in range(S.value + 1)], "nb2": bool(nb2.value), "scale_exp": e.value}
        return out, coef_out, plan

    def op_conv_skip(self, src0, coef, silu, weight, bias, skip, wskip):
        """conv3x3(act(src0)) + conv1x1(skip) + bias on NHWC device tensors (cddpm_op_conv_skip)"""
        B, H, W, C0 = src0.shape
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        wt, bs, ws = f(weight), f(bias), f(wskip)
        Cout = wt.shape[0]
        out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_conv_skip(self._h, src0.data_ptr(), C0, coef.data_ptr() if coef is not None else None, int(silu),
                                             wt.ctypes.data, bs.ctypes.data, Cout, skip.data_ptr(), skip.shape[-1], ws.ctypes.data,
                                             out.data_ptr(), B, H, W, _stream_ptr(self.device)), "cddpm_op_conv_skip")
        return out

    def op_conv_gn(self, src0, weight, bias, gamma, beta):
        """conv3x3(src0) + bias with the epilogue's GroupNorm statistics -> (out NHWC, coef [3,B,Cout]) (cddpm_op_conv_gn)"""
        B, H, W, C0 = src0.shape
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        wt, bs, g, b = f(weight), f(bias), f(gamma), f(beta)
        Cout = wt.shape[0]
        out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=self.device)
        coef = torch.empty((3, B, Cout), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_conv_gn(self._h, src0.data_ptr(), C0, wt.ctypes.data, bs.ctypes.data, Cout, g.ctypes.data,
                                           b.ctypes.data, out.data_ptr(), coef.data_ptr(), B, H, W, _stream_ptr(self.device)),
                 "cddpm_op_conv_gn")
        return out, coef

    # ---- training pieces (row f4, kernel level only) ----------------------------------------------------------------
    def op_conv_dgrad(self, dy, weight):
        """dL/d(input) of Conv2d(k, padding k // 2): dy NHWC [B,H,W,Cout] on the device, weight the FORWARD tensor [Cout,Cin,k,k]"""
        B, H, W, Cout = dy.shape
        wt = np.ascontiguousarray(weight.detach().cpu().numpy(), dtype=np.float32)
        Cin, k = wt.shape[1], wt.shape[2]
        dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_conv_dgrad(self._h, dy.data_ptr(), Cout, wt.ctypes.data, Cin, k, dx.data_ptr(), B, H, W,
                                              _stream_ptr(self.device)), "cddpm_op_conv_dgrad")
        return dx

    def op_conv_wgrad(self, x0, x1, coef, silu, dy, ksize=3, upsample=False):
        """dL/dW [Cout,Cin,k,k] and dL/db [Cout] of y = conv_k(act(cat[x0, x1])) for dy NHWC [B,H,W,Cout]; x0 / x1 NHWC, coef [3,B,Cin] or None"""
        B, H, W, C0 = x0.shape
        C1 = x1.shape[-1] if x1 is not None else 0
        Cout = dy.shape[-1]
        dw = torch.empty((Cout, C0 + C1, ksize, ksize), dtype=torch.float32, device=self.device)
        db = torch.empty((Cout,), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_conv_wgrad(self._h, x0.data_ptr(), C0, x1.data_ptr() if x1 is not None else None, C1,
                                              coef.data_ptr() if coef is not None else None, int(bool(silu)), int(bool(upsample)),
                                              dy.data_ptr(), Cout, ksize, dw.data_ptr(), db.data_ptr(), dy.shape[0], dy.shape[1], dy.shape[2],
                                              _stream_ptr(self.device)), "cddpm_op_conv_wgrad")
        return dw, db

    def op_attention_backward(self, qkv, da, precision=32, family="f32"):
        """dL/dqkv [B,N,3C] of the attention core for da = dL/d(output) [B,N,C]; precision 16: the fp16-MFMA kernels
        (cddpm_op_attention_backward_p16, the backward of op_attention(..., precision=16)), whatever the engine's own and whatever
        `family`; family 'h3' at precision 32: the fp32-grade split kernels (cddpm_op_attention_backward_h3)"""
        what = _attention_symbol("cddpm_op_attention_backward", precision, family)
        fn = getattr(self.lib, what)
        B, N, C3 = qkv.shape
        dqkv = torch.empty_like(qkv)
        self._ck(fn(self._h, qkv.data_ptr(), da.data_ptr(), dqkv.data_ptr(), B, N, C3 // 3, _stream_ptr(self.device)), what)
        return dqkv

    def op_linear_backward(self, x, w, dy, silu_in=False):
        """backward of y = [SiLU](x) W^T + b: x [M,K], w [N,K], dy [M,N] on the device -> (dW, db, dx)"""
        M, K = x.shape
        N = w.shape[0]
        dw, db, dx = torch.empty_like(w), torch.empty((N,), dtype=torch.float32, device=self.device), torch.empty_like(x)
        self._ck(self.lib.cddpm_op_linear_backward(self._h, x.data_ptr(), w.data_ptr(), dy.data_ptr(), M, N, K, int(bool(silu_in)),
                                                   dw.data_ptr(), db.data_ptr(), dx.data_ptr(), _stream_ptr(self.device)),
                 "cddpm_op_linear_backward")
        return dw, db, dx

    def op_gn_silu_backward(self, x, da, gamma, beta, film, silu=True):
        """backward of act(GroupNorm32(x) * (1 + scale) + shift): x, da NHWC [B,H,W,C] -> (dx, dgamma, dbeta, dfilm or None)"""
        B, H, W, C = x.shape
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        g, b = f(gamma), f(beta)
        dx = torch.empty_like(x)
        dg = torch.empty((C,), dtype=torch.float32, device=self.device)
        db = torch.empty((C,), dtype=torch.float32, device=self.device)
        dfilm = torch.empty((B, 2 * C), dtype=torch.float32, device=self.device) if film is not None else None
        self._ck(self.lib.cddpm_op_gn_silu_backward(self._h, x.data_ptr(), None, 0, da.data_ptr(), g.ctypes.data, b.ctypes.data,
                                                    film.data_ptr() if film is not None else None, int(bool(silu)), dx.data_ptr(), None,
                                                    dg.data_ptr(), db.data_ptr(), dfilm.data_ptr() if dfilm is not None else None, None, 0, None,
                                                    B, H * W, C, _stream_ptr(self.device)), "cddpm_op_gn_silu_backward")
        return dx, dg, db, dfilm

    def op_gn_coef(self, src0, src1, gamma, beta, film):
        B = src0.shape[0]
        HW = src0.shape[1] * src0.shape[2]
        C0 = src0.shape[-1]
        C1 = src1.shape[-1] if src1 is not None else 0
        g = np.ascontiguousarray(gamma.detach().cpu().numpy(), dtype=np.float32)
        b = np.ascontiguousarray(beta.detach().cpu().numpy(), dtype=np.float32)
        coef = torch.empty((3, B, C0 + C1), dtype=torch.float32, device=self.device)
        self._ck(self.lib.cddpm_op_gn_coef(self._h, src0.data_ptr(), C0, src1.data_ptr() if src1 is not None else None, C1,
                                           g.ctypes.data, b.ctypes.data, film.data_ptr() if film is not None else None,
                                           coef.data_ptr(), B, HW, _stream_ptr(self.device)), "cddpm_op_gn_coef")
        return coef

    def op_attention(self, qkv, precision=32, family="f32"):
        """the attention core on qkv [B,N,3C]; precision 16: the fp16-MFMA kernel (cddpm_op_attention_p16), whatever the engine's own
        and whatever `family`; family 'h3' at precision 32: the fp32-grade split kernel (cddpm_op_attention_h3)"""
        what = _attention_symbol("cddpm_op_attention", precision, family)
        fn = getattr(self.lib, what)
        B, N, C3 = qkv.shape
        out = torch.empty((B, N, C3 // 3), dtype=torch.float32, device=self.device)
        self._ck(fn(self._h, qkv.data_ptr(), out.data_ptr(), B, N, C3 // 3, _stream_ptr(self.device)), what)
        return out

    def op_act_dropout(self, x, coef, silu, *, seed, step, slice0, stream_id, p):
        """mask / (1 - p) * [SiLU]((x - mean) a + d) with coef [3][B][C] (None: mask / (1 - p) * x); x NHWC [B,H,W,C]; the mask is
        synth.dropout_mask's (stream_id = synth.STREAM_DROPOUT + layer)"""
        B, H, W, C = x.shape
        out = torch.empty_like(x)
        self._ck(self.lib.cddpm_op_act_dropout(self._h, x.data_ptr(), coef.data_ptr() if coef is not None else None, int(bool(silu)), out.data_ptr(),
                                               seed, step, slice0, stream_id, p, B, H * W, C, _stream_ptr(self.device)), "cddpm_op_act_dropout")
        return out

    def op_dropout_scale(self, da, *, seed, step, slice0, stream_id, p):
        """da *= mask / (1 - p) in place (NHWC [B,H,W,C]); returns da"""
        B, H, W, C = da.shape
        self._ck(self.lib.cddpm_op_dropout_scale(self._h, da.data_ptr(), seed, step, slice0, stream_id, p, B, H * W, C, _stream_ptr(self.device)),
                 "cddpm_op_dropout_scale")
        return da
