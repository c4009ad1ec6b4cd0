"""Raw volumes preprocessed on the device: smooth, crop or pad, rescale, resample.

What the reference's datamodule does to a volume on the CPU before it reaches a model (src/datamodules/create_dataset.py): `sitk_reader`
(:252-258) applies sitk.CurvatureFlow(timeStep=0.125, numberOfIterations=3) to every scalar image, and `get_transform(cfg)` (:196-218)
composes tio.CropOrPad(imageDim) (under `unisotropic_sampling`), tio.RescaleIntensity((0, 1), percentiles=(perc_low, perc_high),
masking_method='mask') and tio.Resample(rescaleFactor, image_interpolation='bspline'). `Train` (:12-50) caches the result; `Eval` (:52-92) has
no cache and repeats it per test volume in a DataLoader worker. Here one library call (cddpm_prep_volume, csrc/preprocess.hip, through
`CddpmEngine.preprocess_volume`) takes a raw [H, W, D] array to a preprocessed volume on the device: a slot of an `augment.VolumeBank`
(`VolumeBank.from_raw`) or a `test_step` batch (`EvalVolumes`).

Status: PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO AND SIMPLEITK. The stages' rules (include/cddpm.h, "Preprocessed volumes") restate
torchio >=0.18.90,<0.19 and ITK from recollection; neither was available to compare with, numpy and scipy were
(tests/preprocess_reference.py).

Out of scope: reading NIfTI files (no reader is installed, and that work is disk I/O); `resizedEvaluation: False`, which keeps the *_orig
entries at the original size (refused with NotImplementedError, as utils_eval does); volumes whose mask or segmentation has another shape
than the image (Eval :57-58 lets torchio resample them onto the image).
"""
from __future__ import annotations

from typing import Iterator, Mapping, Optional, Sequence, Tuple

import torch

from .mirror_common import _cfg_get

SMOOTH, CROPPAD, RESCALE, RESAMPLE = 1, 2, 4, 8          # stage bits (include/cddpm.h: CDDPM_PREP_*), in the reference's order
BAD_VALUE, BAD_MASK, BAD_RANGE, UNCHANGED = 1, 2, 4, 8   # status bits of the record
RECORD_SLOTS = ("status", "count", "stat_lo_k", "stat_lo_k1", "stat_hi_k", "stat_hi_k1", "cut_lo", "cut_hi", "min", "max")


def record_dict(record: torch.Tensor) -> dict:
    """the call's record as host numbers (one device-to-host copy: for logs and tests, not for the hot path)"""
    r = record.detach().cpu().tolist()
    out = dict(zip(RECORD_SLOTS, r))
    out["status"], out["count"] = int(out["status"]), int(out["count"])
    return out


class VolumePreprocess:
    """The recipe of sitk_reader + get_transform(cfg) for one volume. stages: CDDPM_PREP_* bits; target: imageDim (read under CROPPAD);
    perc: (perc_low, perc_high); factor: rescaleFactor; dt, iterations, flow_spacing: CurvatureFlow's parameters. engine: the handle the
    calls run on (None: a handle of the smallest geometry, made on first use on the input's device)."""

    def __init__(self, stages: int, target: Optional[Sequence[int]] = None, perc: Sequence[float] = (1.0, 99.0), factor: float = 1.0,
                 dt: float = 0.125, iterations: int = 3, flow_spacing: Sequence[float] = (1.0, 1.0, 1.0), engine=None):
        self.stages = int(stages)
        if self.stages & ~15:
            raise ValueError(f"unknown stage bits in {stages!r}")
        if self.stages & CROPPAD and (target is None or len(tuple(target)) != 3):
            raise ValueError(f"CROPPAD needs a target (h, w, d), got {target!r}")
        self.target = tuple(int(t) for t in target) if target is not None else None
        self.perc = (float(perc[0]), float(perc[1]))
        if not 0.0 <= self.perc[0] <= self.perc[1] <= 100.0:
            raise ValueError(f"percentiles must satisfy 0 <= lo <= hi <= 100, got {perc!r}")
        self.factor = float(factor)
        if not self.factor >= 1.0:
            raise ValueError(f"the resample factor must be >= 1, got {factor!r}")
        self.dt, self.iterations = float(dt), int(iterations)
        self.flow_spacing = tuple(float(s) for s in flow_spacing)
        self.engine, self._own = engine, False

    @classmethod
    def from_cfg(cls, cfg, *, smoothed: bool, engine=None) -> "VolumePreprocess":
        """get_transform(cfg) (create_dataset.py:196-218) with the reference's defaults -- imageDim (160, 192, 160), unisotropic_sampling
        True, perc_low 1, perc_high 99, rescaleFactor 3.0 -- preceded by sitk_reader's CurvatureFlow unless `smoothed`: the caller states
        whether the arrays already passed sitk_reader. `resizedEvaluation`, which the reference reads without a default, must be present;
        False is refused."""
        try:
            resized = cfg["resizedEvaluation"] if isinstance(cfg, Mapping) else getattr(cfg, "resizedEvaluation")
        except (KeyError, AttributeError):
            raise KeyError("resizedEvaluation: get_transform reads it without a default") from None
        if not resized:
            raise NotImplementedError("preprocess: resizedEvaluation = False (the *_orig entries at the original size) is not built natively")
        stages = RESCALE | RESAMPLE
        if not smoothed:
            stages |= SMOOTH
        if _cfg_get(cfg, "unisotropic_sampling", True):
            stages |= CROPPAD
        return cls(stages, target=tuple(_cfg_get(cfg, "imageDim", (160, 192, 160))), perc=(_cfg_get(cfg, "perc_low", 1), _cfg_get(cfg, "perc_high", 99)),
                   factor=_cfg_get(cfg, "rescaleFactor", 3.0), engine=engine)

    def output_shape(self, shape: Sequence[int]) -> Tuple[int, int, int]:
        """(H', W', D') of a raw (H, W, D) volume"""
        from .engine import CddpmEngine
        return CddpmEngine.prep_output_shape(shape, self.stages, self.target, self.factor)

    def _engine_on(self, device):
        if self.engine is None:
            from .engine import CddpmEngine
            self.engine, self._own = CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16, device=device), True
        return self.engine

    @staticmethod
    def _to_device(x, device, dtype, name):
        t = torch.as_tensor(x)
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"{name} must be [H, W, D] or [1, H, W, D], got {tuple(t.shape)}")
        if dtype == torch.uint8:
            t = (t != 0) if t.dtype == torch.bool or t.is_floating_point() else t
        return t.to(device=device, dtype=dtype).contiguous()

    def run(self, vol, mask=None, seg=None, device=None, out=None, mask_out=None) -> dict:
        """-> {"vol" [D', H', W'] fp32, "mask", "seg" (None without one) [D', H', W'] uint8, "record"} on the device, slice-major.
        vol, mask, seg: numpy arrays or tensors, on the host or the device. A floating-point or boolean label volume is read as != 0."""
        if device is None:
            device = vol.device if isinstance(vol, torch.Tensor) and vol.is_cuda else (self.engine.device if self.engine is not None else "cuda")
        device = torch.device(device)
        eng = self._engine_on(device)
        v = self._to_device(vol, eng.device, torch.float32, "vol")
        m = None if mask is None else self._to_device(mask, eng.device, torch.uint8, "mask")
        res = eng.preprocess_volume(v, m, stages=self.stages, target=self.target, perc=self.perc, f=self.factor, dt=self.dt,
                                    iterations=self.iterations, spacing=self.flow_spacing, out=out, mask_out=mask_out)
        res["seg"] = None
        if seg is not None:
            res["seg"] = eng.preprocess_labels(self._to_device(seg, eng.device, torch.uint8, "seg"), stages=self.stages, target=self.target,
                                               f=self.factor)
        return res

    def __call__(self, vol, mask=None, seg=None, device=None) -> dict:
        """-> {"vol", "mask", "seg", "record"} on the device in torchio's [1, h', w', d'] view (a permuted view of the slice-major result;
        "seg" is None without a segmentation)"""
        res = self.run(vol, mask, seg, device)
        for k in ("vol", "mask", "seg"):
            if res[k] is not None:
                res[k] = res[k].permute(1, 2, 0).unsqueeze(0)
        return res

    def close(self) -> None:
        if self._own and self.engine is not None:
            self.engine.close()
            self.engine, self._own = None, False


class EvalVolumes:
    """Iterates the batches DDPM_2D.test_step and the patched mirror read (DDPM_2D.py:188-241), one per item, preprocessed on the device as
    the reference's `Eval` dataset does per volume in a worker (create_dataset.py:52-92). items: mappings with "vol" (raw [H, W, D]) and
    optionally "mask", "seg", "ID", "label", "Dataset", "stage". A batch holds vol, vol_orig, mask_orig ({"data": [1, 1, h', w', d']}), seg_orig
    when the item has a segmentation, seg_available, ID, label, Dataset and stage. Under resizedEvaluation: True -- the only form
    built -- the *_orig entries are the same resampled tensors as the transformed ones, as in the reference. Label entries are fp32, the
    dtype torchio's LabelMap tensors reach the metrics in."""

    def __init__(self, items, device, preprocess: VolumePreprocess):
        self.items, self.device, self.preprocess = list(items), torch.device(device), preprocess

    def __len__(self) -> int:
        return len(self.items)

    def __iter__(self) -> Iterator[dict]:
        for item in self.items:
            res = self.preprocess(item["vol"], item.get("mask"), item.get("seg"), device=self.device)
            vol = res["vol"].unsqueeze(0)
            batch = {"vol": {"data": vol}, "vol_orig": {"data": vol}, "mask_orig": {"data": res["mask"].unsqueeze(0).to(torch.float32)},
                     "seg_available": res["seg"] is not None, "ID": item.get("ID"), "label": item.get("label"), "Dataset": item.get("Dataset"),
                     "stage": item.get("stage"), "record": res["record"]}
            if res["seg"] is not None:
                batch["seg_orig"] = {"data": res["seg"].unsqueeze(0).to(torch.float32)}
            yield batch
