"""Augmented training slices drawn on the device from a bank of preprocessed volumes resident in HBM.

What the reference's training datamodule does per item on the CPU (src/datamodules/create_dataset.py): `get_augment(cfg)` (:220-250) applies,
for `aug_intensity: True` -- which all three mirrored experiments set -- torchio's RandomGamma(p=.5), RandomBiasField(p=.25),
RandomBlur(p=.25) and RandomGhosting(p=.5) to the whole preloaded volume, a new draw for every item, and `vol2slice` (:143-193) keeps one
random slice. Here the volumes live in a `VolumeBank`, `IntensityAugment.draw` makes the random draws on the host (two small tables per
batch), and one library call (cddpm_aug_slices, csrc/augment.hip, through `CddpmEngine.augment_slices`) returns the batch of augmented
slices on the device, in the `{"vol": {"data": [B, 1, H, W, 1]}}` layout the mirrors' training_step and validation_step read.

Status: PINNED TO NUMPY / SCIPY, UNPINNED TO TORCHIO. The four transforms' rules (include/cddpm.h, "Augmented training slices") restate
torchio 0.18.9x from recollection; torchio was not available to compare with, numpy and scipy were (tests/augment_reference.py). The
sequence of random draws is this module's own: the reference draws inside 4 DataLoader workers with per-worker seeds and does not
reproduce against itself. Here every value is a function of (seed, epoch, position in the epoch's global order) alone -- not of the batch
size, the rank or the call history -- from synth's counter RNG on stream ids of its own.

A bank is built from preprocessed volumes (`VolumeBank(...)`) or from raw ones (`VolumeBank.from_raw`, through preprocess.py: sitk_reader's
smoothing and get_transform's crop, rescale and resample on the device, every volume written straight into its slot).

The other get_augment keys -- what someone training on a smaller data set switches on first -- go through `SliceAugment` and a second
library call (cddpm_aug_pipeline, `CddpmEngine.augment_pipeline`): get_augment's whole order as eleven gated slots, random_bias (p .25),
random_noise, random_ghosting, random_blur, random_gamma, random_affine and random_flip (.5 each), then the policy group above. The
rules of the new stages (noise from a counter RNG, the affine as a trilinear gather padded with the volume's minimum, the flip) are in
include/cddpm.h, "The augmentation pipeline", restated in tests/augment_pipeline_reference.py. `IntensityAugment` stays what it was,
refusals included. Mask and label volumes are not transformed: the mirrors' training_step reads `vol` only.

Out of scope: reading NIfTI; random_elastic and random_motion (their rules live in SimpleITK's B-spline transform and in a k-space
composite) and the vol2slice variants the training datamodule does not use (refused with NotImplementedError, the convention of
DDPM_encoder.py).
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import synth
from .mirror_common import _cfg_get

STREAM_AUGMENT = 0x6000        # counter word 3 of a sample's draws (clear of synth's 0x1001-4 and its 0x2000 ... 0x5000 + ordinal ranges)
STREAM_AUG_ORDER = 0x6001      # ... of the epoch's permutation
STREAM_AUG_NOISE = 0x6002      # ... of the noise stage's voxels, on the device (keyed by a sample's own two key words)

GAMMA, BIAS, BLUR, GHOST = 1, 2, 4, 8          # flag bits (include/cddpm.h: CDDPM_AUG_*), in Compose's order
META, PAR = 4, 28
# get_augment keys other than aug_intensity: individual transforms (with other probabilities than the policy's) and the geometric ones
REFUSED_KEYS = ("random_bias", "random_motion", "random_noise", "random_ghosting", "random_blur", "random_gamma", "random_elastic",
                "random_affine", "random_flip")
# slots of a sample's 32 draws (8 Philox quads)
_U_GATE, _U_GAMMA, _U_COEF, _U_STD, _U_INTENSITY, _W_GHOSTS, _W_AXIS, _W_Z = 0, 4, 5, 25, 28, 29, 30, 31

# the eleven slots of cddpm_aug_pipeline (include/cddpm.h: CDDPM_PIPE_*), in get_augment's order
SLOT_BIAS, SLOT_NOISE, SLOT_GHOST, SLOT_BLUR, SLOT_GAMMA, SLOT_AFFINE, SLOT_FLIP = 1, 2, 4, 8, 16, 32, 64
POLICY_GAMMA, POLICY_BIAS, POLICY_BLUR, POLICY_GHOST = 128, 256, 512, 1024
SLOTS = (SLOT_BIAS, SLOT_NOISE, SLOT_GHOST, SLOT_BLUR, SLOT_GAMMA, SLOT_AFFINE, SLOT_FLIP, POLICY_GAMMA, POLICY_BIAS, POLICY_BLUR, POLICY_GHOST)
PIPE_META, PIPE_PAR = 8, 64
_SET = 25                      # a parameter set {gamma, sigma0..2, I, c[20]}: the slot set at column 0, the policy set at 25
_COL_NOISE_STD, _COL_MATRIX = 50, 51
PIPELINE_KEYS = {"random_bias": SLOT_BIAS, "random_noise": SLOT_NOISE, "random_ghosting": SLOT_GHOST, "random_blur": SLOT_BLUR,
                 "random_gamma": SLOT_GAMMA, "random_affine": SLOT_AFFINE, "random_flip": SLOT_FLIP}
PIPELINE_REFUSED_KEYS = ("random_motion", "random_elastic")
# words 32 .. 75 of a sample's draws (quads 8 .. 18): the seven gates and the flip's inner draw, the slot set, the noise, the affine
_V_GATE, _V_FLIP_INNER, _V_GAMMA, _V_COEF, _V_STD, _V_INTENSITY, _X_GHOSTS, _X_AXIS, _V_NOISE_STD, _X_KEY, _V_SCALES, _V_DEGREES = (
    32, 39, 40, 41, 61, 64, 65, 66, 67, 68, 70, 73)
_PIPE_QUADS = 19


def _words(seed: int, c1: int, c2, stream: int, nquads: int) -> np.ndarray:
    """uint32 [len(c2), 4 nquads]: Philox4x32-10 keyed by seed at counters (quad, c1, c2, stream)"""
    c2 = np.asarray(c2, dtype=np.int64).reshape(-1, 1)
    q = np.arange(nquads, dtype=np.uint32).reshape(1, -1)
    xs = synth.philox4x32(q, np.uint32(c1 & 0xFFFFFFFF), (c2 & 0xFFFFFFFF).astype(np.uint32), np.uint32(stream), seed & 0xFFFFFFFF,
                          (seed >> 32) & 0xFFFFFFFF)
    return np.stack(xs, axis=-1).reshape(c2.shape[0], 4 * nquads)


def _below(words: np.ndarray, n: int) -> np.ndarray:
    """uint32 words -> integers uniform in 0 .. n-1 (the high bits of word * n)"""
    return ((words.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def epoch_order(seed: int, epoch: int, n: int, shuffle: bool = True) -> np.ndarray:
    """the epoch's global order of the n volumes: a permutation keyed by (seed, epoch), or 0 .. n-1"""
    if not shuffle:
        return np.arange(n, dtype=np.int64)
    w = _words(seed, epoch, np.arange(n), STREAM_AUG_ORDER, 1)
    key = (w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1].astype(np.uint64)
    return np.argsort(key, kind="stable").astype(np.int64)


class IntensityAugment:
    """The recipe of `aug_intensity: True`: Compose(RandomGamma(p=.5), RandomBiasField(p=.25), RandomBlur(p=.25), RandomGhosting(p=.5)) with
    torchio's default ranges. `p`: stage bit -> probability; a stage that is not built has none."""

    DEFAULT_P = {GAMMA: 0.5, BIAS: 0.25, BLUR: 0.25, GHOST: 0.5}
    LOG_GAMMA = (-0.3, 0.3)        # RandomGamma: gamma = exp(U)
    COEF = (-0.5, 0.5)             # RandomBiasField: coefficients = 0.5, order = 3 -> 20 coefficients
    STD = (0.0, 2.0)               # RandomBlur: std per axis in mm
    NUM_GHOSTS = (4, 10)           # RandomGhosting: num_ghosts, axes = (0, 1, 2), intensity
    INTENSITY = (0.5, 1.0)

    def __init__(self, p=None):
        self.p = dict(self.DEFAULT_P if p is None else p)
        for bit, v in self.p.items():
            if bit not in (GAMMA, BIAS, BLUR, GHOST) or not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"stage {bit!r} with probability {v!r}")

    @property
    def stages(self) -> Tuple[int, ...]:
        return tuple(b for b in (GAMMA, BIAS, BLUR, GHOST) if b in self.p)

    @classmethod
    def from_cfg(cls, cfg, onlyBrain=False, slice=None, seq_slices=None) -> "IntensityAugment":
        """get_augment(cfg) (create_dataset.py:220-250) as far as it is built: the four stages when `aug_intensity` is true, none when it is
        false. Every other key of get_augment that is set, `unique_slice`, and vol2slice's onlyBrain / slice / seq_slices are refused."""
        def refuse(what):
            raise NotImplementedError(f"augment: {what} is not built natively (aug_intensity, which the cDDPM experiments set, is)")
        for key in REFUSED_KEYS:
            if _cfg_get(cfg, key, False):
                refuse(f"get_augment's {key}")
        if _cfg_get(cfg, "unique_slice", False):
            refuse("vol2slice's unique_slice")
        for name, v in (("onlyBrain", onlyBrain), ("slice", slice is not None), ("seq_slices", seq_slices is not None)):
            if v:
                refuse(f"vol2slice({name}=...)")
        return cls() if _cfg_get(cfg, "aug_intensity", False) else cls(p={})

    def draw(self, seed: int, epoch: int, positions, D: int, spacing: Sequence[float] = (2.0, 2.0, 2.0), volumes=None):
        """-> (meta [P, 4] int32, par [P, 28] fp32), the host tables of cddpm_aug_slices for the samples at `positions` of epoch `epoch`'s
        global order. Row p is a function of (seed, epoch, positions[p]) alone. A stage's flag is set iff its uniform is below its p;
        gamma = exp(U(-0.3, 0.3)), c_i ~ U(-0.5, 0.5), std ~ U(0, 2) per axis (par holds std / spacing, in voxels), g uniform in 4 .. 10,
        axis uniform in 0 .. 2, I ~ U(0.5, 1), z uniform in 0 .. D-1. volumes: column 0 of meta (the loader's epoch order), else zeros."""
        positions = np.asarray(positions, dtype=np.int64).reshape(-1)
        w = _words(int(seed), int(epoch), positions, STREAM_AUGMENT, 8)
        u = synth._u01(w).astype(np.float64)
        P = positions.shape[0]
        flags = np.zeros(P, dtype=np.int32)
        for k, bit in enumerate((GAMMA, BIAS, BLUR, GHOST)):
            if bit in self.p:
                flags |= np.where(u[:, _U_GATE + k] < self.p[bit], bit, 0).astype(np.int32)

        def span(lo_hi, x):
            return lo_hi[0] + (lo_hi[1] - lo_hi[0]) * x
        meta = np.zeros((P, META), dtype=np.int32)
        par = np.zeros((P, PAR), dtype=np.float32)
        if volumes is not None:
            meta[:, 0] = np.asarray(volumes).reshape(-1)
        meta[:, 1] = _below(w[:, _W_Z], int(D))
        meta[:, 2] = flags
        lo, hi = self.NUM_GHOSTS
        meta[:, 3] = (lo + _below(w[:, _W_GHOSTS], hi - lo + 1)) | (_below(w[:, _W_AXIS], 3) << 8)
        par[:, 0] = np.exp(span(self.LOG_GAMMA, u[:, _U_GAMMA]))
        par[:, 1:4] = span(self.STD, u[:, _U_STD:_U_STD + 3]) / np.asarray(spacing, dtype=np.float64).reshape(1, 3)
        par[:, 4] = span(self.INTENSITY, u[:, _U_INTENSITY])
        par[:, 5:25] = span(self.COEF, u[:, _U_COEF:_U_COEF + 20])
        return meta, par


def euler_matrix(degrees) -> np.ndarray:
    """R = Rz Rx Ry in float64 (the order of ITK's Euler3DTransform by default) for the angles about axes 0, 1, 2 in degrees"""
    ax, ay, az = (float(np.deg2rad(d)) for d in degrees)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return Rz @ Rx @ Ry


def affine_matrix(degrees, scales, spacing) -> np.ndarray:
    """the affine's output-to-source voxel matrix M = diag(1 / s) diag(1 / scales) R^T diag(s) in float64, s the voxel spacing: an
    offset from the centre in output voxels goes to mm, through the inverse of the rotation and of the scaling, and back to voxels"""
    s = np.asarray(spacing, dtype=np.float64)
    return np.diag(1.0 / s) @ np.diag(1.0 / np.asarray(scales, dtype=np.float64)) @ euler_matrix(degrees).T @ np.diag(s)


class SliceAugment:
    """The general recipe: get_augment's order as the eleven slots of cddpm_aug_pipeline -- RandomBiasField(p=.25), RandomNoise(p=.5),
    RandomGhosting(p=.5), RandomBlur(p=.5), RandomGamma(p=.5), RandomAffine(p=.5), RandomFlip(axes=0, p=.5), then the `aug_intensity`
    policy group of IntensityAugment -- with torchio's default ranges. `p`: slot bit -> probability; a slot that is not built has none.
    The flip's bit is set when its gate AND RandomFlip's own flip_probability draw fall below their probabilities."""

    KEY_P = {SLOT_BIAS: 0.25, SLOT_NOISE: 0.5, SLOT_GHOST: 0.5, SLOT_BLUR: 0.5, SLOT_GAMMA: 0.5, SLOT_AFFINE: 0.5, SLOT_FLIP: 0.5}
    POLICY_P = {POLICY_GAMMA: 0.5, POLICY_BIAS: 0.25, POLICY_BLUR: 0.25, POLICY_GHOST: 0.5}      # IntensityAugment.DEFAULT_P
    NOISE_STD = (0.0, 0.25)        # RandomNoise: mean = 0, std ~ U(0, 0.25)
    SCALES = (0.9, 1.1)            # RandomAffine: scales = 0.1, degrees = 10, per axis; no translation
    DEGREES = (-10.0, 10.0)
    FLIP_PROBABILITY = 0.5         # RandomFlip's own draw, inside the p = .5 gate

    def __init__(self, p=None):
        self.p = dict({**self.KEY_P, **self.POLICY_P} if p is None else p)
        for bit, v in self.p.items():
            if bit not in SLOTS or not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"slot {bit!r} with probability {v!r}")

    @property
    def stages(self) -> Tuple[int, ...]:
        """the slots that are built, in the order they are applied"""
        return tuple(b for b in SLOTS if b in self.p)

    @classmethod
    def from_cfg(cls, cfg, onlyBrain=False, slice=None, seq_slices=None) -> "SliceAugment":
        """get_augment(cfg) (create_dataset.py:220-250): every key of PIPELINE_KEYS that is set builds its slot with the reference's
        probability, `aug_intensity` the four policy slots, in any combination. random_elastic, random_motion, `unique_slice` and
        vol2slice's onlyBrain / slice / seq_slices are refused."""
        def refuse(what):
            raise NotImplementedError(f"augment: {what} is not built natively")
        for key in PIPELINE_REFUSED_KEYS:
            if _cfg_get(cfg, key, False):
                refuse(f"get_augment's {key}")
        if _cfg_get(cfg, "unique_slice", False):
            refuse("vol2slice's unique_slice")
        for name, v in (("onlyBrain", onlyBrain), ("slice", slice is not None), ("seq_slices", seq_slices is not None)):
            if v:
                refuse(f"vol2slice({name}=...)")
        p = {bit: cls.KEY_P[bit] for key, bit in PIPELINE_KEYS.items() if _cfg_get(cfg, key, False)}
        if _cfg_get(cfg, "aug_intensity", False):
            p.update(cls.POLICY_P)
        return cls(p=p)

    def draw(self, seed: int, epoch: int, positions, D: int, spacing: Sequence[float] = (2.0, 2.0, 2.0), volumes=None):
        """-> (meta [P, 8] int32, par [P, 64] fp32), the host tables of cddpm_aug_pipeline for the samples at `positions` of epoch
        `epoch`'s global order; row p is a function of (seed, epoch, positions[p]) alone. Quads 0 .. 7 of the sample's draws mean what
        they mean to IntensityAugment.draw: z, the policy gates and the policy set are its values bit for bit. Quads 8 .. 18 hold the
        seven gates, the slot set (same ranges as the policy's), std ~ U(0, 0.25) and the two key words of the noise, and the affine's
        scales ~ U(0.9, 1.1) and degrees ~ U(-10, 10) per axis, from which affine_matrix builds M in float64."""
        positions = np.asarray(positions, dtype=np.int64).reshape(-1)
        w = _words(int(seed), int(epoch), positions, STREAM_AUGMENT, _PIPE_QUADS)
        u = synth._u01(w).astype(np.float64)
        P = positions.shape[0]
        policy = IntensityAugment(p={1 << k: self.p[bit] for k, bit in enumerate(SLOTS[7:]) if bit in self.p})
        m4, p28 = policy.draw(seed, epoch, positions, D, spacing, volumes)
        flags = m4[:, 2].astype(np.int32) << 7
        for k, bit in enumerate(SLOTS[:7]):
            if bit in self.p:
                on = u[:, _V_GATE + k] < self.p[bit]
                if bit == SLOT_FLIP:
                    on &= u[:, _V_FLIP_INNER] < self.FLIP_PROBABILITY
                flags |= np.where(on, bit, 0).astype(np.int32)

        def span(lo_hi, x):
            return lo_hi[0] + (lo_hi[1] - lo_hi[0]) * x
        I = IntensityAugment
        meta = np.zeros((P, PIPE_META), dtype=np.int32)
        par = np.zeros((P, PIPE_PAR), dtype=np.float32)
        meta[:, 0:2] = m4[:, 0:2]
        meta[:, 2] = flags
        lo, hi = I.NUM_GHOSTS
        meta[:, 3] = (lo + _below(w[:, _X_GHOSTS], hi - lo + 1)) | (_below(w[:, _X_AXIS], 3) << 8)
        meta[:, 4] = m4[:, 3]
        meta[:, 5:7] = w[:, _X_KEY:_X_KEY + 2].view(np.int32)
        par[:, 0] = np.exp(span(I.LOG_GAMMA, u[:, _V_GAMMA]))
        par[:, 1:4] = span(I.STD, u[:, _V_STD:_V_STD + 3]) / np.asarray(spacing, dtype=np.float64).reshape(1, 3)
        par[:, 4] = span(I.INTENSITY, u[:, _V_INTENSITY])
        par[:, 5:25] = span(I.COEF, u[:, _V_COEF:_V_COEF + 20])
        par[:, _SET:2 * _SET] = p28[:, :_SET]
        par[:, _COL_NOISE_STD] = span(self.NOISE_STD, u[:, _V_NOISE_STD])
        scales, degrees = span(self.SCALES, u[:, _V_SCALES:_V_SCALES + 3]), span(self.DEGREES, u[:, _V_DEGREES:_V_DEGREES + 3])
        for r in range(P):
            par[r, _COL_MATRIX:_COL_MATRIX + 9] = affine_matrix(degrees[r], scales[r], spacing).reshape(9)
        return meta, par


class VolumeBank:
    """Preprocessed volumes of one shape, resident on the device as [N, D, H, W] fp32 (slice-major: a slice is a contiguous [H, W] image).
    volumes: a list or tensor of [H, W, D] or [1, H, W, D] volumes -- torchio's layout, what the reference's cached subjects hold in
    subject['vol'].data after get_transform; permuted once here. spacing: the voxel size in mm per axis (H, W, D) after Resample."""

    def __init__(self, volumes, device, spacing: Sequence[float] = (2.0, 2.0, 2.0)):
        if isinstance(volumes, (torch.Tensor, np.ndarray)):
            volumes = list(volumes) if volumes.ndim in (4, 5) else [volumes]
        vols = []
        for v in volumes:
            v = torch.as_tensor(v)
            if v.dim() == 4 and v.shape[0] == 1:
                v = v[0]
            if v.dim() != 3:
                raise ValueError(f"a volume must be [H, W, D] or [1, H, W, D], got {tuple(v.shape)}")
            vols.append(v)
        if not vols:
            raise ValueError("an empty bank")
        if any(v.shape != vols[0].shape for v in vols):
            raise ValueError(f"every volume of a bank has one shape, got {sorted({tuple(v.shape) for v in vols})}")
        if max(vols[0].shape) > 1024:
            raise ValueError(f"every extent must be <= 1024, got {tuple(vols[0].shape)}")
        self.device = torch.device(device)
        self.spacing = tuple(float(s) for s in spacing)
        if len(self.spacing) != 3 or min(self.spacing) <= 0:
            raise ValueError(f"spacing must be three positive numbers, got {spacing!r}")
        self.data = torch.stack([v.to(torch.float32).permute(2, 0, 1) for v in vols]).contiguous().to(self.device)

    @classmethod
    def from_raw(cls, volumes, masks, device, preprocess, spacing: Optional[Sequence[float]] = None) -> "VolumeBank":
        """A bank of RAW volumes of one shape ([H, W, D] arrays or tensors, on the host or the device), each preprocessed on the device
        by `preprocess` (a preprocess.VolumePreprocess) straight into its slot: no staging copy. masks: one per volume, or None (each
        mask is then vol > 0, as `Train` builds it without a mask path, create_dataset.py:31). spacing: the voxel size after Resample,
        by default `rescaleFactor` per axis (raw volumes at 1 mm). The calls' records ([N, 16] float64, on the device) are kept in
        `records`, the preprocessed masks ([N, D', H', W'] uint8) in `masks`."""
        volumes = list(volumes)
        if not volumes:
            raise ValueError("an empty bank")
        masks = [None] * len(volumes) if masks is None else list(masks)
        if len(masks) != len(volumes):
            raise ValueError(f"{len(volumes)} volumes and {len(masks)} masks")
        shapes = {tuple(torch.as_tensor(v).shape[-3:]) for v in volumes}
        if len(shapes) != 1:
            raise ValueError(f"every volume of a bank has one shape, got {sorted(shapes)}")
        h, w, d = preprocess.output_shape(next(iter(shapes)))
        self = cls.__new__(cls)
        self.device = torch.device(device)
        self.spacing = tuple(float(s) for s in (spacing if spacing is not None else (preprocess.factor,) * 3))
        if len(self.spacing) != 3 or min(self.spacing) <= 0:
            raise ValueError(f"spacing must be three positive numbers, got {spacing!r}")
        self.data = torch.empty(len(volumes), d, h, w, dtype=torch.float32, device=self.device)
        self.masks = torch.empty(len(volumes), d, h, w, dtype=torch.uint8, device=self.device)
        records = [preprocess.run(v, m, device=self.device, out=self.data[n], mask_out=self.masks[n])["record"]
                   for n, (v, m) in enumerate(zip(volumes, masks))]
        self.records = torch.stack(records)
        return self

    def __len__(self) -> int:
        return self.data.shape[0]

    @property
    def shape(self) -> Tuple[int, int, int]:
        """(H, W, D)"""
        return (self.data.shape[2], self.data.shape[3], self.data.shape[1])


class DeviceSliceLoader:
    """Iterates one epoch of training batches {"vol": {"data": x}}, x [B, 1, H, W, 1] fp32 on the bank's device: one random slice of every
    volume in the epoch's order (vol2slice over the volume dataset), augmented as `augment` draws (None: plain slices).
    The epoch's order and every sample's draws are keyed by (seed, epoch, position in the global order). Global batch k holds positions
    [k world B, (k + 1) world B) and rank r takes its rows [r B, (r + 1) B): the union over the ranks is the one-rank run of batch
    world * B, bit for bit. drop_last=False keeps a last, shorter global batch; a rank whose rows fall outside it yields nothing for it.
    Each step is one asynchronous host-to-device copy of the two tables and one cddpm_aug_slices call (CddpmEngine.augment_slices); the
    workspace is asked for once. augment: an IntensityAugment or None (that call), or a SliceAugment, whose tables go to
    cddpm_aug_pipeline (CddpmEngine.augment_pipeline) instead. engine: the handle the call runs on (None: a handle of the smallest geometry, made here)."""

    def __init__(self, bank: VolumeBank, batch_size: int, seed: int, augment=None, shuffle: bool = True,
                 drop_last: bool = True, rank: int = 0, world: int = 1, engine=None):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"batch_size {batch_size}, rank {rank} of world {world}")
        self.bank, self.B, self.seed, self.shuffle, self.drop_last = bank, int(batch_size), int(seed), bool(shuffle), bool(drop_last)
        self.augment = augment if augment is not None else IntensityAugment(p={})
        self.rank, self.world, self.epoch = int(rank), int(world), 0
        self._own = engine is None
        if engine is None:
            from .engine import CddpmEngine
            engine = CddpmEngine(timesteps=2, max_batch=1, max_h=16, max_w=16, device=bank.device)
        self.engine = engine

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _rows(self):
        """per global batch: this rank's (first position, count)"""
        n, G = len(self.bank), self.world * self.B
        out = []
        for k in range(n // G if self.drop_last else -(-n // G)):
            lo = k * G + self.rank * self.B
            cnt = min(self.B, min(n, (k + 1) * G) - lo)
            if cnt > 0:
                out.append((lo, cnt))
        return out

    def __len__(self) -> int:
        return len(self._rows())

    def tables(self, first: int, count: int):
        """(meta, par) of the positions [first, first + count) of the current epoch"""
        order = epoch_order(self.seed, self.epoch, len(self.bank), self.shuffle)
        pos = np.arange(first, first + count)
        return self.augment.draw(self.seed, self.epoch, pos, self.bank.shape[2], self.bank.spacing, volumes=order[pos])

    def __iter__(self) -> Iterator[dict]:
        H, W, _D = self.bank.shape
        for first, count in self._rows():
            meta, par = self.tables(first, count)
            call = self.engine.augment_pipeline if isinstance(self.augment, SliceAugment) else self.engine.augment_slices
            x = call(self.bank, meta, par)
            yield {"vol": {"data": x.view(count, 1, H, W, 1)}}

    def close(self) -> None:
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None
