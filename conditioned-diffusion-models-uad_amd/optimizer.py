"""What the trainers of this package share of the optimizer (training.UNetTrainer, encoder_training.EncoderTrainer,
spark_training.SparKTrainer): the four things include/cddpm.h fixes for all of them, each stated once.

  flat buffers    every tensor padded to 64 floats (256 bytes) inside ONE fp32 buffer (`flat`, views `p[name]`), the gradients in a second
                  (`gflat`, `g[name]`), Adam's moments in two more (`state["m"]`, `state["v"]`, made at the first use)
  control block   `ctrl`, int32[8] on the device: {non-finite flag, optimizer step, skip, skipped so far, bias corrections}
  guarded update  "Per optimisation step" of the header: cddpm_op_grad_check on every gradient buffer, one cddpm_op_guard_commit (`guard`),
                  one Adam / AdamW launch per parameter buffer (`update`), one cddpm_op_scaler_update (`update_loss_scale`)
  loss scaler     torch GradScaler's rule on the device block `scaler`, int32[4]: its checked settings, creation, reads, checkpoint entry

The rule: ONE optimizer is one control block plus at most one scaler, and any number of flat buffers are stepped under it -- `guard` and
`update` take the optimizer and the buffer owners apart. A trainer is a FlatOptimizer: it owns one buffer and a control block; whether it
is also the optimizer of a step is the caller's choice (the UNet trainer's blocks serve the jointly trained encoder, the SparK trainer's
its sparse encoder). The class asks of its subclass what the operators need: `lib`, `h`, `_ck(rc, what)`, `_s()`."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------- the loss scaler's settings and device block
def _power_of_two(x) -> bool:
    try:
        x = float(x)
    except (TypeError, ValueError):
        return False
    return math.isfinite(x) and x > 0 and math.frexp(x)[0] == 0.5


def _integer(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and int(x) == x


def _scale_of(block: torch.Tensor) -> torch.Tensor:
    """the fp32 loss scale inside a scaler block, as a view of its first word"""
    return block[:1].view(torch.float32)


def _scaler_block(scale: float, tracker: int, skips: int, dev) -> torch.Tensor:
    """the device scaler state of include/cddpm.h: int32[4] = {bits of the fp32 loss scale, growth tracker, consecutive skips, 0}"""
    blk = torch.tensor([0, int(tracker), int(skips), 0], dtype=torch.int32)
    _scale_of(blk).fill_(float(scale))
    return blk.to(dev)


def loss_scaling_settings(init_scale=None, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, growth_tracker=0) -> Dict[str, object]:
    """the checked arguments of enable_loss_scaling (torch GradScaler's defaults; init_scale None: the trainer's default start).
    The scale and both factors must be powers of two (growth > 1, backoff < 1) so that unscaling stays exact; ValueError otherwise."""
    if init_scale is not None and not (_power_of_two(init_scale) and float(init_scale) < 2.0 ** 127):
        raise ValueError(f"init_scale must be a finite power of two, got {init_scale!r}")
    if not (_power_of_two(growth_factor) and float(growth_factor) > 1.0):
        raise ValueError(f"growth_factor must be a power of two > 1, got {growth_factor!r}")
    if not (_power_of_two(backoff_factor) and float(backoff_factor) < 1.0):
        raise ValueError(f"backoff_factor must be a power of two < 1, got {backoff_factor!r}")
    if not (_integer(growth_interval) and 1 <= growth_interval < 2 ** 31):
        raise ValueError(f"growth_interval must be an integer >= 1, got {growth_interval!r}")
    if not (_integer(growth_tracker) and 0 <= growth_tracker < 2 ** 31):
        raise ValueError(f"growth_tracker must be an integer >= 0, got {growth_tracker!r}")
    return {"init_scale": None if init_scale is None else float(init_scale), "growth_factor": float(growth_factor),
            "backoff_factor": float(backoff_factor), "growth_interval": int(growth_interval), "growth_tracker": int(growth_tracker)}


def loss_scaling_from_grad_scaler(state) -> Dict[str, object]:
    """enable_loss_scaling's arguments from a torch GradScaler.state_dict() -- what Lightning 1.5's native AMP plugin stores in
    a checkpoint under `native_amp_scaling_state`: {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}.
    Values outside what enable_loss_scaling accepts raise ValueError."""
    return loss_scaling_settings(float(state["scale"]), state.get("growth_factor", 2.0), state.get("backoff_factor", 0.5),
                                 state.get("growth_interval", 2000), state.get("_growth_tracker", 0))


# ---------------------------------------------------------------------- the guarded update: one optimizer, any number of buffers
def moments(owner):
    """Adam's (m, v) of a buffer owner, zero until its first update"""
    st = owner.state
    if "m" not in st:
        st["m"], st["v"] = torch.zeros_like(owner.flat), torch.zeros_like(owner.flat)
    return st["m"], st["v"]


def guard(opt, owners, betas=(0.9, 0.999)):
    """checks the gradient buffers of `owners` for inf / NaN and commits the decision for this step in `opt.ctrl`, on the device: a step
    with a non-finite gradient anywhere neither updates parameters / moments nor advances the step count"""
    for o in owners:
        opt._ck(opt.lib.cddpm_op_grad_check(opt.h, _p(o.gflat), o.gflat.numel(), _p(opt.ctrl), opt._s()), "op_grad_check")
    opt._ck(opt.lib.cddpm_op_guard_commit(opt.h, _p(opt.ctrl), C.c_float(betas[0]), C.c_float(betas[1]), opt._s()), "op_guard_commit")


def update(opt, owner, lr, betas, eps, *, weight_decay=None, unscale=1.0, scaler=None):
    """one launch over `owner`'s flat buffers (anything with flat, gflat, state) under the decision `guard` left in `opt.ctrl`.
    weight_decay None: torch.optim.Adam's update, a number: AdamW's (decoupled decay first) -- two entry points of their own, not one
    with a zero decay. The gradient is gflat * unscale; with `scaler` (the block this step's loss was formed with) it is divided by the
    device scale as well (the header's extra_unscale)."""
    lib, (m, v) = opt.lib, moments(owner)
    if weight_decay is None:
        op, what = (lib.cddpm_op_adam_guarded, "op_adam_guarded") if scaler is None else (lib.cddpm_op_adam_scaled, "op_adam_scaled")
        decay = ()
    else:
        op, what = (lib.cddpm_op_adamw_guarded, "op_adamw_guarded") if scaler is None else (lib.cddpm_op_adamw_scaled, "op_adamw_scaled")
        decay = (C.c_float(weight_decay),)
    blocks = (_p(opt.ctrl),) if scaler is None else (_p(opt.ctrl), _p(scaler))
    opt._ck(op(opt.h, _p(owner.flat), _p(owner.gflat), _p(m), _p(v), owner.flat.numel(), C.c_float(lr), C.c_float(betas[0]), C.c_float(betas[1]),
               C.c_float(eps), *decay, C.c_float(unscale), *blocks, opt._s()), what)


class FlatOptimizer:
    """One flat parameter buffer with its gradients and moments, a control block, and an optional loss scaler (module docstring)."""

    DEFAULT_INIT_SCALE: Optional[float] = None      # where the scaler starts when no init_scale is given. None: the block is made at the
                                                    # first loss, from its batch (_start_scaler); a number: at once, by enable_loss_scaling
    LAYOUT_ERROR = "optimizer state was saved for another parameter layout"
    grad_scale: Optional[float] = None              # the fixed loss scale of the last loss, for a trainer that forms one

    def __init__(self, params: Dict[str, torch.Tensor], names, device):
        """`names`: the keys of `params` that are trained, in the order they take in the buffer"""
        self.dev = torch.device(device)
        sizes = [(int(params[k].numel()) + 63) // 64 * 64 for k in names]       # 256-byte aligned views
        self.flat = torch.zeros(sum(sizes), dtype=torch.float32, device=self.dev)
        self.gflat = torch.zeros_like(self.flat)
        self.p: Dict[str, torch.Tensor] = {}
        self.g: Dict[str, torch.Tensor] = {}
        off = 0
        for k, n in zip(names, sizes):
            v = params[k]
            self.p[k] = self.flat[off:off + v.numel()].view(v.shape)
            self.g[k] = self.gflat[off:off + v.numel()].view(v.shape)
            self.p[k].copy_(v.detach().to(self.dev, torch.float32))
            off += n
        self.state: Dict[str, object] = {}
        self.ctrl = torch.zeros(8, dtype=torch.int32, device=self.dev)
        self.loss_scaling = False           # dynamic loss scaling (enable_loss_scaling); off: a fixed scale, or none
        self.scaler: Optional[torch.Tensor] = None

    def join_side(self):
        """runs before the host reads or writes the scaler block; a trainer with work on a side stream makes the main stream wait for it"""

    # ------------------------------------------------------------------ control block
    @property
    def step_count(self) -> int:
        """optimizer steps taken (skipped ones do not count); reads the device counter (synchronises)"""
        return int(self.ctrl[1].item())

    @property
    def skipped_steps(self) -> int:
        return int(self.ctrl[3].item())

    # ------------------------------------------------------------------ checkpoint pieces: layout, moments
    def layout(self):
        return [(k, int(v.numel())) for k, v in self.p.items()]

    def check_layout(self, saved) -> None:
        if [tuple(x) for x in saved] != self.layout():
            raise ValueError(self.LAYOUT_ERROR)

    def load_moments(self, m, v) -> None:
        self.state["m"], self.state["v"] = m.to(self.dev, torch.float32).clone(), v.to(self.dev, torch.float32).clone()

    # ------------------------------------------------------------------ dynamic loss scaling (torch's GradScaler, the scale on the device)
    def enable_loss_scaling(self, init_scale=None, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, growth_tracker=0):
        """turns on dynamic loss scaling with torch.cuda.amp.GradScaler's rule (torch._amp_update_scale_) on the device block of
        include/cddpm.h ("Dynamic loss scaling"): a skipped step multiplies the scale by backoff_factor, `growth_interval` clean steps in
        a row by growth_factor. Scale and factors must be powers of two (the unscale is then exact: a step at scale S is bit-identical to
        the same step at the fixed scale S); invalid values raise ValueError. init_scale None: the class's DEFAULT_INIT_SCALE. Starts a
        fresh scaler state (growth tracker `growth_tracker`, no skips) -- at once where the class has a default start, else at the next
        loss. No step reads the scale back."""
        cfg = loss_scaling_settings(self.DEFAULT_INIT_SCALE if init_scale is None else init_scale, growth_factor, backoff_factor,
                                    growth_interval, growth_tracker)
        self.scaler_init = cfg["init_scale"]
        self.scaler_cfg = (cfg["growth_factor"], cfg["backoff_factor"], cfg["growth_interval"])
        self.scaler_tracker0 = cfg["growth_tracker"]
        self.scaler = None
        self.loss_scaling = True
        if self.DEFAULT_INIT_SCALE is not None:
            self._start_scaler()

    def disable_loss_scaling(self):
        """back to the fixed scale (or unscaled gradients) and the plain guarded update. A trainer whose precision-16 backward needs the
        scale (SparKTrainer) then trains its encoder on flushed gradients unless the loss weights carry a scale themselves."""
        self.loss_scaling, self.scaler = False, None

    def _start_scaler(self, default=None):
        """the device block, made once per enable_loss_scaling: at the configured start, or at `default` where none was configured"""
        if self.scaler is None:
            self.scaler = _scaler_block(self.scaler_init if self.scaler_init is not None else default, self.scaler_tracker0, 0, self.dev)

    def step_scaler(self, grad_scale=None) -> Optional[torch.Tensor]:
        """the scaler block the updates of this step unscale by; None: the step runs at a fixed scale (scaling off, or grad_scale given)"""
        if not self.loss_scaling or grad_scale is not None:
            return None
        if self.scaler is None:
            raise RuntimeError("adam_step with dynamic loss scaling: no loss was formed yet (loss_and_grad)")
        return self.scaler

    def update_loss_scale(self):
        """step (d) of include/cddpm.h's dynamic loss scaling: after every update of the step, the scale follows the step's skip
        decision (one single-thread launch on the main stream)"""
        self.join_side()
        g, b, n = self.scaler_cfg
        self._ck(self.lib.cddpm_op_scaler_update(self.h, _p(self.ctrl), _p(self.scaler), C.c_float(g), C.c_float(b), n, self._s()),
                 "op_scaler_update")

    def loss_scale_tensor(self) -> torch.Tensor:
        """the device scale as a 0-d fp32 view of the scaler block: for logging without a read-back"""
        return _scale_of(self.scaler)[0]

    def _scaler_read(self, i):
        self.join_side()
        if self.scaler is None:
            return None
        return _scale_of(self.scaler).item() if i == 0 else int(self.scaler[i].item())

    @property
    def loss_scale(self) -> Optional[float]:
        """the loss scale the next step is formed with: the device scale when dynamic scaling is on (reads it: synchronises; before the
        block exists the configured start, None for the batch-size default), else the fixed scale of the last loss (None: there is none)"""
        if not self.loss_scaling:
            return self.grad_scale
        return self._scaler_read(0) if self.scaler is not None else self.scaler_init

    @property
    def growth_tracker(self) -> int:
        """clean steps since the scale last changed (dynamic scaling; reads the device counter)"""
        if self.scaler is not None:
            return self._scaler_read(1)
        return self.scaler_tracker0 if self.loss_scaling else 0

    @property
    def consecutive_skips(self) -> int:
        """skipped steps in a row up to now (dynamic scaling; reads the device counter)"""
        return self._scaler_read(2) if self.scaler is not None else 0

    def scaler_state(self) -> Dict[str, object]:
        """the "scaler" entry of optimizer_state(): the settings and the device block (None before it exists)"""
        self.join_side()
        g, b, n = self.scaler_cfg
        return {"init_scale": self.scaler_init, "growth_factor": g, "backoff_factor": b, "growth_interval": n,
                "growth_tracker": self.scaler_tracker0, "state": None if self.scaler is None else self.scaler.detach().clone()}

    def load_scaler_state(self, sc) -> None:
        """restores what scaler_state returned. None (a state saved without dynamic loss scaling): the scaler is left as it is"""
        if sc is None:
            return
        self.enable_loss_scaling(init_scale=sc["init_scale"], growth_factor=sc["growth_factor"], backoff_factor=sc["backoff_factor"],
                                 growth_interval=sc["growth_interval"], growth_tracker=sc["growth_tracker"])
        if sc.get("state") is not None:
            self.join_side()
            self.scaler = sc["state"].to(self.dev, torch.int32).clone()
