"""The segmentation fine-tuning loss on the HIP path: fused Dice + CE / Dice + BCE with deep supervision, and its logit gradient.

The classes carry the reference's names and constructor signatures (nnunetv2/training/loss/compound_losses.py, dice.py,
deep_supervision.py), so nnUNetTrainer._build_loss (nnUNetTrainer.py:342-365) ports by changing an import; `build_loss` restates it.

    loss_fn = build_loss(num_levels=5, batch_dice=True)                # DeepSupervisionWrapper(DC_and_CE_loss(...), weights)
    outputs = net(data)                                                # five fp32 logits tensors [B,K,D,H,W], finest first
    targets = data_mod.deep_supervision_targets(target, scales)       # strided int16 views: consumed as they are, no copy
    loss = loss_fn(outputs, targets)                                   # 0-dim fp32 tensor on the device
    loss.backward()                                                    # fills .grad of every logits tensor that requires it

Per level three launches compute the loss (ops.seg_loss_sums: one sweep of the logits -> per-class sums, folded in fp64 in a fixed
order; ops.seg_loss_coeffs: sums -> loss and gradient coefficients on the device) and one the gradient (ops.seg_loss_grad, in backward,
scaled by the upstream gradient read from device memory).  Nothing is read back to the host; two calls on the same input give the same bits.

What differs from the reference, on purpose:
  * a label outside [0, K) that is not the ignore label belongs to no class (y = 0 everywhere, its CE term is the log-sum-exp); the
    reference's scatter_ raises there;
  * DeepSupervisionWrapper skips a level whose weight is 0 (nnU-Net's last level); the reference evaluates it and multiplies by 0: the
    same value for finite logits.  Its logits receive a zero gradient;
  * MemoryEfficientSoftDiceLoss and SoftDiceLoss are the same function of the sums here (2 tp + fp + fn = sum_pred + sum_gt): they are
    the `dice_class` tag and hold the Dice keyword arguments; they are not callable on their own.
Not served (NotImplementedError naming the argument): clip_tp, non-empty ce_kwargs / bce_kwargs (class weights, label smoothing),
a caller's apply_nonlin, inputs that are not 5-D, and batch Dice with ddp=True in a process group of more than one rank: the reference
sums tp / fp / fn across ranks there (AllGatherGrad); the seam for that is the sums table between ops.seg_loss_sums and
ops.seg_loss_coeffs.  CPU tensors raise RuntimeError: there is no CPU path."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import ops

__all__ = ["MemoryEfficientSoftDiceLoss", "SoftDiceLoss", "DC_and_CE_loss", "DC_and_BCE_loss", "DeepSupervisionWrapper", "build_loss"]


class MemoryEfficientSoftDiceLoss(nn.Module):
    """dice.py:58-70: holder of (batch_dice, do_bg, smooth, ddp) for DC_and_CE_loss / DC_and_BCE_loss, which set the nonlinearity."""

    def __init__(self, apply_nonlin=None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1., ddp: bool = True):
        super().__init__()
        if apply_nonlin is not None:
            raise NotImplementedError("apply_nonlin: the fused loss applies softmax (DC_and_CE_loss) or sigmoid (DC_and_BCE_loss) itself")
        self.apply_nonlin, self.batch_dice, self.do_bg, self.smooth, self.ddp = None, bool(batch_dice), bool(do_bg), float(smooth), bool(ddp)

    def forward(self, x, y, loss_mask=None):
        raise NotImplementedError(f"{type(self).__name__} is evaluated inside DC_and_CE_loss / DC_and_BCE_loss only (one fused pass)")


class SoftDiceLoss(MemoryEfficientSoftDiceLoss):
    """dice.py:8-20: as MemoryEfficientSoftDiceLoss; clip_tp is not served."""

    def __init__(self, apply_nonlin=None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1., ddp: bool = True,
                 clip_tp: Optional[float] = None):
        if clip_tp is not None:
            raise NotImplementedError(f"clip_tp={clip_tp}: clipping the true positives is not implemented")
        super().__init__(apply_nonlin, batch_dice, do_bg, smooth, ddp)
        self.clip_tp = None


def _make_dice(dice_class, soft_dice_kwargs) -> MemoryEfficientSoftDiceLoss:
    if dice_class not in (MemoryEfficientSoftDiceLoss, SoftDiceLoss):
        raise NotImplementedError(f"dice_class={dice_class!r}: MemoryEfficientSoftDiceLoss or SoftDiceLoss of this module")
    if "apply_nonlin" in soft_dice_kwargs:
        raise NotImplementedError("apply_nonlin in soft_dice_kwargs: the compound loss sets the nonlinearity itself")
    return dice_class(**soft_dice_kwargs)


class _FusedLevels(torch.autograd.Function):
    """sum_i w_i loss(logits_i, target_i) over the levels with w_i != 0: the levels' kernels issue back to back on the current stream and
    add into one device scalar.  backward: one gradient launch per level, scaled by (upstream gradient on the device) * w_i."""

    @staticmethod
    def forward(ctx, spec: "_Compound", weights, targets, *logits):
        dev = logits[0].device
        total = torch.zeros(1, device=dev, dtype=torch.float32)
        lses, coefs = [], []
        for i, (x, t, w) in enumerate(zip(logits, targets, weights)):
            if w == 0:
                lses.append(None)
                coefs.append(None)
                continue
            sums, lse = ops.seg_loss_sums(spec.mode, x, t, spec.kernel_ignore, keep_lse=ctx.needs_input_grad[3 + i])
            coef, _ = ops.seg_loss_coeffs(spec.mode, sums, x.shape[2] * x.shape[3] * x.shape[4], spec.dc.batch_dice, spec.dc.do_bg,
                                          spec.kernel_ignore is not None, spec.dc.smooth, spec.weight_dice, spec.weight_ce, w, total)
            lses.append(lse)
            coefs.append(coef)
        ctx.spec, ctx.weights, ctx.n = spec, weights, len(logits)
        ctx.save_for_backward(*logits, *targets, *lses, *coefs)
        return total.reshape(())

    @staticmethod
    def backward(ctx, gout):
        n, sv = ctx.n, ctx.saved_tensors
        logits, targets, lses, coefs = sv[:n], sv[n:2 * n], sv[2 * n:3 * n], sv[3 * n:4 * n]
        g = gout.detach().to(torch.float32).reshape(1).contiguous()
        grads = []
        for i in range(n):
            if not ctx.needs_input_grad[3 + i]:
                grads.append(None)
            elif ctx.weights[i] == 0:
                grads.append(torch.zeros_like(logits[i]))
            else:
                grads.append(ops.seg_loss_grad(ctx.spec.mode, logits[i], targets[i], ctx.spec.kernel_ignore, lses[i], coefs[i], g,
                                               ctx.weights[i]))
        return (None, None, None, *grads)


class _Compound(nn.Module):
    mode: int
    kernel_ignore: Optional[int]          # softmax: the ignore label; sigmoid: anything but None = the last target channel is the mask

    def _prepare_target(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _check(self, net_output: torch.Tensor, target: torch.Tensor):
        if not isinstance(net_output, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise TypeError("net_output and target must be tensors")
        if net_output.dim() != 5:
            raise NotImplementedError(f"net_output of {net_output.dim()} dimensions: [B, K, D, H, W] (3-D volumes) only")
        if self.dc.ddp and self.dc.batch_dice and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("ddp=True with batch_dice in a process group of more than one rank: the cross-rank sums of "
                                      "tp / fp / fn (AllGatherGrad) are not implemented")
        if net_output.device.type != "cuda" or target.device.type != "cuda":
            raise RuntimeError("the segmentation loss runs on the HIP kernels: move net_output and target to a cuda (ROCm) device first")
        if net_output.dtype != torch.float32:
            raise NotImplementedError(f"net_output of dtype {net_output.dtype}: fp32 logits only")

    def _levels(self, outputs: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], weights: Sequence[float]) -> torch.Tensor:
        xs, ts = [], []
        for x, t in zip(outputs, targets):
            self._check(x, t)
            xs.append(x if x.is_contiguous() else x.contiguous())
            ts.append(self._prepare_target(x, t))
        return _FusedLevels.apply(self, tuple(float(w) for w in weights), tuple(ts), *xs)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self._levels([net_output], [target], [1.0])


class DC_and_CE_loss(_Compound):
    """compound_losses.py:8-57.  target: labels [B,1,D,H,W] (or [B,D,H,W]); int16 is read as it is (any strides), other integer or float
    dtypes are converted to int16 first."""
    mode = ops.SEG_SOFTMAX

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None, dice_class=SoftDiceLoss):
        super().__init__()
        if ce_kwargs:
            raise NotImplementedError(f"ce_kwargs={ce_kwargs}: class weights, label smoothing and other CrossEntropyLoss options are not implemented")
        self.weight_dice, self.weight_ce, self.ignore_label = float(weight_dice), float(weight_ce), ignore_label
        if ignore_label is not None and not -32768 <= int(ignore_label) <= 32767:
            raise ValueError(f"ignore_label={ignore_label} does not fit the int16 labels")
        self.kernel_ignore = None if ignore_label is None else int(ignore_label)
        self.dc = _make_dice(dice_class, soft_dice_kwargs)

    def _prepare_target(self, net_output, target):
        if target.dim() == 4:
            target = target.unsqueeze(1)
        if target.dtype == torch.bool or target.is_complex():
            raise TypeError(f"label target of dtype {target.dtype}")
        return target if target.dtype == torch.int16 else target.to(torch.int16)


class DC_and_BCE_loss(_Compound):
    """compound_losses.py:60-100.  target: region channels [B,K,D,H,W] holding 0 / 1, with use_ignore_label one more channel, the ignore
    mask, last; uint8 and bool are read as they are (any strides), float targets are converted to uint8 first."""
    mode = ops.SEG_SIGMOID

    def __init__(self, bce_kwargs, soft_dice_kwargs, weight_ce=1, weight_dice=1, use_ignore_label: bool = False,
                 dice_class=MemoryEfficientSoftDiceLoss):
        super().__init__()
        if bce_kwargs:
            raise NotImplementedError(f"bce_kwargs={bce_kwargs}: weights and other BCEWithLogitsLoss options are not implemented")
        self.weight_dice, self.weight_ce, self.use_ignore_label = float(weight_dice), float(weight_ce), bool(use_ignore_label)
        self.kernel_ignore = 1 if use_ignore_label else None
        self.dc = _make_dice(dice_class, soft_dice_kwargs)

    def _prepare_target(self, net_output, target):
        if target.dtype in (torch.uint8, torch.bool):
            return target
        if not target.is_floating_point():
            raise TypeError(f"region target of dtype {target.dtype}: uint8, bool or a float dtype")
        return target.to(torch.uint8)


class DeepSupervisionWrapper(nn.Module):
    """deep_supervision.py:4-35: l = sum_i w_i loss(outputs[i], targets[i]), weights 1 when None.  `loss` is a DC_and_CE_loss or a
    DC_and_BCE_loss of this module; a level of weight 0 is skipped."""

    def __init__(self, loss, weight_factors=None):
        super().__init__()
        if not isinstance(loss, _Compound):
            raise NotImplementedError(f"loss={type(loss).__name__}: DeepSupervisionWrapper wraps DC_and_CE_loss / DC_and_BCE_loss of this module")
        self.weight_factors = weight_factors
        self.loss = loss

    def forward(self, *args):
        if len(args) != 2 or not all(isinstance(a, (tuple, list)) for a in args) or len(args[0]) != len(args[1]):
            raise ValueError("DeepSupervisionWrapper(outputs, targets): two lists (or tuples) of the same length, one entry per level")
        weights = [1.0] * len(args[0]) if self.weight_factors is None else list(self.weight_factors)
        if len(weights) < len(args[0]):
            raise ValueError(f"{len(weights)} weight factors for {len(args[0])} levels")
        return self.loss._levels(args[0], args[1], weights[:len(args[0])])


def build_loss(num_levels: int, batch_dice: bool, regions: bool = False, ignore_label: Optional[int] = None) -> DeepSupervisionWrapper:
    """nnUNetTrainer._build_loss (nnUNetTrainer.py:342-365): Dice (smooth 1e-5) + CE without background, or + BCE with it for region-based
    labels; weights 1 / 2^i over the levels, the last one zeroed, normalised to sum 1."""
    is_ddp = torch.distributed.is_available() and torch.distributed.is_initialized()
    if regions:
        loss = DC_and_BCE_loss({}, {"batch_dice": batch_dice, "do_bg": True, "smooth": 1e-5, "ddp": is_ddp},
                               use_ignore_label=ignore_label is not None, dice_class=MemoryEfficientSoftDiceLoss)
    else:
        loss = DC_and_CE_loss({"batch_dice": batch_dice, "smooth": 1e-5, "do_bg": False, "ddp": is_ddp}, {}, weight_ce=1, weight_dice=1,
                              ignore_label=ignore_label, dice_class=MemoryEfficientSoftDiceLoss)
    weights = np.ldexp(1.0, -np.arange(num_levels))          # halved per level; the coarsest level does not count
    weights[-1] = 0.0
    return DeepSupervisionWrapper(loss, weights / weights.sum())
