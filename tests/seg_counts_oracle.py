"""Test-side CPU restatement of the hard tp / fp / fn counts of a validation step (what am_seg_hard_counts computes): plain torch integer
arithmetic on the CPU, written from the definition (anatomask_amd/include: am_seg_hard_counts) and not from the kernel.  Nothing here
runs on the HIP library.

    softmax: pred = torch.argmax over the classes (the first index of the maximum), y = the label, m = (label != ignore_label);
             a label outside [0, K) that is not the ignore label is counted (m = 1) and belongs to no class.
    sigmoid: pred_k = x_k > 0, y_k = the region channel != 0, m = the last channel == 0 when there is an ignore channel.
    tp_k = #(pred_k, y_k, m), fp_k = #(pred_k, not y_k, m), fn_k = #(not pred_k, y_k, m), summed over the batch and all voxels.

`dice_from_counts` restates on_validation_epoch_end's Dice (nnUNetTrainer.py:1005-1007) and `poly_lr` the reference's PolyLRScheduler for the
tests of SegTrainer's bookkeeping."""
from typing import Optional

import numpy as np
import torch

SOFTMAX, SIGMOID = 0, 1


def hard_counts(mode: int, logits: torch.Tensor, target: torch.Tensor, ignore_label: Optional[int] = None) -> torch.Tensor:
    """int64 [K, 3] = (tp, fp, fn).  logits [B,K,D,H,W] (any float dtype, CPU); target int labels [B,1,D,H,W] (softmax) or 0 / nonzero region
    channels [B,K(+1),D,H,W] (sigmoid; ignore_label is not None: the last channel is the ignore mask)."""
    logits, target = logits.detach().cpu(), target.detach().cpu()
    B, K = logits.shape[:2]
    ks = torch.arange(K).view(1, K, 1, 1, 1)
    if mode == SOFTMAX:
        lab = target.long()
        m = torch.ones_like(lab, dtype=torch.bool) if ignore_label is None else lab != int(ignore_label)
        pred = logits.argmax(1, keepdim=True) == ks
        y = lab == ks
    else:
        t = target != 0
        if ignore_label is not None:
            m, t = ~t[:, -1:], t[:, :-1]
        else:
            m = torch.ones_like(t[:, :1])
        pred = logits > 0
        y = t
    axes = (0, 2, 3, 4)
    tp = (pred & y & m).sum(axes)
    fp = (pred & ~y & m).sum(axes)
    fn = (~pred & y & m).sum(axes)
    return torch.stack([tp, fp, fn], 1).to(torch.int64)


def dice_from_counts(counts, drop_background: bool) -> np.ndarray:
    """2 tp / (2 tp + fp + fn) per class in fp64, NaN where the denominator is 0; softmax drops class 0."""
    c = np.asarray(counts, dtype=np.float64)
    if drop_background:
        c = c[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2 * c[:, 0] / (2 * c[:, 0] + c[:, 1] + c[:, 2])


def poly_lr(lr0: float, epoch: int, total: int, exponent: float = 0.9) -> float:
    """PolyLRScheduler.step (nnunetv2/training/lr_scheduler/polylr.py): initial_lr * (1 - current_step / max_steps) ** exponent"""
    return lr0 * (1 - epoch / total) ** exponent
