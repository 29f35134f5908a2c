"""Test-side restatement of the segmentation loss in plain torch, generic in dtype and device: the yardstick of the GPU tests of
anatomask_amd.seg_loss (tests/test_seg_loss_cpu.py pins it, in fp64, to the reference's own results in tests/golden/seg_loss_*.npz).
Written from the formulas, not from the reference's code; gradients come from autograd.  Nothing here runs on the HIP library.

With p the softmax (sigmoid) of the logits over the classes, y the one-hot labels (region channels), m the voxel mask (0 where the label
is the ignore label / the ignore channel is set) and, per class (and per sample unless batch_dice), I = sum p y m, P = sum p m, G = sum y m:

    dice = -mean_c (2 I_c + smooth) / max(G_c + P_c + smooth, 1e-8)        (c from 1 when do_bg is False)
    ce   = sum_v m (lse - sum_k y_k x_k) / sum_v m                         (0 when no voxel is left)
    bce  = sum m (softplus(x) - x y) / (B K N)   or, with the ignore channel,   / max(sum_v m, 1e-8)
    loss = weight_ce ce (bce) + weight_dice dice

A label outside [0, K) that is not the ignore label has y = 0 in every class: its CE term is lse."""
from typing import Optional, Sequence

import torch


def _dice(I: torch.Tensor, P: torch.Tensor, G: torch.Tensor, batch_dice: bool, do_bg: bool, smooth: float) -> torch.Tensor:
    if batch_dice:
        I, P, G = I.sum(0, keepdim=True), P.sum(0, keepdim=True), G.sum(0, keepdim=True)
    dc = (2 * I + smooth) / torch.clamp(G + P + smooth, min=1e-8)
    if not do_bg:
        dc = dc[:, 1:]
    return -dc.mean()


def dice_ce(logits: torch.Tensor, labels: torch.Tensor, batch_dice: bool, do_bg: bool = False, smooth: float = 1e-5, weight_ce: float = 1.0,
            weight_dice: float = 1.0, ignore_label: Optional[int] = None) -> torch.Tensor:
    """logits [B,K,...] (any float dtype), labels [B,1,...] (any integer / float dtype holding integers) -> 0-dim loss in logits.dtype."""
    B, K = logits.shape[:2]
    x = logits.reshape(B, K, -1)
    lab = labels.reshape(B, -1).long()
    valid = torch.ones_like(lab, dtype=torch.bool) if ignore_label is None else lab != ignore_label
    m = valid.to(x.dtype)
    y = ((lab[:, None, :] == torch.arange(K, device=x.device)[None, :, None]) & valid[:, None, :]).to(x.dtype)
    lse = torch.logsumexp(x, dim=1)
    p = torch.exp(x - lse[:, None, :])
    dice = _dice((p * y).sum(-1), (p * m[:, None, :]).sum(-1), y.sum(-1), batch_dice, do_bg, smooth)
    n = m.sum()
    ce = (m * (lse - (y * x).sum(1))).sum() / n if bool(n > 0) else x.new_zeros(())
    return weight_ce * ce + weight_dice * dice


def dice_bce(logits: torch.Tensor, regions: torch.Tensor, batch_dice: bool, do_bg: bool = True, smooth: float = 1e-5, weight_ce: float = 1.0,
             weight_dice: float = 1.0, use_ignore_label: bool = False) -> torch.Tensor:
    """logits [B,K,...], regions [B,K(+1),...] holding 0 / 1 (the last channel is the ignore mask with use_ignore_label)."""
    B, K = logits.shape[:2]
    x = logits.reshape(B, K, -1)
    r = regions.reshape(B, regions.shape[1], -1).to(x.dtype)
    if use_ignore_label:
        m, y = 1 - r[:, -1:, :], r[:, :-1, :]
    else:
        m, y = torch.ones_like(r[:, :1, :]), r
    y = y * m
    p = torch.sigmoid(x)
    dice = _dice((p * y).sum(-1), (p * m).sum(-1), y.sum(-1), batch_dice, do_bg, smooth)
    elem = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))) * m
    bce = elem.sum() / torch.clamp(m.sum(), min=1e-8) if use_ignore_label else elem.sum() / x.numel()
    return weight_ce * bce + weight_dice * dice


def deep_supervision(level_loss, outputs: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], weights: Sequence[float]) -> torch.Tensor:
    """sum_i w_i level_loss(outputs[i], targets[i]); every level is evaluated, also one of weight 0."""
    total = None
    for x, t, w in zip(outputs, targets, weights):
        l = float(w) * level_loss(x, t)
        total = l if total is None else total + l
    return total


def nnunet_weights(num_levels: int):
    """1 / 2^i, the last one zeroed, normalised to sum 1 (python floats)."""
    w = [1.0 / (2 ** i) for i in range(num_levels)]
    w[-1] = 0.0
    s = sum(w)
    return [v / s for v in w]


def loss_and_grads(fn, xs: Sequence[torch.Tensor], dtype: torch.dtype):
    """evaluate fn on copies of xs in `dtype` with autograd -> (loss, [d loss / d x_i])."""
    leaves = [x.detach().to(dtype).requires_grad_(True) for x in xs]
    loss = fn(*leaves)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return loss.detach(), [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
