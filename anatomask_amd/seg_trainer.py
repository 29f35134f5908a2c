"""The segmentation fine-tuning trainer: the step bodies of nnUNetTrainer.train_step / validation_step / on_validation_epoch_end
(nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py:900-1012) with STUNetTrainer's optimizer (clip_grad_norm_(12) + AdamW(lr 1e-4,
weight_decay 1e-5, eps 1e-4) under CosineAnnealingLR(T_max = num_epochs), or nnU-Net's PolyLRScheduler), on the HIP path:

    net = seg_train.STUNet(1, K, depth, dims).to(dev)                       # deep supervision on (the default)
    net.load_state_dict(checkpoint.encoder_weights_for_finetuning(...), strict=False)
    tr = SegTrainer(net, num_epochs=1000)
    for e in range(start, 1000):
        tr.set_epoch(e)                                                     # the epoch's learning rate
        for data, target in train_batches: out = tr.train_step(data, target)        # {'loss', 'grad_norm'}: device tensors
        for data, target in val_batches:   tr.validation_step(data, target)         # tp / fp / fn accumulate on the device
        m = tr.on_validation_epoch_end()                                    # ONE read-back: Dice per class, its mean, the EMA, is_best
        tr.save(path, e)

train_step:  zero the flat gradient -> forward (seg_train.STUNet: the engine's tape) -> seg_loss.build_loss over the deep-supervision
views of `target` (data.deep_supervision_targets: no copy) -> backward through autograd, which ACCUMULATES into the parameters' .grad =
views of one flat fp32 buffer -> ||g||^2 (ops.sumsq) -> clip + AdamW in ONE pass over the whole flat parameter buffer (ops.adamw_ema with
ema = None) -> the packed compute-dtype weight copies are invalidated.  Nothing is read back to the host.

The parameters are views of one flat fp32 buffer (each tensor padded to a multiple of 4 elements, as GenericTrainer._flatten; the padding
stays 0 through every step: p = g = m = v = 0 gives p' = 0), their gradients views of a second, exp_avg / exp_avg_sq are flat as well.
Every parameter is live, as under torch.optim.AdamW: with nnU-Net's loss weights the coarsest level has weight 0, and seg_loss hands its
logits a ZERO gradient (not None), so seg_train.STUNet's backward returns a gradient for every head and nothing is skipped (checked by
tests/test_seg_train_gpu.py: seg_outputs.0.* receive exact zeros, no .grad is None).  Such a parameter still takes the weight-decay step,
exactly as torch's AdamW does with a zero gradient.  The trainer goes through autograd (loss.backward()); calling the engine directly
would save the one zero-fill + add per parameter that autograd's accumulation costs, which has not been measured.

validation_step runs under torch.no_grad() (the network takes segmentation.STUNet's inference path), evaluates the same loss and adds
the finest level's hard tp / fp / fn to one int64 [K, 3] table on the device (ops.seg_hard_counts(accumulate=True): exact integers, one pass
over the logits).  on_validation_epoch_end reads the table and the summed loss back once and does the reference's bookkeeping in fp64:
Dice 2 tp / (2 tp + fp + fn) per class (NaN where the denominator is 0; softmax drops class 0), its nanmean, the logger's EMA
(0.9 previous + 0.1 new; the first value as it is) and nnU-Net's `_best_ema` rule.

Not served, each with a named error: more than one rank (NotImplementedError: cross-rank batch Dice is not built and seg_loss refuses
it), gradient accumulation (NotImplementedError), a grad scaler (NotImplementedError: there is no fp16 path), a network that is not a
seg_train.STUNet with deep supervision (TypeError) or not on a cuda device (RuntimeError)."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops, seg_loss, seg_train
from .data import deep_supervision_targets

__all__ = ["SegTrainer", "lr_at", "validation_summary", "adamw_state_dict"]

DS_SCALES = [1, 1 / 2, 1 / 4, 1 / 8, 1 / 16]


def lr_at(schedule: str, initial_lr: float, epoch: int, num_epochs: int) -> float:
    """the learning rate of `epoch` in closed form.  'cosine': torch's CosineAnnealingLR(T_max = num_epochs, eta_min = 0) stepped `epoch`
    times, 0.5 lr0 (1 + cos(pi e / T)) (STUNetTrainer); 'poly': the reference's PolyLRScheduler, lr0 (1 - e / T)^0.9 (nnU-Net's default)."""
    if schedule == "cosine":
        return 0.5 * initial_lr * (1.0 + math.cos(math.pi * epoch / num_epochs))
    if schedule == "poly":
        return initial_lr * (1 - epoch / num_epochs) ** 0.9
    raise ValueError(f"schedule {schedule!r}: 'cosine' or 'poly'")


def validation_summary(counts, regions: bool, previous_ema: Optional[float], best_ema: Optional[float]) -> Dict:
    """on_validation_epoch_end's arithmetic (nnUNetTrainer.py:1005-1031, nnunet_logger.py:48-52) on a [K, 3] table of (tp, fp, fn), in fp64:
    Dice per class (NaN where 2 tp + fp + fn = 0; softmax drops class 0, regions keep all), their nanmean, the EMA (0.9 previous + 0.1 new;
    without a previous value the new one) and whether that EMA is a new best (no best yet, or strictly above it)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 3)
    if not regions:
        c = c[1:]
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = 2 * tp / (2 * tp + fp + fn)
    mean = float(np.nanmean(dice)) if np.isfinite(dice).any() else float("nan")
    ema = mean if previous_ema is None else previous_ema * 0.9 + 0.1 * mean
    is_best = best_ema is None or ema > best_ema
    return {"mean_fg_dice": mean, "dice_per_class_or_region": [float(d) for d in dice], "ema_fg_dice": ema, "is_best": bool(is_best)}


def adamw_state_dict(exp_avg: Sequence[torch.Tensor], exp_avg_sq: Sequence[torch.Tensor], step: int, lr: float, betas, eps: float,
                     weight_decay: float, initial_lr: Optional[float] = None) -> Dict:
    """torch.optim.AdamW.state_dict() of ONE parameter group over len(exp_avg) parameters: index-keyed `state` holding step / exp_avg /
    exp_avg_sq in the parameters' shapes (CPU copies; empty before the first step, as torch creates state lazily) and `param_groups`
    carrying lr, betas, eps, weight_decay.  The remaining keys of the group are those of the running torch's own AdamW, at their defaults."""
    probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    group = {k: v for k, v in probe.state_dict()["param_groups"][0].items()}
    group.update({"lr": float(lr), "betas": tuple(float(b) for b in betas), "eps": float(eps), "weight_decay": float(weight_decay),
                  "initial_lr": float(lr if initial_lr is None else initial_lr), "params": list(range(len(exp_avg)))})
    state = {}
    if step > 0:
        for i, (m, v) in enumerate(zip(exp_avg, exp_avg_sq)):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.detach().cpu().clone(), "exp_avg_sq": v.detach().cpu().clone()}
    return {"state": state, "param_groups": [group]}


class SegTrainer:
    def __init__(self, net, num_epochs: int = 1000, initial_lr: float = 1e-4, weight_decay: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-4,
                 clip: float = 12.0, schedule: str = "cosine", batch_dice: bool = True, regions: bool = False, ignore_label: Optional[int] = None,
                 ds_scales=None, gradient_accumulation_steps: int = 1, grad_scaler=None):
        if not isinstance(net, seg_train.STUNet):
            raise TypeError(f"SegTrainer drives seg_train.STUNet (the trainable segmentation network), not {type(net).__name__}")
        if not net.decoder.deep_supervision:
            raise TypeError("SegTrainer needs the network's deep supervision (enable_deep_supervision=True): the loss weighs its five levels")
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("SegTrainer runs on the HIP engine: move the network to a cuda (ROCm) device first")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("more than one rank: the cross-rank sums of batch Dice and the gradient exchange are not implemented")
        if int(gradient_accumulation_steps) != 1:
            raise NotImplementedError(f"gradient_accumulation_steps={gradient_accumulation_steps}: one optimizer step per batch only")
        if grad_scaler is not None:
            raise NotImplementedError("a grad scaler: there is no fp16 path (compute dtypes are bf16 and fp32)")
        lr_at(schedule, initial_lr, 0, num_epochs)                      # (an unknown schedule raises here)
        self.net, self.device = net, dev
        self.num_epochs, self.initial_lr, self.schedule = int(num_epochs), float(initial_lr), schedule
        self.wd, self.betas, self.eps, self.clip = float(weight_decay), (float(betas[0]), float(betas[1])), float(eps), float(clip)
        self.regions, self.ignore_label, self.batch_dice = bool(regions), ignore_label, bool(batch_dice)
        self.ds_scales = list(DS_SCALES if ds_scales is None else ds_scales)
        if len(self.ds_scales) != 5:
            raise NotImplementedError(f"{len(self.ds_scales)} deep-supervision scales: the network has five levels")
        self.mode = ops.SEG_SIGMOID if self.regions else ops.SEG_SOFTMAX
        self.loss_fn = seg_loss.build_loss(len(self.ds_scales), self.batch_dice, self.regions, ignore_label)
        self.K = int(net.num_classes)
        net.train()
        # ---- flat storage: parameters -> views of `flat`, their gradients -> views of `gflat` (GenericTrainer's layout)
        self._params = list(net.named_parameters())
        self.offsets: Dict[str, tuple] = {}                             # name -> (offset, elements) in the flat buffers
        self._shapes = {n: tuple(p.shape) for n, p in self._params}
        o = 0
        for n, p in self._params:
            self.offsets[n] = (o, p.numel())
            o += (p.numel() + 3) // 4 * 4
        self.n = o
        self.flat = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.gflat = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self._pviews = [self._view(self.flat, n) for n, _ in self._params]
        self._gviews = [self._view(self.gflat, n) for n, _ in self._params]
        for (_, p), pv in zip(self._params, self._pviews):
            pv.copy_(p.data.float())
            p.data = pv
            p.grad = None
        self.sumsq = torch.zeros(1, device=dev, dtype=torch.float64)
        self.gnorm = torch.zeros(1, device=dev)
        self.step_count = 0
        # ---- schedule and bookkeeping
        self.current_epoch, self.lr = 0, lr_at(schedule, self.initial_lr, 0, self.num_epochs)
        self.counts = torch.zeros(self.K, 3, device=dev, dtype=torch.int64)
        self._val_loss = torch.zeros(1, device=dev, dtype=torch.float32)
        self._val_steps = 0
        self.best_ema: Optional[float] = None
        self.logging: Dict[str, list] = {"mean_fg_dice": [], "ema_fg_dice": [], "dice_per_class_or_region": [], "train_losses": [],
                                         "val_losses": [], "lrs": []}

    def _view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        o, num = self.offsets[name]
        return buf[o:o + num].view(self._shapes[name])

    def _rebind(self):
        """.to() / load_state_dict(assign=True) may have replaced parameter storage: the step needs the views back"""
        for (_, p), v in zip(self._params, self._pviews):
            if p.data_ptr() != v.data_ptr():
                v.copy_(p.data.float())
                p.data = v

    def _targets(self, target: torch.Tensor) -> List[torch.Tensor]:
        if target.dim() == 4:
            target = target.unsqueeze(1)
        if self.regions:
            if target.dtype not in (torch.uint8, torch.bool):
                target = target.to(torch.uint8)
        elif target.dtype != torch.int16:
            target = target.to(torch.int16)
        return deep_supervision_targets(target, self.ds_scales)

    # ------------------------------------------------------------------ schedule
    def set_epoch(self, epoch: int):
        """on_train_epoch_start: lr_scheduler.step(current_epoch)"""
        self.current_epoch = int(epoch)
        self.lr = lr_at(self.schedule, self.initial_lr, self.current_epoch, self.num_epochs)

    # ------------------------------------------------------------------ steps
    def train_step(self, data: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
        """data (B,1,D,H,W) fp32 and target (int16 labels (B,1,D,H,W), or uint8 region channels) on the device.  Returns device tensors."""
        net = self.net
        self._rebind()
        targets = self._targets(target)
        self.gflat.zero_()
        for (_, p), g in zip(self._params, self._gviews):
            p.grad = g
        with torch.enable_grad():
            loss = self.loss_fn(list(net(data)), targets)
            loss.backward()
        with torch.no_grad():
            ops.sumsq(self.gflat, self.sumsq)
            self.step_count += 1
            ops.adamw_ema(self.flat, self.gflat, self.m, self.v, None, self.n, self.lr, self.betas, self.eps, self.wd, self.step_count,
                          self.sumsq, self.clip, 0.0, self.gnorm, grad_scale=1.0)
        self._weights_changed()
        return {"loss": loss.detach().reshape(1), "grad_norm": self.gnorm.clone()}

    def _weights_changed(self):
        sa = self.net.__dict__.get("_sa")
        if sa is not None:
            sa.pack.invalidate()                              # the compute-dtype copies are repacked from the stepped masters

    def validation_step(self, data: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
        self._rebind()
        with torch.no_grad():
            targets = self._targets(target)
            outs = list(self.net(data))
            loss = self.loss_fn(outs, targets).reshape(1)
            ops.seg_hard_counts(self.mode, outs[0], targets[0], self.ignore_label, out=self.counts, accumulate=True)
            self._val_loss += loss
            self._val_steps += 1
        return {"loss": loss}

    def on_validation_epoch_end(self) -> Dict:
        """one read-back (the counts and the summed loss in one tensor; counts below 2^53 are exact in it), then the bookkeeping; the
        device table and the loss sum are reset."""
        host = torch.cat([self.counts.double().flatten(), self._val_loss.double()]).cpu().numpy()
        self.counts.zero_()
        self._val_loss.zero_()
        steps, self._val_steps = self._val_steps, 0
        prev = self.logging["ema_fg_dice"][-1] if self.logging["ema_fg_dice"] else None
        out = validation_summary(host[:-1].reshape(self.K, 3), self.regions, prev, self.best_ema)
        out["val_loss"] = float(host[-1]) / steps if steps else float("nan")
        if out["is_best"]:
            self.best_ema = out["ema_fg_dice"]
        self.logging["mean_fg_dice"].append(out["mean_fg_dice"])
        self.logging["ema_fg_dice"].append(out["ema_fg_dice"])
        self.logging["dice_per_class_or_region"].append(out["dice_per_class_or_region"])
        self.logging["val_losses"].append(out["val_loss"])
        return out

    def on_train_epoch_end(self, losses: Sequence[torch.Tensor]) -> float:
        """the epoch's mean training loss (one read-back), logged with the epoch's learning rate"""
        mean = float(torch.cat([l.reshape(1) for l in losses]).mean().cpu()) if len(losses) else float("nan")
        self.logging["train_losses"].append(mean)
        self.logging["lrs"].append(self.lr)
        return mean

    # ------------------------------------------------------------------ checkpoints
    def reference_checkpoint(self, epoch: int) -> Dict:
        """nnUNetTrainer.save_checkpoint's dict (nnUNetTrainer.py:1054-1066): tensors and plain python containers only."""
        names = [n for n, _ in self._params]
        return {"network_weights": {k: v.detach().cpu().clone() for k, v in self.net.state_dict().items()},
                "optimizer_state": adamw_state_dict([self._view(self.m, n) for n in names], [self._view(self.v, n) for n in names],
                                                    self.step_count, self.lr, self.betas, self.eps, self.wd, self.initial_lr),
                "grad_scaler_state": None,
                "logging": {k: list(v) for k, v in self.logging.items()},
                "_best_ema": self.best_ema,
                "current_epoch": int(epoch) + 1,
                "init_args": {"num_epochs": self.num_epochs, "initial_lr": self.initial_lr, "weight_decay": self.wd, "betas": self.betas,
                              "eps": self.eps, "clip": self.clip, "schedule": self.schedule, "batch_dice": self.batch_dice,
                              "regions": self.regions, "ignore_label": self.ignore_label, "ds_scales": [float(s) for s in self.ds_scales]},
                "trainer_name": type(self).__name__,
                "inference_allowed_mirroring_axes": None}

    def save(self, path: str, epoch: int, extra: Optional[dict] = None):
        """the reference's checkpoint plus the step count, written atomically; `load`, predict.load_weights and
        torch.load(weights_only=True) read it"""
        ck = self.reference_checkpoint(epoch)
        ck["step_count"] = self.step_count
        ck["param_names"] = [n for n, _ in self._params]
        ck["extra"] = dict(extra or {})
        tmp = path + ".tmp"
        torch.save(ck, tmp)
        os.replace(tmp, path)

    def load(self, path: str) -> Dict:
        """resume from `save`'s file (never unpickles code).  Returns {'current_epoch': the next epoch, 'extra'}."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        self.net.load_state_dict(ck["network_weights"])
        self._rebind()
        opt = ck.get("optimizer_state") or {}
        names = [n for n, _ in self._params]
        if ck.get("param_names", names) != names:
            raise ValueError(f"{path}: the checkpoint's parameters are not this network's")
        self.m.zero_()
        self.v.zero_()
        steps = []
        for i, st in opt.get("state", {}).items():
            n = names[int(i)]
            self._view(self.m, n).copy_(st["exp_avg"])
            self._view(self.v, n).copy_(st["exp_avg_sq"])
            steps.append(int(float(st["step"])))
        self.step_count = int(ck.get("step_count", max(steps, default=0)))
        for k, v in (ck.get("logging") or {}).items():
            if k in self.logging:
                self.logging[k] = list(v)
        self.best_ema = ck.get("_best_ema")
        self.set_epoch(int(ck.get("current_epoch", 0)))
        self._weights_changed()
        return {"current_epoch": int(ck.get("current_epoch", 0)), "extra": ck.get("extra", {})}
