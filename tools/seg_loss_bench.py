"""Milliseconds for forward + logit gradient of the fused Dice + CE deep-supervision loss (anatomask_amd.seg_loss, loss_ops.hip) against
the same loss written with torch ops and autograd on the same GPU, and the fraction of the HBM traffic floor the fused path reaches.

    python tools/seg_loss_bench.py [--repeats 15] [--classes 105] [--size 128] [--batch 2]

Workloads: (a) one level, K = 105 classes, 128^3, B = 2 (one logits tensor: 1.76 GB); (b) nnU-Net's five-level pyramid 128^3 .. 8^3 with
the weights of _build_loss (the last level has weight 0: the fused path skips it, torch evaluates it).  Logits 3 N(0, 1), labels uniform,
batch Dice, no ignore label; the targets of (b) are the strided views of data.deep_supervision_targets.
Each timed window is loss = f(logits, targets); loss.backward() between two device events, after two warm-up rounds; fused and torch
alternate; the median of `--repeats` windows is reported with min and max.  A window is milliseconds long, so the host's launch cost
(tens of microseconds) is inside it and small.
Traffic floor: the arithmetic needs the logits read twice and the gradient written once, 12 B K N bytes, at 8 TB/s (0.66 ms for (a));
`floor_fraction` = floor / measured.  Targets, partial sums and the per-voxel (max, log-sum) pair are not counted: the floor is a bound,
not the kernels' own traffic.  Kernel times proper: rocprofv3 --kernel-trace --stats -- python tools/seg_loss_bench.py.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anatomask_amd import data as D, seg_loss as SL  # noqa: E402

HBM_BYTES_PER_S = 8e12


def torch_dice_ce(x, t, smooth=1e-5):
    """Dice (batch, no background) + CE with torch ops, the way a torch user writes it: softmax, one-hot scatter, three reductions,
    cross_entropy; autograd does the way back."""
    p = torch.softmax(x, 1)
    with torch.no_grad():
        y = torch.zeros(x.shape, device=x.device, dtype=torch.bool)
        y.scatter_(1, t.long(), 1)
        y = y[:, 1:]
        g = y.sum((0, 2, 3, 4))
    p = p[:, 1:]
    i = (p * y).sum((0, 2, 3, 4))
    s = p.sum((0, 2, 3, 4))
    dc = (2 * i + smooth) / torch.clip(g + s + smooth, 1e-8)
    return F.cross_entropy(x, t[:, 0].long()) - dc.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--classes", type=int, default=105)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_loss_bench needs a GPU")
    dev, K, S, B = "cuda:0", a.classes, a.size, a.batch
    g = torch.Generator().manual_seed(0)
    scales = [1.0, 0.5, 0.25, 0.125, 0.0625]
    target = torch.randint(0, K, (B, 1, S, S, S), generator=g).to(torch.int16).to(dev)
    targets = D.deep_supervision_targets(target, scales)
    logits = [(3 * torch.randn(B, K, *t.shape[2:], generator=g)).to(dev).requires_grad_(True) for t in targets]
    fused = SL.build_loss(len(scales), batch_dice=True)
    weights = [float(w) for w in fused.weight_factors]
    tcont = [t.contiguous() for t in targets]                 # torch's scatter_ / cross_entropy want dense targets

    kinds = {
        "fused_single": lambda: fused.loss(logits[0], targets[0]),
        "torch_single": lambda: torch_dice_ce(logits[0], tcont[0]),
        "fused_pyramid": lambda: fused(logits, targets),
        "torch_pyramid": lambda: sum(w * torch_dice_ce(x, t) for w, x, t in zip(weights, logits, tcont)),
    }

    def once(fn):
        for x in logits:
            x.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = fn()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), float(loss)

    values = {}
    for _ in range(2):
        for k, fn in kinds.items():
            values[k] = once(fn)[1]
    runs = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for k, fn in kinds.items():
            runs[k].append(once(fn)[0])

    def floor_ms(levels):
        return sum(12 * x.numel() for x in levels) / HBM_BYTES_PER_S * 1e3

    floors = {"single": floor_ms(logits[:1]), "pyramid": floor_ms([x for x, w in zip(logits, weights) if w != 0])}
    res = {"workload": f"Dice + CE forward + logit gradient, K={K}, {S}^3, B={B}; pyramid = 5 levels {S}^3 .. {S // 16}^3, nnU-Net weights",
           "repeats": a.repeats, "hbm_TBps_assumed": HBM_BYTES_PER_S / 1e12}
    for k in kinds:
        res[k] = {"ms": round(statistics.median(runs[k]), 4), "min_ms": round(min(runs[k]), 4), "max_ms": round(max(runs[k]), 4),
                  "loss": values[k]}
    for w in ("single", "pyramid"):
        res[f"floor_ms_{w}"] = round(floors[w], 4)
        res[f"floor_fraction_{w}"] = round(floors[w] / res[f"fused_{w}"]["ms"], 4)
        res[f"torch_over_fused_{w}"] = round(res[f"torch_{w}"]["ms"] / res[f"fused_{w}"]["ms"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
