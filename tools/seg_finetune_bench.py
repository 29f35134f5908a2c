"""Milliseconds of (a) one SegTrainer.train_step (forward + deep-supervision Dice + CE + backward + clip + AdamW on flat buffers) of
STUNet-B against the same network stepped the way it was before the trainer existed -- seg_train.STUNet + seg_loss.build_loss +
torch.nn.utils.clip_grad_norm_(12) + torch.optim.AdamW(lr 1e-4, weight_decay 1e-5, eps 1e-4) -- and (b) am_seg_hard_counts against the
reference's online evaluation written in torch ops (nnUNetTrainer.validation_step: argmax, one-hot scatter, get_tp_fp_fn_tn's three
products and fp32 sums over axes [0, 2, 3, 4]), both on the same GPU in ONE process.

    python tools/seg_finetune_bench.py [--repeats 5] [--size 128] [--batch 2] [--classes 105] [--dtype bf16|f32] [--skip-network]
                                       [--skip-torch] [--lib PATH]

Workload: STUNet-B, one --size^3 patch per sample, B = 2, K = 105, seeded weights, a smoothed random volume, uniform random labels.
Device events around each call, one warm-up each, the paths alternated, median of --repeats.  The counts kernel is also given as a fraction
of its traffic floor, (4 K + 2) B N bytes (the logits once, the int16 labels once) at the 8.0 TB/s HBM peak.  --lib binds another build of
the library (the tools-only ablation build, whose AM_SEG_COUNTS_DBG=1 adds the counts with integer atomics straight on the table instead
of per-tile partials and a fold).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anatomask_amd import hip, modules, ops, seg_loss, seg_train  # noqa: E402
from anatomask_amd.data import deep_supervision_targets  # noqa: E402
from anatomask_amd.seg_trainer import SegTrainer  # noqa: E402
from seg_bench import seeded_state  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
SCALES = [1, 1 / 2, 1 / 4, 1 / 8, 1 / 16]


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def alternate(fns, repeats):
    for f in fns:
        once(f)
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for r, f in zip(runs, fns):
            r.append(once(f))
    return [statistics.median(r) for r in runs], runs


def reference_counts(output, target):
    """nnUNetTrainer.validation_step's online evaluation (softmax, no ignore label) in torch ops -> (tp, fp, fn) fp32 [K] each"""
    axes = [0] + list(range(2, output.dim()))
    seg = output.argmax(1)[:, None]
    onehot = torch.zeros(output.shape, device=output.device, dtype=torch.float32)
    onehot.scatter_(1, seg, 1)
    del seg
    y = torch.zeros(output.shape, device=output.device)
    y.scatter_(1, target.long(), 1)
    tp = (onehot * y).sum(axes)
    fp = (onehot * (1 - y)).sum(axes)
    fn = ((1 - onehot) * y).sum(axes)
    return tp, fp, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--classes", type=int, default=105)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--skip-network", action="store_true", help="time am_seg_hard_counts only")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--lib", default=None, help="bind this build of the library instead of the in-tree one")
    a = ap.parse_args()
    if a.lib:
        hip.use_library(a.lib)
    dev = "cuda:0"
    cfg = modules.STUNET_CONFIGS["B"]
    B, K, n = a.batch, a.classes, (a.size,) * 3
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 1, *n, generator=g)
    for d in range(2, 5):
        x = (x + x.roll(1, d) + x.roll(-1, d)) / 3
    x = x.to(dev)
    labels = torch.randint(0, K, (B, 1, *n), generator=g).to(torch.int16).to(dev)
    out = {"workload": f"STUNet-B K={K} B={B} patch {a.size}^3 deep supervision", "dtype": a.dtype}

    if not a.skip_network:
        def make():
            net = seg_train.STUNet(1, K, depth=cfg["depth"], dims=cfg["dims"], enable_deep_supervision=True)
            net.load_state_dict(seeded_state(net, 0))
            net.compute_dtype = dtype
            return net.to(dev)
        tr = SegTrainer(make())
        fns = [lambda: tr.train_step(x, labels)["loss"]]
        if not a.skip_torch:
            net = make()
            opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-5, eps=1e-4)
            loss_fn = seg_loss.build_loss(5, True)
            targets = deep_supervision_targets(labels, SCALES)

            def parent_step():
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(net(x), targets)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(net.parameters(), 12)
                opt.step()
                return loss.detach()
            fns.append(parent_step)
        med, runs = alternate(fns, a.repeats)
        step = {"seg_trainer_ms": round(med[0], 2), "seg_trainer_runs_ms": [round(t, 2) for t in runs[0]], "parameters": tr.n}
        if len(fns) == 2:
            step.update({"torch_clip_adamw_ms": round(med[1], 2), "torch_runs_ms": [round(t, 2) for t in runs[1]],
                         "speedup": round(med[1] / med[0], 3)})
            del net, opt
        out["train_step"] = step
        del tr, fns
        torch.cuda.empty_cache()

    # ---- am_seg_hard_counts alone, the finest level
    N = a.size ** 3
    gd = torch.Generator(device=dev).manual_seed(1)
    logits = torch.empty(B, K, *n, device=dev)
    for k in range(K):
        logits[:, k] = torch.randn(B, *n, device=dev, generator=gd)
    table = torch.zeros(K, 3, dtype=torch.int64, device=dev)
    fns = [lambda: ops.seg_hard_counts(ops.SEG_SOFTMAX, logits, labels, out=table)]
    if not a.skip_torch:
        fns.append(lambda: reference_counts(logits, labels))
    med, runs = alternate(fns, max(a.repeats, 5))
    floor_bytes = (4 * K + 2) * B * N
    floor_ms = floor_bytes / HBM_PEAK * 1e3
    cnt = {"shape": f"logits [{B},{K},{a.size}^3] fp32, labels int16", "floor_bytes": floor_bytes, "floor_ms_at_8TBps": round(floor_ms, 4),
           "hip_ms": round(med[0], 4), "hip_runs_ms": [round(t, 4) for t in runs[0]], "hip_fraction_of_floor": round(floor_ms / med[0], 4),
           "workspace_bytes": ops.seg_hard_counts_workspace_bytes(B, N, K), "variant": os.environ.get("AM_SEG_COUNTS_DBG", "0") if a.lib else "0"}
    if not a.skip_torch:
        tp, fp, fn = reference_counts(logits, labels)
        same = bool(torch.equal(torch.stack([tp, fp, fn], 1).to(torch.int64), table))
        cnt.update({"torch_ops_ms": round(med[1], 4), "torch_runs_ms": [round(t, 4) for t in runs[1]], "speedup": round(med[1] / med[0], 3),
                    "equal_to_torch_ops": same})
    out["seg_hard_counts"] = cnt
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
