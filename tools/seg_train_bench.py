"""Milliseconds of one segmentation fine-tuning step without the optimizer (forward + deep-supervision Dice + CE loss + backward) of
STUNet-B on this package's HIP path (seg_train.STUNet + seg_loss.build_loss) against the same network as plain torch ops + autograd
under torch.autocast bf16 on the same GPU, and of am_seg_head_bwd alone at the finest level against torch.einsum.

    python tools/seg_train_bench.py [--repeats 5] [--size 128] [--batch 2] [--classes 105] [--dtype bf16|f32] [--skip-torch] [--skip-network]

Workload: STUNet-B, one --size^3 patch per sample, B = 2, K = 105, deep supervision on, seeded weights, a smoothed random volume and
uniform random labels.  Device events around each step, one warm-up each, the two paths alternated in ONE process, median of --repeats.
The torch baseline is built as tools/seg_bench.py builds its own (functional torch on the state dict); its loss is the same Dice + CE
(batch Dice, no background, smooth 1e-5, weights 1 / 2^i with the last level zeroed) written with torch ops.
am_seg_head_bwd (dlogits fp32 [B,K,N] -> df, dw, db) is also given as a fraction of its traffic floor, 4 B K N bytes of dlogits +
2 elt B N C bytes of features read and gradient written, at the 8.0 TB/s HBM peak.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anatomask_amd import modules, ops, seg_loss, seg_train  # noqa: E402
from anatomask_amd.data import deep_supervision_targets  # noqa: E402
from seg_bench import _block, seeded_state  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
SCALES = [1, 1 / 2, 1 / 4, 1 / 8, 1 / 16]


def torch_forward_ds(W, x, depth):
    """P/STUNet.py:70-93 with deep supervision: the five levels' logits, finest first."""
    skips = []
    for s in range(6):
        for b in range(depth[s]):
            x = _block(W, f"conv_blocks_context.{s}.{b}", x, 2 if (b == 0 and 1 <= s <= 4) else 1, b == 0)
        skips.append(x)
    x, segs = skips[5], []
    for u in range(5):
        x = F.interpolate(x, scale_factor=1 if u == 0 else 2, mode="nearest")
        x = F.conv3d(x, W[f"upsample_layers.{u}.conv.weight"], W[f"upsample_layers.{u}.conv.bias"])
        x = torch.cat((x, skips[4 - u]), 1)
        for b in range(depth[4 - u]):
            x = _block(W, f"conv_blocks_localization.{u}.{b}", x, 1, b == 0)
        segs.append(F.conv3d(x, W[f"seg_outputs.{u}.weight"], W[f"seg_outputs.{u}.bias"]))
    return [segs[-1]] + segs[:-1][::-1]


def torch_dice_ce(logits, labels, smooth=1e-5):
    """batch Dice without background + CE, as seg_loss.build_loss(.., batch_dice=True) composes them (fp32)."""
    x = logits.float()
    lab = labels[:, 0].long()
    p = torch.softmax(x, 1)
    y = F.one_hot(lab, x.shape[1]).permute(0, 4, 1, 2, 3).to(p.dtype)
    axes = (0, 2, 3, 4)
    inter, sp, sy = (p * y).sum(axes), p.sum(axes), y.sum(axes)
    dc = (2 * inter + smooth) / torch.clamp(sy + sp + smooth, min=1e-8)
    return F.cross_entropy(x, lab) - dc[1:].mean()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--classes", type=int, default=105)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-network", action="store_true", help="time am_seg_head_bwd only")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = modules.STUNET_CONFIGS["B"]
    B, K, n = a.batch, a.classes, (a.size,) * 3
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    net = seg_train.STUNet(1, K, depth=cfg["depth"], dims=cfg["dims"], enable_deep_supervision=True)
    sd = seeded_state(net, 0)
    net.load_state_dict(sd)
    net.compute_dtype = dtype
    net = net.to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 1, *n, generator=g)
    for d in range(2, 5):
        x = (x + x.roll(1, d) + x.roll(-1, d)) / 3
    x = x.to(dev)
    labels = torch.randint(0, K, (B, 1, *n), generator=g).to(torch.int16).to(dev)
    targets = deep_supervision_targets(labels, SCALES)
    loss_fn = seg_loss.build_loss(5, True)
    weights = [float(w) for w in loss_fn.weight_factors]

    def hip_step():
        for p in net.parameters():
            p.grad = None
        loss = loss_fn(net(x), targets)
        loss.backward()
        return loss.detach()

    fns = [] if a.skip_network else [hip_step]
    if not a.skip_torch and not a.skip_network:
        W = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}

        def torch_step():
            for p in W.values():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                outs = torch_forward_ds(W, x, cfg["depth"])
            loss = sum(w * torch_dice_ce(o, t) for w, o, t in zip(weights, outs, targets) if w != 0)
            loss.backward()
            return loss.detach()
        fns.append(torch_step)
    med, runs = alternate(fns, a.repeats)
    out = {"workload": f"STUNet-B K={K} B={B} patch {a.size}^3 deep supervision: forward + Dice/CE loss + backward", "dtype": a.dtype}
    if fns:
        out.update({"hip_ms": round(med[0], 2), "hip_runs_ms": [round(t, 2) for t in runs[0]]})
    if len(fns) == 2:
        out.update({"torch_autocast_bf16_ms" if dtype == torch.bfloat16 else "torch_fp32_ms": round(med[1], 2),
                    "torch_runs_ms": [round(t, 2) for t in runs[1]], "speedup": round(med[1] / med[0], 3)})
        del W
    del net
    torch.cuda.empty_cache()

    # ---- am_seg_head_bwd alone, the finest level
    C, N = cfg["dims"][0], a.size ** 3
    gd = torch.Generator(device=dev).manual_seed(1)
    dl = torch.empty(B, K, *n, device=dev)
    for k in range(K):
        dl[:, k] = torch.randn(B, *n, device=dev, generator=gd)
    f = torch.randn(B, *n, C, device=dev, generator=gd).to(dtype)
    w = torch.randn(K, C, device=dev, generator=gd) / C ** 0.5
    dw, db = torch.zeros(K, C, device=dev), torch.zeros(K, device=dev)
    df = torch.empty_like(f)

    def hip_head():
        return ops.seg_head_bwd(dl, f, w, dw, db, df=df)

    def torch_head():
        d2 = dl.reshape(B, K, N)
        tdf = torch.einsum("bkn,kc->bnc", d2, w).to(dtype)
        tdw = torch.einsum("bkn,bnc->kc", d2, f.reshape(B, N, C).float())
        return tdf, tdw, d2.sum((0, 2))
    hm, hr = alternate([hip_head] if a.skip_torch else [hip_head, torch_head], max(a.repeats, 5))
    floor_bytes = 4 * B * K * N + 2 * f.element_size() * B * N * C
    floor_ms = floor_bytes / HBM_PEAK * 1e3
    head = {"shape": f"dlogits [{B},{K},{a.size}^3] fp32, features C={C} {a.dtype}", "floor_bytes": floor_bytes,
            "floor_ms_at_8TBps": round(floor_ms, 4), "hip_ms": round(hm[0], 4), "hip_runs_ms": [round(t, 4) for t in hr[0]],
            "hip_fraction_of_floor": round(floor_ms / hm[0], 4), "gflop": round(4e-9 * B * K * N * C, 2)}
    if not a.skip_torch:
        head.update({"torch_einsum_ms": round(hm[1], 4), "torch_runs_ms": [round(t, 4) for t in hr[1]], "speedup": round(hm[1] / hm[0], 3)})
    out["seg_head_bwd"] = head
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
