"""Seconds per volume of STUNet sliding-window inference: this package's HIP path vs the same network as plain torch under
torch.autocast fp16 with torch.flip mirroring (the reference predictor's configuration, predict_from_raw_data.py:595-754) on the same GPU.

    python tools/seg_bench.py [--repeats 3] [--size 256] [--dtype bf16|f32] [--skip-torch] [--export]

Workload: STUNet-B, 105 classes, patch 128^3, step 0.5, mirroring over (0, 1, 2), Gaussian on; a seeded synthetic 1 x 256^3 volume
(27 tiles x 8 mirrors).  Host clock around device-synchronised work, one warm-up volume, median of --repeats.  The HIP path's phase
split (gather / network / head + accumulate) comes from a separate timed volume (device events per phase, synchronised per tile).
Prints one JSON line.

--export adds a second JSON line: ops.seg_export (softmax probabilities + labels in one pass) at K = 105 on a --size^3 accumulator against
the torch sequence it replaces on the same device (ops.seg_finalize logits, torch.softmax(dim=0), argmax(0)).  Device events around each
call, one warm-up each, the two alternated, median of max(--repeats, 5).  Both are also given as a fraction of the traffic floor: K N 4
bytes read + K N 4 written at the 8.0 TB/s HBM peak."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anatomask_amd import modules, segmentation as S  # noqa: E402


def seeded_state(net, seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for k, v in net.state_dict().items():
        z = rs.standard_normal(tuple(v.shape)).astype(np.float32)
        if v.dim() == 5:
            z *= np.float32(1.0 / np.sqrt(np.prod(v.shape[1:])))
        elif ".norm" in k and k.endswith("weight"):
            z = 1 + np.float32(0.1) * z
        else:
            z *= np.float32(0.1)
        sd[k] = torch.from_numpy(z)
    return sd


# ---- plain torch restatement of P/STUNet.py:70-117 (forward) on a state dict
def _block(W, p, x, stride, sc):
    y = F.conv3d(x, W[f"{p}.conv1.weight"], W[f"{p}.conv1.bias"], stride=stride, padding=1)
    y = F.leaky_relu(F.instance_norm(y, weight=W[f"{p}.norm1.weight"], bias=W[f"{p}.norm1.bias"]), 0.01)
    y = F.instance_norm(F.conv3d(y, W[f"{p}.conv2.weight"], W[f"{p}.conv2.bias"], padding=1), weight=W[f"{p}.norm2.weight"], bias=W[f"{p}.norm2.bias"])
    if sc:
        x = F.conv3d(x, W[f"{p}.conv3.weight"], W[f"{p}.conv3.bias"], stride=stride)
    return F.leaky_relu(y + x, 0.01)


def torch_forward(W, x, depth):
    skips = []
    for s in range(6):
        for b in range(depth[s]):
            x = _block(W, f"conv_blocks_context.{s}.{b}", x, 2 if (b == 0 and 1 <= s <= 4) else 1, b == 0)
        skips.append(x)
    x = skips[5]
    for u in range(5):
        x = F.interpolate(x, scale_factor=1 if u == 0 else 2, mode="nearest")
        x = F.conv3d(x, W[f"upsample_layers.{u}.conv.weight"], W[f"upsample_layers.{u}.conv.bias"])
        x = torch.cat((x, skips[4 - u]), 1)
        for b in range(depth[4 - u]):
            x = _block(W, f"conv_blocks_localization.{u}.{b}", x, 1, b == 0)
    return F.conv3d(x, W["seg_outputs.4.weight"], W["seg_outputs.4.bias"])


def torch_predict(W, depth, img, patch, step, gauss):
    """predict_sliding_window_return_logits as the reference runs it: fp16 autocast, fp16 accumulators, torch.flip mirroring."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        steps = S.compute_steps_for_sliding_window(img.shape[1:], patch, step)
        data = img
        K = W["seg_outputs.4.weight"].shape[0]
        logits = torch.zeros((K, *data.shape[1:]), dtype=torch.half, device=img.device)
        nump = torch.zeros(data.shape[1:], dtype=torch.half, device=img.device)
        g = gauss.half()
        mirrors = [(), (2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4)]
        for sx in steps[0]:
            for sy in steps[1]:
                for sz in steps[2]:
                    sl = (slice(None), slice(sx, sx + patch[0]), slice(sy, sy + patch[1]), slice(sz, sz + patch[2]))
                    x = data[sl][None]
                    pred = torch_forward(W, x, depth)
                    for fl in mirrors[1:]:
                        pred += torch.flip(torch_forward(W, torch.flip(x, fl), depth), fl)
                    pred /= len(mirrors)
                    logits[sl] += pred[0] * g
                    nump[sl[1:]] += g
        logits /= nump
    return logits


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


HBM_PEAK = 8.0e12      # bytes / s, MI355X specification


def export_bench(size, repeats, dev):
    from anatomask_amd import ops
    K, n = 105, (size,) * 3
    g = torch.Generator(device=dev).manual_seed(0)
    acc = torch.empty(K, *n, device=dev)
    for k in range(K):
        acc[k] = 8 * torch.randn(*n, device=dev, generator=g)
    wsum = torch.rand(*n, device=dev, generator=g) + 0.5

    def fused():
        return ops.seg_export(acc, wsum, (0, 0, 0), n)

    def sequence():
        logits = ops.seg_finalize(acc, wsum, (0, 0, 0), n, True, False)[0]
        probs = torch.softmax(logits, dim=0)
        return probs, probs.argmax(0)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        return e0.elapsed_time(e1) / 1e3

    once(fused), once(sequence)
    tf, ts = [], []
    for _ in range(max(repeats, 5)):
        tf.append(once(fused))
        ts.append(once(sequence))
    f, q = statistics.median(tf), statistics.median(ts)
    floor_bytes = 2 * K * size ** 3 * 4
    floor_s = floor_bytes / HBM_PEAK
    return {"workload": f"export K={K} on {size}^3: softmax probabilities + labels", "floor_bytes": floor_bytes,
            "floor_s_at_8TBps": round(floor_s, 6), "fused_s": round(f, 6), "fused_runs": [round(t, 6) for t in tf],
            "fused_fraction_of_floor": round(floor_s / f, 4), "torch_sequence_s": round(q, 6), "torch_runs": [round(t, 6) for t in ts],
            "torch_fraction_of_floor": round(floor_s / q, 4), "speedup": round(q / f, 3), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--export", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = modules.STUNET_CONFIGS["B"]
    K, patch = 105, (128, 128, 128)
    net = S.STUNet(1, K, depth=cfg["depth"], dims=cfg["dims"], enable_deep_supervision=False)
    sd = seeded_state(net, 0)
    net.load_state_dict(sd)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    net = net.to(dev).requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(1, a.size, a.size, a.size, generator=g)
    for d in range(1, 4):
        img = (img + img.roll(1, d) + img.roll(-1, d)) / 3
    pred = S.SlidingWindowPredictor(net, patch, 0.5, True, True)
    with torch.no_grad():
        hip_s, hip_all = timed(lambda: pred.predict_labels(img), a.repeats)
        pred._run(img, False, True, timed=True)
        phases = {k: round(v, 4) for k, v in pred.phase_seconds.items()}
    n_tiles = int(np.prod([len(s) for s in S.compute_steps_for_sliding_window((a.size,) * 3, patch, 0.5)]))
    out = {"workload": f"STUNet-B K={K} patch 128^3 step 0.5 mirror 8 gaussian, volume 1x{a.size}^3 ({n_tiles} tiles)",
           "dtype": a.dtype, "hip_s_per_volume": round(hip_s, 4), "hip_runs": [round(t, 4) for t in hip_all], "hip_phase_s": phases}
    if not a.skip_torch:
        W = {k: v.to(dev) for k, v in sd.items()}
        gauss = S.compute_gaussian(patch).to(dev)
        imgd = img.to(dev)
        t_s, t_all = timed(lambda: torch_predict(W, cfg["depth"], imgd, patch, 0.5, gauss).argmax(0), a.repeats)
        out.update({"torch_autocast_fp16_s_per_volume": round(t_s, 4), "torch_runs": [round(t, 4) for t in t_all],
                    "speedup": round(t_s / hip_s, 3)})
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if a.export:
        del pred, net
        torch.cuda.empty_cache()
        print(json.dumps(export_bench(a.size, a.repeats, dev)))


if __name__ == "__main__":
    main()
