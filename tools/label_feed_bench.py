"""Milliseconds per sample of the label resampling kernel of the supervised feed (am_resample_labels, order 1) against the float
order-1 resampling of the same shapes and affine (am_resample_affine), the yardstick: both gather the 8 corners of every output voxel.

    python tools/label_feed_bench.py [--repeats 15] [--inner 20]

Workload: one 205^3 enlarged patch -> 128^3 (the 128^3 recipe's shapes, data.get_patch_size), rotated by (0.30, -0.20, 0.25) rad and
scaled by 1.1, all flips on; int16 labels 0..4 in 16^3 blocks with a slab of -1, fp32 N(0,1) for the yardstick.  Three launches are timed:
labels only (int16 out), labels + 3 region planes (uint8), and the float kernel.  Device events around `--inner` back-to-back launches
of one kind, queued behind a ~10 ms device-side sleep so that the window holds kernel time + the device's dispatch gap and not the
host's launch rate (a launch through ctypes costs about as much host time as one of these kernels runs); one warm-up each, the three
kinds alternated, median of `--repeats`.  Kernel times proper: rocprofv3 --kernel-trace --stats -- python tools/label_feed_bench.py.
GB/s counts the bytes the algorithm asks for: the output plus 8 gathered source elements per output voxel (voxels that fall outside the
source gather nothing, and neighbouring voxels share corners through the caches: it is a figure for comparing the three launches, not
HBM traffic).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anatomask_amd import data as D, ops  # noqa: E402

ENL, FINAL, REGIONS, N_LABELS = (205, 205, 205), (128, 128, 128), ((1, 2), (2,), 3), 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    dev = "cuda:0"
    aug = D.SpatialAugmenter(FINAL, seed=0)
    p = {"angles": (0.30, -0.20, 0.25), "scale": 1.1, "modified": True, "mirror": [True, True, True]}
    A = aug.affine(p, ENL).reshape(-1)
    rs = np.random.RandomState(0)
    coarse = rs.randint(0, 5, size=[(n + 15) // 16 for n in ENL])
    seg = np.kron(coarse, np.ones((16, 16, 16), dtype=np.int64))[:ENL[0], :ENL[1], :ENL[2]].astype(np.int16)
    seg[:, :, :20] = -1
    seg = torch.from_numpy(np.ascontiguousarray(seg)).to(dev)
    img = torch.randn(ENL, generator=torch.Generator().manual_seed(0)).to(dev)
    lut = D.region_lut(REGIONS, N_LABELS).to(dev)
    lab = torch.empty(FINAL, dtype=torch.int16, device=dev)
    reg = torch.empty((len(REGIONS), *FINAL), dtype=torch.uint8, device=dev)
    out = torch.empty(FINAL, dtype=torch.float32, device=dev)
    n = int(np.prod(FINAL))
    kinds = {
        "labels_order1": (lambda: ops.resample_labels(seg, lab, A, 1), n * (2 + 8 * 2)),
        "labels_order1_3_regions": (lambda: ops.resample_labels(seg, lab, A, 1, -1, (-1, 0), lut, len(REGIONS), reg), n * (2 + len(REGIONS) + 8 * 2)),
        "float_order1": (lambda: ops.resample_affine(img, out, A, 1), n * (4 + 8 * 4)),
    }

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(20_000_000)                 # ~10 ms of device time: the launches below are all queued before the first one runs
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for fn, _ in kinds.values():
        once(fn)
    runs = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for k, (fn, _) in kinds.items():
            runs[k].append(once(fn))
    res = {"workload": "205^3 -> 128^3, rotation (0.30, -0.20, 0.25) rad, scale 1.1, flips; ms per sample, GB/s of output + 8 gathered elements per voxel",
           "inner": a.inner, "repeats": a.repeats}
    for k, (_, nbytes) in kinds.items():
        ms = statistics.median(runs[k])
        res[k] = {"ms": round(ms, 4), "min_ms": round(min(runs[k]), 4), "max_ms": round(max(runs[k]), 4), "bytes": nbytes,
                  "GBps": round(nbytes / ms / 1e6, 1)}
    res["labels_over_float"] = round(res["labels_order1"]["ms"] / res["float_order1"]["ms"], 3)
    res["regions_over_float"] = round(res["labels_order1_3_regions"]["ms"] / res["float_order1"]["ms"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
