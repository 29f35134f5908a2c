"""Sliding-window STUNet inference on one nnU-Net preprocessed case:

    python -m anatomask_amd.predict CASE.npz|CASE.npy CHECKPOINT.pth OUT_PREFIX [--model B|L|H] [--num-classes K]
           [--patch-size 128 128 128] [--dtype bf16|f32] [--step 0.5] [--no-mirroring] [--no-gaussian] [--save-logits]
           [--folds CKPT [CKPT ...]] [--save-probabilities] [--regions-class-order I [I ...]]

CASE: `.npz` with key `data` or `.npy`, [C=1, X, Y, Z] (nnU-Net's preprocessed layout).  CHECKPOINT: a torch file with `network_weights`
(an nnU-Net checkpoint) or a bare state dict.  Writes OUT_PREFIX_labels.npy (uint8 when the largest label is <= 255, else int16) and, with
--save-logits, OUT_PREFIX_logits.npy (fp32 [K, X, Y, Z]).  Without --model the network's dims / depth / classes are read off the weights'
shapes.  The predictor is nnUNetPredictor(tile_step_size=0.5, use_gaussian=True, use_mirroring=True) of P/direct_infer.py by default.

--folds names further checkpoints of the same architecture: the logits are the mean over CHECKPOINT and every fold
(predict_logits_from_preprocessed_data), and everything written comes from that mean.  --save-probabilities writes OUT_PREFIX.npz with key
`probabilities` (fp32 [K, X, Y, Z]; the file nnUNetv2_ensemble reads).  --regions-class-order selects region-based labels: sigmoid instead of
softmax, labels = 0, then I_i wherever p_i > 0.5, in order (LabelManager.convert_probabilities_to_segmentation)."""
from __future__ import annotations

import argparse
import re
import sys

import numpy as np
import torch

from . import modules, ops, segmentation


def load_case(path: str) -> np.ndarray:
    if path.endswith(".npz"):
        with np.load(path) as z:
            a = z["data"]
    else:
        a = np.load(path)
    if a.ndim != 4:
        raise ValueError(f"{path}: expected [C, X, Y, Z], got shape {a.shape}")
    return a


def load_weights(path: str):
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["network_weights"] if isinstance(ck, dict) and "network_weights" in ck else ck
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def architecture_of(sd) -> dict:
    """dims / depth / classes of a STUNet state dict."""
    dims, depth = [], []
    for s in range(6):
        blocks = {int(m.group(1)) for k in sd for m in [re.match(rf"conv_blocks_context\.{s}\.(\d+)\.conv1\.weight$", k)] if m}
        if not blocks:
            raise ValueError(f"no conv_blocks_context.{s} in the checkpoint: not a STUNet segmentation network")
        depth.append(max(blocks) + 1)
        dims.append(int(sd[f"conv_blocks_context.{s}.0.conv1.weight"].shape[0]))
    return dict(dims=dims, depth=depth, num_classes=int(sd["seg_outputs.4.weight"].shape[0]))


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m anatomask_amd.predict", description=__doc__.split("\n\n")[0])
    ap.add_argument("case")
    ap.add_argument("checkpoint")
    ap.add_argument("out_prefix")
    ap.add_argument("--model", choices=["B", "L", "H"], default=None)
    ap.add_argument("--num-classes", type=int, default=None)
    ap.add_argument("--patch-size", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--no-mirroring", action="store_true")
    ap.add_argument("--no-gaussian", action="store_true")
    ap.add_argument("--save-logits", action="store_true")
    ap.add_argument("--folds", nargs="+", default=[], metavar="CKPT")
    ap.add_argument("--save-probabilities", action="store_true")
    ap.add_argument("--regions-class-order", type=int, nargs="+", default=None, metavar="I")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)

    sd = load_weights(a.checkpoint)
    arch = architecture_of(sd)
    if a.model is not None:
        cfg = modules.STUNET_CONFIGS[a.model]
        if (list(cfg["dims"]), list(cfg["depth"])) != (arch["dims"], arch["depth"]):
            raise SystemExit(f"--model {a.model} does not match the checkpoint (dims {arch['dims']}, depth {arch['depth']})")
    if a.num_classes is not None and a.num_classes != arch["num_classes"]:
        raise SystemExit(f"--num-classes {a.num_classes} does not match the checkpoint's heads ({arch['num_classes']})")
    folds = [sd]
    for path in a.folds:
        fsd = load_weights(path)
        try:
            farch = architecture_of(fsd)
        except (ValueError, KeyError) as e:
            raise SystemExit(f"--folds {path}: {e}")
        if farch != arch:
            raise SystemExit(f"--folds {path} is another architecture ({farch}) than {a.checkpoint} ({arch})")
        folds.append(fsd)
    if a.regions_class_order is not None:
        if len(a.regions_class_order) != arch["num_classes"]:
            raise SystemExit(f"--regions-class-order has {len(a.regions_class_order)} entries for {arch['num_classes']} regions")
        if any(c < 0 or c > 32767 for c in a.regions_class_order):
            raise SystemExit(f"--regions-class-order {a.regions_class_order}: labels must lie in [0, 32767]")
    net = segmentation.STUNet(1, arch["num_classes"], depth=arch["depth"], dims=arch["dims"], enable_deep_supervision=False)
    net.load_state_dict(sd)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    net = net.to(a.device).requires_grad_(False)
    pred = segmentation.SlidingWindowPredictor(net, a.patch_size, tile_step_size=a.step, use_gaussian=not a.no_gaussian,
                                               use_mirroring=not a.no_mirroring)
    image = torch.from_numpy(np.ascontiguousarray(load_case(a.case), dtype=np.float32))
    params = folds if a.folds else None
    export = a.save_probabilities or a.regions_class_order is not None
    logits = probs = None
    with torch.no_grad():
        acc, wsum, below, size = pred.accumulate(image, params)
        if export:
            probs, labels = ops.seg_export(acc, wsum, below, size, "sigmoid" if a.regions_class_order is not None else "softmax",
                                           a.regions_class_order, a.save_probabilities, True)
            if a.save_logits:
                logits = ops.seg_finalize(acc, wsum, below, size, True, False)[0]
        else:
            logits, labels = ops.seg_finalize(acc, wsum, below, size, a.save_logits, True)
    np.save(a.out_prefix + "_labels.npy", labels.cpu().numpy())
    if a.save_logits:
        np.save(a.out_prefix + "_logits.npy", logits.cpu().numpy())
    if a.save_probabilities:
        np.savez_compressed(a.out_prefix + ".npz", probabilities=probs.cpu().numpy())
    print(f"{a.case}: {tuple(image.shape[1:])} -> {a.out_prefix}_labels.npy ({arch['num_classes']} classes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
