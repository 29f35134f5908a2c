"""Segmentation fine-tuning of a STUNet (P/STUNet.py) on nnU-Net preprocessed data, one GPU:

    python -m anatomask_amd.finetune --model B --num-classes 105 --input-size 128 128 128 --epochs 1000 --iters-per-epoch 250 --val-iters 50
           --batch-size 2 --lr 1e-4 --schedule cosine|poly --dtype bf16|f32 [--pretrained CKPT] [--data FOLDER] [--regions [JSON]]
           [--ignore-label L] [--out DIR] [--resume CKPT]

The loop of nnUNetTrainer.run_training around seg_trainer.SegTrainer: per epoch set_epoch -> --iters-per-epoch train steps ->
--val-iters validation steps -> on_validation_epoch_end; checkpoint_latest.pth every epoch, checkpoint_best.pth when the EMA pseudo Dice
improves, checkpoint_final.pth at the end -- all three SegTrainer.save's file (nnU-Net's keys; predict.py reads them).  One JSON line per
epoch.  --pretrained: a pretraining checkpoint of this package or of the reference; its encoder is loaded through
checkpoint.encoder_weights_for_finetuning (load_stunet_ssl_weights).  --data: a preprocessed folder, fed by data.SupervisedFeed (80 / 20
split of the cases, augmentation on the training half).  Without --data the pairs are seeded synthetic volumes whose labels are
quantile bands of a smooth field: enough to smoke-test the loop.  --regions: region-based training (sigmoid, Dice + BCE); with --data it takes
the regions as JSON (e.g. "[[1,2,3],[2,3],[3]]"), the number of regions must equal --num-classes."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from . import checkpoint, seg_train
from .modules import STUNET_CONFIGS
from .seg_trainer import SegTrainer


def synthetic_pairs(batch, size, K, seed, regions: bool, ignore=None):
    """(data fp32 (B,1,*size), target) forever on the CPU: int16 labels 0..K-1 (bands of a smooth field the image is a noisy copy of), or
    K nested uint8 region channels (band >= k + 1, as tumour regions are).  ignore (None: none): 5 % of the voxels carry that label, or, for
    regions, are set in one more channel, the ignore mask."""
    g = torch.Generator().manual_seed(seed)
    while True:
        f = torch.randn(batch, 1, *size, generator=g)
        for _ in range(3):
            for d in range(2, 5):
                f = (f + f.roll(1, d) + f.roll(-1, d)) / 3
        f = (f - f.mean()) / f.std()
        n_bands = K + 1 if regions else K
        edges = torch.quantile(f.flatten()[:1 << 16], torch.linspace(0, 1, n_bands + 1)[1:-1]) if n_bands > 1 else torch.zeros(0)
        lab = torch.bucketize(f, edges).to(torch.int16)
        data = f + 0.3 * torch.randn(batch, 1, *size, generator=g)
        if regions:
            chans = [(lab >= k + 1) for k in range(K)]
            if ignore is not None:
                chans.append(torch.rand(batch, 1, *size, generator=g) < 0.05)
            yield data, torch.cat(chans, 1).to(torch.uint8)
        else:
            if ignore is not None:
                lab = torch.where(torch.rand(batch, 1, *size, generator=g) < 0.05, torch.tensor(int(ignore), dtype=torch.int16), lab)
            yield data, lab


def load_pretrained_encoder(net, path: str):
    """load_stunet_ssl_weights (nnunetv2/run/load_pretrained_weights.py:66-106): the encoder entries of a pretraining checkpoint (of this
    package or of the reference; a dict with `network_weights`, or a bare state dict) into the full STUNet, everything else left as
    initialised.  Returns the names that were loaded."""
    ck = checkpoint.read_checkpoint(path)
    enc = checkpoint.encoder_weights_for_finetuning(ck["network_weights"] if "network_weights" in ck else ck)
    if not enc:
        raise SystemExit(f"--pretrained {path}: no encoder weights in it")
    own = net.state_dict()
    bad = sorted(k for k, v in enc.items() if k not in own or tuple(own[k].shape) != tuple(v.shape))
    if bad:
        raise SystemExit(f"--pretrained {path}: entries this network does not have (or of another shape): {bad[:4]} ...")
    net.load_state_dict(enc, strict=False)
    return sorted(enc)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m anatomask_amd.finetune", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="B", choices=list(STUNET_CONFIGS))
    ap.add_argument("--dims", type=int, nargs=6, default=None, help="channel widths instead of --model's")
    ap.add_argument("--depth", type=int, nargs=6, default=None, help="blocks per stage instead of --model's")
    ap.add_argument("--num-classes", type=int, required=True)
    ap.add_argument("--input-size", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--iters-per-epoch", type=int, default=250)
    ap.add_argument("--val-iters", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--schedule", choices=["cosine", "poly"], default="cosine")
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--pretrained", default=None, metavar="CKPT")
    ap.add_argument("--data", default=None, metavar="FOLDER")
    ap.add_argument("--regions", nargs="?", const="", default=None, metavar="JSON")
    ap.add_argument("--ignore-label", type=int, default=None)
    ap.add_argument("--out", default="anatomask_finetune")
    ap.add_argument("--resume", default=None, metavar="CKPT")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    dev = torch.device(a.device)
    cfg = STUNET_CONFIGS[a.model]
    K, size, regions = a.num_classes, tuple(a.input_size), a.regions is not None
    torch.manual_seed(a.seed)
    net = seg_train.STUNet(1, K, depth=list(a.depth or cfg["depth"]), dims=list(a.dims or cfg["dims"]), enable_deep_supervision=True)
    if a.pretrained:
        load_pretrained_encoder(net, a.pretrained)
    net.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    net = net.to(dev)
    tr = SegTrainer(net, num_epochs=a.epochs, initial_lr=a.lr, schedule=a.schedule, regions=regions, ignore_label=a.ignore_label)
    start = tr.load(a.resume)["current_epoch"] if a.resume else 0
    os.makedirs(a.out, exist_ok=True)

    feeds = []
    if a.data:
        from .data import PreprocessedDataset, SupervisedFeed
        from .pretrain import split_cases
        region_spec = json.loads(a.regions) if a.regions else None
        if regions and (region_spec is None or len(region_spec) != K):
            raise SystemExit("--regions with --data takes the regions as JSON, one entry per class of --num-classes")
        n_labels = None if region_spec is None else 1 + max(int(c) for r in region_spec for c in (r if isinstance(r, list) else [r]))
        train_cases, val_cases = split_cases(PreprocessedDataset(a.data).keys())
        train = SupervisedFeed(a.data, train_cases, a.batch_size, size, dev, 0, a.workers, True, a.seed, regions=region_spec, n_labels=n_labels)
        val = SupervisedFeed(a.data, val_cases or train_cases, a.batch_size, size, dev, 0, max(1, a.workers // 2), False, a.seed + 1,
                             regions=region_spec, n_labels=n_labels)
        feeds = [train, val]
    else:
        ign = a.ignore_label
        train = ((d.to(dev), t.to(dev)) for d, t in synthetic_pairs(a.batch_size, size, K, a.seed + 1, regions, ign))
        val = ((d.to(dev), t.to(dev)) for d, t in synthetic_pairs(a.batch_size, size, K, a.seed + 2, regions, ign))

    try:
        for epoch in range(start, a.epochs):
            tr.set_epoch(epoch)
            losses = [tr.train_step(*next(train))["loss"] for _ in range(a.iters_per_epoch)]
            train_loss = tr.on_train_epoch_end(losses)
            for _ in range(a.val_iters):
                tr.validation_step(*next(val))
            m = tr.on_validation_epoch_end()
            tr.save(os.path.join(a.out, "checkpoint_latest.pth"), epoch)
            if m["is_best"]:
                tr.save(os.path.join(a.out, "checkpoint_best.pth"), epoch)
            print(json.dumps({"epoch": epoch, "lr": tr.lr, "train_loss": train_loss, "val_loss": m["val_loss"], "mean_fg_dice": m["mean_fg_dice"],
                              "ema_fg_dice": m["ema_fg_dice"], "is_best": m["is_best"]}), flush=True)
        tr.save(os.path.join(a.out, "checkpoint_final.pth"), max(a.epochs - 1, 0))
    finally:
        for f in feeds:
            f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
