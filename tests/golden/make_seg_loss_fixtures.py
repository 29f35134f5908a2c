"""Golden vectors of the segmentation loss, produced by the REFERENCE's own loss classes (nnunetv2/training/loss/compound_losses.py,
dice.py, deep_supervision.py, robust_ce_loss.py) and its autograd -- run in the build container only:

    python tests/golden/make_seg_loss_fixtures.py     # -> tests/golden/seg_loss_tiny.npz, seg_loss_tiny_k105.npz, seg_loss_tiny_ds.npz

The loss files are imported where they lie and are not copied.  Inputs are stored as fp32; for each case three pairs (loss, logit gradient):
    L64 / g64          the reference evaluated in fp64 on the fp32 inputs (the truth)
    L32ref / g32ref    the reference evaluated in fp32
    L32plain / g32plain  the same loss written with plain torch ops (tests/seg_loss_oracle.py) in fp32: the independent fp32 baseline the
                       bounds of the GPU tests are measured against
`cases` is a JSON list of the cases' settings.  Cases, B = 2 over 5 x 6 x 7, logits 3 randn:
    ce_k2 / ce_k4 / ce_k105 (batch Dice), ce_k4_nobatch, ce_k4_ignore (ignore_label = K, labels 0..K), ce_k4_allignored (every voxel the
    ignore label), ce_k4_weights (weight_ce 2, weight_dice 0.5); bce_r3_batch / bce_r3_nobatch / bce_r3_batch_ign / bce_r3_nobatch_ign (3
    regions, the ignore channel last where present); all with smooth 1e-5 and do_bg as nnUNetTrainer._build_loss sets them.
    ds: DeepSupervisionWrapper with nnU-Net's weights over five levels, K = 4, int16 target 16^3, scales 1 .. 1/16, logits 16^3 .. 1^3; the
    reference is fed contiguous copies of the strided targets (anatomask_amd.data.deep_supervision_targets).
One file may not exceed 1 MiB, hence three: the K = 105 case and the deep-supervision case have files of their own."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from nnunetv2.training.loss.compound_losses import DC_and_BCE_loss, DC_and_CE_loss  # noqa: E402
from nnunetv2.training.loss.deep_supervision import DeepSupervisionWrapper  # noqa: E402
from nnunetv2.training.loss.dice import MemoryEfficientSoftDiceLoss  # noqa: E402

import seg_loss_oracle as O  # noqa: E402
from anatomask_amd.data import deep_supervision_targets  # noqa: E402

SEED = 20251
B, SP = 2, (5, 6, 7)


def ref_ce(c):
    return DC_and_CE_loss({"batch_dice": c["batch_dice"], "smooth": 1e-5, "do_bg": False, "ddp": False}, {}, weight_ce=c["weight_ce"],
                          weight_dice=c["weight_dice"], ignore_label=c["ignore_label"], dice_class=MemoryEfficientSoftDiceLoss)


def ref_bce(c):
    return DC_and_BCE_loss({}, {"batch_dice": c["batch_dice"], "do_bg": True, "smooth": 1e-5, "ddp": False}, weight_ce=c["weight_ce"],
                           weight_dice=c["weight_dice"], use_ignore_label=c["use_ignore_label"], dice_class=MemoryEfficientSoftDiceLoss)


def plain(c):
    if c["kind"] == "ce":
        return lambda x, t: O.dice_ce(x, t, c["batch_dice"], False, 1e-5, c["weight_ce"], c["weight_dice"], c["ignore_label"])
    return lambda x, t: O.dice_bce(x, t, c["batch_dice"], True, 1e-5, c["weight_ce"], c["weight_dice"], c["use_ignore_label"])


def three_pairs(out, name, ref_fn, plain_fn, xs):
    """ref_fn / plain_fn: callables of the logits list (targets bound) -> loss."""
    for tag, fn, dt in (("64", ref_fn, torch.float64), ("32ref", ref_fn, torch.float32), ("32plain", plain_fn, torch.float32)):
        L, gs = O.loss_and_grads(fn, xs, dt)
        out[f"{name}.L{tag}"] = L.numpy()
        for i, g in enumerate(gs):
            out[f"{name}.g{tag}" + (f"_{i}" if len(xs) > 1 else "")] = g.numpy()
    e = [float(abs(out[f"{name}.L{t}"].astype(np.float64) - out[f"{name}.L64"])) for t in ("32ref", "32plain")]
    print(f"{name}: L64 {float(out[f'{name}.L64']):+.12f}  |L32ref - L64| {e[0]:.2e}  |L32plain - L64| {e[1]:.2e}")


def case(kind, K, g, batch_dice=True, ignore_label=None, all_ignored=False, weight_ce=1.0, weight_dice=1.0, use_ignore_label=False):
    c = dict(kind=kind, K=K, batch_dice=batch_dice, ignore_label=ignore_label, weight_ce=weight_ce, weight_dice=weight_dice,
             use_ignore_label=use_ignore_label)
    x = 3 * torch.randn(B, K, *SP, generator=g)
    if kind == "ce":
        t = torch.randint(0, K + (1 if ignore_label is not None else 0), (B, 1, *SP), generator=g).to(torch.int16)
        if all_ignored:
            t[:] = ignore_label
    else:
        t = (torch.rand(B, K + (1 if use_ignore_label else 0), *SP, generator=g) < 0.4).to(torch.uint8)
    return c, x, t


def main():
    g = torch.Generator().manual_seed(SEED)
    small = {
        "ce_k2": case("ce", 2, g), "ce_k4": case("ce", 4, g), "ce_k4_nobatch": case("ce", 4, g, batch_dice=False),
        "ce_k4_ignore": case("ce", 4, g, ignore_label=4), "ce_k4_allignored": case("ce", 4, g, batch_dice=False, ignore_label=4, all_ignored=True),
        "ce_k4_weights": case("ce", 4, g, weight_ce=2.0, weight_dice=0.5),
        "bce_r3_batch": case("bce", 3, g), "bce_r3_nobatch": case("bce", 3, g, batch_dice=False),
        "bce_r3_batch_ign": case("bce", 3, g, use_ignore_label=True), "bce_r3_nobatch_ign": case("bce", 3, g, batch_dice=False, use_ignore_label=True),
    }
    big = {"ce_k105": case("ce", 105, g)}
    for fname, cases in (("seg_loss_tiny.npz", small), ("seg_loss_tiny_k105.npz", big)):
        out, meta = {"seed": np.array(SEED)}, {}
        for name, (c, x, t) in cases.items():
            meta[name] = c
            out[f"{name}.x"], out[f"{name}.t"] = x.numpy(), t.numpy()
            ref = ref_ce(c) if c["kind"] == "ce" else ref_bce(c)
            tf = t.float()                                    # nnU-Net's targets are float tensors; exact for these values in every dtype
            three_pairs(out, name, lambda xx: ref(xx, tf.to(xx.dtype)), lambda xx: plain(c)(xx, t), [x])
        out["cases"] = np.array(json.dumps(meta))
        save(fname, out)

    # deep supervision
    K, top = 4, 16
    c = dict(kind="ce", K=K, batch_dice=True, ignore_label=None, weight_ce=1.0, weight_dice=1.0, use_ignore_label=False)
    scales = [1.0, 0.5, 0.25, 0.125, 0.0625]
    target = torch.randint(0, K, (B, 1, top, top, top), generator=g).to(torch.int16)
    views = deep_supervision_targets(target, scales)
    xs = [3 * torch.randn(B, K, *v.shape[2:], generator=g) for v in views]
    weights = np.array(O.nnunet_weights(len(scales)))          # nnUNetTrainer._build_loss: 1 / 2^i, the last one zeroed, normalised
    ref = DeepSupervisionWrapper(ref_ce(c), weights)
    tcs = [v.contiguous().float() for v in views]
    out = {"seed": np.array(SEED), "cases": np.array(json.dumps({"ds": dict(c, scales=scales)})), "ds.t": target.numpy(),
           "ds.weights": weights, "ds.scales": np.array(scales)}
    for i, x in enumerate(xs):
        out[f"ds.x_{i}"] = x.numpy()
    three_pairs(out, "ds", lambda *xx: ref(list(xx), [t.to(xx[0].dtype) for t in tcs]),
                lambda *xx: O.deep_supervision(plain(c), xx, [v.contiguous() for v in views], list(weights)), xs)
    save("seg_loss_tiny_ds.npz", out)


def save(fname, out):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print(fname, "bytes", n)
    assert n < 1 << 20, "a committed file may not exceed 1 MiB"


if __name__ == "__main__":
    main()
