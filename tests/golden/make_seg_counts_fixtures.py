"""Golden vectors of the online evaluation of a validation step, produced by the REFERENCE's own get_tp_fp_fn_tn
(nnunetv2/training/loss/dice.py) -- run in the build container only:

    python tests/golden/make_seg_counts_fixtures.py     # -> tests/golden/seg_counts_tiny.npz

dice.py is imported where it lies and is not copied.  The few lines of nnUNetTrainer.validation_step around the call (argmax + one-hot
scatter, or sigmoid > 0.5; the ignore mask; axes [0, 2, 3, 4]) are restated in `reference_counts` below.  Inputs fp32, counts as the
reference returns them (fp32 sums, exact at these sizes) stored as int64.

Cases, B = 2 over 5 x 6 x 7 (N = 210: no multiple of 4, less than one tile), logits round(6 randn) / 2 -- a grid of half-integers, so
many voxels tie at the maximum (printed per case), the sigmoid logits hit exactly 0 and none lies in (0, 1e-7): on such inputs
argmax / sigmoid > 0.5 and the kernel's first-index / x > 0 rules agree exactly.
    softmax_k2 / softmax_k5 / softmax_k105, softmax_k5_ignore (ignore_label = 5, labels 0..5), softmax_k5_allignored,
    regions_r3, regions_r3_ignore (the ignore channel last).
`cases` is a JSON list of the cases' settings."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
from nnunetv2.training.loss.dice import get_tp_fp_fn_tn  # noqa: E402

SEED = 20252
B, SP = 2, (5, 6, 7)


def reference_counts(output: torch.Tensor, target: torch.Tensor, regions: bool, ignore_label):
    """nnUNetTrainer.validation_step (nnUNetTrainer.py:937-961) on the finest level's output and target (a float tensor, as nnU-Net's)."""
    target = target.clone()
    axes = [0] + list(range(2, len(output.shape)))
    if regions:
        onehot = (torch.sigmoid(output) > 0.5).long()
    else:
        seg = output.argmax(1)[:, None]
        onehot = torch.zeros(output.shape, dtype=torch.float32)
        onehot.scatter_(1, seg, 1)
    if ignore_label is not None:
        if not regions:
            mask = (target != ignore_label).float()
            target[target == ignore_label] = 0
        else:
            mask = 1 - target[:, -1:]
            target = target[:, :-1]
    else:
        mask = None
    tp, fp, fn, _ = get_tp_fp_fn_tn(onehot, target, axes=axes, mask=mask)
    return torch.stack([tp, fp, fn], 1)


def main():
    g = torch.Generator().manual_seed(SEED)
    out, meta = {"seed": np.array(SEED)}, {}

    def add(name, K, regions=False, ignore_label=None, all_ignored=False):
        x = torch.round(6 * torch.randn(B, K, *SP, generator=g)) / 2
        if regions:
            t = (torch.rand(B, K + (1 if ignore_label is not None else 0), *SP, generator=g) < 0.4).to(torch.uint8)
        else:
            t = torch.randint(0, K + (1 if ignore_label is not None else 0), (B, 1, *SP), generator=g).to(torch.int16)
            if all_ignored:
                t[:] = ignore_label
        c = reference_counts(x, t.float(), regions, ignore_label)
        ci = c.to(torch.int64)
        assert torch.equal(ci.to(c.dtype), c)
        srt = x.sort(1, descending=True).values
        ties = int((srt[:, 0] == srt[:, 1]).sum()) if K > 1 else 0
        zeros, tiny = int((x == 0).sum()), int(((x > 0) & (x < 1e-7)).sum())
        meta[name] = dict(K=K, regions=regions, ignore_label=ignore_label)
        out[f"{name}.x"], out[f"{name}.t"], out[f"{name}.counts"] = x.numpy(), t.numpy(), ci.numpy()
        print(f"{name}: voxels tied at the maximum {ties} of {B * int(np.prod(SP))}, logits == 0: {zeros}, in (0, 1e-7): {tiny}, "
              f"sum tp {int(ci[:, 0].sum())} fp {int(ci[:, 1].sum())} fn {int(ci[:, 2].sum())}")

    add("softmax_k2", 2)
    add("softmax_k5", 5)
    add("softmax_k105", 105)
    add("softmax_k5_ignore", 5, ignore_label=5)
    add("softmax_k5_allignored", 5, ignore_label=5, all_ignored=True)
    add("regions_r3", 3, regions=True)
    add("regions_r3_ignore", 3, regions=True, ignore_label=1)
    out["cases"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "seg_counts_tiny.npz")
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print("seg_counts_tiny.npz bytes", n)
    assert n < 1 << 20, "a committed file may not exceed 1 MiB"


if __name__ == "__main__":
    main()
