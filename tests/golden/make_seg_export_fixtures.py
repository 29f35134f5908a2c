"""Golden vectors of the logits -> probabilities -> segmentation step, produced by the REFERENCE's own LabelManager
(nnunetv2/utilities/label_handling/label_handling.py:128-175) -- run in the build container only:

    python tests/golden/make_seg_export_fixtures.py        # -> tests/golden/seg_export_tiny.npz

label_handling.py is imported where it lies and is not copied; the two names it imports from packages that are not installed
(acvl_utils' bounding_box_to_slice, batchgenerators' join; neither is called here) are in-memory stand-ins.

  softmax (ordinary labels): K = 3 and K = 105 over 5 x 6 x 7, logits 8 randn, three planted voxels (all classes +200; class 0 +200 and the
    rest -200; linspace(-100, 100, K)) on which a kernel that does not subtract the maximum overflows.  sm{K}.logits / .probs / .seg.
  regions: label dict {background 0, whole [1,2,3], core [2,3], enh 3}, regions_class_order [1,2,3] and [5,1,300] (non-monotone, needs
    int16) over 9 x 10 x 11, logits 4 randn pushed away from zero, three planted voxels (all 0; (1e-9, -1e-9, 1e-9), whose sigmoids round
    to exactly 0.5: background, where an `l > 0` shortcut says 3; (90, -90, 200)).  rg.logits / rg.probs / rg.seg0 / rg.seg1 / rg.order0/1."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _stand_in(name, **attrs):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


_stand_in("acvl_utils.cropping_and_padding.bounding_boxes", bounding_box_to_slice=None)
_stand_in("batchgenerators.utilities.file_and_folder_operations", join=os.path.join)
sys.path.insert(0, REF)
from nnunetv2.utilities.label_handling.label_handling import LabelManager  # noqa: E402

SEED = 20240
PLANTED = [(0, 0, 0), (2, 3, 4), (4, 5, 6)]
out = {"seed": np.array(SEED)}

for K in (3, 105):
    g = torch.Generator().manual_seed(SEED + K)
    logits = 8 * torch.randn(K, 5, 6, 7, generator=g)
    logits[(slice(None),) + PLANTED[0]] = 200.0
    logits[(slice(None),) + PLANTED[1]] = -200.0
    logits[(0,) + PLANTED[1]] = 200.0
    logits[(slice(None),) + PLANTED[2]] = torch.linspace(-100, 100, K)
    lm = LabelManager({"background": 0, **{f"c{i}": i for i in range(1, K)}}, None)
    assert not lm.has_regions
    probs = lm.apply_inference_nonlin(logits.numpy())
    seg = lm.convert_probabilities_to_segmentation(probs)
    assert torch.isfinite(probs).all()
    mism = int((seg != logits.argmax(0)).sum())
    print(f"softmax K={K}: reference segmentation vs argmax of the logits: {mism} mismatches")
    assert mism == 0, "regenerate with another seed"
    out[f"sm{K}.logits"] = logits.numpy()
    out[f"sm{K}.probs"] = probs.numpy().astype(np.float32)
    out[f"sm{K}.seg"] = seg.numpy().astype(np.int16)
    out[f"sm{K}.planted"] = np.array(PLANTED)

g = torch.Generator().manual_seed(SEED)
l = 4 * torch.randn(3, 9, 10, 11, generator=g)
l = torch.sign(l) * (l.abs() + 0.01)
RP = [(0, 0, 0), (4, 5, 6), (8, 9, 10)]
l[(slice(None),) + RP[0]] = 0.0
l[(slice(None),) + RP[1]] = torch.tensor([1e-9, -1e-9, 1e-9])
l[(slice(None),) + RP[2]] = torch.tensor([90.0, -90.0, 200.0])
out["rg.logits"] = l.numpy()
out["rg.planted"] = np.array(RP)
for j, order in enumerate(([1, 2, 3], [5, 1, 300])):
    lm = LabelManager({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, order)
    assert lm.has_regions
    probs = lm.apply_inference_nonlin(l.numpy())
    seg = lm.convert_probabilities_to_segmentation(probs)
    out["rg.probs"] = probs.numpy().astype(np.float32)
    out[f"rg.seg{j}"] = seg.numpy().astype(np.int16)
    out[f"rg.order{j}"] = np.array(order, dtype=np.int32)
    print(f"regions {order}: planted voxels -> {[int(seg[p]) for p in RP]}")
    assert int(seg[RP[0]]) == 0 and int(seg[RP[1]]) == 0 and int(seg[RP[2]]) == order[2]

path = os.path.join(HERE, "seg_export_tiny.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()})
print("bytes", os.path.getsize(path))
