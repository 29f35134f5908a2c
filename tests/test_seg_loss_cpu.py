"""CPU: the test-side restatement of the segmentation loss (tests/seg_loss_oracle.py) is pinned, in fp64, to the reference's own fp64 loss
and autograd gradient of every fixture case (tests/golden/seg_loss_*.npz, written by make_seg_loss_fixtures.py from nnunetv2's loss
classes); build_loss reproduces the reference's weights; the loss classes refuse what the kernels do not serve without needing a GPU."""
import json
import os

import numpy as np
import pytest
import torch

from anatomask_amd import seg_loss as SL
from anatomask_amd.data import deep_supervision_targets
from tests import seg_loss_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("seg_loss_tiny.npz", "seg_loss_tiny_k105.npz", "seg_loss_tiny_ds.npz")


def load_cases():
    """{case name: (settings, arrays of that case)} over the three fixture files."""
    out = {}
    for f in FILES:
        z = np.load(os.path.join(GOLD, f))
        for name, c in json.loads(str(z["cases"])).items():
            out[name] = (c, {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")})
    return out


CASES = load_cases()
SINGLE = sorted(n for n in CASES if n != "ds")


def oracle_fn(c):
    if c["kind"] == "ce":
        return lambda x, t: O.dice_ce(x, t, c["batch_dice"], False, 1e-5, c["weight_ce"], c["weight_dice"], c["ignore_label"])
    return lambda x, t: O.dice_bce(x, t, c["batch_dice"], True, 1e-5, c["weight_ce"], c["weight_dice"], c["use_ignore_label"])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm((a - b).ravel())
    n = np.linalg.norm(b.ravel())
    return d / n if n > 0 else d


def test_fixture_holds_the_cases_the_gpu_tests_need():
    assert set(CASES) == {"ce_k2", "ce_k4", "ce_k105", "ce_k4_nobatch", "ce_k4_ignore", "ce_k4_allignored", "ce_k4_weights", "bce_r3_batch",
                          "bce_r3_nobatch", "bce_r3_batch_ign", "bce_r3_nobatch_ign", "ds"}
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLD, f)) < 1 << 20
    c, a = CASES["ce_k4_allignored"]
    assert (a["t"] == c["ignore_label"]).all() and float(a["L64"]) == -1.0 and not a["g64"].any()
    assert CASES["ce_k105"][1]["x"].shape == (2, 105, 5, 6, 7) and CASES["ce_k105"][1]["x"].dtype == np.float32


@pytest.mark.parametrize("name", SINGLE)
def test_restatement_fp64_reproduces_reference(name):
    c, a = CASES[name]
    t = torch.from_numpy(a["t"])
    L, (g,) = O.loss_and_grads(lambda x: oracle_fn(c)(x, t), [torch.from_numpy(a["x"])], torch.float64)
    assert abs(float(L) - float(a["L64"])) <= 1e-12 * max(1.0, abs(float(a["L64"])))
    assert rel(g.numpy(), a["g64"]) <= 1e-12


def test_restatement_fp64_reproduces_reference_deep_supervision():
    c, a = CASES["ds"]
    target = torch.from_numpy(a["t"])
    views = deep_supervision_targets(target, c["scales"])
    assert all(not v.is_contiguous() and v.data_ptr() >= target.data_ptr() for v in views[1:])
    xs = [torch.from_numpy(a[f"x_{i}"]) for i in range(5)]
    L, gs = O.loss_and_grads(lambda *xx: O.deep_supervision(oracle_fn(c), xx, views, a["weights"]), xs, torch.float64)
    assert abs(float(L) - float(a["L64"])) <= 1e-12 * abs(float(a["L64"]))
    for i, g in enumerate(gs):
        assert rel(g.numpy(), a[f"g64_{i}"]) <= 1e-12, i
    assert not a["g64_4"].any()                               # nnU-Net's last level has weight 0


def test_build_loss_reproduces_reference_weights_and_settings():
    a = CASES["ds"][1]
    w = SL.build_loss(5, batch_dice=True)
    assert isinstance(w, SL.DeepSupervisionWrapper) and isinstance(w.loss, SL.DC_and_CE_loss)
    assert np.array_equal(np.asarray(w.weight_factors, np.float64), a["weights"])
    assert np.allclose(O.nnunet_weights(5), a["weights"], rtol=1e-15, atol=0)
    dc = w.loss.dc
    assert isinstance(dc, SL.MemoryEfficientSoftDiceLoss) and (dc.batch_dice, dc.do_bg, dc.smooth) == (True, False, 1e-5)
    assert (w.loss.weight_ce, w.loss.weight_dice, w.loss.ignore_label) == (1.0, 1.0, None)
    r = SL.build_loss(3, batch_dice=False, regions=True, ignore_label=4)
    assert isinstance(r.loss, SL.DC_and_BCE_loss) and r.loss.use_ignore_label
    assert (r.loss.dc.batch_dice, r.loss.dc.do_bg, r.loss.dc.smooth) == (False, True, 1e-5)
    assert np.array_equal(np.asarray(r.weight_factors), np.array([2 / 3, 1 / 3, 0.0]))
    assert SL.build_loss(2, True, ignore_label=7).loss.ignore_label == 7


def test_unsupported_arguments_name_themselves():
    with pytest.raises(NotImplementedError, match="clip_tp"):
        SL.SoftDiceLoss(clip_tp=0.1)
    with pytest.raises(NotImplementedError, match="clip_tp"):
        SL.DC_and_CE_loss({"clip_tp": 0.1}, {}, dice_class=SL.SoftDiceLoss)
    with pytest.raises(NotImplementedError, match="ce_kwargs"):
        SL.DC_and_CE_loss({}, {"label_smoothing": 0.1})
    with pytest.raises(NotImplementedError, match="ce_kwargs"):
        SL.DC_and_CE_loss({}, {"weight": torch.ones(3)})
    with pytest.raises(NotImplementedError, match="bce_kwargs"):
        SL.DC_and_BCE_loss({"pos_weight": torch.ones(3)}, {})
    with pytest.raises(NotImplementedError, match="apply_nonlin"):
        SL.MemoryEfficientSoftDiceLoss(apply_nonlin=torch.sigmoid)
    with pytest.raises(NotImplementedError, match="apply_nonlin"):
        SL.DC_and_CE_loss({"apply_nonlin": torch.sigmoid}, {})
    with pytest.raises(NotImplementedError, match="dice_class"):
        SL.DC_and_CE_loss({}, {}, dice_class=torch.nn.Identity)
    with pytest.raises(NotImplementedError, match="loss"):
        SL.DeepSupervisionWrapper(torch.nn.MSELoss())
    with pytest.raises(NotImplementedError):
        SL.MemoryEfficientSoftDiceLoss()(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2))


def test_non_5d_and_cpu_tensors_are_refused():
    ce = SL.DC_and_CE_loss({"batch_dice": True, "do_bg": False, "smooth": 1e-5, "ddp": False}, {}, dice_class=SL.MemoryEfficientSoftDiceLoss)
    with pytest.raises(NotImplementedError, match="net_output"):
        ce(torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 8, 8, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="cuda"):
        ce(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4, dtype=torch.int16))
    bce = SL.DC_and_BCE_loss({}, {"batch_dice": False, "do_bg": True, "smooth": 1e-5, "ddp": False})
    with pytest.raises(RuntimeError, match="cuda"):
        bce(torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 3, 4, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="cuda"):
        SL.build_loss(2, True)([torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 2, 2, 2)],
                               [torch.zeros(1, 1, 4, 4, 4, dtype=torch.int16), torch.zeros(1, 1, 2, 2, 2, dtype=torch.int16)])


def test_ddp_batch_dice_across_ranks_is_refused(monkeypatch):
    """the check precedes the device check, so it shows without a GPU and without a second process"""
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    x, t = torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4, dtype=torch.int16)
    with pytest.raises(NotImplementedError, match="ddp"):
        SL.DC_and_CE_loss({"batch_dice": True, "ddp": True}, {})(x, t)
    with pytest.raises(RuntimeError, match="cuda"):          # no batch Dice: ranks do not interact, only the device is wrong here
        SL.DC_and_CE_loss({"batch_dice": False, "ddp": True}, {})(x, t)
