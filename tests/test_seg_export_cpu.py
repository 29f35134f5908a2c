"""CPU: the fixture of the export step (tests/golden/seg_export_tiny.npz, made by the reference's LabelManager through
tests/golden/make_seg_export_fixtures.py), the new flags of anatomask_amd.predict, and the C ABI's am_seg_export declaration."""
import ctypes
import os

import numpy as np
import pytest
import torch

from anatomask_amd import build, hip, predict, segmentation
from tests import seg_oracle as SO


@pytest.fixture(scope="module")
def ex(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "seg_export_tiny.npz")))


def test_fixture_invariants(ex):
    for K in (3, 105):
        lg, pr, seg = ex[f"sm{K}.logits"], ex[f"sm{K}.probs"], ex[f"sm{K}.seg"]
        assert lg.shape == (K, 5, 6, 7) and pr.shape == lg.shape and pr.dtype == np.float32 and seg.shape == (5, 6, 7)
        assert np.array_equal(seg, lg.argmax(0))                         # the reference's argmax of the probabilities = argmax of the logits here
        assert np.isfinite(pr).all() and np.abs(pr.sum(0) - 1).max() < 1e-5
        p0, p1, p2 = (tuple(p) for p in ex[f"sm{K}.planted"])
        assert (lg[(slice(None),) + p0] == 200).all() and seg[p0] == 0
        assert lg[(0,) + p1] == 200 and (lg[(slice(1, None),) + p1] == -200).all() and seg[p1] == 0
        assert seg[p2] == K - 1
    lg = ex["rg.logits"]
    assert lg.shape == (3, 9, 10, 11)
    r0, r1, r2 = (tuple(p) for p in ex["rg.planted"])
    assert lg[(slice(None),) + r1].tolist() == [np.float32(1e-9), np.float32(-1e-9), np.float32(1e-9)]
    for j, order in enumerate(([1, 2, 3], [5, 1, 300])):
        seg = ex[f"rg.seg{j}"]
        assert ex[f"rg.order{j}"].tolist() == order
        assert seg[r0] == 0 and seg[r1] == 0 and seg[r2] == order[2]      # (an `l > 0` shortcut would label r1 order[2])
        want = np.zeros(seg.shape, dtype=np.int16)
        for i, c in enumerate(order):
            want[ex["rg.probs"][i] > 0.5] = c
        assert np.array_equal(seg, want)
    away = np.ones(lg.shape[1:], dtype=bool)
    away[r0] = away[r1] = False
    assert np.abs(lg[:, away]).min() >= 0.01


def test_new_flags_parse():
    a = predict.parser().parse_args(["case.npz", "ck.pth", "out", "--folds", "f1.pth", "f2.pth", "--save-probabilities",
                                     "--regions-class-order", "5", "1", "300", "--save-logits"])
    assert a.folds == ["f1.pth", "f2.pth"] and a.save_probabilities and a.regions_class_order == [5, 1, 300] and a.save_logits
    b = predict.parser().parse_args(["case.npz", "ck.pth", "out"])
    assert b.folds == [] and not b.save_probabilities and b.regions_class_order is None


def test_fold_of_another_architecture_is_refused_before_the_device(tmp_path, monkeypatch):
    t = SO.TINY
    torch.save({"network_weights": SO.seeded_weights(SO.state_keys(t["dims"], t["depth"], 3), 1)}, tmp_path / "a.pth")
    torch.save({"network_weights": SO.seeded_weights(SO.state_keys(t["dims"], t["depth"], 3), 2)}, tmp_path / "same.pth")
    torch.save({"network_weights": SO.seeded_weights(SO.state_keys(t["dims"], t["depth"], 4), 3)}, tmp_path / "other_classes.pth")
    torch.save(SO.seeded_weights(SO.state_keys([8, 16, 32, 64, 64, 64], t["depth"], 3), 4), tmp_path / "other_dims.pth")
    np.savez(tmp_path / "case.npz", data=np.zeros((1, 32, 32, 32), np.float32))

    def no_network(*a, **k):
        raise AssertionError("the network was built before the folds were checked")
    monkeypatch.setattr(segmentation, "STUNet", no_network)
    for bad in ("other_classes.pth", "other_dims.pth"):
        with pytest.raises(SystemExit) as e:
            predict.main([str(tmp_path / "case.npz"), str(tmp_path / "a.pth"), str(tmp_path / "out"), "--folds", str(tmp_path / "same.pth"),
                          str(tmp_path / bad)])
        assert bad in str(e.value) and "same.pth" not in str(e.value).split(" is another ")[0]
    with pytest.raises(SystemExit, match="regions-class-order"):
        predict.main([str(tmp_path / "case.npz"), str(tmp_path / "a.pth"), str(tmp_path / "out"), "--regions-class-order", "1", "2"])


def test_header_declares_seg_export_and_the_library_exports_it():
    decl = hip.declared_functions()
    assert "am_seg_export" in decl
    v, i = ctypes.c_void_p, ctypes.c_int
    assert decl["am_seg_export"] == [v, v] + [i] * 10 + [i, v, v, v, i, v]
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in decl:
        assert hasattr(lib, name), name
    txt = open(hip.HEADER).read()
    assert "#define AM_SEG_SOFTMAX 0" in txt and "#define AM_SEG_SIGMOID 1" in txt
