"""CPU: the parts of the segmentation fine-tuning trainer that need no GPU.

  * tests/seg_counts_oracle.hard_counts (the plain torch restatement the GPU tests compare am_seg_hard_counts with) equals the counts of the
    REFERENCE's get_tp_fp_fn_tn stored in tests/golden/seg_counts_tiny.npz exactly, in every case;
  * seg_trainer.lr_at against torch.optim.lr_scheduler.CosineAnnealingLR stepped e times on a dummy optimizer, and against the
    reference's poly formula, e in {0, 1, 500, 999} of T = 1000, to 1e-12 relative;
  * the Dice / nanmean / EMA / best bookkeeping on a hand-made table with one class of zero denominator;
  * the optimizer_state layout: torch.optim.AdamW.load_state_dict accepts it and finds exp_avg / exp_avg_sq / step where it looks."""
import json
import math
import os

import numpy as np
import pytest
import torch

from anatomask_amd import seg_trainer as T
from tests import seg_counts_oracle as CO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_counts_tiny.npz")
CASES = ("softmax_k2", "softmax_k5", "softmax_k105", "softmax_k5_ignore", "softmax_k5_allignored", "regions_r3", "regions_r3_ignore")


def test_fixture_holds_every_case():
    with np.load(GOLDEN) as z:
        meta = json.loads(str(z["cases"]))
        assert tuple(meta) == CASES
        assert os.path.getsize(GOLDEN) < 1 << 20
        for name, c in meta.items():
            x, t, counts = z[f"{name}.x"], z[f"{name}.t"], z[f"{name}.counts"]
            assert x.dtype == np.float32 and x.shape == (2, c["K"], 5, 6, 7) and counts.dtype == np.int64 and counts.shape == (c["K"], 3)
            assert t.dtype == (np.uint8 if c["regions"] else np.int16)
            assert np.array_equal(x * 2, np.round(x * 2))                # the half-integer grid: ties at the maximum, exact zeros
            if c["regions"]:
                assert (x == 0).any() and not ((x > 0) & (x < 1e-7)).any()
            elif c["K"] > 1:
                top = np.sort(x, 1)
                assert (top[:, -1] == top[:, -2]).sum() >= 10            # voxels whose maximum is tied
        assert int(z["softmax_k5_allignored.counts"].sum()) == 0 and int(z["softmax_k5_ignore.t"].max()) == 5


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_the_reference_counts(name):
    with np.load(GOLDEN) as z:
        c = json.loads(str(z["cases"]))[name]
        got = CO.hard_counts(CO.SIGMOID if c["regions"] else CO.SOFTMAX, torch.from_numpy(z[f"{name}.x"]), torch.from_numpy(z[f"{name}.t"]),
                             c["ignore_label"])
        assert got.dtype == torch.int64 and torch.equal(got, torch.from_numpy(z[f"{name}.counts"]))


def test_oracle_labels_outside_the_classes_add_to_fp_only():
    x = torch.tensor([0.0, 1.0, 0.5]).view(1, 3, 1, 1, 1).expand(1, 3, 1, 1, 4).contiguous()
    t = torch.tensor([-1, 1, 6, 0], dtype=torch.int16).view(1, 1, 1, 1, 4)
    got = CO.hard_counts(CO.SOFTMAX, x, t)
    assert got.tolist() == [[0, 0, 1], [1, 3, 0], [0, 0, 0]]


@pytest.mark.parametrize("e", [0, 1, 500, 999])
def test_schedules_in_closed_form(e):
    T_, lr0 = 1000, 1e-4
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_)
    for _ in range(e):
        opt.step()
        sched.step()
    want = opt.param_groups[0]["lr"]
    got = T.lr_at("cosine", lr0, e, T_)
    assert abs(got - want) <= 1e-12 * want, (e, got, want)
    want = CO.poly_lr(lr0, e, T_)
    got = T.lr_at("poly", lr0, e, T_)
    assert abs(got - want) <= 1e-12 * want, (e, got, want)
    with pytest.raises(ValueError):
        T.lr_at("linear", lr0, e, T_)


def test_dice_nanmean_ema_and_best_bookkeeping():
    counts = np.array([[100, 3, 4], [5, 1, 1], [0, 0, 0], [3, 1, 2]])                # class 2: nothing predicted, nothing labelled
    s = T.validation_summary(counts, False, None, None)
    d = s["dice_per_class_or_region"]
    assert len(d) == 3 and d[0] == 10 / 12 and math.isnan(d[1]) and d[2] == 6 / 9    # class 0 dropped
    assert np.array_equal(np.array(d), CO.dice_from_counts(counts, True), equal_nan=True)
    mean = (10 / 12 + 6 / 9) / 2
    assert s["mean_fg_dice"] == mean and s["ema_fg_dice"] == mean and s["is_best"] is True      # the first value is taken as it is
    s2 = T.validation_summary(counts, False, 0.5, 0.9)
    assert s2["ema_fg_dice"] == 0.5 * 0.9 + 0.1 * mean and s2["is_best"] is False
    s3 = T.validation_summary(counts, False, 0.5, s2["ema_fg_dice"])
    assert s3["is_best"] is False                                                    # equal is not better
    s4 = T.validation_summary(counts, False, 0.5, 0.5)
    assert s4["is_best"] is True
    r = T.validation_summary(counts, True, None, None)                               # regions keep every channel
    assert len(r["dice_per_class_or_region"]) == 4 and r["dice_per_class_or_region"][0] == 200 / 207
    assert r["mean_fg_dice"] == (200 / 207 + 10 / 12 + 6 / 9) / 3


def test_optimizer_state_layout_loads_into_torch_adamw():
    g = torch.Generator().manual_seed(3)
    shapes = [(4, 3, 1, 1, 1), (4,), (2, 5)]
    m = [torch.randn(*s, generator=g) for s in shapes]
    v = [torch.rand(*s, generator=g) for s in shapes]
    sd = T.adamw_state_dict(m, v, 7, 5e-5, (0.9, 0.999), 1e-4, 1e-5, initial_lr=1e-4)
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 1 and sorted(sd["state"]) == [0, 1, 2]
    params = [torch.nn.Parameter(torch.zeros(*s)) for s in shapes]
    opt = torch.optim.AdamW(params)
    opt.load_state_dict(sd)
    grp = opt.param_groups[0]
    assert grp["lr"] == 5e-5 and tuple(grp["betas"]) == (0.9, 0.999) and grp["eps"] == 1e-4 and grp["weight_decay"] == 1e-5
    for p, a, b in zip(params, m, v):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], a) and torch.equal(st["exp_avg_sq"], b) and float(st["step"]) == 7.0
        assert st["exp_avg"].shape == p.shape
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()                                                                       # the loaded state steps
    assert float(opt.state[params[0]]["step"]) == 8.0
    empty = T.adamw_state_dict(m, v, 0, 1e-4, (0.9, 0.999), 1e-4, 1e-5)              # before the first step: torch has no state yet
    assert empty["state"] == {}
    torch.optim.AdamW(params).load_state_dict(empty)


def test_driver_loads_a_pretrained_encoder(tmp_path):
    """--pretrained: the entries whose key contains 'encoder', stripped up to 'sp_cnn.', land in conv_blocks_context; the decoder and the
    heads keep their initialisation; a checkpoint of another width is refused."""
    from anatomask_amd import finetune, seg_train
    from tests import seg_oracle as SO
    dims = SO.TINY["dims"]
    src = seg_train.STUNet(1, 3, depth=[1] * 6, dims=dims)
    dst = seg_train.STUNet(1, 3, depth=[1] * 6, dims=dims)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    ck = {"network_weights": {("module.sparse_encoder.sp_cnn." + k if k.startswith("conv_blocks_context.") else "module.dense_decoder." + k): v
                              for k, v in src.state_dict().items()}, "current_epoch": 3}
    path = str(tmp_path / "pretrain.pth")
    torch.save(ck, path)
    names = finetune.load_pretrained_encoder(dst, path)
    assert names and all(n.startswith("conv_blocks_context.") for n in names)
    assert len(names) == sum(k.startswith("conv_blocks_context.") for k in before)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, src.state_dict()[k] if k in names else before[k]), k
    wide = seg_train.STUNet(1, 3, depth=[1] * 6, dims=[16] + dims[1:])
    with pytest.raises(SystemExit, match="another shape"):
        finetune.load_pretrained_encoder(wide, path)
    torch.save({"network_weights": {"module.dense_decoder.x": torch.zeros(1)}}, path)
    with pytest.raises(SystemExit, match="no encoder weights"):
        finetune.load_pretrained_encoder(dst, path)
