"""GPU: am_seg_hard_counts (anatomask_amd/csrc/seg_eval_ops.hip) and the segmentation fine-tuning trainer (anatomask_amd.seg_trainer,
anatomask_amd.finetune).

Counts: every comparison is torch.equal on int64 -- against the REFERENCE's get_tp_fp_fn_tn (tests/golden/seg_counts_tiny.npz) and
against tests/seg_counts_oracle.hard_counts (plain torch on the CPU, pinned to that fixture by tests/test_seg_trainer_cpu.py).  Logits lie
on the half-integer grid round(6 randn) / 2 unless a test says otherwise: many voxels tie at the maximum and the sigmoid logits hit 0.

Trainer, tiny network of tests/seg_oracle.py at 32^3, B = 2, nnU-Net's five-level loss.  Bounds, none from the code under test:
  gradient     the trainer's flat gradient against seg_train.STUNet + build_loss + backward on the same weights and batch (the path
               the trainer is built from): 1e-4 relative L2 per tensor, the run-to-run bound of
               test_seg_train_gpu.test_backward_reads_no_uninitialised_memory_and_repeats (the weight gradients add with fp32 atomics)
  grad_norm    2 ulp (fp32) of the fp64 norm of the flat gradient read back (am_sumsq is within 4u of the sum, 2u of the root, and the
               norm is rounded to fp32 once: 3u < 2 ulp = 4u)
  p, m, v      step_oracle.adamw_ema_step_ref within adamw_K u S per element (test_step_ops_gpu.check_adamw), and torch's
               clip_grad_norm_ + AdamW (step_oracle.adamw_torch_ref) within that plus adamw_scalar_terms
  descent      twenty steps lower the loss by more than half of what the same network under torch.optim.AdamW(eps=1e-4) +
               clip_grad_norm_(12) achieves on the same batch
  validation   Dice per class equal (fp64, NaN = NaN) to the value from the oracle's counts of the network's own logits
Every test prints what it measured.  On an MI355X: every count equal; the flat gradient within 6.1e-7 of the parent path's per tensor;
p / m / v at most 0.47 of the kernel-contract bound and 0.36 of the bound against torch; twenty steps at lr 1e-3 take the loss
1.1241 -> 0.2647 (fp32; torch AdamW on the same network 0.2647) and 1.1245 -> 0.2691 (bf16; 0.2679)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from anatomask_amd import finetune, hip, ops, predict, seg_loss, seg_train, segmentation
from anatomask_amd.data import deep_supervision_targets
from anatomask_amd.seg_trainer import SegTrainer
from tests import seg_counts_oracle as CO
from tests import seg_oracle as SO
from tests import step_oracle as S
from tests.test_seg_train_gpu import SCALES, _case, _net, _poison_allocator
from tests.test_step_ops_gpu import check_adamw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_counts_tiny.npz")
CASES = ("softmax_k2", "softmax_k5", "softmax_k105", "softmax_k5_ignore", "softmax_k5_allignored", "regions_r3", "regions_r3_ignore")
SIZE, DEPTH = (32, 32, 32), (1,) * 6
K_TINY = SO.TINY["num_classes"]


# ====================================================================================== am_seg_hard_counts
def _grid(g, *shape):
    return torch.round(6 * torch.randn(*shape, generator=g)) / 2


def _gpu(mode, x, t, ign=None, **kw):
    out = ops.seg_hard_counts(mode, x.to(DEV), t.to(DEV), ign, **kw)
    assert out.dtype == torch.int64 and tuple(out.shape) == (x.shape[1], 3)
    return out.cpu()


@pytest.mark.parametrize("name", CASES)
def test_counts_fixture(name):
    with np.load(GOLDEN) as z:
        c = json.loads(str(z["cases"]))[name]
        x, t, want = torch.from_numpy(z[f"{name}.x"]), torch.from_numpy(z[f"{name}.t"]), torch.from_numpy(z[f"{name}.counts"])
    got = _gpu(ops.SEG_SIGMOID if c["regions"] else ops.SEG_SOFTMAX, x, t, c["ignore_label"])
    assert torch.equal(got, want), (name, got.tolist(), want.tolist())


@pytest.mark.parametrize("K", [1, 2, 3, 5, 105, 260])
@pytest.mark.parametrize("shape", [(2, 9, 8, 24), (1, 1, 1, 1), (2, 16, 16, 16)])
def test_counts_ragged_shapes(shape, K):
    """6.75 tiles, one voxel, 16 whole tiles; K < 4 leaves waves without classes, K = 260 exceeds anything sized 256"""
    g = torch.Generator().manual_seed(100 * K + shape[1])
    B, sp = shape[0], shape[1:]
    x = _grid(g, B, K, *sp)
    lab = torch.randint(0, K + 1, (B, 1, *sp), generator=g).to(torch.int16)          # K: the ignore label where one is given
    for ign in (None, K):
        want = CO.hard_counts(CO.SOFTMAX, x, lab, ign)
        assert torch.equal(_gpu(ops.SEG_SOFTMAX, x, lab, ign), want), ("softmax", shape, K, ign)
    for ign in (None, 1):
        t = (torch.rand(B, K + (ign is not None), *sp, generator=g) < 0.4).to(torch.uint8)
        want = CO.hard_counts(CO.SIGMOID, x, t, ign)
        assert torch.equal(_gpu(ops.SEG_SIGMOID, x, t, ign), want), ("sigmoid", shape, K, ign)
        assert torch.equal(_gpu(ops.SEG_SIGMOID, x, t.bool(), ign), want)


def test_counts_ties_across_and_inside_waves():
    """voxel (a, j): classes a and a + j (j = 1: different waves, j = 4: the same wave) tie at the maximum 5, everything else lies below: the
    prediction is a.  The label is a + j, so a kernel that let the larger index win would count a true positive."""
    K = 12
    pairs = [(a, a + j) for j in (1, 4) for a in range(K - j)]
    g = torch.Generator().manual_seed(5)
    x = torch.round(4 * torch.rand(1, K, 1, 1, len(pairs), generator=g)) / 2          # 0 .. 2
    lab = torch.zeros(1, 1, 1, 1, len(pairs), dtype=torch.int16)
    want = torch.zeros(K, 3, dtype=torch.int64)
    for i, (a, b) in enumerate(pairs):
        x[0, a, 0, 0, i] = x[0, b, 0, 0, i] = 5.0
        lab[0, 0, 0, 0, i] = b
        want[a, 1] += 1
        want[b, 2] += 1
    assert torch.equal(CO.hard_counts(CO.SOFTMAX, x, lab), want)
    got = _gpu(ops.SEG_SOFTMAX, x, lab)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    # the same ties repeated over several tiles and both samples
    xx = x.expand(2, K, 3, 11, len(pairs)).contiguous()
    ll = lab.expand(2, 1, 3, 11, len(pairs)).contiguous()
    assert torch.equal(_gpu(ops.SEG_SOFTMAX, xx, ll), want * 66)


def test_counts_labels_outside_the_classes():
    """-1 and K + 3 without an ignore label: counted voxels of no class, they add to fp of the predicted class only"""
    K, g = 5, torch.Generator().manual_seed(6)
    x = _grid(g, 2, K, 7, 6, 10)
    lab = torch.randint(0, K, (2, 1, 7, 6, 10), generator=g).to(torch.int16)
    sel = torch.rand(lab.shape, generator=g)
    lab[sel < 0.2] = -1
    lab[sel > 0.8] = K + 3
    want = CO.hard_counts(CO.SOFTMAX, x, lab)
    inside = CO.hard_counts(CO.SOFTMAX, x, lab.clamp(0, K - 1))
    assert int(want[:, 2].sum()) < int(inside[:, 2].sum()) and int((want[:, 0] + want[:, 1]).sum()) == lab.numel()
    assert torch.equal(_gpu(ops.SEG_SOFTMAX, x, lab), want)


def test_counts_strided_targets():
    g = torch.Generator().manual_seed(7)
    K = 4
    target = torch.randint(0, K, (2, 1, 8, 12, 16), generator=g).to(torch.int16).to(DEV)
    view = deep_supervision_targets(target, [1, 0.5])[1]
    assert not view.is_contiguous() and view.data_ptr() != target.data_ptr()
    x = _grid(g, 2, K, 4, 6, 8)
    got = ops.seg_hard_counts(ops.SEG_SOFTMAX, x.to(DEV), view).cpu()
    assert torch.equal(got, ops.seg_hard_counts(ops.SEG_SOFTMAX, x.to(DEV), view.contiguous()).cpu())
    assert torch.equal(got, CO.hard_counts(CO.SOFTMAX, x, view.cpu()))
    for ign in (None, 1):
        wide = (torch.rand(2, K + (ign is not None), 4, 6, 16, generator=g) < 0.4).to(torch.uint8).to(DEV)
        rv = wide[..., ::2]
        assert not rv.is_contiguous()
        got = ops.seg_hard_counts(ops.SEG_SIGMOID, x.to(DEV), rv, ign).cpu()
        assert torch.equal(got, ops.seg_hard_counts(ops.SEG_SIGMOID, x.to(DEV), rv.contiguous(), ign).cpu())
        assert torch.equal(got, CO.hard_counts(CO.SIGMOID, x, rv.cpu(), ign))


def test_counts_accumulate_and_overwrite():
    g = torch.Generator().manual_seed(8)
    K = 5
    x, lab = _grid(g, 2, K, 5, 6, 7), torch.randint(0, K, (2, 1, 5, 6, 7), generator=g).to(torch.int16)
    want = CO.hard_counts(CO.SOFTMAX, x, lab)
    table = torch.full((K, 3), 2 ** 40 + 7, dtype=torch.int64, device=DEV)
    ret = ops.seg_hard_counts(ops.SEG_SOFTMAX, x.to(DEV), lab.to(DEV), out=table, accumulate=True)
    assert ret.data_ptr() == table.data_ptr() and torch.equal(table.cpu(), want + (2 ** 40 + 7))
    ops.seg_hard_counts(ops.SEG_SOFTMAX, x.to(DEV), lab.to(DEV), out=table, accumulate=True)
    assert torch.equal(table.cpu(), 2 * want + (2 ** 40 + 7))
    poisoned = torch.full((K, 3), -0x0123456789ABCDEF, dtype=torch.int64, device=DEV)
    ops.seg_hard_counts(ops.SEG_SOFTMAX, x.to(DEV), lab.to(DEV), out=poisoned, accumulate=False)
    assert torch.equal(poisoned.cpu(), want)


def test_counts_above_two_to_the_24():
    """16 842 752 voxels, all labelled and predicted class 1: an fp32 sum would stop at 16 777 216"""
    shape = (256, 256, 257)
    n = shape[0] * shape[1] * shape[2]
    x = torch.zeros(1, 2, *shape, device=DEV)
    x[:, 1] = 1.0
    lab = torch.ones(1, 1, *shape, dtype=torch.int16, device=DEV)
    got = ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab).cpu()
    assert n == 16842752 and n > 2 ** 24
    assert got.tolist() == [[0, 0, 0], [n, 0, 0]], got.tolist()


def test_counts_repeat_on_poisoned_memory():
    g = torch.Generator().manual_seed(9)
    K = 105
    x, lab = _grid(g, 2, K, 9, 8, 24).to(DEV), torch.randint(0, K, (2, 1, 9, 8, 24), generator=g).to(torch.int16).to(DEV)
    t = (torch.rand(2, K, 9, 8, 24, generator=g) < 0.4).to(torch.uint8).to(DEV)
    first = ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab).cpu(), ops.seg_hard_counts(ops.SEG_SIGMOID, x, t).cpu()
    _poison_allocator()
    second = ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab).cpu(), ops.seg_hard_counts(ops.SEG_SIGMOID, x, t).cpu()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert torch.equal(first[0], CO.hard_counts(CO.SOFTMAX, x, lab))


def test_counts_bad_arguments_raise():
    x = torch.zeros(1, 3, 4, 4, 4, device=DEV)
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.int16, device=DEV)
    reg = torch.zeros(1, 3, 4, 4, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x.cpu(), lab.cpu())
    with pytest.raises(RuntimeError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab.cpu())
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x.double(), lab)
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x.permute(0, 1, 2, 4, 3), lab)               # not contiguous
    with pytest.raises(ValueError):
        ops.seg_hard_counts(7, x, lab)
    with pytest.raises(TypeError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab.int())
    with pytest.raises(TypeError):
        ops.seg_hard_counts(ops.SEG_SIGMOID, x, reg.to(torch.int16))
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x, reg.to(torch.int16))                      # 3 channels of labels
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SIGMOID, x, reg, 1)                                   # the ignore channel is missing
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab, out=torch.zeros(3, 3, device=DEV))   # a float table
    with pytest.raises(ValueError):
        ops.seg_hard_counts(ops.SEG_SOFTMAX, x, lab, accumulate=True)                     # nothing to add to
    # the ABI itself: -1, nothing launched, the table untouched
    need = ops.seg_hard_counts_workspace_bytes(1, 64, 3)
    assert need == 1 * 1 * 3 * 16
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    table = torch.full((4, 3), 77, dtype=torch.int64, device=DEV)
    st = lab.stride()

    def call(mode=ops.SEG_SOFTMAX, xp=x.data_ptr(), K=3, tp=lab.data_ptr(), wp=ws.data_ptr(), wb=need, cp=table.data_ptr()):
        hip.lib().seg_hard_counts(mode, xp, 1, K, 4, 4, 4, tp, *st, 0, 0, wp, wb, cp, 0, torch.cuda.current_stream().cuda_stream)
    for bad in (dict(K=0), dict(mode=2), dict(xp=None), dict(tp=None), dict(wp=None), dict(cp=None), dict(wb=need - 1),
                dict(cp=table.data_ptr() + 4), dict(wp=ws.data_ptr() + 8)):
        with pytest.raises(RuntimeError, match="am_seg_hard_counts failed with code -1"):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((table == 77).all())
    call()
    assert torch.equal(table[:3].cpu(), CO.hard_counts(CO.SOFTMAX, x, lab)) and bool((table[3] == 77).all())


# ====================================================================================== SegTrainer
def _trainer(dtype=torch.float32, weights=None, **kw):
    W, x, labels = _case(SIZE, DEPTH)
    net = _net(W if weights is None else weights, DEPTH, dtype)
    return SegTrainer(net, **kw), x.to(DEV), labels.to(DEV)


def _pad_mask(tr):
    pad = torch.ones(tr.n, dtype=torch.bool)
    for o, num in tr.offsets.values():
        pad[o:o + num] = False
    return pad


def test_train_step_is_clip_adamw_on_the_parents_gradient():
    tr, xd, ld = _trainer(num_epochs=10)
    W, _, _ = _case(SIZE, DEPTH)
    ref = _net(W, DEPTH, torch.float32)
    loss_fn = seg_loss.build_loss(5, True)
    targets = deep_supervision_targets(ld, SCALES)
    pad = _pad_mask(tr)
    assert int(pad.sum()) > 0 and tr.n % 4 == 0 and all(p.grad is None for p in tr.net.parameters())
    kw = dict(betas=(0.9, 0.999), eps=1e-4, wd=1e-5, ema_decay=0.0, max_norm=12.0, grad_scale=1.0)
    worst_g = 0.0
    for i, epoch in enumerate((0, 3, 7)):
        tr.set_epoch(epoch)
        lr = 0.5 * 1e-4 * (1 + math.cos(math.pi * epoch / 10))
        assert tr.lr == lr
        p0, m0, v0 = (t.cpu().numpy().copy() for t in (tr.flat, tr.m, tr.v))
        ref.load_state_dict(tr.net.state_dict())
        for p in ref.parameters():
            p.grad = None
        ref_loss = loss_fn(ref(xd), targets)
        ref_loss.backward()
        out = tr.train_step(xd, ld)
        assert set(out) == {"loss", "grad_norm"} and all(t.is_cuda for t in out.values())
        assert torch.equal(out["loss"].reshape(()), ref_loss.detach())               # the forward and the loss are deterministic
        g = tr.gflat.cpu()
        # (i) the flat gradient is the parent path's gradient
        for (n, p), (_, q) in zip(tr.net.named_parameters(), ref.named_parameters()):
            o, num = tr.offsets[n]
            assert p.grad.data_ptr() == tr.gflat[o:o + num].data_ptr()
            a, b = g[o:o + num].double(), q.grad.flatten().double().cpu()
            if float(b.norm()) == 0.0:
                assert float(a.abs().max()) == 0.0, n
            else:
                e = float((a - b).norm() / b.norm())
                worst_g = max(worst_g, e)
                assert e <= 1e-4, (n, e)
        # (ii) the norm
        want = float(np.sqrt(np.sum(g.numpy().astype(np.float64) ** 2)))
        gn = float(out["grad_norm"])
        assert abs(gn - want) <= 2 * float(np.spacing(np.float32(want))), (gn, want)
        # (iii) the kernel's contract, (iv) torch's clip_grad_norm_ + AdamW, from the state before the step
        r = S.adamw_ema_step_ref(p0, g.numpy(), m0, v0, None, lr=lr, step=i + 1, sumsq=float(tr.sumsq.cpu()), **kw)
        got = dict(p=tr.flat.cpu().numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy())
        check_adamw(f"SegTrainer step {i + 1} lr {lr:.3e} gnorm {gn:.4f}", got, r)
        tp, tm, tv, _, tt = S.adamw_torch_ref(p0, g.numpy(), m0, v0, None, lr=lr, step=i + 1, **kw)
        rt = dict(r, p=tp.numpy(), m=tm.numpy(), v=tv.numpy())
        check_adamw(f"SegTrainer step {i + 1} against torch", got, rt, extra=S.adamw_scalar_terms(r, kw["betas"], 0.0))
        assert not np.array_equal(got["p"], p0)
        # (v) the padding
        for name, t in (("p", tr.flat), ("g", tr.gflat), ("m", tr.m), ("v", tr.v)):
            assert float(t.cpu()[pad].abs().max()) == 0.0, name
    print(f"SegTrainer: flat gradient against the parent's path, worst per-tensor relative L2 {worst_g:.3e}")
    assert tr.step_count == 3


@functools.lru_cache(maxsize=None)
def _parent_descent(dtype, steps, lr):
    W, x, labels = _case(SIZE, DEPTH)
    net = _net(W, DEPTH, dtype)
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=1e-5, eps=1e-4)
    loss_fn = seg_loss.build_loss(5, True)
    xd, targets = x.to(DEV), deep_supervision_targets(labels.to(DEV), SCALES)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = loss_fn(net(xd), targets)
        losses.append(loss.detach())
        if len(losses) <= steps:
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 12)
            opt.step()
    return float(losses[0]), float(losses[-1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_twenty_steps_descend(dtype):
    steps, lr = 20, 1e-3
    tr, xd, ld = _trainer(dtype, num_epochs=1000, initial_lr=lr)
    losses = [tr.train_step(xd, ld)["loss"] for _ in range(steps)]
    with torch.no_grad():
        last = float(tr.loss_fn(list(tr.net(xd)), deep_supervision_targets(ld, SCALES)))
    first = float(losses[0])
    o_first, o_last = _parent_descent(dtype, steps, lr)
    print(f"SegTrainer {dtype}: loss {first:.5f} -> {last:.5f} after {steps} steps; torch AdamW on the same network {o_first:.5f} -> {o_last:.5f}")
    assert o_first - o_last > 0
    assert first - last > 0.5 * (o_first - o_last), (first, last, o_first, o_last)


def test_validation_counts_dice_and_touches_nothing():
    tr, xd, ld = _trainer()
    tr.train_step(xd, ld)                                                             # .grad are views now, m and v are live
    before = [t.clone() for t in (tr.flat, tr.gflat, tr.m, tr.v)]
    want = torch.zeros(K_TINY, 3, dtype=torch.int64)
    losses = []
    for j in range(3):
        x, lab = xd.roll(3 * j + 1, 2 + j), ld.roll(5 * j, 4 - j)
        out = tr.validation_step(x, lab)
        assert set(out) == {"loss"} and out["loss"].is_cuda
        losses.append(float(out["loss"]))
        with torch.no_grad():
            logits = tr.net(x)[0]
        assert not logits.requires_grad
        want += CO.hard_counts(CO.SOFTMAX, logits, lab)
    assert torch.equal(tr.counts.cpu(), want) and int(want.sum()) > 0
    m = tr.on_validation_epoch_end()
    assert set(m) == {"mean_fg_dice", "dice_per_class_or_region", "ema_fg_dice", "val_loss", "is_best"}
    dice = CO.dice_from_counts(want.numpy(), True)
    print(f"SegTrainer validation: Dice per class {dice}, losses {losses}")
    assert len(m["dice_per_class_or_region"]) == K_TINY - 1
    assert np.array_equal(np.array(m["dice_per_class_or_region"]), dice, equal_nan=True)
    assert m["mean_fg_dice"] == float(np.nanmean(dice)) and m["ema_fg_dice"] == m["mean_fg_dice"] and m["is_best"] is True
    assert abs(m["val_loss"] - sum(losses) / 3) <= 1e-6 * abs(sum(losses) / 3)
    assert int(tr.counts.abs().sum()) == 0 and float(tr._val_loss) == 0.0             # reset
    for a, b in zip(before, (tr.flat, tr.gflat, tr.m, tr.v)):
        assert torch.equal(a, b)
    assert tr.step_count == 1
    # a second epoch: the EMA rule
    tr.validation_step(xd, ld)
    m2 = tr.on_validation_epoch_end()
    assert m2["ema_fg_dice"] == m["ema_fg_dice"] * 0.9 + 0.1 * m2["mean_fg_dice"]
    assert m2["is_best"] == (m2["ema_fg_dice"] > m["ema_fg_dice"])
    # a fresh trainer's validation leaves every .grad None
    tr2, _, _ = _trainer()
    tr2.validation_step(xd, ld)
    assert all(p.grad is None for p in tr2.net.parameters())


@pytest.mark.parametrize("ignore", [None, 1])
def test_validation_regions(ignore):
    tr, xd, ld = _trainer(regions=True, ignore_label=ignore)
    g = torch.Generator().manual_seed(11)
    chans = [(ld >= k + 1).cpu() for k in range(K_TINY - 1)] + [torch.rand(2, 1, *SIZE, generator=g) < 0.3]
    if ignore is not None:
        chans.append(torch.rand(2, 1, *SIZE, generator=g) < 0.1)
    target = torch.cat(chans, 1).to(torch.uint8).to(DEV)
    before = tr.flat.clone()
    tr.validation_step(xd, target)
    with torch.no_grad():
        logits = tr.net(xd)[0]
    want = CO.hard_counts(CO.SIGMOID, logits, target, ignore)
    assert torch.equal(tr.counts.cpu(), want)
    m = tr.on_validation_epoch_end()
    assert len(m["dice_per_class_or_region"]) == K_TINY                                # regions keep every channel
    assert np.array_equal(np.array(m["dice_per_class_or_region"]), CO.dice_from_counts(want.numpy(), False), equal_nan=True)
    assert int(tr.counts.abs().sum()) == 0 and torch.equal(before, tr.flat) and all(p.grad is None for p in tr.net.parameters())
    out = tr.train_step(xd, target)                                                   # and the region loss trains
    assert bool(torch.isfinite(out["loss"]).all()) and not torch.equal(before, tr.flat)


def test_checkpoint_round_trip(tmp_path):
    tr, xd, ld = _trainer(num_epochs=10)
    tr.set_epoch(2)
    for _ in range(2):
        tr.train_step(xd, ld)
    tr.validation_step(xd, ld)
    tr.on_validation_epoch_end()
    path = str(tmp_path / "seg.pth")
    tr.save(path, 2)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {"network_weights", "optimizer_state", "grad_scaler_state", "logging", "_best_ema", "current_epoch", "trainer_name"} <= set(ck)
    assert ck["current_epoch"] == 3 and ck["grad_scaler_state"] is None and ck["_best_ema"] == tr.best_ema
    assert not any(k.startswith("module.") for k in ck["network_weights"])
    # a fresh trainer around OTHER weights loads it
    other = SO.seeded_weights(SO.state_keys(SO.TINY["dims"], list(DEPTH), K_TINY), 99)
    tr2, _, _ = _trainer(weights=other, num_epochs=10)
    info = tr2.load(path)
    assert info["current_epoch"] == 3 and tr2.current_epoch == 3 and tr2.step_count == 2
    tr2.set_epoch(2)
    assert tr2.lr == tr.lr and tr2.best_ema == tr.best_ema and json.dumps(tr2.logging) == json.dumps(tr.logging)
    for a, b in ((tr.flat, tr2.flat), (tr.m, tr2.m), (tr.v, tr2.v)):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(tr.net(xd), tr2.net(xd)))
    o1, o2 = tr.train_step(xd, ld), tr2.train_step(xd, ld)
    assert torch.equal(o1["loss"], o2["loss"])                                        # the step's forward saw the same bits
    for n, (o, num) in tr.offsets.items():
        for a, b in ((tr.flat, tr2.flat), (tr.m, tr2.m), (tr.v, tr2.v)):
            d, s = float((a[o:o + num] - b[o:o + num]).norm()), float(a[o:o + num].norm())
            assert d <= 1e-4 * s, (n, d, s)
    # nnU-Net's layout: torch's AdamW takes the optimizer state, predict.load_weights the file
    ref = tr.reference_checkpoint(2)
    opt = torch.optim.AdamW(tr.net.parameters())
    opt.load_state_dict(ref["optimizer_state"])
    for (n, p) in tr.net.named_parameters():
        o, num = tr.offsets[n]
        st = opt.state[p]
        assert torch.equal(st["exp_avg"].flatten().to(DEV), tr.m[o:o + num]) and torch.equal(st["exp_avg_sq"].flatten().to(DEV), tr.v[o:o + num])
        assert float(st["step"]) == 3.0 and st["exp_avg"].shape == p.shape
    grp = opt.param_groups[0]
    assert grp["lr"] == tr.lr and grp["eps"] == 1e-4 and grp["weight_decay"] == 1e-5 and tuple(grp["betas"]) == (0.9, 0.999)
    sd = predict.load_weights(path)
    assert predict.architecture_of(sd) == dict(dims=SO.TINY["dims"], depth=list(DEPTH), num_classes=K_TINY)
    assert all(torch.equal(sd[k], v.cpu()) for k, v in ck["network_weights"].items())


def test_not_served_raises():
    W, _, _ = _case(SIZE, DEPTH)
    with pytest.raises(RuntimeError, match="cuda"):
        net = seg_train.STUNet(1, K_TINY, depth=list(DEPTH), dims=SO.TINY["dims"])
        SegTrainer(net)
    with pytest.raises(TypeError, match="seg_train.STUNet"):
        SegTrainer(_net(W, DEPTH, torch.float32, segmentation.STUNet))
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        SegTrainer(_net(W, DEPTH, torch.float32), gradient_accumulation_steps=2)
    with pytest.raises(NotImplementedError, match="grad scaler"):
        SegTrainer(_net(W, DEPTH, torch.float32), grad_scaler=object())
    with pytest.raises(ValueError, match="schedule"):
        SegTrainer(_net(W, DEPTH, torch.float32), schedule="step")


def test_finetune_driver_on_synthetic_data(tmp_path, capsys):
    out = str(tmp_path / "run")
    rc = finetune.main(["--num-classes", "3", "--dims", *[str(d) for d in SO.TINY["dims"]], "--depth", *["1"] * 6, "--input-size", "32", "32", "32",
                        "--epochs", "2", "--iters-per-epoch", "2", "--val-iters", "1", "--batch-size", "2", "--dtype", "f32", "--out", out])
    assert rc == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["epoch"] for l in lines] == [0, 1]
    for l in lines:
        assert all(math.isfinite(l[k]) for k in ("lr", "train_loss", "val_loss", "mean_fg_dice", "ema_fg_dice")), l
    assert lines[0]["is_best"] is True and lines[0]["lr"] == 1e-4 and lines[1]["lr"] == 0.5e-4 * (1 + math.cos(math.pi / 2))
    for name in ("checkpoint_latest.pth", "checkpoint_best.pth", "checkpoint_final.pth"):
        ck = torch.load(os.path.join(out, name), map_location="cpu", weights_only=True)
        assert ck["trainer_name"] == "SegTrainer" and ck["current_epoch"] in (1, 2)
    assert torch.load(os.path.join(out, "checkpoint_final.pth"), weights_only=True)["current_epoch"] == 2
