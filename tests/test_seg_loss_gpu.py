"""GPU: anatomask_amd.seg_loss (fused Dice + CE / BCE with deep supervision, loss_ops.hip) against the reference's fp64 results
(tests/golden/seg_loss_*.npz) and against the test-side restatement (tests/seg_loss_oracle.py, pinned to the reference by
tests/test_seg_loss_cpu.py) run in fp64 on the GPU.

Bounds -- none of them comes from the code under test.  With L64 / g64 the fp64 truth and the fp32 baselines (the reference in fp32 and the
plain-torch restatement in fp32, from the fixture; for shapes outside the fixture the restatement in fp32 on the GPU):
    loss      |L - L64| <= max(4 max_baselines |L32 - L64|, (K + 8) 2^-23 (max|x| + ln K + 1))
    gradient  relative L2 error against g64 <= max(4 max_baselines (their relative L2 error), (K + 8) 2^-23)
The factor 4 covers the difference in summation order between the kernel's wave / LDS / fp64 fold and torch's reductions; the floor is the
softmax error bound tests/test_seg_export_gpu.py derives (expf <= 2 ulp, a K-term sum, one division), scaled by the magnitude of the terms.

Measured on an MI355X (every test prints its figures; also in DESIGN.md section 5):
    fixture cases        loss error <= 1.5e-7 (bounds >= 1.4e-5); gradient 5.5e-8 .. 8.5e-8 (bounds >= 1.19e-6; fp32 baselines 4.4e-8 .. 1.5e-7)
    other shapes         gradient <= 1.0e-7, the single voxel 2.0e-7 (bound 1.31e-6: the largest ratio, 0.15)
    logits x100 + 1000   loss 2.7e-6 (bound 1.8e-3), gradient 4.4e-8 (plain fp32 torch: 8.6e-6); shifted vs unshifted gradients bit-equal
    2.2e9 logits         loss 1.5e-7 (bound 3.2e-5), gradient 8.6e-8, last plane of the last class 1.8e-7 (bound 4.9e-6)
    every voxel ignored  loss -1 exactly, gradient 0"""
import json
import math
import os

import numpy as np
import pytest
import torch

from anatomask_amd import ops, seg_loss as SL
from anatomask_amd.data import deep_supervision_targets
from tests import seg_loss_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("seg_loss_tiny.npz", "seg_loss_tiny_k105.npz", "seg_loss_tiny_ds.npz")
EPS = 2.0 ** -23


def load_cases():
    out = {}
    for f in FILES:
        z = np.load(os.path.join(GOLD, f))
        for name, c in json.loads(str(z["cases"])).items():
            out[name] = (c, {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")})
    return out


CASES = load_cases()
SINGLE = sorted(n for n in CASES if n != "ds")


def make_loss(c):
    if c["kind"] == "ce":
        return SL.DC_and_CE_loss({"batch_dice": c["batch_dice"], "smooth": 1e-5, "do_bg": False, "ddp": False}, {}, weight_ce=c["weight_ce"],
                                 weight_dice=c["weight_dice"], ignore_label=c["ignore_label"], dice_class=SL.MemoryEfficientSoftDiceLoss)
    return SL.DC_and_BCE_loss({}, {"batch_dice": c["batch_dice"], "do_bg": True, "smooth": 1e-5, "ddp": False}, weight_ce=c["weight_ce"],
                              weight_dice=c["weight_dice"], use_ignore_label=c["use_ignore_label"], dice_class=SL.MemoryEfficientSoftDiceLoss)


def oracle_fn(c):
    if c["kind"] == "ce":
        return lambda x, t: O.dice_ce(x, t, c["batch_dice"], False, 1e-5, c["weight_ce"], c["weight_dice"], c["ignore_label"])
    return lambda x, t: O.dice_bce(x, t, c["batch_dice"], True, 1e-5, c["weight_ce"], c["weight_dice"], c["use_ignore_label"])


def CE(batch_dice=True, ignore_label=None, weight_ce=1.0, weight_dice=1.0):
    return dict(kind="ce", batch_dice=batch_dice, ignore_label=ignore_label, weight_ce=weight_ce, weight_dice=weight_dice, use_ignore_label=False)


def BCE(batch_dice=True, use_ignore_label=False):
    return dict(kind="bce", batch_dice=batch_dice, ignore_label=None, weight_ce=1.0, weight_dice=1.0, use_ignore_label=use_ignore_label)


def rel_l2(a, b):
    """relative L2 error of a against b (fp64); the absolute one where b is zero"""
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    d, n = float(torch.linalg.vector_norm(a - b)), float(torch.linalg.vector_norm(b))
    return d / n if n > 0 else d


def check(tag, K, xmax, L, L64, L32s, gs, g64s, g32s):
    """gs / g64s: lists over the logits tensors; L32s, g32s: one entry per fp32 baseline (g32s[j] a list like gs)"""
    L, L64 = float(L), float(L64)
    assert math.isfinite(L), (tag, L)
    lb = max(4 * max(abs(float(v) - L64) for v in L32s), (K + 8) * EPS * (xmax + math.log(K) + 1))
    print(f"[{tag}] loss {L:+.9f} fp64 {L64:+.12f} |err| {abs(L - L64):.3e} bound {lb:.3e}")
    ok = abs(L - L64) <= lb
    for i, (g, g64) in enumerate(zip(gs, g64s)):
        assert bool(torch.isfinite(torch.as_tensor(g)).all()), (tag, i)
        gb = max(4 * max(rel_l2(b[i], g64) for b in g32s), (K + 8) * EPS)
        e = rel_l2(g, g64)
        print(f"[{tag}] grad[{i}] rel L2 err {e:.3e} bound {gb:.3e} (fp32 baselines {[f'{rel_l2(b[i], g64):.2e}' for b in g32s]})")
        ok = ok and e <= gb
    assert ok, tag


def run(loss_fn, xs, ts):
    """loss and gradients of the HIP path on leaf copies of xs"""
    leaves = [x.detach().clone().requires_grad_(True) for x in xs]
    L = loss_fn(leaves, ts) if len(leaves) > 1 else loss_fn(leaves[0], ts[0])
    assert L.dim() == 0 and L.dtype == torch.float32 and L.is_cuda
    L.backward()
    return L.detach(), [l.grad for l in leaves]


def against_oracle(tag, c, x, t):
    """a shape outside the fixture: truth = the restatement in fp64 on the GPU, baseline = the restatement in fp32 on the GPU"""
    K = x.shape[1]
    L64, g64 = O.loss_and_grads(lambda xx: oracle_fn(c)(xx, t), [x], torch.float64)
    L32, g32 = O.loss_and_grads(lambda xx: oracle_fn(c)(xx, t), [x], torch.float32)
    L, g = run(make_loss(c), [x], [t])
    check(tag, K, float(x.abs().max()), L, L64, [L32], g, g64, [g32])
    return L, g


def randn(*shape, seed=0, scale=3.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


def randint(lo, hi, shape, seed=0):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).to(torch.int16).to(DEV)


# ---------------------------------------------------------------- 1. the fixture's cases
@pytest.mark.parametrize("name", SINGLE)
def test_fixture_case(name):
    c, a = CASES[name]
    x, t = torch.from_numpy(a["x"]).to(DEV), torch.from_numpy(a["t"]).to(DEV)
    L, g = run(make_loss(c), [x], [t])
    check(name, c["K"], float(np.abs(a["x"]).max()), L, a["L64"], [a["L32ref"], a["L32plain"]], g, [torch.from_numpy(a["g64"])],
          [[torch.from_numpy(a["g32ref"])], [torch.from_numpy(a["g32plain"])]])
    if name == "ce_k4_allignored":
        assert float(L) == -1.0 and not bool(g[0].any())      # Dice = smooth / smooth, no CE term, no gradient


# ---------------------------------------------------------------- 2. deep supervision from strided views
def test_deep_supervision_from_views():
    c, a = CASES["ds"]
    target = torch.from_numpy(a["t"]).to(DEV)
    views = deep_supervision_targets(target, c["scales"])
    assert views[0] is target
    for v in views[1:]:
        assert not v.is_contiguous() and v.untyped_storage().data_ptr() == target.untyped_storage().data_ptr()
    xs = [torch.from_numpy(a[f"x_{i}"]).to(DEV) for i in range(5)]
    loss_fn = SL.build_loss(5, batch_dice=True)
    assert np.array_equal(np.asarray(loss_fn.weight_factors), a["weights"])
    L, gs = run(loss_fn, xs, views)
    n = range(5)
    check("ds", c["K"], max(float(np.abs(a[f"x_{i}"]).max()) for i in n), L, a["L64"], [a["L32ref"], a["L32plain"]], gs,
          [torch.from_numpy(a[f"g64_{i}"]) for i in n],
          [[torch.from_numpy(a[f"g32ref_{i}"]) for i in n], [torch.from_numpy(a[f"g32plain_{i}"]) for i in n]])
    assert not bool(gs[4].any())


# ---------------------------------------------------------------- 3. shapes where the kernels can go wrong
def test_single_voxel():
    against_oracle("n1", CE(), randn(2, 3, 1, 1, 1, seed=1), randint(0, 3, (2, 1, 1, 1, 1), seed=2))


def test_many_classes_odd_volume():
    against_oracle("k700", CE(), randn(2, 700, 5, 6, 7, seed=3), randint(0, 700, (2, 1, 5, 6, 7), seed=4))


def test_several_workgroups_and_partial_rows():
    against_oracle("wg420", CE(), randn(2, 5, 40, 48, 56, seed=5), randint(0, 5, (2, 1, 40, 48, 56), seed=6))


def test_three_samples_per_sample_dice():
    against_oracle("b3", CE(batch_dice=False), randn(3, 4, 5, 6, 7, seed=7), randint(0, 4, (3, 1, 5, 6, 7), seed=8))


def test_class_absent_from_target():
    t = randint(0, 3, (2, 1, 5, 6, 7), seed=10)
    t[t == 2] = 3                                             # class 2 never occurs
    assert not bool((t == 2).any())
    against_oracle("absent", CE(batch_dice=False), randn(2, 4, 5, 6, 7, seed=9), t)


def test_regions_strided_target_odd_volume():
    """sigmoid mode at N = 990 (no multiple of 4: the unaligned row path), several tiles, the target a strided view, bool and uint8"""
    x = randn(2, 3, 9, 10, 11, seed=11)
    base = (torch.rand(2, 4, 18, 20, 22, generator=torch.Generator().manual_seed(12)) < 0.4).to(torch.uint8).to(DEV)
    t = base[:, :, 1::2, 1::2, 1::2]
    assert not t.is_contiguous()
    L, g = against_oracle("bce_view", BCE(batch_dice=False, use_ignore_label=True), x, t)
    Lb, gb = run(make_loss(BCE(batch_dice=False, use_ignore_label=True)), [x], [t.bool()])
    assert torch.equal(L, Lb) and torch.equal(g[0], gb[0])


def test_label_outside_the_classes_touches_nothing():
    """a label >= K (or < 0) without an ignore label is in no class (documented deviation: the reference's scatter_ raises).  The kernels
    never index by a label; the gradient is written into the front of a larger buffer whose tail must keep its canary."""
    K, sp = 4, (5, 6, 7)
    x = randn(2, K, *sp, seed=13)
    t = randint(0, K, (2, 1, *sp), seed=14)
    t[0, 0, 0, 0, 0], t[0, 0, 2, 3, 4], t[1, 0, 4, 5, 6], t[1, 0, 1, 1, 1] = K, K + 5, 32767, -3
    c = CE()
    against_oracle("stray", c, x, t)
    L64, g64 = O.loss_and_grads(lambda xx: oracle_fn(c)(xx, t), [x], torch.float64)
    n, pad = x.numel(), 4096
    buf = torch.full((n + pad,), 12345.0, device=DEV)
    sums, lse = ops.seg_loss_sums(ops.SEG_SOFTMAX, x, t)
    coef, loss = ops.seg_loss_coeffs(ops.SEG_SOFTMAX, sums, 5 * 6 * 7, True, False, False, 1e-5, 1.0, 1.0)
    out = ops.seg_loss_grad(ops.SEG_SOFTMAX, x, t, None, lse, coef, torch.ones(1, device=DEV), 1.0, out=buf[:n].view_as(x))
    torch.cuda.synchronize()
    assert bool((buf[n:] == 12345.0).all())
    assert rel_l2(out, g64[0]) <= (K + 8) * EPS and abs(float(loss) - float(L64)) <= (K + 8) * EPS * (float(x.abs().max()) + math.log(K) + 1)


# ---------------------------------------------------------------- 4. range
def test_large_and_shifted_logits():
    t = randint(0, 4, (2, 1, 5, 6, 7), seed=16)
    x = randn(2, 4, 5, 6, 7, seed=15, scale=1.0)
    against_oracle("x100+1000", CE(), 100 * x + 1000, t)
    # softmax is invariant under a shift: x + 1000 (rounded to fp32, which moves each logit by up to 3e-5) is served as precisely as x
    _, g1 = against_oracle("x+1000", CE(), 3 * x + 1000, t)
    _, g0 = run(make_loss(CE()), [(3 * x + 1000) - 1000], [t])             # the same rounded logits, unshifted (the subtraction is exact)
    e = rel_l2(g1[0], g0[0])
    print(f"[shift] shifted vs unshifted kernel gradients: rel L2 {e:.3e}")
    assert e <= 2 * (4 + 8) * EPS
    r = (torch.rand(2, 3, 5, 6, 7, generator=torch.Generator().manual_seed(17)) < 0.5).to(torch.uint8).to(DEV)
    against_oracle("bce_x100", BCE(), 100 * randn(2, 3, 5, 6, 7, seed=18, scale=1.0), r)


# ---------------------------------------------------------------- 5. autograd
def test_scaling_the_loss_scales_the_gradient(monkeypatch):
    x, t = randn(2, 5, 9, 10, 11, seed=19), randint(0, 5, (2, 1, 9, 10, 11), seed=20)
    fn = make_loss(CE())
    _, g1 = run(fn, [x], [t])
    leaf = x.clone().requires_grad_(True)
    (3 * fn(leaf, t)).backward()
    ref = 3 * g1[0]
    assert bool(((leaf.grad - ref).abs() <= EPS * ref.abs()).all())          # 1 ulp
    calls = []
    real = ops.seg_loss_grad
    monkeypatch.setattr(ops, "seg_loss_grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    L0 = fn(x, t)                                             # requires_grad=False: no gradient pass, the same value
    assert not L0.requires_grad and not calls
    leaf = x.clone().requires_grad_(True)
    L1 = fn(leaf, t)
    assert not calls and torch.equal(L0, L1.detach())
    L1.backward()
    assert len(calls) == 1 and torch.equal(leaf.grad, g1[0])


# ---------------------------------------------------------------- 6. determinism
def test_two_runs_give_the_same_bits():
    x, t = randn(2, 5, 40, 48, 56, seed=21), randint(0, 6, (2, 1, 40, 48, 56), seed=22)
    fn = make_loss(CE(ignore_label=5))
    (La, ga), (Lb, gb) = run(fn, [x], [t]), run(fn, [x], [t])
    assert torch.equal(La, Lb) and torch.equal(ga[0], gb[0])
    x = randn(2, 3, 17, 18, 19, seed=23)
    r = (torch.rand(2, 4, 17, 18, 19, generator=torch.Generator().manual_seed(24)) < 0.4).to(torch.uint8).to(DEV)
    fn = make_loss(BCE(use_ignore_label=True))
    (La, ga), (Lb, gb) = run(fn, [x], [r]), run(fn, [x], [r])
    assert torch.equal(La, Lb) and torch.equal(ga[0], gb[0])


# ---------------------------------------------------------------- 7. beyond 2^31 elements, closed form
def test_beyond_2_31_elements_closed_form():
    """B = 1, K = 33, 256 x 512 x 512: 2.2e9 logits.  x[k] = c_k everywhere and target(v) = v mod 33, so the loss and the gradient of every
    (class, label) pair are 33 x 33 numbers, evaluated here in fp64 from the formulas.  A size test: every access is in bounds."""
    K, sp = 33, (256, 512, 512)
    N = sp[0] * sp[1] * sp[2]
    c = np.linspace(-2.0, 2.0, K).astype(np.float32)
    c64 = c.astype(np.float64)
    lse = np.log(np.exp(c64 - c64.max()).sum()) + c64.max()
    p = np.exp(c64 - lse)
    cnt = np.array([N // K + (1 if j < N % K else 0) for j in range(K)], np.float64)
    smooth, Cp = 1e-5, K - 1
    num, den = 2 * p * cnt + smooth, cnt + p * N + smooth
    dice = -(num[1:] / den[1:]).mean()
    ce = float((cnt * (lse - c64)).sum() / N)
    L64 = ce + dice
    a_c, b_c = -2 / (Cp * den), num / (Cp * den ** 2)
    a_c[0] = b_c[0] = 0.0
    T = a_c * p + (b_c * p).sum()                            # sum_j p_j g_j for a voxel of label j
    eye = np.eye(K)
    E = p[:, None] * ((a_c[:, None] * eye + b_c[:, None]) - T[None, :]) + (p[:, None] - eye) / N      # E[k, label]

    x = torch.empty(1, K, *sp, device=DEV)
    x.view(K, N).copy_(torch.from_numpy(c).to(DEV)[:, None].expand(K, N))
    lab = torch.arange(N, device=DEV) % K
    t = lab.to(torch.int16).view(1, 1, *sp)
    x.requires_grad_(True)
    L = make_loss(CE())(x, t)
    L.backward()
    L, g = L.detach(), x.grad.view(K, N)
    Ed = torch.from_numpy(E).to(DEV)
    err2 = torch.zeros((), dtype=torch.float64, device=DEV)
    ref2 = torch.zeros((), dtype=torch.float64, device=DEV)
    for k in range(K):
        want = torch.where(lab == k, Ed[k, k], Ed[k][lab])
        err2 += (g[k].double() - want).square().sum()
        ref2 += want.square().sum()
    e = float((err2 / ref2).sqrt())
    plane = sp[1] * sp[2]
    last_want = Ed[K - 1][lab[-plane:]]
    e_last = float(torch.linalg.vector_norm(g[K - 1, -plane:].double() - last_want) / torch.linalg.vector_norm(last_want))
    lb, gb = (K + 8) * EPS * (2.0 + math.log(K) + 1), (K + 8) * EPS
    print(f"[2^31] loss {float(L):+.9f} fp64 {L64:+.12f} |err| {abs(float(L) - L64):.3e} bound {lb:.3e}; grad rel L2 {e:.3e}, "
          f"last plane of the last class {e_last:.3e}, bound {gb:.3e}")
    assert x.numel() > 2 ** 31 and abs(float(L) - L64) <= lb and e <= gb and e_last <= gb
