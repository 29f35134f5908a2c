"""GPU: the kernels of anatomask_amd/csrc/step_ops.hip, one by one, against the plain fp64 references of tests/step_oracle.py, per element or
per patch, at their edges: sizes on both sides of every block cap, tails, sub-ranges inside larger buffers, NULL arguments, the hipGraph
scalar path, the non-finite guard, ties in the sampler, ill-conditioned patches.  tests/test_step_ops_cpu.py pins the reference side and
shows that each bound below is reachable by a correct fp32 implementation and not by a wrong one.  u = 2^-24.

Bounds (none comes from the code under test):
  am_ema_i64        bit-equal to torch's `(e * decay + (1.0 - decay) * p).to(int64)` on the CPU
  am_sumsq          relative 4u against the fp64 sum of squares (non-negative terms, each pair rounded twice in fp32, fp64 accumulation)
  am_adamw_ema      K u S per element against adamw_ema_step_ref, K = the fp32 roundings on the way to the output (step_oracle.adamw_K:
                    m 4, v 6, p 14, ema 17; 8 / 14 / 22 / 25 when the clip is active), S the magnitude of the terms; gnorm 2u.
                    Against torch (clip_grad_norm_ + AdamW + timm's EMA on fp32 CPU tensors): K u S + the scalar-rounding term
                    2^-24 b / (1 - b) x the term the complement 1 - b multiplies (step_oracle.adamw_scalar_terms)
  am_ema            3u (|ema| + |p|) against fp64 with (float)decay
  patch loss        per patch K u (l2 + 2 sqrt(l2) kappa + kappa^2 u), kappa = |mean| rstd; mean, rstd, drec, loss likewise
                    (step_oracle.patch_loss_bounds; K = 4 x the worst ratio of two fp32 emulations, measured on the CPU)
  am_mask_sampler   bit-equal to mask_sampler_ref (ties by patch id).  NaN losses and NaN keys are out of scope: the kernel's order-preserving
                    map puts them at either end by their sign bit, torch's argsort at the upper end.

Measured on an MI355X, worst error / bound (every test prints its figures):
  am_sumsq 0.12 (of 4u);  am_ema 0.64 (of 3u (|ema| + |p|));  am_ema_i64 and am_mask_sampler bit-equal in every case
  am_adamw_ema against adamw_ema_step_ref, 24 regime x size cases, chained steps, sub-range, NULL arguments:  m 0.24, v 0.48, p 0.29, ema 0.08
               against torch, three steps:  m 0.15, v 0.24, p 0.18, ema 0.10;  gnorm within 2u everywhere
  patch loss   l2 0.31, mean 0.25, rstd 0.22, drec 0.24, loss 0.22, inv_count 0.38 (of 2u); the teacher pass 0.10
  (the CPU emulations of tests/test_step_ops_cpu.py sit at 0.25 of the patch-loss bounds by construction and at <= 0.4 of the AdamW ones:
  the kernels are no further from fp64 than a plain fp32 evaluation is)"""
import math

import numpy as np
import pytest
import torch

from anatomask_amd import hip, ops
from tests import step_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = S.U
CANARY = -12345.678


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(t):
    """a host copy to compare bit for bit (NaN payloads and signed zeros included)"""
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.uint8).clone()


def rejects(fn, *args):
    with pytest.raises(RuntimeError, match="failed with code -1"):
        fn(*args)


# ------------------------------------------------------------------ am_ema_i64
@pytest.mark.parametrize("decay", S.EMA_DECAYS)
def test_ema_i64_is_timm_on_torch_cpu(decay):
    """fails at 0.9999 with a product fused into the sum (846 of the 4096 `ema = p` cases, tests/test_step_ops_cpu.py)"""
    for name, (e, p) in S.ema_i64_inputs().items():
        want = S.ema_i64_ref(torch.from_numpy(e), torch.from_numpy(p), decay)
        ed, pd = dev(e), dev(p)
        ops.ema_i64(ed, pd, decay)
        got = host(ed)
        bad = np.flatnonzero(got != want.numpy())
        assert bad.size == 0, f"{name} at {decay}: {bad.size} differ, first e = {e[bad[0]]}, p = {p[bad[0]]}: {got[bad[0]]} != {int(want[bad[0]])}"
        assert np.array_equal(host(pd), p)


def test_ema_i64_edges():
    e = np.arange(1000, 1300, dtype=np.int64)
    p = e + 20000                                                                                 # the update moves every counter by about 2
    want = S.ema_i64_ref(torch.from_numpy(e), torch.from_numpy(p), 0.9999).numpy()
    ed, pd = dev(e), dev(p)
    hip.lib().ema_i64(ed.data_ptr(), pd.data_ptr(), 0, 0.9999, None, stream())                   # n = 0 returns 0
    assert np.array_equal(host(ed), e)
    hip.lib().ema_i64(ed.data_ptr(), pd.data_ptr(), 257, 0.9999, None, stream())                 # the second block and its bound check
    got = host(ed)
    assert np.array_equal(got[:257], want[:257]) and np.array_equal(got[257:], e[257:]) and not np.array_equal(want[257:], e[257:])
    ed = dev(e)
    guard = torch.tensor([1, 5, 9, 0], dtype=torch.int32, device=DEV)
    ops.ema_i64(ed, pd, 0.9999, guard)                                                            # latched: untouched
    assert np.array_equal(host(ed), e) and guard.tolist() == [1, 5, 9, 0]
    guard.zero_()
    ops.ema_i64(ed, pd, 0.9999, guard)
    assert np.array_equal(host(ed), want)


# ------------------------------------------------------------------ am_sumsq
SUMSQ_N = (1, 2, 3, 4, 5, 1023, 1024 * 256 * 4 - 1, 2048 * 256 * 4 + 4 * 300 + 3)           # the last: past the block cap, with a tail


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_sumsq(scale):
    rng = np.random.default_rng(11)
    g = rng.standard_normal(SUMSQ_N[-1] + 8).astype(np.float32)
    g[rng.random(g.size) < 0.1] = 0
    g[4] = 0                                                                                     # n = 1 at offset 4: an exact zero sum
    g = (g * np.float32(scale)).astype(np.float32)
    gd = dev(g)
    out = torch.full((2,), 7.0, device=DEV, dtype=torch.float64)
    worst = 0.0
    for n in SUMSQ_N:
        for a in (0, 4):                                                                         # g[4 : 4 + n]: a 16-byte-aligned sub-range
            want = float(np.sum(g[a:a + n].astype(np.float64) ** 2))
            ops.sumsq(gd[a:a + n], out)
            got = out[0].item()
            ops.sumsq(gd[a:a + n], out)                                                          # the memset: a second call does not accumulate
            again = out[0].item()                                                                # (the blocks' atomic adds come in any order: not bit-equal)
            assert out[1].item() == 7.0
            worst = max(worst, max(abs(got - want), abs(again - want)) / (4 * U * want) if want > 0 else 0.0)
            assert abs(got - want) <= 4 * U * want and abs(again - want) <= 4 * U * want, (n, a, got, again, want)
    print(f"[sumsq x{scale:g}] worst error / (4u sum) {worst:.3f}")


# ------------------------------------------------------------------ am_adamw_ema
ADAMW_N = (4, 1024, 4 * 50000, 4 * (4096 * 256) + 4 * 1000)                                      # the last: past the block cap


def call_adamw(p, g, m, v, ema, n, kw, ss=None, gn=None, dyn=None, guard=None):
    hip.lib().adamw_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(ema), n, kw["lr"], kw["betas"][0], kw["betas"][1], kw["eps"],
                        kw["wd"], kw["step"], ptr(ss), kw["max_norm"], kw["ema_decay"], kw["grad_scale"], ptr(gn), ptr(dyn), ptr(guard), stream())


def draw(name, n, seed=0):
    p, g, m, v, e, kw, _ = S.adamw_draw(name, n, seed)
    return p, g, m, v, e, dict(kw)


def check_adamw(tag, got, r, extra=None, sl=slice(None)):
    """got: name -> host fp32 array; r: adamw_ema_step_ref's result; extra: name -> a term added to K u S"""
    K = S.adamw_K(r["k_coef"])
    ratios = {}
    for o in got:
        b = K[o] * U * r["S_" + o][sl] + (0.0 if extra is None else extra[o][sl])
        ratios[o] = S.worst_ratio(got[o][sl], r[o][sl], b)
    print(f"[{tag}] clip {'on' if r['clipped'] else 'off'}, K {K}: error / bound", {k: f"{x:.3f}" for k, x in ratios.items()})
    for o, x in ratios.items():
        assert x <= 1.0, (tag, o, x)
    return ratios


@pytest.mark.parametrize("n", ADAMW_N)
@pytest.mark.parametrize("name", sorted(S.ADAMW_REGIMES))
def test_adamw_ema_one_step(name, n):
    p, g, m, v, e, kw = draw(name, n)
    pd, gd, md, vd, ed = (dev(t) for t in (p, g, m, v, e))
    ss = torch.zeros(1, device=DEV, dtype=torch.float64)
    gn = torch.full((1,), 7.0, device=DEV)
    ops.sumsq(gd, ss)
    call_adamw(pd, gd, md, vd, ed, n, kw, ss, gn)
    r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=ss.item(), **kw)                               # the one-step contract: the kernel's own sumsq
    got = dict(p=host(pd), m=host(md), v=host(vd), ema=host(ed))
    check_adamw(f"{name} n={n}", got, r)
    assert np.array_equal(host(gd), g)
    assert abs(gn.item() - r["gnorm"]) <= 2 * U * r["gnorm"], (gn.item(), r["gnorm"])
    if n > 64:                                                                                   # the end of the buffer, explicitly
        check_adamw(f"{name} n={n} last 64", got, r, sl=slice(n - 64, n))
        assert (got["p"][-64:] != p[-64:]).any() and (got["ema"][-64:] != e[-64:]).any()


def test_adamw_ema_three_chained_steps():
    """reference of step k from the device's own state after step k - 1: the bounds do not compound"""
    n = 4 * 50000
    p, g, m, v, e, kw = draw("clip_step1", n)
    pd, gd, md, vd, ed = (dev(t) for t in (p, g, m, v, e))
    ss = torch.zeros(1, device=DEV, dtype=torch.float64)
    for step in (1, 2, 3):
        kw["step"] = step
        gs = (g * np.float32(0.01 ** (step - 1))).astype(np.float32)                              # norms 850, 8.5, 0.085: step 1 clips, 2 and 3 do not
        gd.copy_(dev(gs))
        before = [host(t).copy() for t in (pd, md, vd, ed)]
        ops.sumsq(gd, ss)
        call_adamw(pd, gd, md, vd, ed, n, kw, ss)
        r = S.adamw_ema_step_ref(before[0], gs, before[1], before[2], before[3], sumsq=ss.item(), **kw)
        assert bool(r["clipped"]) == (step == 1)
        check_adamw(f"chained step {step}", dict(p=host(pd), m=host(md), v=host(vd), ema=host(ed)), r)


def test_adamw_ema_against_torch():
    """m and v (both checkpointed), p and ema against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW + timm's EMA on fp32 CPU tensors,
    three steps from zero state, each torch step started from the device's state before it.  Bound per element:
        K u S + c(b) |T|,   c(b) = 2^-24 b / (1 - b) + 2^-24,
    T the term the complement multiplies: (gk - m)(1 - b1) for m, (1 - b2) gk^2 for v, both carried through m' / denom (and 2u on
    lr / bc1) for p, (1 - d) p' plus (1 - d) x p's term for ema  (step_oracle.adamw_scalar_terms)."""
    n = 4 * 50000
    rng = np.random.default_rng(5)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.5).astype(np.float32)
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-5, step=1, ema_decay=0.9999, max_norm=12.0, grad_scale=1.0)
    pd, md, vd, ed = dev(p), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), dev(p)
    ss = torch.zeros(1, device=DEV, dtype=torch.float64)
    gn = torch.zeros(1, device=DEV)
    for step in (1, 2, 3):
        kw["step"] = step
        gs = (g * np.float32(0.05 * step ** 3)).astype(np.float32)                                # norms 11, 89, 302: clip off, on, on
        gd = dev(gs)
        before = [host(t).copy() for t in (pd, md, vd, ed)]
        ops.sumsq(gd, ss)
        call_adamw(pd, gd, md, vd, ed, n, kw, ss, gn)
        r = S.adamw_ema_step_ref(before[0], gs, before[1], before[2], before[3], sumsq=ss.item(), **kw)
        tp, tm, tv, te, tt = S.adamw_torch_ref(before[0], gs, before[1], before[2], before[3], **kw)
        assert bool(r["clipped"]) == (step > 1)
        rt = dict(r, p=tp.numpy(), m=tm.numpy(), v=tv.numpy(), ema=te.numpy())
        check_adamw(f"torch step {step}", dict(p=host(pd), m=host(md), v=host(vd), ema=host(ed)), rt, extra=S.adamw_scalar_terms(r, kw["betas"], kw["ema_decay"]))
        assert abs(gn.item() - float(tt)) <= (2 + math.log2(n)) * U * float(tt)                   # torch's norm is an fp32 sum of n terms


def test_adamw_ema_null_arguments_and_dyn():
    n = 4 * 3000
    p, g, m, v, e, kw = draw("ranks2_step1000", n)
    gd = dev(g)
    ss = torch.zeros(1, device=DEV, dtype=torch.float64)
    ops.sumsq(gd, ss)

    def run(ema=True, sumsq=True, dyn=None, kwc=kw):
        t = [dev(x) for x in (p, m, v, e)]
        gn = torch.full((1,), 7.0, device=DEV)
        call_adamw(t[0], gd, t[1], t[2], t[3] if ema else None, n, kwc, ss if sumsq else None, gn, dyn)
        return [bits(x) for x in t], gn.item()

    base, gn = run()
    r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=ss.item(), **kw)
    assert r["clipped"] and abs(gn - r["gnorm"]) <= 2 * U * r["gnorm"]
    # ema = NULL: the same p, m, v bits, the EMA buffer untouched
    noema, _ = run(ema=False)
    assert all(torch.equal(a, b) for a, b in zip(noema[:3], base[:3])) and torch.equal(noema[3], bits(dev(e)))
    # sumsq = NULL: no clip, gnorm_out = 0
    t = [dev(x) for x in (p, m, v, e)]
    gn0 = torch.full((1,), 7.0, device=DEV)
    call_adamw(t[0], gd, t[1], t[2], t[3], n, kw, None, gn0)
    r0 = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=None, **kw)
    assert gn0.item() == 0.0 and not r0["clipped"]
    check_adamw("sumsq NULL", dict(p=host(t[0]), m=host(t[1]), v=host(t[2]), ema=host(t[3])), r0)
    # dyn (the hipGraph path): lr, bc1, sqrt(bc2), decay come from device memory; the by-value ones are then ignored
    dyn = torch.tensor(ops.adam_dyn_scalars(kw["lr"], kw["betas"], kw["step"], kw["ema_decay"]), dtype=torch.float32).to(DEV)
    viadyn, gnd = run(dyn=dyn, kwc=dict(kw, lr=0.5, step=7, ema_decay=0.5))
    assert all(torch.equal(a, b) for a, b in zip(viadyn, base)) and gnd == gn


def test_adamw_ema_sub_range_and_rejected_n():
    N, a, n = 4 * 700, 4 * 37, 4 * 300
    full = [np.full(N, CANARY + i, np.float32) for i in range(5)]                                # p, g, m, v, ema: canaries outside [a, a + n)
    p, g, m, v, e, kw = draw("noclip_step3", n)
    for buf, x in zip(full, (p, g, m, v, e)):
        buf[a:a + n] = x
    t = [dev(x) for x in full]
    ss = torch.zeros(1, device=DEV, dtype=torch.float64)
    ops.sumsq(t[1][a:a + n], ss)
    # n % 4 != 0 is rejected and changes nothing
    rejects(call_adamw, t[0][a:], t[1][a:], t[2][a:], t[3][a:], t[4][a:], n - 1, kw, ss)
    assert all(np.array_equal(host(x), y) for x, y in zip(t, full))
    call_adamw(t[0][a:], t[1][a:], t[2][a:], t[3][a:], t[4][a:], n, kw, ss)
    got = [host(x) for x in t]
    for x, y in zip(got, full):
        assert np.array_equal(x[:a], y[:a]) and np.array_equal(x[a + n:], y[a + n:])
    assert np.array_equal(got[1], full[1])
    r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=ss.item(), **kw)
    check_adamw("sub-range", dict(p=got[0][a:a + n], m=got[2][a:a + n], v=got[3][a:a + n], ema=got[4][a:a + n]), r)


# ------------------------------------------------------------------ the non-finite guard
@pytest.mark.parametrize("badval", [float("nan"), float("inf")])
def test_guard_latches_on_a_non_finite_norm(badval):
    """non-finite VALUES as data; nothing here faults"""
    n, c = 4 * 500, 41
    p, g, m, v, e, kw = draw("noclip_step3", n)
    t = [dev(x) for x in (p, g, m, v, e)]
    start = [bits(x) for x in t]
    guard = torch.tensor([0, 0, c, 0], dtype=torch.int32, device=DEV)
    bad = torch.tensor([badval], dtype=torch.float64, device=DEV)
    good = torch.zeros(1, device=DEV, dtype=torch.float64)
    ops.sumsq(t[1], good)
    gn = torch.zeros(1, device=DEV)
    go = lambda ss, gd: call_adamw(t[0], t[1], t[2], t[3], t[4], n, kw, ss, gn, None, gd)
    go(bad, guard)
    assert guard.tolist() == [1, c + 1, c + 1, 0] and not math.isfinite(gn.item())
    assert all(torch.equal(bits(x), y) for x, y in zip(t, start))
    go(good, guard)                                                                              # latched: a finite call is skipped, only the count advances
    assert guard.tolist() == [1, c + 1, c + 2, 0] and math.isfinite(gn.item())
    assert all(torch.equal(bits(x), y) for x, y in zip(t, start))
    guard.zero_()
    go(good, guard)                                                                              # cleared: the next call updates
    assert guard.tolist() == [0, 0, 1, 0]
    r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=good.item(), **kw)
    check_adamw("after clearing the guard", dict(p=host(t[0]), m=host(t[2]), v=host(t[3]), ema=host(t[4])), r)
    # guard = NULL: the unguarded path does update, with the non-finite norm
    t2 = [dev(x) for x in (p, g, m, v, e)]
    call_adamw(t2[0], t2[1], t2[2], t2[3], t2[4], n, kw, bad, gn, None, None)
    assert not math.isfinite(gn.item()) and not torch.equal(bits(t2[0]), start[0]) and not torch.equal(bits(t2[2]), start[2])


# ------------------------------------------------------------------ am_ema
@pytest.mark.parametrize("decay", [0.5, 0.999, 0.9999])
def test_ema(decay):
    rng = np.random.default_rng(21)
    worst = 0.0
    for n in (1, 3, 255, 4096 * 256 + 5):                                                        # the last: past the block cap, odd
        e, p = rng.standard_normal(n + 3).astype(np.float32), rng.standard_normal(n + 3).astype(np.float32)
        ed, pd = dev(e), dev(p)
        ops.ema(ed[:n], pd[:n], decay)
        d = S.f32(decay)
        want = e[:n].astype(np.float64) * d + (1.0 - d) * p[:n].astype(np.float64)
        got = host(ed)
        worst = max(worst, S.worst_ratio(got[:n], want, 3 * U * (np.abs(e[:n]) + np.abs(p[:n])).astype(np.float64)))
        assert np.array_equal(got[n:], e[n:]) and np.array_equal(host(pd), p)
        guard = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=DEV)
        ed2 = dev(e)
        ops.ema(ed2[:n], pd[:n], decay, guard)                                                   # latched: skipped
        assert np.array_equal(host(ed2), e)
    print(f"[ema {decay}] worst error / (3u (|ema| + |p|)) {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ am_guard_restore
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
def test_guard_restore(dtype):
    g = torch.Generator().manual_seed(31)
    for nbytes in (4, 8 * 3, 1024 * 256 * 4 + 8):                                                # the last: past the block cap
        numel = (nbytes + 7) // 8 * (8 // torch.empty(0, dtype=dtype).element_size()) + 4        # whole elements, and a tail that must stay
        mk = lambda: (torch.randn(numel, generator=g) * 1000).to(dtype).to(DEV)
        dst, snap = mk(), mk()
        d0, s0 = bits(dst), bits(snap)
        assert not torch.equal(d0[:nbytes], s0[:nbytes])
        guard = torch.zeros(4, dtype=torch.int32, device=DEV)
        call = lambda nb, gd: hip.lib().guard_restore(dst.data_ptr(), snap.data_ptr(), nb, ptr(gd), stream())
        call(nbytes, guard)                                                                      # not latched: untouched
        assert torch.equal(bits(dst), d0) and torch.equal(bits(snap), s0)
        guard[0] = 1
        call(0, guard)                                                                           # nbytes = 0 returns 0
        assert torch.equal(bits(dst), d0)
        rejects(call, nbytes + 2, guard)
        rejects(call, nbytes, None)
        assert torch.equal(bits(dst), d0)
        call(nbytes, guard)                                                                      # latched: the snapshot comes back
        d1 = bits(dst)
        assert torch.equal(d1[:nbytes], s0[:nbytes]) and torch.equal(d1[nbytes:], d0[nbytes:]) and torch.equal(bits(snap), s0)
    a, b = torch.arange(6, dtype=dtype, device=DEV), torch.arange(6, dtype=dtype, device=DEV) + 10
    ops.guard_restore(a, b, torch.ones(4, dtype=torch.int32, device=DEV))
    assert torch.equal(a, b)


# ------------------------------------------------------------------ patch loss
def call_patch_fwd(inp, rec, vis_u8, geo, normalized, want_loss=True):
    B, D, H, W = geo
    n = vis_u8.numel()
    l2m, pm, pr = (torch.full((n + 1,), CANARY, device=DEV) for _ in range(3))
    info = torch.full((3,), CANARY, device=DEV)
    hip.lib().patch_loss_fwd(inp.data_ptr(), rec.data_ptr(), vis_u8.data_ptr(), B, D, H, W, int(normalized), l2m.data_ptr(),
                             pm.data_ptr() if want_loss else None, pr.data_ptr() if want_loss else None, info.data_ptr() if want_loss else None, stream())
    return l2m, pm, pr, info


def call_patch_bwd(inp, rec, vis_u8, geo, pm, pr, info, gout):
    B, D, H, W = geo
    drec = torch.full((inp.numel() + 4096,), CANARY, device=DEV)                                 # one extra patch behind the tensor: a canary
    g = None if gout is None else torch.tensor([gout], device=DEV)
    hip.lib().patch_loss_bwd(inp.data_ptr(), rec.data_ptr(), vis_u8.data_ptr(), B, D, H, W, pm.data_ptr(), pr.data_ptr(), info.data_ptr(), ptr(g),
                             drec.data_ptr(), stream())
    return drec


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("geo", S.PATCH_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_patch_loss(geo, normalized):
    """(3, 16, 16, 16) is the layout SparK's loss uses: B * L one-patch samples.  The constant and the high-offset patches are masked ones."""
    B, D, H, W = geo
    f = (D // 16, H // 16, W // 16)
    worst = {}
    for mask_name, vis in S.patch_masks(B, *f).items():
        inp, rec, fam = S.patch_families(B, *f, vis)
        if not vis.all() and (~vis).sum() >= 4:
            assert set(fam[~vis.reshape(B, -1)].tolist()) >= {0, 1, 2, 3}
        ind, recd, visd = dev(inp), dev(rec), dev(vis.astype(np.uint8))
        n = vis.size
        l2m, pm, pr, info = call_patch_fwd(ind, recd, visd, geo, normalized)
        ref = S.patch_loss_ref(inp, rec, vis, normalized)
        b = S.patch_loss_bounds(ref)
        got = dict(l2m=host(l2m), mean=host(pm), rstd=host(pr), info=host(info))
        assert got["l2m"][n] == np.float32(CANARY) and got["mean"][n] == np.float32(CANARY) and got["rstd"][n] == np.float32(CANARY)
        assert got["info"][2] == np.float32(CANARY)
        l2g = got["l2m"][:n].reshape(B, -1)
        assert (l2g[ref["vis"]] == 0).all()
        rat = dict(l2=S.worst_ratio(l2g, ref["l2m"], b["l2"]), loss=S.worst_ratio(got["info"][0], ref["loss"], b["loss"]),
                   inv_count=S.worst_ratio(got["info"][1], ref["inv_count"], b["inv_count"]))
        if normalized:
            rat["mean"] = S.worst_ratio(got["mean"][:n].reshape(B, -1), ref["mean"], b["mean"])
            rat["rstd"] = S.worst_ratio(got["rstd"][:n].reshape(B, -1), ref["rstd"], b["rstd"])
        else:
            assert (got["mean"][:n] == 0).all() and (got["rstd"][:n] == 1).all()
        if mask_name == "all_visible":
            assert got["info"][0] == 0.0 and got["info"][1] == np.float32(1e8)
        for gout in (None, 0.25, -3.0):
            drec = host(call_patch_bwd(ind, recd, visd, geo, pm, pr, info, gout))
            assert (drec[inp.size:] == np.float32(CANARY)).all()
            dp = S.patches(drec[:inp.size].reshape(geo), *f)
            assert np.isfinite(dp).all() and (dp[ref["vis"]] == 0).all()
            refg = ref if gout is None else S.patch_loss_ref(inp, rec, vis, normalized, gout)
            bg = b if gout is None else S.patch_loss_bounds(refg)
            rat[f"drec gout={gout}"] = S.worst_ratio(np.abs(dp - refg["drec_p"]).max(-1), 0.0, bg["drec"])
        for k, x in rat.items():
            worst[k] = max(worst.get(k, 0.0), x)
            assert x <= 1.0, (geo, mask_name, k, x)
    print(f"[patch loss {geo} normalized={normalized}] worst error / bound", {k: f"{x:.3f}" for k, x in worst.items()})


def test_patch_loss_non_finite_loss_gives_nan_gradients():
    """a rec holding +inf in one masked patch: the loss is non-finite, so the gradient is NaN on every masked patch (it must reach the
    optimizer's guard on every rank) and exactly 0 on the visible ones"""
    geo = (2, 32, 48, 32)
    f = (2, 3, 2)
    vis = S.patch_masks(2, *f)["random"]
    inp, rec, _ = S.patch_families(2, *f, vis)
    rp = S.patches(rec, *f).copy()
    rp[1, np.flatnonzero(~vis[1].reshape(-1))[0], 77] = np.inf
    rec = S.unpatches(rp, *f)
    ind, recd, visd = dev(inp), dev(rec), dev(vis.astype(np.uint8))
    l2m, pm, pr, info = call_patch_fwd(ind, recd, visd, geo, True)
    assert not math.isfinite(info[0].item())
    dp = S.patches(host(call_patch_bwd(ind, recd, visd, geo, pm, pr, info, 0.25))[:inp.size].reshape(geo), *f)
    v = vis.reshape(2, -1)
    assert np.isnan(dp[~v]).all() and (dp[v] == 0).all()


def test_patch_loss_teacher_pass_never_reads_visible_patches():
    """want_loss = False (pmean / prstd / lossinfo NULL) at (1, 16, 32, 64): NaN-filled visible patches do not leak"""
    geo = (1, 16, 32, 64)
    f = (1, 2, 4)
    vis = S.patch_masks(1, *f)["random"]
    assert vis.any() and not vis.all()
    inp, rec, _ = S.patch_families(1, *f, vis)
    ref = S.patch_loss_ref(inp, rec, vis, False)
    rp = S.patches(rec, *f).copy()
    rp[vis.reshape(1, -1)] = np.nan
    l2m, _, _, _ = call_patch_fwd(dev(inp), dev(S.unpatches(rp, *f)), dev(vis.astype(np.uint8)), geo, False, want_loss=False)
    got = host(l2m)
    assert got[vis.size] == np.float32(CANARY)
    r = S.worst_ratio(got[:vis.size].reshape(1, -1), ref["l2m"], S.patch_loss_bounds(ref)["l2"])
    print(f"[teacher pass] error / bound {r:.3f}")
    assert r <= 1.0 and (got[:vis.size].reshape(1, -1)[ref["vis"]] == 0).all()


def test_patch_loss_rejects_ragged_sizes():
    for geo in ((1, 24, 16, 16), (1, 16, 40, 16), (1, 16, 16, 17)):
        x = torch.zeros(geo, device=DEV)
        vis = torch.zeros(8, dtype=torch.uint8, device=DEV)
        buf = torch.zeros(8, device=DEV)
        rejects(hip.lib().patch_loss_fwd, x.data_ptr(), x.data_ptr(), vis.data_ptr(), *geo, 1, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), stream())
        rejects(hip.lib().patch_loss_bwd, x.data_ptr(), x.data_ptr(), vis.data_ptr(), *geo, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, x.data_ptr(), stream())


# ------------------------------------------------------------------ am_mask_sampler
def call_sampler(loss, keys, B, L, keep, ll, out):
    hip.lib().mask_sampler(loss.data_ptr(), keys.data_ptr(), B, L, keep, ll, out.data_ptr(), stream())


@pytest.mark.parametrize("L", [1, 2, 27, 256, 257, 512, 513, 1728, 4095, 4096])
def test_mask_sampler(L):
    """a power of two has no padding keys, one above it has half the sort padded; 4096 is the ABI's limit (a 256^3 input)"""
    B = 3
    keep = max(1, round(0.4 * L))
    for name, (loss, keys) in S.sampler_draws(B, L).items():
        ld, kd = loss.to(DEV), keys.to(DEV)
        for ll in sorted({x for x in (0, 1, (L - keep) // 2, L - keep) if 0 <= x <= L - keep}):
            out = torch.full((B + 1, L), 0xAB, dtype=torch.uint8, device=DEV)                    # row B: a canary
            call_sampler(ld, kd, B, L, keep, ll, out)
            got = out.cpu()
            want = S.mask_sampler_ref(loss, keys, keep, ll)
            assert (got[B] == 0xAB).all(), (name, L, ll)
            assert torch.equal(got[:B].bool(), want) and int(got[:B].max()) <= 1, (name, L, ll)
            assert (got[:B].sum(1) == keep).all()
            if ll:
                hard = torch.argsort(loss, dim=1, stable=True)[:, L - ll:]
                assert not got[:B].bool().gather(1, hard).any()


def test_mask_sampler_rejects_bad_arguments():
    x = torch.zeros(2, 4097, device=DEV)
    out = torch.zeros(2, 4097, dtype=torch.uint8, device=DEV)
    rejects(call_sampler, x, x, 2, 4097, 100, 0, out)
    rejects(call_sampler, x, x, 2, 100, 101, 0, out)
    rejects(call_sampler, x, x, 2, 100, 40, 61, out)
    rejects(call_sampler, x, x, 2, 100, 40, -1, out)
    assert not out.any()
