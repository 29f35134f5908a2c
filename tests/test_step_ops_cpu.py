"""CPU: the reference side of the step-kernel tests (tests/step_oracle.py).  Nothing here touches the HIP library: these tests show that
each bound tests/test_step_ops_gpu.py asserts is reachable by a correct fp32 implementation (a numpy emulation of the kernel's sequence
with one rounding per operation) and is NOT reachable by a wrong one, and that the int64 inputs tell a fused product from a rounded one.

Measured here (u = 2^-24; every test prints its figures):
  int64 EMA   torch == the three-rounding emulation on all inputs at 0.999 / 0.9999 / 0.99945; the contracted form differs from it in
              846 of the 4096 `ema = p` cases at 0.9999 and in none at the other two decays
  AdamW       emulation against adamw_ema_step_ref, worst error / (u S) over the six regimes: m 0.94, v 4.9, p 2.9, ema 1.5 (the asserted
              K: 4 / 6 / 14 / 17 without the clip, 8 / 14 / 22 / 25 with it); against adamw_torch_ref at most 0.36 of K u S + the scalar
              term; each of the six wrong variants leaves K u S in at least one regime by a factor >= 68
  patch loss  worst error / (u S) of the kernel-order / the np.sum emulation over the five geometries, three masks, five input families:
              l2 2.37 / 2.22, mean 3.92 / 3.92, rstd 2.16 / 1.51, drec 2.67 / 2.67, loss 0.79 / 0.36 -> K = 10 / 16 / 9 / 11 / 4
              (4 x the larger, rounded up); relative l2 error 0.8u .. 3u at kappa = 0.2 .. 100 and 275u on the constant patch (kappa 1020);
              the five wrong variants leave the bounds by a factor >= 381"""
import numpy as np
import pytest
import torch

from oracle import anatomask_oracle as O
from tests import step_oracle as S

U = S.U


# ------------------------------------------------------------------ int64 EMA
@pytest.mark.parametrize("decay", S.EMA_DECAYS)
def test_ema_i64_ref_is_three_separate_roundings(decay):
    for name, (e, p) in S.ema_i64_inputs().items():
        want = S.ema_i64_ref(torch.from_numpy(e), torch.from_numpy(p), decay).numpy()
        assert np.array_equal(want, S.ema_i64_emulate(e, p, decay)), (name, decay)


def test_ema_i64_inputs_tell_a_fused_product_from_a_rounded_one():
    """the proof that the GPU test's inputs discriminate, without running a wrong kernel"""
    e, p = S.ema_i64_inputs()["equal"]
    diff = {d: int((S.ema_i64_emulate(e, p, d) != S.ema_i64_emulate(e, p, d, contracted=True)).sum()) for d in S.EMA_DECAYS}
    print("contracted != separate, of 4096:", diff)
    assert diff[0.9999] >= 500
    assert S.ema_i64_emulate(e[11:12], p[11:12], 0.9999)[0] == 10 and S.ema_i64_emulate(e[11:12], p[11:12], 0.9999, contracted=True)[0] == 11


# ------------------------------------------------------------------ AdamW + EMA
def test_adamw_complements_distance_to_torch():
    """(float)(1.0 - b) against 1.f - (float)b: the three figures DESIGN.md states, and their bound 2^-24 b / (1 - b) (+ torch's own rounding)"""
    for b, want in ((0.999, 1.29e-5), (0.9, 2.2e-7), (0.9999, 1.66e-4)):
        kernel, torch_ = 1.0 - S.f32(b), S.f32(1.0 - b)
        rel = abs(kernel - torch_) / torch_
        print(f"b = {b}: relative distance of the complements {rel:.3e}, bound {U * b / (1 - b) + U:.3e}")
        assert abs(rel - want) <= 0.02 * want and rel <= U * b / (1 - b) + U
        assert np.float32(S.f32(b)) + np.float32(kernel) == np.float32(1.0) and np.float32(kernel) == np.float32(1.0) - np.float32(b)


@pytest.mark.parametrize("name", sorted(S.ADAMW_REGIMES))
def test_adamw_emulation_stays_inside_the_bounds(name):
    p, g, m, v, e, kw, ss = S.adamw_draw(name)
    assert (g == 0).any() and (m == 0).any() and (v == 0).any()
    r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=ss, **kw)
    K = S.adamw_K(r["k_coef"])
    em = S.adamw_emulate(p, g, m, v, e, sumsq=ss, **kw)
    sc = S.adamw_scalar_terms(r, kw["betas"], kw["ema_decay"])
    tp, tm, tv, te, tt = S.adamw_torch_ref(p, g, m, v, e, **kw)
    for o, t in (("m", tm), ("v", tv), ("p", tp), ("ema", te)):
        raw = S.worst_ratio(em[o], r[o], U * r["S_" + o])
        vs_torch = S.worst_ratio(em[o], t.numpy(), K[o] * U * r["S_" + o] + sc[o])
        print(f"[{name}] {o}: emulation {raw:.2f} u S (K = {K[o]}); against torch {vs_torch:.3f} of K u S + scalar term")
        assert raw <= K[o], (name, o)
        assert vs_torch <= 1.0, (name, o)
    assert abs(float(em["gnorm"]) - r["gnorm"]) <= 2 * U * r["gnorm"]
    assert abs(float(tt) - r["gnorm"]) <= 8 * U * r["gnorm"]                  # torch's fp32 norm of 4096 values


def test_adamw_wrong_variants_leave_the_bounds():
    worst = {var: 0.0 for var in S.ADAMW_WRONG}
    for name in S.ADAMW_REGIMES:
        p, g, m, v, e, kw, ss = S.adamw_draw(name)
        r = S.adamw_ema_step_ref(p, g, m, v, e, sumsq=ss, **kw)
        K = S.adamw_K(r["k_coef"])
        for var in S.ADAMW_WRONG:
            w = S.adamw_emulate(p, g, m, v, e, sumsq=ss, variant=var, **kw)
            worst[var] = max(worst[var], max(S.worst_ratio(w[o], r[o], K[o] * U * r["S_" + o]) for o in ("m", "v", "p", "ema")))
    print("wrong variants, worst error / bound over the regimes:", {k: f"{x:.3g}" for k, x in worst.items()})
    for var, x in worst.items():
        assert x > 4.0, f"the wrong variant {var} hides inside the bounds of every regime ({x:.3g})"


# ------------------------------------------------------------------ patch loss
def _patch_case(geo, mask_name="random"):
    B, D, H, W = geo
    f = (D // 16, H // 16, W // 16)
    vis = S.patch_masks(B, *f)[mask_name]
    inp, rec, fam = S.patch_families(B, *f, vis)
    return inp, rec, vis, fam


@pytest.mark.parametrize("normalized", [True, False])
def test_patch_loss_ref_is_the_oracle(normalized):
    for geo in S.PATCH_GEOMETRIES[:3]:
        inp, rec, vis, _ = _patch_case(geo)
        ref = S.patch_loss_ref(inp, rec, vis, normalized)
        loss, l2m = S.forward_loss_oracle(inp, rec, vis, normalized)
        assert np.allclose(ref["l2m"], l2m, rtol=1e-9, atol=1e-12)
        if normalized:
            # the oracle adds its 1e-8 to an int tensor, in fp32, where it is lost for count >= 1: the two differ by 1e-8 / count
            assert abs(ref["loss"] - loss) <= (1e-8 / ref["count"] + 1e-9) * abs(loss)
            x = torch.tensor(rec, dtype=torch.float64, requires_grad=True)
            cfg = O.Config([8] * 6, [1] * 6, 8, geo[1:])
            act = torch.as_tensor(vis).view(geo[0], 1, *cfg.fmap)
            O.forward_loss(O.patchify(cfg, torch.as_tensor(inp, dtype=torch.float64)[:, None]), O.patchify(cfg, x[:, None]), act)[0].backward()
            assert np.allclose(ref["drec"], x.grad.numpy(), rtol=1e-7, atol=1e-15)


def _patch_ratios(em, ref, normalized):
    b = S.patch_loss_bounds(ref, {k: 1.0 for k in S.PATCH_K})
    out = dict(l2=S.worst_ratio(em["l2m"], ref["l2m"], b["l2"]), rstd=S.worst_ratio(em["rstd"], ref["rstd"], b["rstd"]),
               mean=S.worst_ratio(em["mean"], ref["mean"], b["mean"]),
               drec=S.worst_ratio(np.abs(em["drec_p"] - ref["drec_p"]).max(-1), 0.0, b["drec"]),
               inv_count=S.worst_ratio(em["inv_count"], ref["inv_count"], b["inv_count"]))
    if normalized:
        out["loss"] = S.worst_ratio(em["loss"], ref["loss"], b["loss"])
    return out


def test_patch_loss_emulations_set_K():
    """K = 4 x the larger of the two emulations' worst ratios: neither may pass K / 4"""
    worst = {order: {} for order in ("kernel", "numpy")}
    for geo in S.PATCH_GEOMETRIES:
        for mask_name in ("random", "none_visible", "last_masked"):
            inp, rec, vis, _ = _patch_case(geo, mask_name)
            for normalized in (True, False):
                ref = S.patch_loss_ref(inp, rec, vis, normalized, -3.0)
                for order in worst:
                    for k, x in _patch_ratios(S.patch_loss_emulate(inp, rec, vis, normalized, -3.0, order), ref, normalized).items():
                        worst[order][k] = max(worst[order].get(k, 0.0), x)
    for order, w in worst.items():
        print(f"[{order}] worst error / (u S):", {k: f"{x:.2f}" for k, x in w.items()})
    for order, w in worst.items():
        for k, x in w.items():
            assert 4.0 * x <= (S.PATCH_K[k] if k != "inv_count" else 4.0 * 2.0), (order, k, x)


def test_patch_loss_ill_conditioned_families():
    inp, rec, vis, fam = _patch_case((2, 32, 48, 32), "none_visible")
    ref = S.patch_loss_ref(inp, rec, vis, True)
    em = S.patch_loss_emulate(inp, rec, vis, True)
    rel = np.abs(em["l2m"] - ref["l2"]) / ref["l2"] / U
    for f in range(5):
        print(f"family {f}: kappa {ref['kappa'][fam == f].max():.1f}  relative l2 error {rel[fam == f].max():.1f} u")
    assert ref["kappa"][fam == 3].min() > 1000 and ref["kappa"][fam == 2].min() > 90 and ref["kappa"][fam == 0].max() < 1
    assert abs(ref["rstd"][fam == 3] - 1000.0).max() < 1e-6 and (ref["mean"][fam == 3] == np.float64(np.float32(-1.02))).all()


def test_patch_loss_wrong_variants_leave_the_bounds():
    worst = {var: 0.0 for var in S.PATCH_WRONG}
    for mask_name in ("random", "all_visible"):
        inp, rec, vis, _ = _patch_case((2, 32, 48, 32), mask_name)
        ref = S.patch_loss_ref(inp, rec, vis, True)
        b = S.patch_loss_bounds(ref)
        for var in S.PATCH_WRONG:
            em = S.patch_loss_emulate(inp, rec, vis, True, variant=var)
            r = max(S.worst_ratio(em["l2m"], ref["l2m"], b["l2"]), S.worst_ratio(em["rstd"], ref["rstd"], b["rstd"]),
                    S.worst_ratio(em["loss"], ref["loss"], b["loss"]), S.worst_ratio(em["inv_count"], ref["inv_count"], b["inv_count"]),
                    S.worst_ratio(np.abs(em["drec_p"] - ref["drec_p"]).max(-1), 0.0, b["drec"]))
            worst[var] = max(worst[var], r)
        if mask_name == "all_visible":
            ok = S.patch_loss_emulate(inp, rec, vis, True)
            assert ok["loss"] == 0 and ok["inv_count"] == np.float32(1e8) and ref["loss"] == 0 and abs(ref["inv_count"] - 1e8) < 1e-3
            assert not ok["drec"].any()
    print("wrong variants, worst error / bound:", {k: f"{x:.3g}" for k, x in worst.items()})
    for var, x in worst.items():
        assert x > 4.0, f"the wrong variant {var} hides inside the bounds ({x:.3g})"


# ------------------------------------------------------------------ sampler
SAMPLER_L = (1, 2, 27, 256, 257, 513)


def _sampler_cases(L):
    keep = max(1, round(0.4 * L))
    return keep, sorted({ll for ll in (0, 1, (L - keep) // 2, L - keep) if 0 <= ll <= L - keep})


@pytest.mark.parametrize("L", SAMPLER_L)
def test_mask_sampler_ref_is_the_oracle_without_ties(L):
    cfg = O.Config([8] * 6, [1] * 6, 8, (16, 16, 16 * L))
    keep, lls = _sampler_cases(L)
    cfg.len_keep = keep                                              # max(1, .): Config rounds 0.4 to 0 at L = 1
    assert cfg.L == L
    loss, keys = S.sampler_draws(3, L)["continuous"]
    assert all(len(torch.unique(row)) == L for row in loss) and all(len(torch.unique(row)) == L for row in keys)
    for ll in lls:
        assert torch.equal(S.mask_sampler_ref(loss, keys, keep, ll), O.generate_mask_from_keys(cfg, loss, keys, ll).view(3, L)), (L, ll)


@pytest.mark.parametrize("L", SAMPLER_L)
def test_mask_sampler_ref_breaks_ties_by_id(L):
    keep, lls = _sampler_cases(L)
    for name, (loss, keys) in S.sampler_draws(3, L).items():
        if L >= 27 and name == "tied_loss":
            assert float((loss == 0).float().mean()) > 0.2
        for ll in lls:
            got = S.mask_sampler_ref(loss, keys, keep, ll)
            assert np.array_equal(got.numpy(), S.mask_sampler_loop(loss.numpy(), keys.numpy(), keep, ll)), (name, L, ll)
            assert (got.sum(1) == keep).all()
