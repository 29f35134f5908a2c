"""Test-side references of the step kernels (anatomask_amd/csrc/step_ops.hip): plain fp64 numpy / torch on the CPU, taking the same fp32
inputs the kernels get, the error scales the bounds of tests/test_step_ops_{cpu,gpu}.py are built from, and the numpy fp32 emulations
(one rounding per operation, nothing fused) that tests/test_step_ops_cpu.py uses to show that each bound is reachable by a correct fp32
implementation and not by a wrong one.  Nothing here runs on the HIP library.

u = 2^-24 is the unit roundoff of fp32 throughout.  A bound is K u S: S the magnitude of the terms on the way to an output, K the number
of fp32 roundings on that way, counted from the kernel's source (fusion by the compiler only removes roundings)."""
import math

import numpy as np
import torch

from oracle import anatomask_oracle as O

U = 2.0 ** -24
F32 = np.float32


def f32(x) -> float:
    """a double rounded to fp32, as a python float: what the C ABI makes of a scalar argument"""
    return float(F32(x))


def worst_ratio(got, want, bound) -> float:
    """max |got - want| / bound in fp64; a zero bound demands equality, a NaN or an unexpected infinity counts as infinitely far"""
    got, want, bound = (np.asarray(t, dtype=np.float64) for t in (got, want, bound))
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        err = np.where(np.isnan(err), np.inf, err)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- optimizer
def adam_scalars(lr, betas, eps, wd, step, ema_decay, grad_scale=1.0, sumsq=None, max_norm=12.0):
    """the scalars of am_adamw_ema rounded to fp32 exactly where the ABI rounds them (python floats); the complements 1 - b are NOT
    here: the kernel takes them from the rounded values"""
    return dict(lr=f32(lr), b1=f32(betas[0]), b2=f32(betas[1]), eps=f32(eps), wd=f32(wd), bc1=f32(1.0 - betas[0] ** step),
                bc2_sqrt=f32(math.sqrt(1.0 - betas[1] ** step)), ema_decay=f32(ema_decay), grad_scale=f32(grad_scale),
                max_norm=f32(max_norm), norm=None if sumsq is None else f32(math.sqrt(sumsq)), tiny=f32(1e-6))


def adamw_ema_step_ref(p, g, m, v, ema, *, lr, betas, eps, wd, step, ema_decay, sumsq=None, max_norm=12.0, grad_scale=1.0):
    """ONE call of am_adamw_ema: the kernel's documented formula evaluated in fp64 on fp32 inputs (numpy arrays or tensors; ema may be
    None).  sumsq is the double am_sumsq left (None: no clipping).  Returns the four outputs, the intermediates and the error scales
    S_m = |m| + |gk|, S_v = v', S_p = |p| + step_size (|m| + |gk|) / denom, S_ema = |ema| + |p'|, and k_coef: the fp32 roundings in the
    clip coefficient (total = norm * scale, + 1e-6, the division, * scale: 4 when the clip is active; `1.f * scale` is exact otherwise)."""
    s = adam_scalars(lr, betas, eps, wd, step, ema_decay, grad_scale, sumsq, max_norm)
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    total = s["norm"] * s["grad_scale"] if sumsq is not None else 0.0
    coef = s["max_norm"] / (total + s["tiny"]) if sumsq is not None else 1.0
    clipped = coef < 1.0
    coef = min(coef, 1.0) * s["grad_scale"]
    step_size, decay_mul = s["lr"] / s["bc1"], 1.0 - s["lr"] * s["wd"]
    gk = g * coef
    m2 = m + (gk - m) * (1.0 - s["b1"])
    v2 = v * s["b2"] + (1.0 - s["b2"]) * gk * gk
    denom = np.sqrt(v2) / s["bc2_sqrt"] + s["eps"]
    upd = step_size * (m2 / denom)
    p2 = p * decay_mul - upd
    out = dict(p=p2, m=m2, v=v2, gk=gk, denom=denom, upd=upd, gnorm=total, coef=coef, clipped=clipped, step_size=step_size,
               k_coef=4 if clipped else 0, scalars=s)
    out["S_m"] = np.abs(m) + np.abs(gk)
    out["S_v"] = v2
    out["S_p"] = np.abs(p) + step_size * (np.abs(m) + np.abs(gk)) / denom
    if ema is not None:
        e = np.asarray(ema, dtype=np.float64)
        out["ema"] = e * s["ema_decay"] + (1.0 - s["ema_decay"]) * p2
        out["S_ema"] = np.abs(e) + np.abs(p2)
    return out


def adamw_K(k_coef: int):
    """fp32 roundings on the way to each output of adamw_ema_kernel (step_ops.hip), kc = k_coef those of the clip coefficient.
    1 - b1, 1 - b2, 1 - ema_decay are exact for b in [0.5, 1] (Sterbenz).
      gk = g * coef                                              1 + kc
      m' = m + (gk - m) * (1 - b1)                               gk, -, *, +                         K_m = 4 + kc
      v' = v * b2 + ((1 - b2) * gk) * gk                         gk twice, *, *, *, +                K_v = 6 + 2 kc
      denom = sqrtf(v') / bc2_sqrt + eps                         K_v / 2 (the root halves a relative error) + sqrt, /, +
      p' = p * (1 - lr * wd) - (lr / bc1) * (m' / denom)         K_m + K_v / 2 + 3 on m' / denom, then /, lr / bc1, * on the update;
                                                                 lr * wd, 1 - ., * on the decayed weight; the final -:
                                                                 K_p = K_m + K_v / 2 + 7 = 14 + 2 kc   (each term <= K_p u S_p)
      ema' = ema * d + (1 - d) * p'                              K_p (p' enters with weight 1 - d <= 1), *, *, +   K_ema = K_p + 3"""
    K_m, K_v = 4 + k_coef, 6 + 2 * k_coef
    K_p = K_m + K_v // 2 + 7
    return dict(m=K_m, v=K_v, p=K_p, ema=K_p + 3)


def adamw_torch_ref(p, g, m, v, ema, *, lr, betas, eps, wd, step, ema_decay, max_norm=12.0, grad_scale=1.0, clip=True):
    """the real reference of one step: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW + timm's `e * decay + (1. - decay) * p` on fp32
    CPU tensors with python-double scalars, started from the given state (exp_avg = m, exp_avg_sq = v, step - 1 steps taken).  The
    gradient is the ranks' sum times grad_scale (DDP's mean).  Returns (p, m, v, ema, total_norm) as fp32 tensors."""
    w = torch.nn.Parameter(torch.as_tensor(p, dtype=torch.float32).clone())
    w.grad = torch.as_tensor(g, dtype=torch.float32).clone() * grad_scale
    opt = torch.optim.AdamW([w], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.as_tensor(m, dtype=torch.float32).clone(),
                    "exp_avg_sq": torch.as_tensor(v, dtype=torch.float32).clone()}
    total = torch.nn.utils.clip_grad_norm_([w], max_norm) if clip else torch.zeros(())
    opt.step()
    st = opt.state[w]
    assert int(st["step"]) == step
    e2 = None
    if ema is not None:
        e = torch.as_tensor(ema, dtype=torch.float32)
        with torch.no_grad():
            e2 = e * ema_decay + (1. - ema_decay) * w
    return w.detach(), st["exp_avg"], st["exp_avg_sq"], e2, total


def adamw_scalar_terms(r, betas, ema_decay):
    """how far torch's scalars carry adamw_torch_ref from adamw_ema_step_ref (r = its result), per element.  torch multiplies by
    (float)(1.0 - b), the kernel by 1.f - (float)b: (float)b is off by at most u b, so the complement by u b / (1 - b) relative (1.29e-5
    for b2 = 0.999, 2.2e-7 for b1 = 0.9, 1.66e-4 for decay 0.9999 are the actual figures), times the term the complement multiplies:
      m:   c1 |(gk - m)(1 - b1)|                       c = u b / (1 - b) + u (torch's own rounding of the complement)
      v:   c2 (1 - b2) gk^2
      p:   the two above through m' / denom, denom = sqrt(v') / bc2_sqrt + eps, plus 2u on lr / bc1 (torch rounds the double quotient,
           the kernel divides the rounded values): step_size (dm / denom + |m'| dv / (2 sqrt(v') bc2_sqrt denom^2)) + 2u |upd|
      ema: c3 (1 - d) |p'| + (1 - d) dp"""
    s = r["scalars"]
    c = lambda b: U * b / (1.0 - b) + U
    gk, m2, v2, denom = r["gk"], r["m"], r["v"], r["denom"]
    m0 = (m2 - gk * (1.0 - s["b1"])) / s["b1"]                     # the m the step started from
    dm = c(betas[0]) * np.abs((gk - m0) * (1.0 - s["b1"]))
    dv = c(betas[1]) * (1.0 - s["b2"]) * gk * gk
    root = np.sqrt(v2)
    ddenom = np.where(root > 0, dv / (2.0 * np.maximum(root, 1e-300) * s["bc2_sqrt"]), 0.0)
    dp = r["step_size"] * (dm / denom + np.abs(m2) * ddenom / denom ** 2) + 2.0 * U * np.abs(r["upd"])
    out = dict(m=dm, v=dv, p=dp)
    if "ema" in r:
        out["ema"] = c(ema_decay) * (1.0 - s["ema_decay"]) * np.abs(r["p"]) + (1.0 - s["ema_decay"]) * dp
    return out


def adamw_emulate(p, g, m, v, ema, *, lr, betas, eps, wd, step, ema_decay, sumsq=None, max_norm=12.0, grad_scale=1.0, variant=None):
    """numpy fp32 emulation of adamw_ema_kernel: the kernel's sequence with one rounding per operation, nothing fused.  `variant` names
    one deliberately WRONG form (tests/test_step_ops_cpu.py shows that each leaves the bounds)."""
    s = {k: (None if x is None else F32(x)) for k, x in adam_scalars(lr, betas, eps, wd, step, ema_decay, grad_scale, sumsq, max_norm).items()}
    one = F32(1.0)
    p, g, m, v = (np.asarray(t, dtype=F32) for t in (p, g, m, v))
    total = s["norm"] * s["grad_scale"] if sumsq is not None else F32(0.0)
    coef = one
    if sumsq is not None:
        coef = s["max_norm"] / (total if variant == "no_1e-6" else total + s["tiny"])
    coef = (one if coef > one else coef) * (one if variant == "scale_norm_only" else s["grad_scale"])
    step_size, decay_mul = s["lr"] / s["bc1"], one - s["lr"] * s["wd"]
    gk = g * coef
    w = p if variant == "decay_after" else p * decay_mul
    m2 = m + (gk - m) * (one - s["b1"])
    v2 = v * s["b2"] + (one - s["b2"]) * gk * gk
    if variant == "bc2_not_sqrt":
        denom = np.sqrt(v2) / (s["bc2_sqrt"] * s["bc2_sqrt"]) + s["eps"]
    elif variant == "eps_before_div":
        denom = (np.sqrt(v2) + s["eps"]) / s["bc2_sqrt"]
    else:
        denom = np.sqrt(v2) / s["bc2_sqrt"] + s["eps"]
    w = w - step_size * (m2 / denom)
    if variant == "decay_after":
        w = w * decay_mul
    out = dict(p=w, m=m2, v=v2, gnorm=total)
    assert all(a.dtype == F32 for a in (w, m2, v2))
    if ema is not None:
        e = np.asarray(ema, dtype=F32)
        out["ema"] = e * s["ema_decay"] + (one - s["ema_decay"]) * (p if variant == "ema_old_p" else w)
    return out


ADAMW_WRONG = ("no_1e-6", "bc2_not_sqrt", "eps_before_div", "decay_after", "ema_old_p", "scale_norm_only")

# name: (n, p scale, g scale, step, lr, wd, max_norm, grad_scale, ema_decay) -- clip active / inactive, step 1 .. 100000, grad_scale
# 1 / 0.5 / 0.125, lr 1e-3 .. 1e-6, exact zeros in g, m, v (adamw_draw).  The last two exist for wrong variants that hide in the others:
# a clip at a norm small enough for the 1e-6 of its denominator to matter, and weights small enough for lr * wd * update to show.
ADAMW_REGIMES = {
    "clip_step1":      (4096, 1.0, 2.0, 1, 1e-3, 1e-5, 12.0, 1.0, 0.99),
    "noclip_step3":    (4096, 1.0, 0.05, 3, 1e-4, 1e-5, 12.0, 1.0, 0.999),
    "ranks2_step1000": (4096, 1.0, 1.0, 1000, 1e-5, 1e-5, 12.0, 0.5, 0.9999),
    "ranks8_late":     (4096, 1.0, 0.3, 100000, 1e-6, 1e-5, 12.0, 0.125, 0.9999),
    "tiny_norm_clip":  (1024, 1.0, 1e-4, 1, 1e-3, 1e-5, 1e-3, 1.0, 0.99),
    "small_p_big_wd":  (4096, 1e-3, 0.05, 3, 1e-3, 0.1, 12.0, 1.0, 0.99),
}
ADAMW_BETAS, ADAMW_EPS = (0.9, 0.999), 1e-8


def adamw_draw(name, n=None, seed=0):
    """seeded fp32 state of a regime: (p, g, m, v, ema, kwargs for the references, sumsq as am_sumsq defines it: the fp64 sum of g^2)"""
    n0, ps, gs, step, lr, wd, max_norm, grad_scale, decay = ADAMW_REGIMES[name]
    n = n or n0
    gs = gs * math.sqrt(n0 / n)                                      # the gradient norm, and with it the clip, is the regime's at every n
    rng = np.random.default_rng(1000 + seed + sorted(ADAMW_REGIMES).index(name))
    p = (rng.standard_normal(n) * ps).astype(F32)
    g = (rng.standard_normal(n) * gs).astype(F32)
    if step == 1:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:
        m = (rng.standard_normal(n) * gs * 0.3).astype(F32)
        v = ((rng.standard_normal(n) * gs) ** 2 * (0.5 if step > 100 else 0.003 * step)).astype(F32)
    ema = (p + rng.standard_normal(n).astype(F32) * F32(0.01 * ps)).astype(F32)
    for a in (g, m, v):                                              # exact zeros, overlapping in about 1 element of 1000
        a[rng.random(n) < 0.1] = 0
    kw = dict(lr=lr, betas=ADAMW_BETAS, eps=ADAMW_EPS, wd=wd, step=step, ema_decay=decay, max_norm=max_norm, grad_scale=grad_scale)
    return p, g, m, v, ema, kw, float(np.sum(g.astype(np.float64) ** 2))


# ---------------------------------------------------------------------------------------------------------------- int64 EMA
def ema_i64_ref(e: torch.Tensor, p: torch.Tensor, decay: float) -> torch.Tensor:
    """timm's update of an integer state_dict entry, with torch on the CPU: int64 tensors and a python float"""
    assert e.dtype == p.dtype == torch.int64 and e.device.type == "cpu"
    return (e * decay + (1.0 - decay) * p).to(torch.int64)


def ema_i64_emulate(e: np.ndarray, p: np.ndarray, decay: float, contracted: bool = False) -> np.ndarray:
    """fp32 with three separate roundings (two products, one sum), truncated; contracted=True: fl(fl(om * p) + decay * e) with the second
    product unrounded -- what a fused multiply-add makes of it (an fp64 product of two fp32 numbers is exact)"""
    d, om = F32(decay), F32(1.0 - decay)
    ef, pf = e.astype(F32), p.astype(F32)
    b = om * pf
    if contracted:
        s = (b.astype(np.float64) + np.float64(d) * ef.astype(np.float64)).astype(F32)
    else:
        s = ef * d + b
    return np.trunc(s).astype(np.int64)


def ema_i64_inputs():
    """(e, p) int64 pairs: e = p = 0..4095, p = e + 1, p = e + 7, and three large counters"""
    k = np.arange(4096, dtype=np.int64)
    big = np.array([2 ** 24 + 1, 2 ** 31 + 5, 2 ** 40 + 12345], dtype=np.int64)
    return {"equal": (k, k.copy()), "plus1": (k, k + 1), "plus7": (k, k + 7), "big": (big, big.copy()), "big_plus1": (big, big + 1)}


EMA_DECAYS = (0.999, 0.9999, 0.99945)


# ---------------------------------------------------------------------------------------------------------------- patch loss
def patches(x, fd, fh, fw):
    """[B, 16 fd, 16 fh, 16 fw] -> [B, L, 4096], patches in (d, h, w) order, voxels in (z, y, x) order: the kernel's indexing"""
    B = x.shape[0]
    return x.reshape(B, fd, 16, fh, 16, fw, 16).transpose(0, 1, 3, 5, 2, 4, 6).reshape(B, fd * fh * fw, 4096)


def unpatches(xp, fd, fh, fw):
    B = xp.shape[0]
    return xp.reshape(B, fd, fh, fw, 16, 16, 16).transpose(0, 1, 4, 2, 5, 3, 6).reshape(B, fd * 16, fh * 16, fw * 16)


def patch_loss_ref(inp, rec, active, normalized: bool, gout: float = 1.0):
    """fp64 on fp32 inputs: inp / rec [B, D, H, W], active [B, fd, fh, fw] (non-zero = visible).  Per patch l2 (unmasked), l2m, mean, rstd
    (unbiased variance, + 1e-6; 0 / 1 when not normalized) and kappa = |mean| rstd; loss, inv_count = 1 / (count + 1e-8) and
    drec = gout (1 - active) inv_count 2 (rec - target) / 4096.  Equals O.forward_loss / O.teacher_patch_loss in exact arithmetic."""
    inp, rec = np.asarray(inp, dtype=np.float64), np.asarray(rec, dtype=np.float64)
    act = np.asarray(active) != 0
    B, fd, fh, fw = act.shape
    x, r = patches(inp, fd, fh, fw), patches(rec, fd, fh, fw)
    vis = act.reshape(B, -1)
    if normalized:
        mean = x.mean(-1)
        var = ((x - mean[..., None]) ** 2).sum(-1) / 4095.0
        rstd = 1.0 / np.sqrt(var + 1e-6)
    else:
        mean, rstd = np.zeros(x.shape[:2]), np.ones(x.shape[:2])
    with np.errstate(all="ignore"):
        diff = r - (x - mean[..., None]) * rstd[..., None]
        l2 = (diff ** 2).mean(-1)
        l2m = np.where(vis, 0.0, l2)
        count = float((~vis).sum())
        inv_count = 1.0 / (count + 1e-8)
        loss = l2m.sum() * inv_count
        drec = np.where(vis[..., None], 0.0, gout * inv_count * (2.0 / 4096.0) * diff)
    return dict(l2=l2, l2m=l2m, mean=mean, rstd=rstd, kappa=np.abs(mean) * rstd, loss=loss, inv_count=inv_count, count=count,
                drec=unpatches(drec, fd, fh, fw), drec_p=drec, absmean=np.abs(x).mean(-1), vis=vis)


def _block_sum32(t, order: str):
    """sum over the last axis ([.., 256 threads, 16]) in fp32.  'kernel': 16 serial adds per thread, a 6-level xor butterfly in each of
    the 4 waves, then sh[0] + sh[1] + sh[2] + sh[3]; 'numpy': np.sum over the 4096 values (pairwise, another order)"""
    assert t.dtype == F32
    if order == "numpy":
        return t.reshape(*t.shape[:-2], 4096).sum(-1, dtype=F32)
    s = np.zeros(t.shape[:-1], F32)
    for i in range(16):
        s = s + t[..., i]
    s = s.reshape(*s.shape[:-1], 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    w = s[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def patch_loss_emulate(inp, rec, active, normalized: bool, gout: float = 1.0, order: str = "kernel", variant=None):
    """numpy fp32 emulation of patch_loss_fwd / reduce / bwd (one rounding per operation); `variant` names one deliberately WRONG form"""
    inp, rec = np.asarray(inp, dtype=F32), np.asarray(rec, dtype=F32)
    act = np.asarray(active) != 0
    B, fd, fh, fw = act.shape
    x, r = (patches(t, fd, fh, fw).reshape(B, -1, 256, 16) for t in (inp, rec))
    vis = act.reshape(B, -1)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        if normalized:
            mean = _block_sum32(x, order) * (one / F32(4096.0))
            d = x - mean[..., None, None]
            var = _block_sum32(d * d, order) * (one / F32(4096.0 if variant == "var_4096" else 4095.0))
            if variant == "eps_outside":
                rstd = one / (np.sqrt(var) + F32(1e-6))
            elif variant == "eps_1e-5":
                rstd = one / np.sqrt(var + F32(1e-5))
            else:
                rstd = one / np.sqrt(var + F32(1e-6))
        else:
            mean, rstd = np.zeros(x.shape[:2], F32), np.ones(x.shape[:2], F32)
        diff = r - (x - mean[..., None, None]) * rstd[..., None, None]
        l2 = _block_sum32(diff * diff, order) * (one / F32(4095.0 if variant == "mean_sq_4095" else 4096.0))
        l2m = np.where(vis, F32(0), l2)
        flat, nvis = l2m.reshape(-1), (~vis).reshape(-1).astype(F32)
        pad = (-flat.size) % 256
        if order == "numpy":
            s, c = flat.sum(dtype=F32), nvis.sum(dtype=F32)
        else:                                                        # the reduce kernel: thread t adds elements t, t + 256, ... serially, then the same block fold
            cols = np.concatenate([flat, np.zeros(pad, F32)]).reshape(-1, 256)
            ccols = np.concatenate([nvis, np.zeros(pad, F32)]).reshape(-1, 256)
            ts, tc = np.zeros(256, F32), np.zeros(256, F32)
            for row, crow in zip(cols, ccols):
                ts, tc = ts + row, tc + crow
            fold = lambda t: _block_sum32(np.stack([t] + [np.zeros_like(t)] * 15, -1), "kernel")
            s, c = fold(ts), fold(tc)
        cden = c if variant == "no_1e-8" else c + F32(1e-8)
        loss, inv_count = s / cden, one / cden
        k = (F32(gout) * inv_count) * (F32(2.0) / F32(4096.0)) if np.isfinite(loss) else F32(np.nan)
        drec = np.where(vis[..., None, None], F32(0), k * diff)
    return dict(l2m=l2m, mean=mean, rstd=rstd, loss=loss, inv_count=inv_count, drec=unpatches(drec.reshape(B, -1, 4096), fd, fh, fw),
                drec_p=drec.reshape(B, -1, 4096))


PATCH_WRONG = ("var_4096", "eps_outside", "eps_1e-5", "mean_sq_4095", "no_1e-8")

# K of the patch-loss bounds: 4 x the larger of the two emulations' worst error / (u S) over the input families (measured by
# tests/test_step_ops_cpu.py, which asserts that neither emulation passes K / 4; the figures are in its docstring)
PATCH_K = dict(l2=10.0, mean=16.0, rstd=9.0, drec=11.0, loss=4.0)


def patch_loss_bounds(ref, K=PATCH_K):
    """per patch, with kappa = |mean| rstd (the cancellation of inp - mean, amplified by rstd):
      l2    K u (l2 + 2 sqrt(l2) kappa + kappa^2 u)        the target is off by ~ u kappa, the difference is squared
      mean  K u mean|inp|
      rstd  K u rstd (1 + kappa^2 u)                        d rstd / rstd = -1/2 d var / (var + 1e-6); var gains (mean error)^2
      drec  K u (1 + kappa) max|drec| over the patch
      loss  sum of the masked patches' l2 bounds / count + K u loss (the 256-thread sum);  inv_count  2 u inv_count"""
    l2, kap = ref["l2"], ref["kappa"]
    b_l2 = K["l2"] * U * (l2 + 2.0 * np.sqrt(l2) * kap + kap * kap * U)
    masked = ~ref["vis"]
    return dict(l2=b_l2, mean=K["mean"] * U * ref["absmean"], rstd=K["rstd"] * U * ref["rstd"] * (1.0 + kap * kap * U),
                drec=K["drec"] * U * (1.0 + kap) * np.abs(ref["drec_p"]).max(-1),
                loss=float(b_l2[masked].sum()) * ref["inv_count"] + K["loss"] * U * abs(ref["loss"]), inv_count=2.0 * U * ref["inv_count"])


def patch_families(B, fd, fh, fw, vis, seed=0):
    """seeded fp32 (inp, rec) [B, 16 fd, 16 fh, 16 fw]: patch i of the MASKED ones (in index order) gets family i mod 5 --
    0: 1.7 z + 0.3 (the existing tests' input)   1: small std with offset, 0.05 z + 3   2: large offset, z + 100
    3: a constant patch, -1.02 (CT air)          4: as 0, rec a thousand times smaller than the target
    visible patches get family 0."""
    rng = np.random.default_rng(77 + seed)
    L = fd * fh * fw
    z = rng.standard_normal((B, L, 4096))
    x = 1.7 * z + 0.3
    r = rng.standard_normal((B, L, 4096))
    fam = np.zeros((B, L), dtype=np.int64)
    ids = np.flatnonzero(~np.asarray(vis).reshape(-1))
    fam.reshape(-1)[ids] = np.arange(ids.size) % 5
    x = np.where((fam == 1)[..., None], 0.05 * z + 3.0, x)
    x = np.where((fam == 2)[..., None], z + 100.0, x)
    x = np.where((fam == 3)[..., None], -1.02, x)
    r = np.where((fam == 4)[..., None], 1e-3 * r, r)
    return unpatches(x, fd, fh, fw).astype(F32), unpatches(r, fd, fh, fw).astype(F32), fam


# ---------------------------------------------------------------------------------------------------------------- sampler
def mask_sampler_ref(loss: torch.Tensor, keys: torch.Tensor, len_keep: int, len_loss: int) -> torch.Tensor:
    """O.generate_mask_from_keys with BOTH argsorts stable: the kernel breaks every tie by patch id, in the loss sort and in the key
    sort, so among equal losses the higher ids are the harder ones.  -> bool [B, L].  NaN losses / keys are out of scope."""
    B, L = loss.shape
    k = keys.clone().to(torch.float64)
    if len_loss > 0:
        hard = torch.argsort(loss, dim=1, stable=True)[:, L - len_loss:]
        k.scatter_(1, hard, float("inf"))
    visible = torch.argsort(k, dim=1, stable=True)[:, :len_keep]
    return torch.zeros(B, L, dtype=torch.bool).scatter_(1, visible, True)


def mask_sampler_loop(loss, keys, len_keep: int, len_loss: int):
    """'ties by id' as a direct python loop over (value, id) pairs"""
    loss, keys = np.asarray(loss), np.asarray(keys)
    out = np.zeros(loss.shape, dtype=bool)
    for b in range(loss.shape[0]):
        L = loss.shape[1]
        by_loss = sorted(range(L), key=lambda i: (float(loss[b, i]), i))
        hard = set(by_loss[L - len_loss:]) if len_loss > 0 else set()
        rest = sorted((i for i in range(L) if i not in hard), key=lambda i: (float(keys[b, i]), i))
        out[b, rest[:len_keep]] = True
    return out


def sampler_draws(B, L, seed=0):
    """name -> (loss, keys) fp32 [B, L]: continuous loss >= 0 with randn keys (both branches of the kernel's order-preserving map);
    losses quantised to 8 levels with 40 % exact zeros (the teacher's loss is exactly 0 on its visible patches); keys quantised to 8
    levels; a loss row with a few +inf"""
    g = torch.Generator().manual_seed(900 + 7 * L + seed)
    cont, keys = torch.rand(B, L, generator=g), torch.randn(B, L, generator=g)
    ql = torch.floor(torch.rand(B, L, generator=g) * 8) / 8 + 0.125
    ql[torch.rand(B, L, generator=g) < 0.4] = 0.0
    qk = torch.floor(torch.randn(B, L, generator=g) * 2).clamp(-4, 3) / 2
    inf = cont.clone()
    inf[0, torch.randperm(L, generator=g)[:min(3, L)]] = float("inf")
    return {"continuous": (cont, keys), "tied_loss": (ql, keys), "tied_keys": (cont, qk), "inf_loss": (inf, keys)}


def forward_loss_oracle(inp, rec, active, normalized):
    """O.forward_loss / O.teacher_patch_loss in fp64 through O.patchify: (loss or None, l2m [B, L])"""
    B, D, H, W = inp.shape
    cfg = O.Config([8] * 6, [1] * 6, 8, (D, H, W))
    ip = O.patchify(cfg, torch.as_tensor(inp, dtype=torch.float64)[:, None])
    rp = O.patchify(cfg, torch.as_tensor(rec, dtype=torch.float64)[:, None])
    act = torch.as_tensor(np.asarray(active) != 0).view(B, 1, *cfg.fmap)
    if normalized:
        loss, l2m = O.forward_loss(ip, rp, act)
        return float(loss), l2m.numpy()
    return None, O.teacher_patch_loss(ip, rp, act).numpy()


PATCH_GEOMETRIES = ((1, 16, 16, 16), (3, 16, 16, 16), (2, 32, 48, 32), (1, 16, 32, 64), (2, 48, 16, 32))       # (B, D, H, W)


def patch_masks(B, fd, fh, fw, seed=0):
    """name -> visible [B, fd, fh, fw] (bool): random (about 40 % visible, patch 0 masked), all visible, none visible, exactly one masked
    patch (the first; the last of the last sample)"""
    rng = np.random.default_rng(55 + seed)
    rand = rng.random((B, fd, fh, fw)) < 0.4
    rand.reshape(-1)[0] = False
    first, last = np.ones((B, fd, fh, fw), bool), np.ones((B, fd, fh, fw), bool)
    first.reshape(-1)[0] = False
    last.reshape(-1)[-1] = False
    return {"random": rand, "all_visible": np.ones((B, fd, fh, fw), bool), "none_visible": np.zeros((B, fd, fh, fw), bool),
            "first_masked": first, "last_masked": last}
