"""Test-side references of the sparse layer zoo (anatomask_amd/csrc/layer_ops.hip behind anatomask_amd/sparse_layers.py): plain fp64
numpy / torch restatements on the CPU, the error scale S every bound is taken against, the bounds themselves, the seeded inputs that
tests/test_layer_zoo_{cpu,gpu}.py share, and numpy fp32 emulations in the kernels' operation order (one rounding per operation) that
tests/test_layer_zoo_cpu.py uses to show that each bound is met by a correct fp32 evaluation and broken by a wrong one.  Nothing here
runs on the HIP library and nothing differentiates the code under test.

Layout: activations are channels-last [B, D, H, W, C] float64 arrays, voxel masks bool [B, D, H, W] (None: dense).  All activations and
upstream gradients are bf16-representable (q_bf16), so the fp32 and the bf16-storage runs see the same numbers and share one
reference; parameters stay fp32 (the modules keep fp32 masters in both modes).

A bound is K u S (u = 2^-24): S the sum of the magnitudes of the terms on the way to an output, K the number of fp32 roundings a term
can pass through, counted from the kernel's source.  bf16 storage adds the half-ulp of the rounded store: 2^-9 |ref| at the top of a
binade, 2^-8 |ref| at its bottom (half_ulp_bf16; a round-to-nearest store cannot meet 2^-9 |ref| everywhere).
Where K cannot be counted (erff / __expf in GELU, rsqrtf in the group norms) K is 4 x the ratio err / (u S) measured on an MI355X
(K_MEASURED below; the factor covers inputs other than the seeded ones)."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F32 = np.float32
LAYER_REP = 64          # replicated accumulator rows of the per-channel gradients (sparse_layers.LAYER_REP)
EPS6 = float(F32(1e-6))  # the kernels' 1e-6f


def q_bf16(a):
    """round to bf16 (nearest even), returned as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(np.float64)


def up(active, size):
    """patch mask bool (B, 1, fd, fh, fw) -> voxel mask bool [B, D, H, W]"""
    a = np.asarray(active)
    a = a.reshape(a.shape[0], *a.shape[-3:])
    for ax, n in enumerate(size):
        r = n // a.shape[ax + 1]
        assert r * a.shape[ax + 1] == n, (size, a.shape)
        a = np.repeat(a, r, axis=ax + 1)
    return a


def worst_ratio(got, want, bound) -> float:
    """max |got - want| / bound in fp64; a zero bound demands equality, a NaN or an unexpected infinity counts as infinitely far"""
    got, want, bound = (np.asarray(t, dtype=np.float64) for t in (got, want, bound))
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        err = np.where(np.isnan(err), np.inf, err)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def half_ulp_bf16(a):
    """half the spacing of bf16 (8 significant bits) in the binade of |a|: 2^(floor(log2 |a|) - 8), between 2^-9 |a| and 2^-8 |a|"""
    _, e = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))               # |a| = m 2^e, m in [0.5, 1)
    return np.where(np.asarray(a) != 0, np.ldexp(1.0, e - 9), 0.0)


def bound(K, S, ref=None, bf16=False):
    """K u S, plus the half-ulp of a bf16 store of the result (taken at |ref| + K u S: the fp32 value may sit in the next binade)"""
    b = K * U * np.asarray(S, dtype=np.float64)
    return b + half_ulp_bf16(np.abs(ref) + b) if bf16 else b


def _m(mask):
    return True if mask is None else mask[..., None]


def _zf(x, mask):
    """the tensor as every kernel reads it: zeros at the inactive voxels, whatever bits they hold"""
    x = np.asarray(x, dtype=np.float64)
    return x if mask is None else np.where(mask[..., None], x, 0.0)


def _ceil(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- depthwise conv
def dwconv_ref(x, w, b, k, s, m_in=None, m_out=None, dy=None):
    """depthwise k^3 convolution, stride s in {1, 2}, padding k // 2, of the zero-filled input, output masked; with dy also the data,
    weight and bias gradients.  w [C, k, k, k], b [C] or None.  Every result r comes with S_r, the same sum on absolute values:
    S_y = |b| + sum_t |w_t| |x_t|, S_dx = sum_t |w_t| |dy_t|, S_dw = sum_v |dy_v| |x_{v+t}|, S_db = sum_v |dy_v|."""
    B, D, H, W, C = x.shape
    P = k // 2
    assert s == 1 or (D % 2 == 0 and H % 2 == 0 and W % 2 == 0)
    Do, Ho, Wo = D // s, H // s, W // s
    w = np.asarray(w, dtype=np.float64).reshape(C, k, k, k)
    xp = np.pad(_zf(x, m_in), ((0, 0), (P, P), (P, P), (P, P), (0, 0)))
    axp = np.abs(xp)
    y = np.zeros((B, Do, Ho, Wo, C)); Sy = np.zeros_like(y)
    if dy is not None:
        dy0 = _zf(dy, m_out); ady = np.abs(dy0)
        dxp = np.zeros_like(xp); Sdxp = np.zeros_like(xp)
        dw = np.zeros((C, k, k, k)); Sdw = np.zeros_like(dw)
    for td in range(k):
        for th in range(k):
            for tw in range(k):
                sl = (slice(None), slice(td, td + s * Do, s), slice(th, th + s * Ho, s), slice(tw, tw + s * Wo, s))
                wt = w[:, td, th, tw]
                y += wt * xp[sl]; Sy += np.abs(wt) * axp[sl]
                if dy is not None:
                    dxp[sl] += wt * dy0; Sdxp[sl] += np.abs(wt) * ady
                    dw[:, td, th, tw] = np.einsum("bdhwc,bdhwc->c", dy0, xp[sl]); Sdw[:, td, th, tw] = np.einsum("bdhwc,bdhwc->c", ady, axp[sl])
    if b is not None:
        y += np.asarray(b, dtype=np.float64); Sy += np.abs(np.asarray(b, dtype=np.float64))
    out = dict(y=y * _m(m_out), S_y=Sy * _m(m_out))
    if dy is not None:
        un = (slice(None), slice(P, P + D), slice(P, P + H), slice(P, P + W))
        out.update(dx=dxp[un] * _m(m_in), S_dx=Sdxp[un] * _m(m_in), dw=dw, S_dw=Sdw, db=dy0.sum((0, 1, 2, 3)), S_db=ady.sum((0, 1, 2, 3)))
    return out


def K_dw(k):
    """dwconv_kernel / dwconv_s2_kernel: the accumulator starts at the bias and takes one (fused or not) multiply-add per tap: k^3
    additions, and the products' own roundings add up to one more u S"""
    return k ** 3 + 1


def K_dw_s2_dgrad(k):
    """dwconv_s2_kernel<MODE 1>: only the taps of the right parity, at most ceil(k / 2) per axis"""
    return ((k + 1) // 2) ** 3 + 1


def dw_nslot(nbrick, C, epc):
    """launch_dw_wgrad: workgroups per channel chunk"""
    nslot = max(8, 1024 // (C // epc) // 8 * 8)
    return min(nslot, _ceil(nbrick, 8) * 8)


def K_dw_wgrad(k, B, D, H, W, C, epc):
    """dwconv_wgrad_kernel: a lane adds 4 voxels of every NSUB-th of a brick's 64 (row, quad) items, over all bricks of its workgroup
    (ceil(nbrick / nslot)), in one fma chain; then 4 waves x NSUB lanes are folded, then nslot workgroups flush one atomic each."""
    nbrick = B * _ceil(D, 8) * _ceil(H, 8) * _ceil(W, 16)
    nslot, nsub = dw_nslot(nbrick, C, epc), 64 // (k * k)
    return _ceil(nbrick, nslot) * _ceil(64, nsub) * 4 + 4 * nsub + nslot


def K_dw_s2_wgrad(nvox, C, epc):
    """dwconv_s2_wgrad_kernel: `per` workgroups per chunk, each adds every per-th active output voxel (product + sum), one flush each"""
    per = min(max(1, 2048 // (C // epc)), nvox)
    return _ceil(nvox, per) + 1 + per


# ---------------------------------------------------------------------------------------------------------------- per-voxel norms
def K_chan_fold(nvox, C, epc, cap):
    """per-channel accumulators of voxel_norm_bwd (cap 1024 workgroups) and scale_residual (cap 2048): a thread adds one voxel of each
    of its workgroup's tiles, the NV voxel lanes are folded in order, ceil(nb / 64) workgroups flush into each of the 64 replicated
    rows, and the rows are summed"""
    nv = 256 // (C // epc)
    ntile = _ceil(nvox, nv)
    nb = min(ntile, cap)
    return _ceil(ntile, nb) + nv + _ceil(nb, LAYER_REP) + LAYER_REP


# worst err / (u S) measured on an MI355X over every case of tests/test_layer_zoo_gpu.py, fp32 storage (bf16 adds the store's half-ulp);
# measured 2.7370, 2.6315, 0.7449, 1.4301, 2.4045, rounded up.  Set an entry to None to measure again (the GPU module then only prints).
K_MEASURED = {"gn_y": 2.74, "gn_dx": 2.64, "gn_dgamma": 0.75, "gelu_y": 1.44, "gelu_dx": 2.41}


def K_meas(name):
    """4 x the measured ratio"""
    assert K_MEASURED[name] is not None, f"{name}: not measured yet"
    return 4.0 * K_MEASURED[name]


def group_norm_ref(x, gamma, beta, groups, eps, mask=None, dy=None):
    """per voxel and channel group: y = (x - mean) rstd gamma + beta, biased variance (groups = 1: LayerNorm over C).  Scales: with
    X = rstd (|x| + mean|x|), S_y = |gamma| X + |beta|; with gg = gamma dy, S_dx = rstd (|gg| + mean|gg| + X mean(|gg| X));
    S_dgamma = sum_v |dy| X, S_dbeta = sum_v |dy|."""
    x0 = _zf(x, mask)
    sh, C = x0.shape[:-1], x0.shape[-1]
    cg = C // groups
    gamma, beta = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    xg = x0.reshape(*sh, groups, cg)
    mean = xg.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((xg - mean) ** 2).mean(-1, keepdims=True) + eps)
    xh = (xg - mean) * rstd
    X = (np.abs(xg) + np.abs(xg).mean(-1, keepdims=True)) * rstd
    out = dict(y=(xh.reshape(x0.shape) * gamma + beta) * _m(mask), S_y=(X.reshape(x0.shape) * np.abs(gamma) + np.abs(beta)) * _m(mask))
    if dy is not None:
        dy0 = _zf(dy, mask)
        gg = (dy0 * gamma).reshape(xg.shape)
        dx = rstd * (gg - gg.mean(-1, keepdims=True) - xh * (gg * xh).mean(-1, keepdims=True))
        Sdx = rstd * (np.abs(gg) + np.abs(gg).mean(-1, keepdims=True) + X * (np.abs(gg) * X).mean(-1, keepdims=True))
        ax = tuple(range(len(sh)))
        out.update(dx=dx.reshape(x0.shape) * _m(mask), S_dx=Sdx.reshape(x0.shape) * _m(mask),
                   dgamma=(dy0 * xh.reshape(x0.shape)).sum(ax), S_dgamma=(np.abs(dy0) * X.reshape(x0.shape)).sum(ax),
                   dbeta=dy0.sum(ax), S_dbeta=np.abs(dy0).sum(ax))
    return out


def grn_ref(x, gamma, beta, mask=None, dy=None, drop_kx=False):
    """sparse GRN: G = |x|_2 over C, n = G / (G + 1e-6), y = gamma x n + beta; dx = gamma n dy + k x with
    k = (sum_c gamma x dy) 1e-6 / ((G + 1e-6)^2 G).  drop_kx: the WRONG gradient without the k x term (for the CPU module)."""
    x0 = _zf(x, mask)
    gamma = np.asarray(gamma, dtype=np.float64)
    beta = np.zeros_like(gamma) if beta is None else np.asarray(beta, dtype=np.float64)
    G = np.sqrt((x0 * x0).sum(-1, keepdims=True))
    n = G / (G + EPS6)
    out = dict(y=(gamma * x0 * n + beta) * _m(mask), S_y=(np.abs(gamma * x0) * n + np.abs(beta)) * _m(mask))
    if dy is not None:
        dy0 = _zf(dy, mask)
        with np.errstate(all="ignore"):
            kk = np.where(G > 0, EPS6 / ((G + EPS6) ** 2) / np.where(G > 0, G, 1.0), 0.0)
        t1 = gamma * n * dy0
        dx = t1 + (0.0 if drop_kx else kk * (gamma * x0 * dy0).sum(-1, keepdims=True) * x0)
        Sdx = np.abs(t1) + kk * np.abs(gamma * x0 * dy0).sum(-1, keepdims=True) * np.abs(x0)
        ax = tuple(range(x0.ndim - 1))
        out.update(dx=dx * _m(mask), S_dx=Sdx * _m(mask), dgamma=(dy0 * x0 * n).sum(ax), S_dgamma=np.abs(dy0 * x0 * n).sum(ax),
                   dbeta=dy0.sum(ax), S_dbeta=np.abs(dy0).sum(ax))
    return out


def _lg(C, epc):
    L = max(1, C // epc)
    return (L - 1).bit_length()


def K_grn(C, epc):
    """roundings of the GRN kernels.  s = sum f^2: epc squares and adds in the thread, lg = log2(P2) tree levels: (epc + lg + 1) u
    relative; G = sqrtf(s) halves that and rounds once: K_G; n = G / (G + 1e-6): the error of G enters n damped (d ln n / d ln G < 1),
    plus the sum and the quotient: K_n = K_G + 2.
      y  = ga (f n) + be                       K_n + 3
      dx = ga n gy + k f, k = S 1e-6 / ((G + 1e-6)^2) / G with S = sum ga f gy: (epc + lg + 2) on S, the product with 1e-6, twice
           (K_G + 1) and the square's own rounding, two quotients with K_G on the last divisor, then k f and the sum:
           K_k = (epc + lg + 2) + 1 + 2 (K_G + 1) + 1 + 2 + K_G + 2; the first term has K_n + 2 < K_k
      dgamma addend gy f n                     K_n + 2, then the accumulator chain (K_chan_fold)"""
    lg = _lg(C, epc)
    K_G = (epc + lg + 1 + 1) // 2 + 1
    K_n = K_G + 2
    return dict(y=K_n + 3, dx=(epc + lg + 2) + 1 + 2 * (K_G + 1) + 1 + 2 + K_G + 2, dgamma_term=K_n + 2)


# ---------------------------------------------------------------------------------------------------------------- pooling
def pool_ref(x, op, k, s, p, cip, m_in=None, m_out_of=None, dy=None):
    """torch's own pooling in fp64 on the zero-filled input, output masked (m_out_of: output extents -> voxel mask or None), and its
    gradient through torch's fp64 graph of that reference.  The maximum is a selection: S_y = 0 (equality, in bf16 too)."""
    xt = torch.from_numpy(np.ascontiguousarray(_zf(x, m_in))).permute(0, 4, 1, 2, 3).requires_grad_(True)

    def run(t):
        return F.max_pool3d(t, k, s, p) if op == "max" else F.avg_pool3d(t, k, s, p, count_include_pad=cip)
    y = run(xt)
    cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).numpy()
    mo = m_out_of(tuple(y.shape[2:])) if m_out_of is not None else None
    out = dict(y=cl(y) * _m(mo), S_y=(np.zeros_like(cl(y)) if op == "max" else cl(run(xt.detach().abs())) * _m(mo)), m_out=mo)
    if dy is not None:
        dy0 = torch.from_numpy(np.ascontiguousarray(_zf(dy, mo))).permute(0, 4, 1, 2, 3)
        dx, = torch.autograd.grad(y, xt, dy0, retain_graph=True)
        Sdx, = torch.autograd.grad(y, xt, dy0.abs())
        out.update(dx=cl(dx) * _m(m_in), S_dx=cl(Sdx) * _m(m_in))
    return out


def K_pool(op, k, s):
    """forward average: k^3 additions and the division.  backward: an input voxel lies in at most ceil(k / s)^3 windows: that many
    additions, and for the average one division per addend (together one more u S)"""
    nwin = _ceil(k, s) ** 3
    return dict(y=0 if op == "max" else k ** 3 + 1, dx=nwin if op == "max" else nwin + 1)


def distinct_values(rs, B, size, C):
    """bf16-representable activations [B, D, H, W, C] whose values are pairwise distinct and nonzero inside every (sample, channel):
    no two elements of any pooling window tie, and none ties with the zero of an inactive voxel"""
    n = int(np.prod(size))
    mant = 1.0 + np.arange(128) / 128.0
    pool = np.concatenate([sg * mant * 2.0 ** e for e in range(-4, 2) for sg in (-1.0, 1.0)])
    assert n <= pool.size and np.unique(pool).size == pool.size and np.array_equal(q_bf16(pool), pool)
    order = np.argsort(rs.rand(B, C, pool.size), axis=-1)[..., :n]
    return np.ascontiguousarray(pool[order].reshape(B, C, *size).transpose(0, 2, 3, 4, 1))


def assert_no_ties(x):
    B, C = x.shape[0], x.shape[-1]
    v = np.sort(x.transpose(0, 4, 1, 2, 3).reshape(B, C, -1), axis=-1)
    assert (np.diff(v, axis=-1) > 0).all() and (x != 0).all()


# ---------------------------------------------------------------------------------------------------------------- pointwise / mean
def gelu_ref(x, mask=None, dy=None):
    """erf form.  S_y = |x| (the factor 0.5 (1 + erf) <= 1 carries erff's ABSOLUTE error), S_dx = |dy| (1 + |x| phi(x))"""
    x0 = _zf(x, mask)
    xt = torch.from_numpy(np.ascontiguousarray(x0))
    cdf = (0.5 * (1.0 + torch.erf(xt / math.sqrt(2.0)))).numpy()
    out = dict(y=x0 * cdf * _m(mask), S_y=np.abs(x0) * _m(mask))
    if dy is not None:
        dy0 = _zf(dy, mask)
        phi = np.exp(-0.5 * x0 * x0) / math.sqrt(2.0 * math.pi)
        out.update(dx=dy0 * (cdf + x0 * phi) * _m(mask), S_dx=np.abs(dy0) * (1.0 + np.abs(x0) * phi) * _m(mask))
    return out


def scale_residual_ref(x, res, gamma, mask=None, dy=None):
    """y = res + gamma x on active voxels, res elsewhere (K = 2: product, sum); dx = gamma dy (K = 1) on active voxels;
    dgamma = sum_v dy x (K = 1 + K_chan_fold)"""
    x0, res, gamma = _zf(x, mask), np.asarray(res, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    out = dict(y=res + gamma * x0, S_y=np.where(_m(mask), np.abs(res) + np.abs(gamma * x0), 0.0))
    if dy is not None:
        dy0 = _zf(dy, mask)
        ax = tuple(range(x0.ndim - 1))
        out.update(dx=gamma * dy0, S_dx=np.abs(gamma * dy0), dgamma=(dy0 * x0).sum(ax), S_dgamma=np.abs(dy0 * x0).sum(ax))
    return out


def masked_mean_ref(x, mask=None, dmean=None):
    """mean[b][c] = sum over the active voxels / (count_b + 1e-6); dx = dmean / (count_b + 1e-6) on the active voxels.
    K_y: a thread adds every 256th voxel, 8 tree levels, count + 1e-6 and the quotient; K_dx = 3 (sum, reciprocal, product)"""
    x0 = _zf(x, mask)
    B, nv = x0.shape[0], int(np.prod(x0.shape[1:4]))
    cnt = (np.full(B, float(nv)) if mask is None else mask.reshape(B, -1).sum(1).astype(np.float64)) + EPS6
    out = dict(y=x0.sum((1, 2, 3)) / cnt[:, None], S_y=np.abs(x0).sum((1, 2, 3)) / cnt[:, None], K_y=_ceil(nv, 256) + 8 + 2, K_dx=3)
    if dmean is not None:
        dx = np.broadcast_to((np.asarray(dmean, dtype=np.float64) / cnt[:, None])[:, None, None, None, :], x0.shape) * _m(mask)
        out.update(dx=dx, S_dx=np.abs(dx))
    return out


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def make_active(rs, B, grid, frac, off=()):
    """patch mask (B, 1, *grid), about `frac` active; patch (0, 0, 0, 0) active, the patches in `off` inactive, both states present"""
    a = rs.rand(B, 1, *grid) < frac
    a[0, 0, 0, 0, 0] = True
    for o in off:
        a[(o[0], 0) + tuple(o[1:])] = False
    flat = a.reshape(-1)
    if flat.all():
        flat[-1] = False
    return a


# name -> B, C, extents, mask grid (None: dense), patches forced inactive.  Bricks are 8 x 8 x 16 voxels.
DW_S1 = {
    "dense_c8": (2, 8, (9, 10, 19), None, ()),              # partial bricks in d, h and w, one 16-byte chunk (bf16) / two (fp32)
    "dense_c24": (2, 24, (9, 10, 19), None, ()),
    "masked_c96": (2, 96, (12, 12, 20), (3, 3, 5), ((0, 2, 2, 4),)),   # bshift 2; brick (1, 1, 1) of sample 0 = patch (2, 2, 4): no active voxel
    "masked_bs0": (2, 8, (5, 6, 9), (5, 6, 9), ()),         # the mask grid is the volume
    "slots_c768": (2, 768, (12, 12, 20), None, ()),         # 16 bricks on nslot = 8 workgroups per chunk: the brick loop, LDS reused
    "slots_c8": (3, 8, (32, 32, 64), None, ()),             # 192 bricks, one workgroup each
}
DW_S2 = {
    "dense_c24": (2, 24, (10, 12, 14), None, ()),
    "masked_c96": (2, 96, (12, 8, 12), (3, 2, 3), ()),      # bshift 2 on the fine side, 1 on the coarse side
    "c768": (1, 768, (8, 8, 8), (2, 2, 2), ()),             # per = 2048 / 96 = 21 workgroups per chunk < active coarse voxels: the e += gridDim.x loop
}


def dw_inputs(table, name, k, s):
    """x, w (random, no symmetry), b, dy, active (patch mask or None), m_in, m_out of a depthwise case"""
    B, C, size, grid, off = table[name]
    rs = _rs("dw", name, k, s)
    osize = tuple(v // s for v in size)
    x = q_bf16(rs.standard_normal((B, *size, C)))
    w = (rs.standard_normal((C, k, k, k)) * (2.0 / k ** 1.5)).astype(np.float32)
    b = (0.5 * rs.standard_normal(C)).astype(np.float32)
    dy = q_bf16(rs.standard_normal((B, *osize, C)))
    active = make_active(rs, B, grid, 0.5 if name in ("masked_bs0", "c768") else 0.4, off) if grid is not None else None
    return dict(x=x, w=w, b=b, dy=dy, active=active, m_in=None if active is None else up(active, size),
                m_out=None if active is None else up(active, osize), B=B, C=C, size=size, osize=osize)


def poison(x, mask):
    """NaN at the inactive voxels: the don't-care bits of the kernels' contract"""
    return x if mask is None else np.where(mask[..., None], x, np.nan)


def vox_inputs(tag, B, C, size, grid, grn=False, frac=0.5):
    """inputs of the per-voxel kernels.  gamma is away from 1, beta away from 0; for GRN the voxels' magnitudes span 1e-5 .. 1: the
    k x term of its gradient is 1e-6 / |x| of the first one, invisible at unit scale"""
    rs = _rs("vox", tag, B, C, size, grid)
    x = rs.standard_normal((B, *size, C))
    if grn:
        x = x * 10.0 ** rs.uniform(-5.0, 0.0, (B, *size, 1))
    active = make_active(rs, B, grid, frac) if grid is not None else None
    return dict(x=q_bf16(x), dy=q_bf16(rs.standard_normal((B, *size, C))), res=q_bf16(rs.standard_normal((B, *size, C))),
                gamma=(1.5 + 0.5 * rs.standard_normal(C)).astype(np.float32), beta=(0.5 * rs.standard_normal(C)).astype(np.float32),
                active=active, mask=None if active is None else up(active, size))


def vox_case(tag, C, grn=False, big=False):
    """the per-voxel cases: 2 x 2 x 2 mask grid, B = 2, about half active; bshift 2 (8^3) below 768 channels, 1 (4^3) from there on.
    big: 4^3 grid at bshift 4, B = 3: > 2^18 active voxels"""
    if big:
        return vox_inputs(tag, 3, C, (64, 64, 64), (4, 4, 4), grn, 0.6)
    n = 8 if C < 768 else 4
    return vox_inputs(tag, 2, C, (n, n, n), (2, 2, 2), grn)


def gelu_inputs():
    """96 channels, x over [-6, 6] with exact zeros among the active voxels"""
    c = dict(vox_case("gelu", 96))
    rs = _rs("gelu-x")
    x = q_bf16(rs.uniform(-6.0, 6.0, c["x"].shape))
    x[rs.rand(*x.shape) < 0.02] = 0.0
    assert (x[c["mask"]] == 0).any() and x.min() < -5.9 and x.max() > 5.9
    c["x"] = x
    return c


def pool_inputs(k, masked):
    """96 channels, B = 2; dense with odd extents (7, 9, 11), or 8^3 on a 2^3 mask grid; values without ties (distinct_values)"""
    rs = _rs("pool", k, masked)
    B, C, size = 2, 96, ((8, 8, 8) if masked else (7, 9, 11))
    x = distinct_values(rs, B, size, C)
    active = make_active(rs, B, (2, 2, 2), 0.5) if masked else None
    return dict(x=x, active=active, m_in=up(active, size) if masked else None, m_out_of=(lambda osz: up(active, osz)) if masked else None,
                dy_of=lambda shape: q_bf16(_rs("pool-dy", k, masked, tuple(shape)).standard_normal(shape)))


# ---------------------------------------------------------------------------------------------------------------- fp32 emulations
def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emu_dwconv(x, w, b, k, s=1, m_in=None, m_out=None, variant=None):
    """dwconv_kernel / dwconv_s2_kernel<MODE 0> in their order: acc = bias, one fma per tap, td outermost.  x may hold NaN at inactive
    voxels.  WRONG variants: mirror (taps mirrored along w), halo (the staged brick one voxel off along w), pad+ / pad- (padding
    k/2 +- 1), no_in_mask (inactive inputs read as stored), no_out_mask (inactive outputs written)."""
    B, D, H, W, C = x.shape
    P = k // 2
    pad = P + {"pad+": 1, "pad-": -1}.get(variant, 0)
    Do, Ho, Wo = D // s, H // s, W // s
    x32 = np.asarray(x).astype(F32)
    if m_in is not None and variant != "no_in_mask":
        x32 = np.where(m_in[..., None], x32, F32(0))
    PP = P + 2
    xp = np.pad(x32, ((0, 0), (PP, PP), (PP, PP), (PP, PP), (0, 0)))
    w32 = np.asarray(w, dtype=F32).reshape(C, k, k, k)
    if variant == "mirror":
        w32 = w32[:, :, :, ::-1]
    acc = np.broadcast_to(np.zeros(C, F32) if b is None else np.asarray(b, dtype=F32), (B, Do, Ho, Wo, C)).copy()
    o = PP - pad
    ow = o + (1 if variant == "halo" else 0)
    for td in range(k):
        for th in range(k):
            for tw in range(k):
                xs = xp[:, o + td:o + td + s * Do:s, o + th:o + th + s * Ho:s, ow + tw:ow + tw + s * Wo:s]
                acc = _fma(np.broadcast_to(w32[:, td, th, tw], xs.shape), xs, acc)
    if m_out is not None and variant != "no_out_mask":
        acc = np.where(m_out[..., None], acc, F32(0))
    return acc


def emu_dwconv_s2_dgrad(dy, w, k, size, m_out=None, m_in=None, variant=None):
    """dwconv_s2_kernel<MODE 1> in gather form: a fine voxel i takes the taps t with (i + P - t) even, from o = (i + P - t) / 2.
    WRONG variant parity: the taps with (i + P - t) ODD (the quotient truncates)."""
    B, Dc, Hc, Wc, C = dy.shape
    P = k // 2
    g32 = np.asarray(dy).astype(F32)
    if m_out is not None:
        g32 = np.where(m_out[..., None], g32, F32(0))
    w32 = np.asarray(w, dtype=F32).reshape(C, k, k, k)
    want = 1 if variant == "parity" else 0

    def pairs(n, nc, t):
        i = np.arange(n)
        num = i + P - t
        ok = (num % 2 == want) & (num >= 0) & (num // 2 < nc)
        return i[ok], (num // 2)[ok]
    acc = np.zeros((B, *size, C), F32)
    for td in range(k):
        fd, cd = pairs(size[0], Dc, td)
        for th in range(k):
            fh, ch = pairs(size[1], Hc, th)
            for tw in range(k):
                fw, cw = pairs(size[2], Wc, tw)
                if not (fd.size and fh.size and fw.size):
                    continue
                fi, ci = np.ix_(fd, fh, fw), np.ix_(cd, ch, cw)
                src = g32[:, ci[0], ci[1], ci[2]]
                wt = np.broadcast_to(w32[:, td, th, tw], src.shape)
                acc[:, fi[0], fi[1], fi[2]] = (acc[:, fi[0], fi[1], fi[2]] + wt * src).astype(F32)
    return acc if m_in is None else np.where(m_in[..., None], acc, F32(0))


def _seq(v):
    """sum over the last axis, left to right in fp32"""
    s = np.zeros(v.shape[:-1], F32)
    for j in range(v.shape[-1]):
        s = s + v[..., j]
    return s


def _seg_sum(vals, L, variant=None):
    """seg_sum of layer_ops.hip on [N, CPV] per-thread values: segments of L consecutive chunks, tree from P2 / 2 down.
    WRONG variants: tree_drop (an odd segment loses its last element), group_shift (segment boundaries one chunk late)."""
    if L == 1:
        return vals
    if variant == "group_shift":
        return np.roll(_seg_sum(np.roll(vals, -1, axis=1), L), 1, axis=1)
    N, cpv = vals.shape
    sm = vals.reshape(N, cpv // L, L).copy()
    lim = L - 1 if (variant == "tree_drop" and L % 2) else L
    s = (1 << (L - 1).bit_length()) >> 1
    while s > 0:
        for pos in range(s):
            if pos + s < lim:
                sm[:, :, pos] = sm[:, :, pos] + sm[:, :, pos + s]
        s >>= 1
    return np.repeat(sm[:, :, 0], L, axis=1)


def emu_group_norm(x, gamma, beta, groups, eps, epc, dy=None, variant=None):
    """voxel_norm_fwd / bwd<VN_GROUP> on the rows [N, C] of the active voxels, fp32, in the kernels' order: the in-chunk branch
    (cg < EPC) sequentially, the segmented one with per-thread partial sums and the seg_sum tree; two-pass biased variance.
    WRONG variants: unbiased (variance over cg - 1), and those of _seg_sum.  Returns y, or (y, dx) with dy."""
    N, C = x.shape
    cg, cpv = C // groups, C // epc
    one, eps32 = F32(1), F32(eps)
    cgf = F32(cg)
    den = F32(cg - 1) if variant == "unbiased" else cgf
    ga, be = np.asarray(gamma, dtype=F32), np.asarray(beta, dtype=F32)
    if cg >= epc:
        f = np.asarray(x).astype(F32).reshape(N, cpv, epc)
        gaf, bef = ga.reshape(cpv, epc), be.reshape(cpv, epc)
        L = cg // epc
        red = lambda v: _seg_sum(_seq(v), L, variant)[..., None]
    else:
        f = np.asarray(x).astype(F32).reshape(N, groups, cg)
        gaf, bef = ga.reshape(groups, cg), be.reshape(groups, cg)
        red = lambda v: _seq(v)[..., None]
    mean = red(f) / cgf
    dlt = f - mean
    rstd = one / np.sqrt(red(dlt * dlt) / den + eps32)
    xh = dlt * rstd
    y = (xh * gaf + bef).reshape(N, C)
    if dy is None:
        return y
    gy = np.asarray(dy).astype(F32).reshape(f.shape)
    gg = gaf * gy
    a = red(gg) / cgf
    bb = red(gg * xh) / cgf
    return y, (rstd * (gg - a - xh * bb)).reshape(N, C)


def emu_grn(x, gamma, beta, epc, dy=None):
    """voxel_norm_fwd / bwd<VN_GRN> on rows [N, C] in fp32"""
    N, C = x.shape
    cpv = C // epc
    f = np.asarray(x).astype(F32).reshape(N, cpv, epc)
    ga, be = np.asarray(gamma, dtype=F32).reshape(cpv, epc), np.asarray(beta, dtype=F32).reshape(cpv, epc)
    e = F32(1e-6)
    G = np.sqrt(_seg_sum(_seq(f * f), cpv))[..., None]
    n = G / (G + e)
    y = (ga * (f * n) + be).reshape(N, C)
    if dy is None:
        return y
    gy = np.asarray(dy).astype(F32).reshape(f.shape)
    S = _seg_sum(_seq(ga * f * gy), cpv)[..., None]
    with np.errstate(all="ignore"):
        kk = np.where(G > 0, S * e / ((G + e) * (G + e)) / G, F32(0)).astype(F32)
    return y, (ga * n * gy + kk * f).reshape(N, C)


def emu_scale_residual_dgamma(x, dy, C, epc, cap=2048):
    """the dgamma fold of scale_residual_kernel<BWD> on the rows [N, C] of the active voxels in walk order: thread (vl, chunk) of
    workgroup blk adds voxel tile * NV + vl of the tiles blk, blk + nb, ...; the NV lanes are folded in order; workgroups flush into
    row blk % 64 (taken in workgroup order here; the atomics' order is free); the 64 rows are summed"""
    N = x.shape[0]
    cpv = C // epc
    nv = 256 // cpv
    ntile = _ceil(N, nv)
    nb = min(ntile, cap)
    rounds = _ceil(ntile, nb)
    pad = rounds * nb * nv - N
    prod = (np.asarray(dy).astype(F32) * np.asarray(x).astype(F32))
    prod = np.concatenate([prod, np.zeros((pad, C), F32)]).reshape(rounds, nb, nv, C)
    ag = np.zeros((nb, nv, C), F32)
    for r in range(rounds):
        ag = ag + prod[r]
    blk = np.zeros((nb, C), F32)
    for q in range(nv):
        blk = blk + ag[:, q]
    rows = np.zeros((LAYER_REP, C), F32)
    for i in range(nb):
        rows[i % LAYER_REP] = rows[i % LAYER_REP] + blk[i]
    return rows.sum(0, dtype=F32)
