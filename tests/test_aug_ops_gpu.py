"""GPU: the two augmentation kernels of csrc/aug_ops.hip (am_spline_prefilter, am_resample_affine) and DeviceAugmenter against scipy
in fp64 on the CPU, at bounds derived from the arithmetic -- none is taken from the kernels' output.  u = 2^-24 (half an fp32 ulp of 1).
Every test prints its measured maximum beside its bound; the `measured` lines are what MI355X gave.

1. prefilter vs ndi.spline_filter(v64, order=3, mode='mirror'):  max|got - want| <= 64u * max|want|
   per axis the causal and the anticausal recursion each pile up <= ~2.7u of the running magnitude (two roundings per step, geometric
   decay 1 / (1 - |z|), z = sqrt(3) - 2), ~3.7u per axis together, and a later axis amplifies what it is given by <= 3 (sum |h| of the
   inverse filter): worst case ~48u.  Lines of length 1, 2, 3, 4, 5 and 39, 40, 41 on every axis (the causal initialisation is the
   exact mirrored sum up to 40 samples and a truncated one above), more than 256 lines per axis, the production length 205; inputs N(0,1),
   0.1 N + 3 (a mean: the largest relative error) and a +-500 step field.
   measured (worst shape of the 27): N(0,1) 3.27u, 0.1 N + 3 7.98u, step field 4.24u; the slice of a batch 3.09u.  Bound 64u.
2. resampling at exactly representable coordinates (affine entries k/8, offsets k/64, indices < 32: every partial sum of
   a0 d + a1 h + a2 w + a3 is an fp32 number whatever the association or contraction, asserted on the CPU in two association orders), so
   the kernel's coordinates ARE the fp64 ones and no voxel is excluded: the inside / outside decision itself is under test, cval = -7.5.
   orders 1, 3 (the same array as coefficients, prefilter=False):  max|got - want| <= 24u * max|src|
     the weights are >= 0 and sum to 1; three weights at ~3 roundings each, two products and a 64-term accumulation: ~20u.
   order 0:  exact equality, with ties (x.5 -> floor(x + 0.5)) and points in [-0.5, 0) and (n-1, n-0.5), which are OUTSIDE for scipy.
   coverage, asserted from the coordinates alone: >= 400 inside points with mirrored taps (a coordinate < 1 or > n-2), >= 50 exactly on
   0 or n-1, >= 25 % outside, >= 20 in the half-voxel bands at in-range rounded indices (where a test of the rounded index reads data).
   measured (worst of the 10 cases): order 1 0.94u, order 3 1.17u, bound 24u, no inside / outside disagreement; order 0: 0 of 18608
   voxels differ (the rounded-index test of the parent differs in the bands).  The cases hold 2030 mirrored-tap, 268 on-boundary,
   10588 of 18608 outside, 1023 band and 2740 tie points.
3. DeviceAugmenter (final 16x16x24 out of 29x27x41: margins 13, 11, 17, all odd; rotation and scaling on; two of six samples forced to
   the crop path, one with all flips, one with none) with a hard maximum over every voxel but those in a band of delta around a decision:
   delta = 512u * max(enl) / 32 = 656u bounds the fp32 coordinate error: four affine entries rounded to fp32 (<= u each, times an index
   < 32 or, for the offset, half an ulp of a value < 64: 32u each) and six operations (3 products, 3 sums) on values < 64 (32u each),
   10 * 32u = 320u counted, 512u allowed, scaled by max(enl) / 32 for the larger extent.
   excluded: a coordinate within delta of 0 or n-1 (the seed is chosen so that the reference has NO such voxel, asserted); for order 0
   those with coord + 0.5 within delta of an integer (<= 0.1 % of a sample, asserted).
   order 3:  |got - want| <= (64u + 24u) max|c| + L delta     order 1:  24u max|c| + L delta     order 0 and the crops: exact
   c = scipy's fp64 coefficients (the raw volume for order 1), L = sum over the axes of max|c[i+1] - c[i]|, the spline's Lipschitz
   constant; the volume is a low-passed field + 5 % noise so that L delta stays below the arithmetic terms' order of magnitude.
   measured: order 3 max error 2.12e-6 at a bound of 3.78e-4 (43u of max|want|; L delta is 3.7e-4 of the bound, the arithmetic terms
   5e-6), order 1 1.63e-6 at 8.72e-5 (39u), order 0 and the crops 0 voxels differ; 0 voxels in the boundary band, <= 2 of 6144 per
   sample in the tie band, 210 voxels of the four resampled samples in the half-voxel bands.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from anatomask_amd.data import DeviceAugmenter, SpatialAugmenter
from tests import seg_oracle as SO
from tests.test_data_feed import _batchgenerators_coords

gpu = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
PRE_BOUND, RES_BOUND, CVAL = 64 * U, 24 * U, -7.5


# ------------------------------------------------------------------ 1. prefilter
_EDGE_N = (1, 2, 3, 4, 5, 39, 40, 41)
PRE_SHAPES = [s for n in _EDGE_N for s in ((n, 7, 9), (7, n, 9), (7, 9, n))] + [(19, 23, 29), (45, 33, 70), (4, 4, 205)]


def _pre_inputs(shape):
    rs = np.random.RandomState(shape[0] * 10000 + shape[1] * 100 + shape[2])
    coarse = rs.choice([-500.0, 500.0], size=[(n + 2) // 3 for n in shape])
    step = np.kron(coarse, np.ones((3, 3, 3)))[:shape[0], :shape[1], :shape[2]]
    return {"normal": rs.standard_normal(shape).astype(np.float32), "mean3": (0.1 * rs.standard_normal(shape) + 3.0).astype(np.float32),
            "step500": np.ascontiguousarray(step, dtype=np.float32)}


def test_scipy_prefilter_of_short_lines():
    """what the reference does with the lines the kernel special-cases"""
    assert np.array_equal(ndi.spline_filter(np.array([5.0]), order=3, mode="mirror"), [5.0])
    assert np.allclose(ndi.spline_filter(np.array([5.0, 7.0]), order=3, mode="mirror"), [3.0, 9.0], rtol=0, atol=1e-13)


@gpu
@pytest.mark.parametrize("shape", PRE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spline_prefilter_within_64u(shape):
    from anatomask_amd import ops
    for name, v in _pre_inputs(shape).items():
        want = ndi.spline_filter(v.astype(np.float64), order=3, mode="mirror")
        got = ops.spline_prefilter(torch.from_numpy(v.copy()).to(DEV)).cpu().numpy()
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"prefilter {shape} {name}: {err / (U * scale):.2f}u (bound 64u)")
        assert err <= PRE_BOUND * scale, (shape, name, err / (U * scale))


@gpu
def test_spline_prefilter_in_place_on_a_batch_slice():
    from anatomask_amd import ops
    x = np.random.RandomState(7).standard_normal((3, 1, 12, 14, 16)).astype(np.float32)
    t = torch.from_numpy(x.copy()).to(DEV)
    ops.spline_prefilter(t[1, 0])
    got = t.cpu().numpy()
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[2])
    want = ndi.spline_filter(x[1, 0].astype(np.float64), order=3, mode="mirror")
    err, scale = np.abs(got[1, 0] - want).max(), np.abs(want).max()
    print(f"prefilter on x[1, 0] of (3,1,12,14,16): {err / (U * scale):.2f}u (bound 64u)")
    assert err <= PRE_BOUND * scale


# ------------------------------------------------------------------ 2. resampling at exact coordinates
R_ROT = np.array([[0.75, -0.5, 0.25], [0.5, 0.875, -0.125], [-0.25, 0.375, 1.0]])
R_FLIP = np.array([[-0.75, 0.5, 0.25], [0.5, -0.875, 0.125], [0.25, 0.375, -1.0]])
RES_SHAPES = [((21, 25, 17), (12, 16, 10)), ((9, 6, 30), (16, 16, 16)), ((2, 3, 4), (8, 8, 8)), ((1, 5, 2), (4, 8, 8)), ((33, 7, 12), (20, 9, 14))]


def _exact_affine(R, src_shape, out_shape):
    R = R.copy()
    for d in range(3):
        if src_shape[d] == 1:
            R[d] = 0.0                                               # the only inside coordinate of a length-1 axis is 0
    ctr_in, ctr_out = (np.array(src_shape) - 1) / 2.0, (np.array(out_shape) - 1) / 2.0
    return np.concatenate([R, (np.round(64.0 * (ctr_in - R @ ctr_out)) / 64.0)[:, None]], axis=1)


def _coords(A, out_shape, dtype=np.float64, right_to_left=False):
    """A (o, 1) for every output index o, every operation rounded to `dtype`, in one of two association orders"""
    d, h, w = np.meshgrid(*[np.arange(n, dtype=dtype) for n in out_shape], indexing="ij")
    A = A.astype(dtype)
    if right_to_left:
        return np.stack([a[0] * d + (a[1] * h + (a[2] * w + a[3])) for a in A])
    return np.stack([((a[0] * d + a[1] * h) + a[2] * w) + a[3] for a in A])


@functools.lru_cache(maxsize=None)
def _res_cases():
    """[(src fp32, out_shape, A, coords fp64)], with the exactness and coverage conditions asserted from the coordinates alone"""
    cases, n_pts = [], 0
    cover = {"mirrored": 0, "on_boundary": 0, "outside": 0, "band": 0, "tie": 0}
    for i, (ss, os_) in enumerate(RES_SHAPES):
        src = np.random.RandomState(20 + i).standard_normal(ss).astype(np.float32)
        for R in (R_ROT, R_FLIP):
            A = _exact_affine(R, ss, os_)
            assert np.array_equal(A * 64, np.round(A * 64)) and np.array_equal(A[:, :3] * 8, np.round(A[:, :3] * 8)) and max(os_) <= 32
            c = _coords(A, os_)
            for rtl in (False, True):
                assert np.array_equal(_coords(A, os_, np.float32, rtl).astype(np.float64), c), (ss, os_, rtl)
            n1 = np.array(ss, dtype=np.float64).reshape(3, 1, 1, 1) - 1
            inside = ((c >= 0) & (c <= n1)).all(0)
            cover["mirrored"] += int((inside & ((c < 1) | (c > n1 - 1)).any(0)).sum())
            cover["on_boundary"] += int((inside & ((c == 0) | (c == n1)).any(0)).sum())
            cover["outside"] += int((~inside).sum())
            cover["band"] += int((~inside & ((c >= -0.5) & (c < n1 + 0.5)).all(0)).sum())     # every rounded index in range
            cover["tie"] += int((inside & (c - np.floor(c) == 0.5).any(0)).sum())
            n_pts += inside.size
            cases.append((src, os_, A, c))
    print(f"resample coverage over {n_pts} points: {cover}")
    assert cover["mirrored"] >= 400 and cover["on_boundary"] >= 50 and cover["outside"] >= 0.25 * n_pts and cover["band"] >= 20, cover
    assert cover["tie"] >= 20, cover
    return cases


def test_resample_cases_are_exact_and_cover_the_edges():
    assert len(_res_cases()) == 2 * len(RES_SHAPES)


def test_scipy_nearest_rejects_the_half_voxel_bands():
    got = ndi.map_coordinates(np.array([10.0, 20, 30, 40]), [[-0.3, 3.3, 0.5, 1.5, 3.0]], order=0, mode="constant", cval=-1.0)
    assert np.array_equal(got, [-1, -1, 20, 30, 40])


@gpu
@pytest.mark.parametrize("order", [1, 3])
def test_resample_affine_exact_coordinates_within_24u(order):
    from anatomask_amd import ops
    worst = 0.0
    for src, os_, A, c in _res_cases():
        want = ndi.map_coordinates(src.astype(np.float64), c, order=order, mode="constant", cval=CVAL, prefilter=False)
        got = ops.resample_affine(torch.from_numpy(src).to(DEV), torch.empty(os_, device=DEV), A.reshape(-1), order, CVAL).cpu().numpy()
        err, scale = np.abs(got - want).max(), np.abs(src).max()
        n_disagree = int(((got == np.float32(CVAL)) != (want == CVAL)).sum())
        print(f"resample order {order} {src.shape}->{os_}: {err / (U * scale):.2f}u (bound 24u), {n_disagree} inside/outside disagreements")
        assert err <= RES_BOUND * scale, (order, src.shape, os_, err / (U * scale), n_disagree)
        worst = max(worst, err / (U * scale))
    print(f"resample order {order}: worst {worst:.2f}u")


@gpu
def test_resample_affine_order0_equals_scipy_exactly():
    from anatomask_amd import ops
    for src, os_, A, c in _res_cases():
        want = ndi.map_coordinates(src.astype(np.float64), c, order=0, mode="constant", cval=CVAL)
        got = ops.resample_affine(torch.from_numpy(src).to(DEV), torch.empty(os_, device=DEV), A.reshape(-1), 0, CVAL).cpu().numpy()
        bad = got.astype(np.float64) != want
        print(f"resample order 0 {src.shape}->{os_}: {int(bad.sum())} of {bad.size} voxels differ")
        assert not bad.any(), (src.shape, os_, int(bad.sum()), c[:, bad][:, :4].T.tolist())


# ------------------------------------------------------------------ 3. DeviceAugmenter
AUG_FINAL, AUG_ENL, AUG_SEED = (16, 16, 24), (29, 27, 41), 9
DELTA = 512 * U * max(AUG_ENL) / 32
CROP_ALL_FLIPS, CROP_NO_FLIP = 1, 4


def _aug_params(seed=AUG_SEED, order=3):
    aug = SpatialAugmenter(AUG_FINAL, seed=seed, p_rot=1.0, p_scale=1.0, order=order)
    params = [aug.draw() for _ in range(6)]
    params[CROP_ALL_FLIPS].update(modified=False, angles=(0.0, 0.0, 0.0), scale=1.0, mirror=[True, True, True])
    params[CROP_NO_FLIP].update(modified=False, angles=(0.0, 0.0, 0.0), scale=1.0, mirror=[False, False, False])
    return aug, params


def _aug_batch(seed):
    rs = np.random.RandomState(seed)
    return np.stack([SO.smooth_input(AUG_ENL, seed * 16 + b).numpy().astype(np.float64) + 0.05 * rs.standard_normal(AUG_ENL)
                     for b in range(6)])[:, None].astype(np.float32)


def _aug_coords(p):
    """source coordinate of every OUTPUT voxel: batchgenerators' mesh, then MirrorTransform on the output array"""
    c = _batchgenerators_coords(AUG_FINAL, AUG_ENL, p)
    for d in range(3):
        if p["mirror"][d]:
            c = np.flip(c, axis=d + 1)
    return np.ascontiguousarray(c)


def _aug_bands(c):
    """(within delta of 0 or n-1 on an axis, coord + 0.5 within delta of an integer on an axis, outside but every rounded index in range)"""
    n1 = np.array(AUG_ENL, dtype=np.float64).reshape(3, 1, 1, 1) - 1
    edge = ((np.abs(c) <= DELTA) | (np.abs(c - n1) <= DELTA)).any(0)
    tie = (np.abs(c + 0.5 - np.round(c + 0.5)) <= DELTA).any(0)
    inside = ((c >= 0) & (c <= n1)).all(0)
    return edge, tie, ~inside & ((c >= -0.5) & (c < n1 + 0.5)).all(0)


@functools.lru_cache(maxsize=None)
def _aug_reference(order):
    """(params, x fp32, [(want fp64, excluded, bound) per sample]); computed once per order and only read by the tests"""
    _, params = _aug_params(order=order)
    x = _aug_batch(3)
    ref, n_half = [], 0
    for b, p in enumerate(params):
        if not p["modified"]:
            lb = [(AUG_ENL[d] - AUG_FINAL[d]) // 2 for d in range(3)]                      # get_lbs_for_center_crop
            want = x[b, 0][tuple(slice(lb[d], lb[d] + AUG_FINAL[d]) for d in range(3))]
            for d in range(3):
                if p["mirror"][d]:
                    want = np.flip(want, axis=d)
            ref.append((want.astype(np.float64), np.zeros(AUG_FINAL, bool), 0.0))
            continue
        c = _aug_coords(p)
        edge, tie, half = _aug_bands(c)
        assert not edge.any(), (b, int(edge.sum()))                  # the seed keeps the reference clear of the boundary band
        x64 = x[b, 0].astype(np.float64)
        coef = ndi.spline_filter(x64, order=3, mode="mirror") if order == 3 else x64
        want = ndi.map_coordinates(x64, c, order=order, mode="constant", cval=0.0)
        excl = edge | tie if order == 0 else edge
        assert excl.mean() <= 1e-3, (b, excl.mean())
        lip = sum(float(np.abs(np.diff(coef, axis=d)).max()) for d in range(3))
        bound = 0.0 if order == 0 else ((64 * U if order == 3 else 0.0) + 24 * U) * float(np.abs(coef).max()) + lip * DELTA
        n_half += int((half & ~excl).sum())
        ref.append((want, excl, bound))
    assert n_half >= 20, n_half                                      # enough voxels where only the coordinate test gives cval
    return params, x, ref


def test_augmenter_reference_meets_its_conditions_on_the_cpu():
    for order in (0, 1, 3):
        params, _, ref = _aug_reference(order)
        assert [p["modified"] for p in params] == [True, False, True, True, False, True]
        assert all(np.isfinite(w).all() for w, _, _ in ref)


@gpu
@pytest.mark.parametrize("order", [3, 1, 0])
def test_device_augmenter_hard_maximum(order):
    params, x, ref = _aug_reference(order)
    aug, _ = _aug_params(order=order)
    out = DeviceAugmenter(aug)(torch.from_numpy(x).to(DEV), params).cpu().numpy().astype(np.float64)
    for b, (want, excl, bound) in enumerate(ref):
        err = np.abs(out[b, 0] - want)[~excl]
        if params[b]["modified"] and order:
            cmax = float(np.abs(want).max())
            print(f"augmenter order {order} sample {b}: max err {err.max():.3e} (bound {bound:.3e}, = {err.max() / bound:.3f} of it; "
                  f"{err.max() / (U * cmax):.1f}u of max|want|), {int(excl.sum())} voxels excluded")
            assert err.max() <= bound, (order, b, err.max(), bound)
        else:
            print(f"augmenter order {order} sample {b} ({'nearest' if params[b]['modified'] else 'crop'}): {int((err != 0).sum())} voxels "
                  f"differ, {int(excl.sum())} excluded")
            assert err.max() == 0.0, (order, b, int((err != 0).sum()))


@gpu
def test_device_augmenter_scratch_reuse_is_bitwise_a_fresh_instance():
    aug, params = _aug_params(order=3)
    x1, x2 = torch.from_numpy(_aug_batch(3)).to(DEV), torch.from_numpy(_aug_batch(4)).to(DEV)
    used = DeviceAugmenter(aug)
    first = used(x1, params).clone()
    second = used(x2, params)
    fresh = DeviceAugmenter(aug)(x2, params)
    assert torch.equal(second, fresh) and not torch.equal(first, second)


# ------------------------------------------------------------------ 5. argument checks
@gpu
def test_resample_affine_refuses_order_2():
    from anatomask_amd import ops
    with pytest.raises(RuntimeError, match="am_resample_affine"):
        ops.resample_affine(torch.zeros(4, 4, 4, device=DEV), torch.empty(4, 4, 4, device=DEV), np.eye(3, 4).reshape(-1), 2)


@gpu
def test_entry_points_refuse_null_pointers_and_empty_extents_without_launching():
    from anatomask_amd import hip, ops
    raw = hip.lib()._lib
    src = torch.ones(4, 5, 6, device=DEV)
    dst = torch.full((3, 4, 5), 123.0, device=DEV)
    A = (ctypes.c_float * 12)(*np.eye(3, 4).reshape(-1))
    a, st = ctypes.addressof(A), ops._stream()
    s, d = src.data_ptr(), dst.data_ptr()
    assert raw.am_resample_affine(None, 4, 5, 6, d, 3, 4, 5, a, 1, 0.0, st) == -2
    assert raw.am_resample_affine(s, 4, 5, 6, None, 3, 4, 5, a, 1, 0.0, st) == -2
    assert raw.am_resample_affine(s, 4, 5, 6, d, 3, 4, 5, None, 1, 0.0, st) == -2
    for k in range(6):
        for bad in (0, -3):
            ext = [4, 5, 6, 3, 4, 5]
            ext[k] = bad
            assert raw.am_resample_affine(s, *ext[:3], d, *ext[3:], a, 0, 0.0, st) == -2, ext
    assert raw.am_spline_prefilter(None, 4, 5, 6, st) == -1
    assert raw.am_spline_prefilter(s, 4, 0, 6, st) == -1
    torch.cuda.synchronize()
    assert bool((dst == 123.0).all()) and bool((src == 1.0).all())                       # nothing ran
    assert raw.am_resample_affine(s, 4, 5, 6, d, 3, 4, 5, a, 1, 0.0, st) == 0            # the same arguments, complete, are served
    assert bool((dst == 1.0).all())
