"""CPU: the label half of the supervised feed -- the reference of am_resample_labels and the host helpers of anatomask_amd.data.

The reference of the label kernel is stated twice and the two are held against each other here, without a GPU:
 (a) batchgenerators' interpolate_img(is_seg=True) restated over scipy.ndimage.map_coordinates (batchgenerators is not installed):
     order 0: map_coordinates(seg.astype(float), coords, order=0, mode='constant', cval=-1).astype(seg.dtype); another order: result =
     zeros, and for every label c of sorted(unique(seg)): result[map_coordinates((seg == c).astype(float), coords, order,
     mode='constant', cval=-1) >= 0.5] = c.
 (b) the closed form of order 1 in fp64: inside [0, n-1] on every axis, W_c = the sum of the trilinear weights of the (up to 8) corners
     that carry label c; the result is the largest c with W_c >= 0.5, 0 when there is none and 0 outside (every mask is -1 there).
tests/test_label_feed_gpu.py compares the kernel with (b) / scipy on the cases built here; their conditions -- exact coordinates,
coverage of the decisions, size of the excluded bands -- are asserted here from the coordinates and W_c alone, never from a kernel's output.

1. exact coordinates (the construction of tests/test_aug_ops_gpu.py section 2): affine entries k/8, offsets k/64, indices < 32, so the fp32
   coordinates ARE the fp64 ones in any association; source extents 5..11, output extents 6..13 (odd W among them), labels {-1, 0..4}
   in 2^3 blocks and per voxel.  Every trilinear weight is a multiple of 2^-18 and every W_c an exact fp32 number: the >= 0.5 decision
   is exact and no voxel is excluded.  Unit-scale cases with offsets x.5 across label boundaries supply the exact 0.5 / 0.5 ties.
2. the augmenter cases: final 16x16x24 out of 29x27x41, SpatialAugmenter(seed=3, p_rot=1, p_scale=1), six samples, two forced to the
   crop path (all flips / none); labels 0..5 in 4^3 blocks with a slab of -1 (the loader's padding).  delta = 512u * 41/32 (the coordinate
   bound of tests/test_aug_ops_gpu.py section 3); a voxel is excluded where some |W_c - 0.5| < 3 delta + 24u (a coordinate error of delta per
   axis moves a trilinear sum of a 0/1 mask by <= 3 delta; the weights and the 8-term sum add < 24u) or a coordinate lies within delta of
   0 or n-1; order 0: where coord + 0.5 lies within delta of an integer.  At most 0.1 % of a sample, none in the boundary band.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from anatomask_amd import build, data as D, hip
from tests.test_aug_ops_gpu import AUG_ENL, AUG_FINAL, CROP_ALL_FLIPS, CROP_NO_FLIP, DELTA, R_FLIP, R_ROT, U, _aug_bands, _aug_coords, _coords, _exact_affine

REGIONS, N_LABELS = ((1, 2), (2,), 3), 5
NONE = np.iinfo(np.int64).min


# ------------------------------------------------------------------ the two references
def bg_interpolate_seg(seg, coords, order, cval=-1):
    """(a): batchgenerators.augmentations.utils.interpolate_img(seg, coords, order, 'constant', cval, is_seg=True)"""
    if order == 0:
        return ndi.map_coordinates(seg.astype(float), coords, order=0, mode="constant", cval=cval).astype(seg.dtype)
    result = np.zeros(coords.shape[1:], seg.dtype)
    for c in sorted(np.unique(seg)):
        r = ndi.map_coordinates((seg == c).astype(float), coords, order=order, mode="constant", cval=cval)
        result[r >= 0.5] = c
    return result


def closed_form(seg, c):
    """(b) in fp64 -> (labels, corner labels [8, ...], W of each corner's label [8, ...], inside)"""
    n1 = np.array(seg.shape, dtype=np.float64).reshape(3, 1, 1, 1) - 1
    inside = ((c >= 0) & (c <= n1)).all(0)
    cc = np.where(inside, c, 0.0)
    b = np.floor(cc).astype(np.int64)
    f = cc - b
    labs, wts = [], []
    for k in range(8):
        off = (k >> 2, (k >> 1) & 1, k & 1)
        idx = [np.minimum(b[a] + off[a], seg.shape[a] - 1) for a in range(3)]
        labs.append(seg[idx[0], idx[1], idx[2]].astype(np.int64))
        wts.append((f[0] if off[0] else 1 - f[0]) * (f[1] if off[1] else 1 - f[1]) * (f[2] if off[2] else 1 - f[2]))
    labs, wts = np.stack(labs), np.stack(wts)
    sums = np.stack([((labs == labs[k]) * wts).sum(0) for k in range(8)])
    win = np.where(sums >= 0.5, labs, NONE).max(0)
    out = np.where((win == NONE) | ~inside, 0, win)
    return out.astype(seg.dtype), labs, sums, inside


def remove_label(a, remove=(-1, 0)):
    a = a.copy()
    a[a == remove[0]] = remove[1]
    return a


# ------------------------------------------------------------------ 1. exact coordinates
LBL_SHAPES = [((5, 7, 9), (6, 8, 13)), ((11, 6, 8), (7, 9, 11)), ((9, 10, 5), (13, 6, 7)), ((7, 11, 6), (8, 7, 9)), ((8, 5, 11), (10, 12, 6)),
              ((6, 9, 7), (9, 13, 7))]
# unit scale: (sign per axis, fractional offset per axis); the integer part of the offset puts output index 1 (sign +) or n-2 (sign -) on
# source index 0, so that one plane per axis lies outside and, on the axes without a fraction, one lies exactly on the boundary
UNIT = [((1, 1, 1), (0.5, 0, 0)), ((1, -1, 1), (0, 0.5, 0)), ((-1, 1, 1), (0, 0, 0.5)), ((1, 1, -1), (0.5, 0.5, 0)), ((-1, -1, -1), (0.5, 0.5, 0.5)),
        ((1, 1, 1), (0, 0.5, 0.5))]


def _unit_affine(sign, frac, out_shape):
    A = np.zeros((3, 4))
    for d in range(3):
        A[d, d] = sign[d]
        A[d, 3] = (-1.0 if sign[d] > 0 else out_shape[d] - 2.0) - frac[d]
    return A


def _labels(shape, seed, blocky):
    rs = np.random.RandomState(seed)
    if not blocky:
        return rs.randint(-1, 5, size=shape).astype(np.int16)
    coarse = rs.randint(-1, 5, size=[(n + 1) // 2 for n in shape])
    return np.ascontiguousarray(np.kron(coarse, np.ones((2, 2, 2), dtype=np.int64))[:shape[0], :shape[1], :shape[2]].astype(np.int16))


@functools.lru_cache(maxsize=None)
def label_cases():
    """[(seg int16, out_shape, A, coords fp64)] with the exactness and coverage conditions asserted from the coordinates and W_c alone"""
    cases, n_pts = [], 0
    cover = {"outside": 0, "on_boundary": 0, "tie": 0, "none": 0, "minus1": 0, "band": 0, "half": 0}
    affines = [(ss, os_, _exact_affine(R_ROT if i % 2 == 0 else R_FLIP, ss, os_)) for i, (ss, os_) in enumerate(LBL_SHAPES)]
    affines += [(ss, os_, _unit_affine(sg, fr, os_)) for (ss, os_), (sg, fr) in zip(LBL_SHAPES, UNIT)]
    for i, (ss, os_, A) in enumerate(affines):
        assert all(5 <= n <= 11 for n in ss) and all(6 <= n <= 13 for n in os_)
        seg = _labels(ss, 40 + i, blocky=(i % 2 == 1) if i < len(LBL_SHAPES) else (i % 2 == 0))
        assert np.array_equal(A * 64, np.round(A * 64)) and np.array_equal(A[:, :3] * 8, np.round(A[:, :3] * 8)) and max(os_) <= 32
        c = _coords(A, os_)
        for rtl in (False, True):
            assert np.array_equal(_coords(A, os_, np.float32, rtl).astype(np.float64), c), (ss, os_, rtl)
        out, labs, sums, inside = closed_form(seg, c)
        assert np.array_equal(sums * 2 ** 18, np.round(sums * 2 ** 18))                   # every W_c is a multiple of 2^-18: exact in fp32
        n1 = np.array(ss, dtype=np.float64).reshape(3, 1, 1, 1) - 1
        half = sums == 0.5
        hi, lo = np.where(half, labs, NONE).max(0), np.where(half, labs, -NONE - 1).min(0)
        cover["outside"] += int((~inside).sum())
        cover["on_boundary"] += int((inside & ((c == 0) | (c == n1)).any(0)).sum())
        cover["tie"] += int((inside & half.any(0) & (hi != lo)).sum())                     # two labels at exactly 0.5 each
        cover["none"] += int((inside & (sums < 0.5).all(0)).sum())
        cover["minus1"] += int((inside & (out == -1)).sum())
        cover["band"] += int((~inside & ((c >= -0.5) & (c < n1 + 0.5)).all(0)).sum())     # order 0: every rounded index in range
        cover["half"] += int((inside & (c - np.floor(c) == 0.5).any(0)).sum())            # order 0: x.5 -> upwards
        n_pts += inside.size
        cases.append((seg, os_, A, c))
    print(f"label coverage over {n_pts} points in {len(cases)} cases: {cover}")
    assert len(cases) >= 10 and any(os_[2] % 2 for _, os_, _, _ in cases) and any(n % 2 for s, _, _, _ in cases for n in s.shape)
    assert cover["outside"] >= 0.25 * n_pts and cover["on_boundary"] >= 50 and cover["tie"] >= 100 and cover["none"] >= 100, cover
    assert cover["minus1"] >= 20 and cover["band"] >= 20 and cover["half"] >= 100, cover
    return cases


def test_label_cases_are_exact_and_cover_the_decisions():
    assert len(label_cases()) == 2 * len(LBL_SHAPES)


def test_closed_form_equals_the_batchgenerators_loop_at_exact_coordinates():
    for seg, os_, A, c in label_cases():
        want = bg_interpolate_seg(seg, c, 1)
        got = closed_form(seg, c)[0]
        assert np.array_equal(got, want), (seg.shape, os_, int((got != want).sum()))


def test_larger_label_wins_an_exact_tie_and_nothing_gives_zero():
    seg = np.array([[[3, 1], [2, 4]]], dtype=np.int16)
    pts = np.array([[0, 0, 0], [0, 0, 0.5], [0, 0.5, 0], [0, 0.5, 0.5], [0, 0, 1.25]], dtype=np.float64).T.reshape(3, 5, 1, 1)
    want = np.array([3, 3, 3, 0, 0], dtype=np.int16).reshape(5, 1, 1)                   # ties 3|1 and 3|2, four quarters, outside
    assert np.array_equal(closed_form(seg, pts)[0], want) and np.array_equal(bg_interpolate_seg(seg, pts, 1), want)
    seg = np.array([[[-1, 0], [-1, -1]]], dtype=np.int16)
    pts = np.array([[0, 0, 0.5], [0, 1, 0.5]], dtype=np.float64).T.reshape(3, 2, 1, 1)
    want = np.array([0, -1], dtype=np.int16).reshape(2, 1, 1)                           # -1 takes part like any label
    assert np.array_equal(closed_form(seg, pts)[0], want) and np.array_equal(bg_interpolate_seg(seg, pts, 1), want)


# ------------------------------------------------------------------ 2. the augmenter cases
LBL_AUG_SEED = 3
LBL_BAND = 3 * DELTA + 24 * U


def aug_params(order=3):
    aug = D.SpatialAugmenter(AUG_FINAL, seed=LBL_AUG_SEED, p_rot=1.0, p_scale=1.0, order=order)
    params = [aug.draw() for _ in range(6)]
    params[CROP_ALL_FLIPS].update(modified=False, angles=(0.0, 0.0, 0.0), scale=1.0, mirror=[True, True, True])
    params[CROP_NO_FLIP].update(modified=False, angles=(0.0, 0.0, 0.0), scale=1.0, mirror=[False, False, False])
    return aug, params


def aug_labels():
    """(6, 1, *AUG_ENL) int16: labels 0..5 in 4^3 blocks, a slab of -1 on one side (what the loader pads with)"""
    rs = np.random.RandomState(11)
    out = []
    for b in range(6):
        coarse = rs.randint(0, 6, size=[(n + 3) // 4 for n in AUG_ENL])
        seg = np.kron(coarse, np.ones((4, 4, 4), dtype=np.int64))[:AUG_ENL[0], :AUG_ENL[1], :AUG_ENL[2]].astype(np.int16)
        seg[:, :, :9 + b] = -1
        out.append(seg)
    return np.stack(out)[:, None]


@functools.lru_cache(maxsize=None)
def aug_label_reference(order):
    """(params, seg, [(want BEFORE the removal, excluded) per sample]); computed once per order and only read by the tests"""
    _, params = aug_params()
    seg = aug_labels()
    ref = []
    for b, p in enumerate(params):
        if not p["modified"]:
            lb = [(AUG_ENL[d] - AUG_FINAL[d]) // 2 for d in range(3)]
            want = seg[b, 0][tuple(slice(lb[d], lb[d] + AUG_FINAL[d]) for d in range(3))]
            for d in range(3):
                if p["mirror"][d]:
                    want = np.flip(want, axis=d)
            ref.append((np.ascontiguousarray(want), np.zeros(AUG_FINAL, bool)))
            continue
        c = _aug_coords(p)
        edge, tie, _ = _aug_bands(c)
        assert not edge.any(), (b, int(edge.sum()))                   # no voxel in the boundary band
        if order == 0:
            want, excl = bg_interpolate_seg(seg[b, 0], c, 0), edge | tie
        else:
            want, _, sums, _ = closed_form(seg[b, 0], c)
            assert np.array_equal(want, bg_interpolate_seg(seg[b, 0], c, 1)), b
            excl = edge | (np.abs(sums - 0.5) < LBL_BAND).any(0)
        assert excl.mean() <= 1e-3, (b, order, int(excl.sum()))
        ref.append((want, excl))
    return params, seg, ref


def test_label_augmenter_reference_meets_its_conditions_on_the_cpu():
    for order in (0, 1):
        params, seg, ref = aug_label_reference(order)
        assert [p["modified"] for p in params] == [True, False, True, True, False, True]
        print(f"order {order}: excluded per sample {[int(e.sum()) for _, e in ref]} of {int(np.prod(AUG_FINAL))}")
        assert sum(int((w == -1).sum()) for w, _ in ref) >= 20 and len({int(v) for w, _ in ref for v in np.unique(w)}) == 7


# ------------------------------------------------------------------ header and library
def test_header_declares_and_library_exports_am_resample_labels():
    decl = hip.declared_functions()
    assert "am_resample_labels" in decl
    C = ctypes
    assert decl["am_resample_labels"] == [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 4 + \
        [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert hasattr(ctypes.CDLL(build.build(verbose=False)), "am_resample_labels")


# ------------------------------------------------------------------ host helpers
def test_region_lut():
    lut = D.region_lut(REGIONS, N_LABELS)
    assert lut.dtype == torch.int32 and lut.tolist() == [0, 1, 3, 4, 0]
    assert D.region_lut([[0]] * 31 + [0], 1).tolist() == [-1]                            # 32 regions fill the word
    with pytest.raises(ValueError):
        D.region_lut([(1,)] * 33, 5)
    with pytest.raises(ValueError):
        D.region_lut(((1, 5),), 5)
    with pytest.raises(ValueError):
        D.region_lut((-1,), 5)


def test_deep_supervision_targets_equal_scipy_grid_mode_zoom():
    t = torch.from_numpy(np.random.RandomState(5).randint(0, 7, size=(2, 1, 16, 8, 32)).astype(np.int16))
    scales = [[1, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0.125, 0.125, 0.125], [0.5, 0.25, 0.125], 0.5]
    outs = D.deep_supervision_targets(t, scales)
    assert outs[0] is t and len(outs) == len(scales)
    for s, o in zip(scales, outs):
        s3 = s if isinstance(s, list) else [s] * 3
        assert o.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()             # a view: nothing was copied
        for b in range(2):
            want = ndi.zoom(t[b, 0].numpy(), s3, order=0, mode="nearest", grid_mode=True)
            assert np.array_equal(o[b, 0].numpy(), want), s
    for bad in ([[0.75, 0.5, 0.5]], [[2, 1, 1]], [[1 / 3, 1, 1]], [[0.5, 0.5, 1 / 64]], [[0.5, 0.5]]):
        with pytest.raises(NotImplementedError):
            D.deep_supervision_targets(t, bad)
    with pytest.raises(NotImplementedError):
        D.deep_supervision_targets(t[0], [[1, 1, 1]])


def test_paired_augmenter_wants_a_label_table_for_regions():
    with pytest.raises(ValueError):
        D.PairedDeviceAugmenter(D.SpatialAugmenter((8, 8, 8)), regions=REGIONS)
