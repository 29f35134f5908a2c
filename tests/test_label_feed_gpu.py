"""GPU: am_resample_labels (csrc/aug_ops.hip) and the paired feed classes of anatomask_amd.data against the references of
tests/test_label_feed_cpu.py (the batchgenerators loop over scipy and its fp64 closed form, held against each other there).  The kernel's
output is integers: every comparison is exact equality, on every voxel at exactly representable coordinates and on every voxel outside
the derived bands for the augmenter draws (the bands and their sizes are conditions of the reference, asserted on the CPU).

1. exact coordinates, 12 cases / 7812 voxels: order 1 == closed form (5102 outside, 516 on a boundary, 516 exact 0.5 / 0.5 ties, 507 where no
   label reaches 0.5, 345 where -1 wins), order 0 == scipy (869 in the half-voxel bands outside, 1672 x.5 ties), each with and without
   the removal of -1, and into a destination that starts 2 bytes off an 8-byte boundary inside a larger buffer whose other elements
   must stay untouched (odd output extents, sizes that are no multiple of the 64-lane wave or of 4).
2. regions: one uint8 plane per region == isin(labels, region), with and without `dst`; -1 (not removed) and labels >= n_lut: no region.
3. PairedDeviceAugmenter: data bitwise DeviceAugmenter's; target exact outside <= 2 of 6144 voxels per sample; crops exact everywhere.
4. argument refusals: -2, nothing written.   5. PairedDeviceFeed.   6. SupervisedFeed.
"""
import ctypes
import itertools
import os
import pickle

import numpy as np
import pytest
import torch

from anatomask_amd import data as D
from tests.test_aug_ops_gpu import AUG_FINAL, _aug_batch
from tests.test_label_feed_cpu import (N_LABELS, REGIONS, aug_label_reference, aug_params, bg_interpolate_seg, closed_form, label_cases,
                                       remove_label)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(seg, os_, A, order, remove, offset=0):
    """ops.resample_labels into a destination `offset` elements into a larger buffer"""
    from anatomask_amd import ops
    n = int(np.prod(os_))
    buf = torch.full((n + 4,), 99, dtype=torch.int16, device=DEV)
    dst = buf[offset:offset + n].view(*os_)
    ops.resample_labels(_dev(seg), dst, A.reshape(-1), order, -1, remove)
    got = buf.cpu().numpy()
    assert (got[:offset] == 99).all() and (got[offset + n:] == 99).all()                  # nothing written around the destination
    return got[offset:offset + n].reshape(os_)


# ------------------------------------------------------------------ 1. exact coordinates
@pytest.mark.parametrize("remove", [(-1, 0), None], ids=["remove", "keep"])
def test_order1_equals_the_closed_form_at_exact_coordinates(remove):
    n_bad = n_all = 0
    for seg, os_, A, c in label_cases():
        want = closed_form(seg, c)[0]
        want = remove_label(want) if remove else want
        for offset in (0, 1):
            got = _run(seg, os_, A, 1, remove, offset)
            bad = got != want
            n_bad, n_all = n_bad + int(bad.sum()), n_all + bad.size
            assert not bad.any(), (seg.shape, os_, offset, int(bad.sum()), c[:, bad][:, :4].T.tolist(), got[bad][:4], want[bad][:4])
    print(f"label order 1 ({'removed' if remove else 'kept'}): {n_bad} of {n_all} voxels differ")


@pytest.mark.parametrize("remove", [(-1, 0), None], ids=["remove", "keep"])
def test_order0_equals_scipy_at_exact_coordinates(remove):
    n_bad = n_all = 0
    for seg, os_, A, c in label_cases():
        want = bg_interpolate_seg(seg, c, 0)
        want = remove_label(want) if remove else want
        for offset in (0, 1):
            got = _run(seg, os_, A, 0, remove, offset)
            bad = got != want
            n_bad, n_all = n_bad + int(bad.sum()), n_all + bad.size
            assert not bad.any(), (seg.shape, os_, offset, int(bad.sum()), c[:, bad][:, :4].T.tolist())
    print(f"label order 0 ({'removed' if remove else 'kept'}): {n_bad} of {n_all} voxels differ")


# ------------------------------------------------------------------ 2. regions
@pytest.mark.parametrize("order", [1, 0])
def test_regions_equal_isin_of_the_labels(order):
    from anatomask_amd import ops
    lut = D.region_lut(REGIONS, N_LABELS).to(DEV)
    for seg, os_, A, c in label_cases():
        raw = closed_form(seg, c)[0] if order else bg_interpolate_seg(seg, c, 0)
        for remove in ((-1, 0), None):
            want = remove_label(raw) if remove else raw
            want_r = np.stack([np.isin(want, r if isinstance(r, tuple) else (r,)) for r in REGIONS]).astype(np.uint8)
            s = _dev(seg)
            dst, reg = torch.empty(os_, dtype=torch.int16, device=DEV), torch.full((3, *os_), 9, dtype=torch.uint8, device=DEV)
            ops.resample_labels(s, dst, A.reshape(-1), order, -1, remove, lut, 3, reg)
            only = torch.full((3, *os_), 9, dtype=torch.uint8, device=DEV)
            ops.resample_labels(s, None, A.reshape(-1), order, -1, remove, lut, 3, only)
            assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(reg.cpu().numpy(), want_r), (seg.shape, os_, remove)
            assert torch.equal(reg, only)
            if remove is None:
                assert (want == -1).any() and not reg.cpu().numpy()[:, want == -1].any()   # -1 belongs to no region


def test_labels_beyond_the_table_belong_to_no_region():
    from anatomask_amd import ops
    table = D.region_lut(((1, 2), (2,), (3, 4)), 5).to(DEV)                                # label 4 has a bit in memory ...
    lut = table[:4]                                                                        # ... but lies beyond the table handed over
    assert table.tolist() == [0, 1, 3, 4, 4] and lut.is_contiguous()
    n4 = 0
    for seg, os_, A, c in label_cases()[:4]:
        want = remove_label(closed_form(seg, c)[0])
        reg = torch.full((3, *os_), 9, dtype=torch.uint8, device=DEV)
        ops.resample_labels(_dev(seg), None, A.reshape(-1), 1, -1, (-1, 0), lut, 3, reg)
        want_r = np.stack([np.isin(want, r) for r in ((1, 2), (2,), (3,))]).astype(np.uint8)
        assert np.array_equal(reg.cpu().numpy(), want_r), (seg.shape, os_)
        n4 += int((want == 4).sum())
    assert n4 >= 20


# ------------------------------------------------------------------ 3. PairedDeviceAugmenter
@pytest.mark.parametrize("order", [1, 0])
def test_paired_augmenter_data_bitwise_and_target_exact_outside_the_bands(order):
    params, seg, ref = aug_label_reference(order)
    aug, _ = aug_params()
    x, s = _dev(_aug_batch(3)), _dev(seg)
    data, target = D.PairedDeviceAugmenter(aug, order_seg=order)(x, s, params)
    assert torch.equal(data, D.DeviceAugmenter(aug)(x, params))
    kept = D.PairedDeviceAugmenter(aug, order_seg=order, remove_label=None)(x, s, params)[1].cpu().numpy()
    regions = D.PairedDeviceAugmenter(aug, order_seg=order, regions=REGIONS, n_labels=N_LABELS)(x, s, params)[1]
    assert target.dtype == torch.int16 and tuple(target.shape) == (6, 1, *AUG_FINAL)
    assert regions.dtype == torch.uint8 and tuple(regions.shape) == (6, 3, *AUG_FINAL)
    target, regions = target.cpu().numpy(), regions.cpu().numpy()
    for b, (want, excl) in enumerate(ref):
        assert params[b]["modified"] or not excl.any()                                     # crops are compared everywhere
        bad_kept, bad = (kept[b, 0] != want) & ~excl, (target[b, 0] != remove_label(want)) & ~excl
        print(f"paired augmenter order {order} sample {b} ({'resampled' if params[b]['modified'] else 'crop'}): {int(bad.sum())} voxels "
              f"differ, {int(excl.sum())} excluded, {int(((target[b, 0] != remove_label(want)) & excl).sum())} of the excluded differ")
        assert not bad.any() and not bad_kept.any(), (order, b, int(bad.sum()), int(bad_kept.sum()))
        for r, members in enumerate(REGIONS):                                              # labels 0..5: label 5 lies beyond the table of 5
            want_r = np.isin(remove_label(want), members if isinstance(members, tuple) else (members,))
            assert np.array_equal(regions[b, r][~excl], want_r[~excl].astype(np.uint8)), (order, b, r)
    assert (target >= 0).all() and (kept == -1).sum() >= 20


def test_paired_augmenter_consumes_the_draws_of_the_data_augmenter_alone():
    _, seg, _ = aug_label_reference(1)
    x, s = _dev(_aug_batch(3)), _dev(seg)
    a, b = D.SpatialAugmenter(AUG_FINAL, seed=21, p_rot=0.5, p_scale=0.5), D.SpatialAugmenter(AUG_FINAL, seed=21, p_rot=0.5, p_scale=0.5)
    data, _ = D.PairedDeviceAugmenter(a)(x, s)
    assert torch.equal(data, D.DeviceAugmenter(b)(x))
    assert all(np.array_equal(u, v) for u, v in zip(a.rs.get_state(), b.rs.get_state()))


# ------------------------------------------------------------------ 4. argument refusals
def test_am_resample_labels_refuses_bad_arguments_without_launching():
    from anatomask_amd import hip, ops
    raw = hip.lib()._lib.am_resample_labels
    src = torch.ones(4, 5, 6, dtype=torch.int16, device=DEV)
    dst = torch.full((3, 4, 5), 123, dtype=torch.int16, device=DEV)
    reg = torch.full((2, 3, 4, 5), 7, dtype=torch.uint8, device=DEV)
    lut = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
    A = (ctypes.c_float * 12)(*np.eye(3, 4).reshape(-1))
    a, st = ctypes.addressof(A), ops._stream()
    s, d, g, t = src.data_ptr(), dst.data_ptr(), reg.data_ptr(), lut.data_ptr()
    ext = [4, 5, 6, 3, 4, 5]

    def call(s_=s, d_=d, e=ext, a_=a, order=1, t_=t, n_regions=2, g_=g):
        return raw(s_, *e[:3], d_, *e[3:], a_, order, -1, -1, 0, t_, 2, n_regions, g_, st)

    assert call(s_=None) == -2 and call(a_=None) == -2 and call(d_=None, g_=None) == -2
    for k in range(6):
        for bad in (0, -3):
            e = list(ext)
            e[k] = bad
            assert call(e=e) == -2, e
    for order in (2, 3, -1):
        assert call(order=order) == -2, order
    for n_regions in (0, -1, 33):
        assert call(n_regions=n_regions) == -2, n_regions
    assert call(t_=None) == -2                                                             # regions_out without region_bits
    torch.cuda.synchronize()
    assert bool((dst == 123).all()) and bool((reg == 7).all()) and bool((src == 1).all())  # nothing ran
    assert call() == 0 and call(d_=None) == 0 and call(g_=None, t_=None, n_regions=0) == 0  # complete arguments are served
    assert bool((dst == 1).all()) and bool((reg == 1).all())
    with pytest.raises(RuntimeError, match="am_resample_labels failed with code -2"):
        ops.resample_labels(src, dst, np.eye(3, 4).reshape(-1), 3)


# ------------------------------------------------------------------ 5. / 6. the feeds
FEED_FINAL, FEED_ENL = (16, 16, 24), (20, 22, 28)


def _seg_of(data):
    """the segmentation of the synthetic cases as a function of their data: a returned pair can be checked voxel by voxel"""
    return np.clip(np.floor(np.abs(data) * 2), 0, 3).astype(np.int16)


def _write_folder(folder, seed=3):
    rs = np.random.RandomState(seed)
    for name, shape in [("c0", (20, 24, 30)), ("c1", (33, 18, 26)), ("c2", (12, 40, 21))]:      # smaller and larger than the crop
        data = rs.standard_normal((1, *shape)).astype(np.float32)
        seg = _seg_of(data)
        np.save(os.path.join(folder, name + ".npy"), data)
        np.save(os.path.join(folder, name + "_seg.npy"), seg)
        with open(os.path.join(folder, name + ".pkl"), "wb") as f:
            pickle.dump({"class_locations": {k: np.argwhere(seg == k)[:64] for k in (1, 2, 3)}}, f)


def _assert_pair(x, s):
    x, s = x.cpu().numpy(), s.cpu().numpy()
    pad = s == -1
    assert np.array_equal(s[~pad], _seg_of(x)[~pad]) and not x[pad].any() and (~pad).any()


def test_paired_feed_keeps_image_and_labels_of_a_crop_together(tmp_path):
    """over a PrefetchLoader with a pinned pool (one loader thread: its batch order is the loader's own)"""
    _write_folder(str(tmp_path))
    ds = D.PreprocessedDataset(str(tmp_path))
    pool = D.PinnedPool((2, 1, *FEED_ENL), n=6)
    pf = D.PrefetchLoader(lambda w: D.PatchLoader3D(ds, 2, FEED_ENL, 0.33, seed=70, final_patch_size=FEED_FINAL, pool=pool), n_workers=1, num_cached=2)
    single = D.PrefetchLoader(lambda w: D.PatchLoader3D(ds, 2, FEED_ENL, 0.33, seed=70, final_patch_size=FEED_FINAL), n_workers=1, num_cached=2)
    feed = None
    try:
        feed, ref = D.PairedDeviceFeed(pf, DEV), D.DeviceFeed(single, DEV)
        n_pad = 0
        for _ in range(6):
            x, s = next(feed)
            assert x.dtype == torch.float32 and s.dtype == torch.int16 and x.is_cuda and s.is_cuda
            assert tuple(x.shape) == tuple(s.shape) == (2, 1, *FEED_ENL)
            _assert_pair(x, s)
            assert torch.equal(x, next(ref))                                               # bitwise what DeviceFeed yields
            n_pad += int((s == -1).sum())
        assert n_pad > 0                                                                   # crops hung over a border: padding was checked
    finally:
        pf.close()
        single.close()
        if feed is not None:
            feed.close()


def test_paired_feed_ends_with_its_iterator_and_returns_every_pool_buffer(tmp_path):
    _write_folder(str(tmp_path))
    ds = D.PreprocessedDataset(str(tmp_path))
    pool = D.PinnedPool((2, 1, *FEED_ENL), n=4)
    batches = itertools.islice(D.PatchLoader3D(ds, 2, FEED_ENL, 0.33, seed=71, final_patch_size=FEED_FINAL, pool=pool), 5)
    feed = D.PairedDeviceFeed(batches, DEV)
    n = 0
    for x, s in feed:
        _assert_pair(x, s)
        n += 1
    assert n == 5
    with pytest.raises(StopIteration):
        next(feed)
    feed.close()
    assert pool.free.qsize() == 4
    # stopped half way: the batch already copied into the other slot is handed back by close() too
    batches = itertools.islice(D.PatchLoader3D(ds, 2, FEED_ENL, 0.33, seed=72, final_patch_size=FEED_FINAL, pool=pool), 5)
    feed = D.PairedDeviceFeed(batches, DEV)
    _assert_pair(*next(feed))
    feed.close()
    assert pool.free.qsize() == 4


def test_supervised_feed_end_to_end(tmp_path):
    _write_folder(str(tmp_path))
    dev = torch.device(DEV)
    feed = D.SupervisedFeed(str(tmp_path), None, 2, FEED_FINAL, dev, 0, 2, True, seed=5)
    with_regions = D.SupervisedFeed(str(tmp_path), None, 2, FEED_FINAL, dev, 0, 2, True, seed=5, regions=REGIONS, n_labels=N_LABELS)
    try:
        seen = set()
        for _ in range(4):
            data, target = next(feed)
            assert data.dtype == torch.float32 and tuple(data.shape) == (2, 1, *FEED_FINAL) and data.is_cuda
            assert target.dtype == torch.int16 and tuple(target.shape) == (2, 1, *FEED_FINAL)
            assert int(target.min()) >= 0 and int(target.max()) <= 3                       # no -1 is left
            seen |= set(target.unique().tolist())
            data, target = next(with_regions)
            assert data.dtype == torch.float32 and tuple(data.shape) == (2, 1, *FEED_FINAL)
            assert target.dtype == torch.uint8 and tuple(target.shape) == (2, 3, *FEED_FINAL) and int(target.max()) <= 1
            assert bool((target[:, 1] <= target[:, 0]).all())                              # region (2,) lies inside region (1, 2)
        assert seen == {0, 1, 2, 3}
        path = str(tmp_path / "state.pt")
        torch.save({"feed_state": feed.state()}, path)
        st = torch.load(path)["feed_state"]                                                # default arguments: weights_only
        assert sorted(st["loader_rng"]) == [0, 1] and st["aug_rng"]["name"] == "MT19937"
        resumed = D.SupervisedFeed(str(tmp_path), None, 2, FEED_FINAL, dev, 0, 2, True, seed=999, state=st)
        try:
            assert [feed.aug.aug.draw() for _ in range(5)] == [resumed.aug.aug.draw() for _ in range(5)]
            data, target = next(resumed)
            assert tuple(data.shape) == (2, 1, *FEED_FINAL) and int(target.min()) >= 0
        finally:
            resumed.close()
    finally:
        feed.close()
        with_regions.close()


def test_supervised_feed_refuses_more_than_one_channel(tmp_path):
    rs = np.random.RandomState(0)
    data = rs.standard_normal((2, 12, 12, 12)).astype(np.float32)
    np.save(str(tmp_path / "m.npy"), data)
    np.save(str(tmp_path / "m_seg.npy"), _seg_of(data[:1]))
    with open(str(tmp_path / "m.pkl"), "wb") as f:
        pickle.dump({"class_locations": {1: np.argwhere(_seg_of(data[:1]) == 1)[:8]}}, f)
    with pytest.raises(NotImplementedError):
        D.SupervisedFeed(str(tmp_path), None, 2, (8, 8, 8), torch.device(DEV), 0, 1, False, seed=0)
