"""No GPU: that the bounds of tests/test_layer_zoo_gpu.py discriminate.  For every bound of tests/layers_ref.py a correct fp32 evaluation
in the kernel's order (the numpy emulations there; torch's own fp32 CPU layers for pooling, GELU and the mean) stays inside it ON THE
INPUTS THE GPU TESTS USE, and each of the wrong variants named in the ids below breaks it -- so a kernel that made that mistake could
not pass.  No element is left out of any comparison.  The only knife edges of these operations are ties of the maximum (the pooling
inputs have none: asserted here) and nothing else: GELU is smooth."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import layers_ref as R

OK, BAD = "accepted", "rejected"


def ratio(got, ref, S, K, bf16=False):
    return R.worst_ratio(got, ref, R.bound(K, S, ref, bf16))


def verdict(r, expect):
    print(f"error / bound = {r:.4g}: {OK if r <= 1.0 else BAD}")
    assert (r <= 1.0) == (expect == OK), r


@functools.lru_cache(maxsize=None)
def dw_case(table, name, k, s):
    inp = R.dw_inputs(getattr(R, table), name, k, s)
    return inp, R.dwconv_ref(inp["x"], inp["w"], inp["b"], k, s, inp["m_in"], inp["m_out"], inp["dy"])


# ---------------------------------------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize("name,k", [(n, k) for n in ("dense_c8", "dense_c24", "masked_c96", "masked_bs0") for k in (3, 5, 7)] + [("slots_c8", 3)])
def test_depthwise_stride1_emulation_accepted(name, k):
    """forward and data gradient (the same kernel on dy with mirrored taps, no bias), inactive voxels poisoned.  (slots_c768, the
    seventh stride-1 case of the GPU module, has the same K and is left to it: 4.4 M elements per tap.)"""
    inp, ref = dw_case("DW_S1", name, k, 1)
    y = R.emu_dwconv(R.poison(inp["x"], inp["m_in"]), inp["w"], inp["b"], k, 1, inp["m_in"], inp["m_out"])
    verdict(ratio(y, ref["y"], ref["S_y"], R.K_dw(k)), OK)
    verdict(ratio(R.q_bf16(y), ref["y"], ref["S_y"], R.K_dw(k), bf16=True), OK)           # ... and stored as bf16
    verdict(ratio(R.q_bf16(y), ref["y"], ref["S_y"], R.K_dw(k)), BAD)                     # (which the fp32 bound does not allow)
    wf = inp["w"].reshape(-1, k ** 3)[:, ::-1].reshape(inp["w"].shape)
    if (name, k) != ("masked_c96", 7):                                                      # (2 s more for nothing new)
        dx = R.emu_dwconv(R.poison(inp["dy"], inp["m_out"]), wf, None, k, 1, inp["m_out"], inp["m_in"])
        verdict(ratio(dx, ref["dx"], ref["S_dx"], R.K_dw(k)), OK)


@pytest.mark.parametrize("name,k,variant", [(n, k, v) for n, k in (("dense_c8", 3), ("masked_bs0", 5), ("masked_c96", 3))
                                            for v in ("mirror", "halo", "pad+", "pad-", "no_in_mask", "no_out_mask") if n != "dense_c8" or "mask" not in v])
def test_depthwise_stride1_wrong_variant_rejected(name, k, variant):
    inp, ref = dw_case("DW_S1", name, k, 1)
    y = R.emu_dwconv(R.poison(inp["x"], inp["m_in"]), inp["w"], inp["b"], k, 1, inp["m_in"], inp["m_out"], variant)
    verdict(ratio(y, ref["y"], ref["S_y"], R.K_dw(k)), BAD)
    verdict(ratio(y, ref["y"], ref["S_y"], R.K_dw(k), bf16=True), BAD)          # the wider bf16 bound rejects it too


@pytest.mark.parametrize("name,k", [(n, k) for n in ("dense_c24", "masked_c96") for k in (3, 5, 7)] + [("c768", 5)])
def test_depthwise_stride2_emulation_accepted(name, k):
    inp, ref = dw_case("DW_S2", name, k, 2)
    y = R.emu_dwconv(R.poison(inp["x"], inp["m_in"]), inp["w"], inp["b"], k, 2, inp["m_in"], inp["m_out"])
    verdict(ratio(y, ref["y"], ref["S_y"], R.K_dw(k)), OK)
    dx = R.emu_dwconv_s2_dgrad(R.poison(inp["dy"], inp["m_out"]), inp["w"], k, inp["size"], inp["m_out"], inp["m_in"])
    verdict(ratio(dx, ref["dx"], ref["S_dx"], R.K_dw_s2_dgrad(k)), OK)


@pytest.mark.parametrize("name,k", [("dense_c24", 3), ("dense_c24", 5), ("masked_c96", 3)])
def test_depthwise_stride2_inverted_parity_rejected(name, k):
    inp, ref = dw_case("DW_S2", name, k, 2)
    dx = R.emu_dwconv_s2_dgrad(R.poison(inp["dy"], inp["m_out"]), inp["w"], k, inp["size"], inp["m_out"], inp["m_in"], "parity")
    verdict(ratio(dx, ref["dx"], ref["S_dx"], R.K_dw_s2_dgrad(k), bf16=True), BAD)
    for variant in ("mirror", "pad+") + (("no_in_mask", "no_out_mask") if inp["m_in"] is not None else ()):      # the forward's taps
        y = R.emu_dwconv(R.poison(inp["x"], inp["m_in"]), inp["w"], inp["b"], k, 2, inp["m_in"], inp["m_out"], variant)
        verdict(ratio(y, ref["y"], ref["S_y"], R.K_dw(k), bf16=True), BAD)


def test_weight_gradient_bounds_stay_below_the_gradient():
    """K_dw_wgrad / K_dw_s2_wgrad count the longest chain of roundings, not the number of voxels: on every case of the GPU module the
    bound stays under 1 % of the typical |dw|, so a wrong tap (an error of the size of dw itself) cannot hide in it"""
    for table, name, k, s in [("DW_S1", "dense_c8", 3, 1), ("DW_S1", "masked_c96", 5, 1), ("DW_S1", "slots_c8", 3, 1), ("DW_S2", "dense_c24", 7, 2),
                              ("DW_S2", "masked_c96", 5, 2)]:
        inp, ref = dw_case(table, name, k, s)
        for epc in (4, 8):
            if s == 1:
                K = R.K_dw_wgrad(k, inp["B"], *inp["size"], inp["C"], epc)
            else:
                K = R.K_dw_s2_wgrad(int(inp["m_out"].sum()) if inp["m_out"] is not None else inp["B"] * int(np.prod(inp["osize"])), inp["C"], epc)
            b = R.bound(K, ref["S_dw"])
            assert b.max() <= 0.01 * np.sqrt((ref["dw"] ** 2).mean()), (name, k, K)
            mirrored = ref["dw"][:, :, :, ::-1]                                 # the gradient of the taps mirrored along w
            verdict(ratio(mirrored, ref["dw"], ref["S_dw"], K), BAD)
    assert R.K_dw_wgrad(3, 2, 12, 12, 20, 768, 8) == 2 * 10 * 4 + 4 * 7 + 8      # two bricks per workgroup, 8 flushes
    assert R.dw_nslot(192, 8, 8) == 192 and R.dw_nslot(192, 8, 4) == 192        # one brick per workgroup


# ---------------------------------------------------------------------------------------------------------------- per-voxel norms
def rows(c, *names):
    m = c["mask"]
    return [np.asarray(c[n])[m] for n in names]


def rows_of(ref, c, name):
    return ref[name][c["mask"]]


NORMS = [("ln", C, 1, epc) for C in (8, 24, 96, 768, 1024) for epc in (4, 8)] + [("ln", 2048, 1, 8)] + \
        [("gn", C, g, epc) for C, g in ((96, 4), (96, 48), (96, 96), (768, 32)) for epc in (4, 8)]


@functools.lru_cache(maxsize=4)
def norm_case(kind, C, groups):
    c = R.vox_case(kind, C, kind == "grn")
    if kind == "grn":
        return c, R.grn_ref(c["x"], c["gamma"], c["beta"], c["mask"], c["dy"])
    return c, R.group_norm_ref(c["x"], c["gamma"], c["beta"], groups, R.EPS6, c["mask"], c["dy"])


def norm_ratios(kind, C, groups, epc, variant=None, bf16=False):
    c, ref = norm_case(kind, C, groups)
    x, dy = rows(c, "x", "dy")
    y, dx = R.emu_group_norm(x, c["gamma"], c["beta"], groups, R.EPS6, epc, dy, variant)
    return (ratio(y, rows_of(ref, c, "y"), rows_of(ref, c, "S_y"), R.K_meas("gn_y"), bf16),
            ratio(dx, rows_of(ref, c, "dx"), rows_of(ref, c, "S_dx"), R.K_meas("gn_dx"), bf16))


@pytest.mark.parametrize("kind,C,groups,epc", NORMS)
def test_group_norm_emulation_accepted(kind, C, groups, epc):
    ry, rdx = norm_ratios(kind, C, groups, epc)
    verdict(ry, OK); verdict(rdx, OK)


def test_layer_norm_emulation_accepted_on_the_grid_stride_case():
    c = R.vox_case("ln", 8, False, True)
    ref = R.group_norm_ref(c["x"], c["gamma"], c["beta"], 1, R.EPS6, c["mask"], c["dy"])
    x, dy = rows(c, "x", "dy")
    for epc in (4, 8):
        y, dx = R.emu_group_norm(x, c["gamma"], c["beta"], 1, R.EPS6, epc, dy)
        verdict(ratio(y, rows_of(ref, c, "y"), rows_of(ref, c, "S_y"), R.K_meas("gn_y")), OK)
        verdict(ratio(dx, rows_of(ref, c, "dx"), rows_of(ref, c, "S_dx"), R.K_meas("gn_dx")), OK)


@pytest.mark.parametrize("kind,C,groups,epc,variant", [
    ("ln", 8, 1, 4, "unbiased"), ("ln", 96, 1, 8, "unbiased"), ("gn", 96, 48, 8, "unbiased"), ("gn", 96, 4, 8, "unbiased"),
    ("gn", 96, 4, 8, "group_shift"), ("gn", 96, 4, 4, "group_shift"), ("gn", 768, 32, 8, "group_shift"),
    ("ln", 24, 1, 8, "tree_drop"), ("gn", 96, 4, 8, "tree_drop"), ("gn", 768, 32, 8, "tree_drop")])
def test_group_norm_wrong_variant_rejected(kind, C, groups, epc, variant):
    """biased vs unbiased variance; a group boundary one chunk late; the seg_sum tree losing the last element of an odd segment
    (L = 3: 24 channels per group in bf16).  Rejected by the bf16 bound too, forward and data gradient each"""
    ry, rdx = norm_ratios(kind, C, groups, epc, variant, bf16=True)
    verdict(ry, BAD); verdict(rdx, BAD)


GRN = [(C, epc) for C in (8, 24, 96, 768, 1024) for epc in (4, 8)] + [(2048, 8)]


@pytest.mark.parametrize("C,epc", GRN)
def test_grn_emulation_accepted_and_missing_term_rejected(C, epc):
    c, ref = norm_case("grn", C, 1)
    x, dy = rows(c, "x", "dy")
    K = R.K_grn(C, epc)
    y, dx = R.emu_grn(x, c["gamma"], c["beta"], epc, dy)
    verdict(ratio(y, rows_of(ref, c, "y"), rows_of(ref, c, "S_y"), K["y"]), OK)
    verdict(ratio(dx, rows_of(ref, c, "dx"), rows_of(ref, c, "S_dx"), K["dx"]), OK)
    wrong = R.grn_ref(c["x"], c["gamma"], c["beta"], c["mask"], c["dy"], drop_kx=True)      # exact but for the k x term
    verdict(ratio(wrong["dx"], ref["dx"], ref["S_dx"], K["dx"], bf16=True), BAD)


# ---------------------------------------------------------------------------------------------------------------- pointwise, mean
def test_gelu_fp32_accepted_and_tanh_form_rejected():
    c = R.gelu_inputs()
    ref = R.gelu_ref(c["x"], c["mask"], c["dy"])
    x = torch.from_numpy(R._zf(c["x"], c["mask"])).float().requires_grad_(True)
    y = F.gelu(x)
    dx, = torch.autograd.grad(y, x, torch.from_numpy(R._zf(c["dy"], c["mask"])).float())
    verdict(ratio(y.detach().numpy(), ref["y"], ref["S_y"], R.K_meas("gelu_y")), OK)
    verdict(ratio(dx.numpy(), ref["dx"], ref["S_dx"], R.K_meas("gelu_dx")), OK)
    yt = F.gelu(x.detach().double(), approximate="tanh").numpy()
    verdict(ratio(yt, ref["y"], ref["S_y"], R.K_meas("gelu_y"), bf16=True), BAD)


@pytest.mark.parametrize("epc", [4, 8])
@pytest.mark.parametrize("C", [96, 768])
def test_scale_residual_fold_emulation_accepted(C, epc):
    c = R.vox_case("scale", C)
    ref = R.scale_residual_ref(c["x"], c["res"], c["gamma"], c["mask"], c["dy"])
    x, dy = rows(c, "x", "dy")
    dg = R.emu_scale_residual_dgamma(x, dy, C, epc)
    K = 1 + R.K_chan_fold(x.shape[0], C, epc, 2048)
    verdict(ratio(dg, ref["dgamma"], ref["S_dgamma"], K), OK)
    lost = R.emu_scale_residual_dgamma(x[:-1], dy[:-1], C, epc)                  # a fold that loses the last voxel of the tail tile
    verdict(ratio(lost, ref["dgamma"], ref["S_dgamma"], K), BAD)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    y = f32(c["res"]) + f32(c["gamma"]) * f32(R._zf(c["x"], c["mask"]))
    verdict(ratio(y, ref["y"], ref["S_y"], 2), OK)
    verdict(ratio(np.where(c["mask"][..., None], y, 0.0), ref["y"], ref["S_y"], 2, bf16=True), BAD)   # inactive voxels must carry res


def test_masked_mean_fp32_accepted_and_full_count_rejected():
    c = R.vox_case("mean", 96)
    dmean = R.q_bf16(np.random.RandomState(4).standard_normal((2, 96)))
    ref = R.masked_mean_ref(c["x"], c["mask"], dmean)
    x0 = R._zf(c["x"], c["mask"]).astype(np.float32)
    cnt = c["mask"].reshape(2, -1).sum(1).astype(np.float32) + np.float32(1e-6)
    y = x0.reshape(2, -1, 96).sum(1, dtype=np.float32) / cnt[:, None]
    verdict(ratio(y, ref["y"], ref["S_y"], ref["K_y"]), OK)
    verdict(ratio(x0.reshape(2, -1, 96).mean(1), ref["y"], ref["S_y"], ref["K_y"], bf16=True), BAD)      # the mean over ALL voxels


# ---------------------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("op,k,s,p,cip", [("max", 3, 2, 1, True), ("avg", 3, 2, 1, True), ("avg", 3, 2, 1, False), ("max", 7, 1, 3, True)])
def test_pooling_fp32_accepted_no_ties_and_unclipped_divisor_rejected(op, k, s, p, cip, masked):
    c = R.pool_inputs(k, masked)
    R.assert_no_ties(c["x"])
    y0 = R.pool_ref(c["x"], op, k, s, p, cip, c["m_in"], c["m_out_of"])
    dy = c["dy_of"](y0["y"].shape)
    ref = R.pool_ref(c["x"], op, k, s, p, cip, c["m_in"], c["m_out_of"], dy)
    K = R.K_pool(op, k, s)
    xt = torch.from_numpy(R._zf(c["x"], c["m_in"])).float().permute(0, 4, 1, 2, 3).requires_grad_(True)
    y = F.max_pool3d(xt, k, s, p) if op == "max" else F.avg_pool3d(xt, k, s, p, count_include_pad=cip)
    mo = torch.from_numpy(np.ascontiguousarray(ref["m_out"]))[:, None] if masked else torch.ones(())
    y = y * mo
    dx, = torch.autograd.grad(y, xt, torch.from_numpy(R._zf(dy, ref["m_out"])).float().permute(0, 4, 1, 2, 3))
    mi = c["m_in"][..., None] if masked else 1.0
    cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).numpy()
    verdict(ratio(cl(y), ref["y"], ref["S_y"], K["y"]), OK)
    verdict(ratio(cl(dx) * mi, ref["dx"], ref["S_dx"], K["dx"]), OK)
    if op == "avg" and not cip:
        wrong = R.pool_ref(c["x"], op, k, s, p, True, c["m_in"], c["m_out_of"], dy)            # the divisor of the unclipped window, k^3
        verdict(ratio(wrong["y"], ref["y"], ref["S_y"], K["y"], bf16=True), BAD)
        verdict(ratio(wrong["dx"], ref["dx"], ref["S_dx"], K["dx"], bf16=True), BAD)
    if masked:                                                                                  # the input mask forgotten on a window tap
        leak = cl(F.max_pool3d(torch.from_numpy(c["x"]).permute(0, 4, 1, 2, 3), k, s, p) if op == "max" else
                  F.avg_pool3d(torch.from_numpy(c["x"]).permute(0, 4, 1, 2, 3), k, s, p, count_include_pad=cip)) * ref["m_out"][..., None]
        verdict(ratio(leak, ref["y"], ref["S_y"], K["y"], bf16=True), BAD)
