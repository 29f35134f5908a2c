"""GPU: every kernel of the sparse layer zoo (csrc/layer_ops.hip) through the public modules / autograd Functions of
anatomask_amd/sparse_layers.py, against the fp64 references and K u S bounds of tests/layers_ref.py, in fp32 and in bf16 storage,
forward and every gradient -- at the widths the backbones have (96 .. 768 channels: 16-byte chunks per voxel that do not divide 256,
idle lanes, ragged folds), the limits (2048 bf16 / 1024 fp32 channels), depthwise k = 5, ragged and multiple bricks, the brick / voxel
loops of the weight gradients, and the grid-stride loop of the norm backward.

Common to every case: the inactive voxels of x and of the upstream gradient hold NaN (the kernels' contract: don't-care bits, read
as 0; the reference uses zeros), y and dx must be EXACTLY 0 at inactive voxels (their bound is 0 there), forward and data gradients
must be bit-equal across two runs (weight gradients go through atomics and are exempt).  tests/test_layer_zoo_cpu.py shows that
every bound used here is met by a correct fp32 evaluation of these very inputs and broken by the wrong variants it lists.

LAYER_ZOO_REPORT=<path> writes the worst error / bound ratio per kernel family and storage type, and the measured err / (u S) behind
the 4 x measured tolerances (layers_ref.K_MEASURED), as JSON."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import layers_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [torch.float32, torch.bfloat16]
RATIOS, MEAS = {}, {}


@pytest.fixture(scope="module")
def SL():
    from anatomask_amd import modules, sparse_layers
    yield sparse_layers
    modules._cur_active = None
    if os.environ.get("LAYER_ZOO_REPORT"):
        with open(os.environ["LAYER_ZOO_REPORT"], "w") as f:
            json.dump({"error_over_bound": {f"{k[0]}.{k[1]}": v for k, v in sorted(RATIOS.items())}, "measured_err_over_uS": MEAS}, f, indent=1)


def set_active(active):
    from anatomask_amd import modules
    modules._cur_active = None if active is None else torch.from_numpy(np.ascontiguousarray(active)).to(DEV)


def dev(a, dtype):
    """channels-last array -> device tensor in the storage type (the values are bf16-representable: nothing is rounded here)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dtype)


def nc(t):
    return t.permute(0, 4, 1, 2, 3)


def cl(t):
    return t.permute(0, 2, 3, 4, 1)


def check(fam, got, ref, S, K, dtype, meas=None, acc=False):
    """|got - ref| <= K u S (+ the bf16 store; acc: an fp32 accumulator in both modes); meas: K is 4 x the measured ratio of that name"""
    bf = dtype == torch.bfloat16 and not acc
    g = got.detach().float().cpu().numpy().astype(np.float64).reshape(np.shape(ref))
    if meas is not None:
        if not bf:
            MEAS[meas] = max(MEAS.get(meas, 0.0), R.worst_ratio(g, ref, R.U * np.asarray(S)))
        if R.K_MEASURED[meas] is None:
            print(f"{fam}: measuring {meas}: err / (u S) = {MEAS.get(meas)}")
            return
        K = R.K_meas(meas)
    r = R.worst_ratio(g, ref, R.bound(K, S, ref, bf))
    key = (fam, "bf16" if dtype == torch.bfloat16 else "fp32")
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"{fam} {key[1]}: K = {K:g}, error / bound = {r:.4f}")
    assert r <= 1.0, (fam, key[1], K, r)


def twice(run):
    """run() -> (y, dx, *parameter gradients); forward and data gradient bit-equal across two runs"""
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "forward / data gradient differ between two runs"
    return a


# ---------------------------------------------------------------------------------------------------------------- depthwise
def dw_case(table, name, k, s):
    """inputs and reference of a depthwise case, shared by the storage types (the 768-channel case runs once and is not kept)"""
    return _dw_case.__wrapped__(table, name, k, s) if "768" in name else _dw_case(table, name, k, s)


@functools.lru_cache(maxsize=None)
def _dw_case(table, name, k, s):
    inp = R.dw_inputs(getattr(R, table), name, k, s)
    return inp, R.dwconv_ref(inp["x"], inp["w"], inp["b"], k, s, inp["m_in"], inp["m_out"], inp["dy"])


def run_dw(SL, table, name, k, s, dtype):
    inp, ref = dw_case(table, name, k, s)
    B, C, size = inp["B"], inp["C"], inp["size"]
    epc = 8 if dtype == torch.bfloat16 else 4
    set_active(inp["active"])
    conv = SL.SparseConv3d(C, C, kernel_size=k, stride=s, padding=k // 2, groups=C).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(inp["w"]).view_as(conv.weight)); conv.bias.copy_(torch.from_numpy(inp["b"]))
    xd, gd = dev(R.poison(inp["x"], inp["m_in"]), dtype), dev(R.poison(inp["dy"], inp["m_out"]), dtype)

    def run():
        conv.zero_grad()
        x = xd.clone().requires_grad_(True)
        y = conv(nc(x))
        assert y.dtype == dtype and tuple(y.shape) == (B, C, *inp["osize"])
        y.backward(nc(gd))
        return cl(y.detach()), x.grad, conv.weight.grad.clone(), conv.bias.grad.clone()
    y, dx, dw, db = twice(run)
    tag = f"dw_s{s}"
    check(tag + "_fwd", y, ref["y"], ref["S_y"], R.K_dw(k), dtype)
    check(tag + "_dgrad", dx, ref["dx"], ref["S_dx"], R.K_dw(k) if s == 1 else R.K_dw_s2_dgrad(k), dtype)
    if s == 1:
        Kw = R.K_dw_wgrad(k, B, *size, C, epc)
    else:
        Kw = R.K_dw_s2_wgrad(int(inp["m_out"].sum()) if inp["m_out"] is not None else B * int(np.prod(inp["osize"])), C, epc)
    check(tag + "_wgrad", dw, ref["dw"], ref["S_dw"], Kw, dtype, acc=True)
    check(tag + "_bgrad", db, ref["db"], ref["S_db"], Kw, dtype, acc=True)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("name", ["dense_c8", "dense_c24", "masked_c96", "masked_bs0"])
def test_depthwise_stride1(SL, name, k, dtype):
    """dense with partial bricks in d, h and w; masked at bshift 2 on a 3 x 3 x 5 grid (12 x 12 x 20: partial bricks, one brick without
    an active voxel); masked with the mask grid at the volume's resolution"""
    if name == "masked_c96":
        a = R.dw_inputs(R.DW_S1, name, k, 1)["m_out"]
        assert not a[0, 8:, 8:, 16:].any() and a[0, :8, :8, :16].any()
    run_dw(SL, "DW_S1", name, k, 1, dtype)


@pytest.mark.parametrize("name,dtype", [("slots_c768", torch.bfloat16), ("slots_c8", torch.float32), ("slots_c8", torch.bfloat16)])
def test_depthwise_weight_gradient_over_many_bricks(SL, name, dtype):
    """C = 768 in bf16: 96 chunks leave nslot = 8 workgroups per chunk for 16 bricks, so every workgroup walks two bricks through the
    same LDS (the `brick += nslot` loop).  C = 8, 192 bricks: launch_dw_wgrad grants 1024 / (C / EPC) slots, so each brick has its own
    workgroup and 192 atomic flushes meet in every element."""
    B, C, size = R.DW_S1[name][:3]
    epc = 8 if dtype == torch.bfloat16 else 4
    nbrick = B * -(-size[0] // 8) * -(-size[1] // 8) * -(-size[2] // 16)
    assert (nbrick > R.dw_nslot(nbrick, C, epc)) == (name == "slots_c768")
    run_dw(SL, "DW_S1", name, 3, 1, dtype)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("name", ["dense_c24", "masked_c96"])
def test_depthwise_stride2(SL, name, k, dtype):
    run_dw(SL, "DW_S2", name, k, 2, dtype)


def test_depthwise_stride2_weight_gradient_voxel_loop(SL):
    """C = 768 in bf16: 21 workgroups per chunk for 32 active coarse voxels: the `e += gridDim.x` loop"""
    inp = R.dw_inputs(R.DW_S2, "c768", 5, 2)
    assert int(inp["m_out"].sum()) > 2048 // (768 // 8)
    run_dw(SL, "DW_S2", "c768", 5, 2, torch.bfloat16)


def test_depthwise_stride2_refused_at_the_mask_resolution(SL):
    set_active(np.ones((1, 1, 4, 4, 4), bool))
    conv = SL.SparseConv3d(8, 8, kernel_size=3, stride=2, padding=1, groups=8).to(DEV)
    with pytest.raises(RuntimeError, match="mask-grid resolution"):
        conv(torch.zeros(1, 8, 4, 4, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- per-voxel norms
@functools.lru_cache(maxsize=2)
def norm_case(kind, C, groups, big):
    c = R.vox_case(kind, C, kind == "grn", big)
    if kind == "grn":
        return c, R.grn_ref(c["x"], c["gamma"], c["beta"], c["mask"], c["dy"])
    return c, R.group_norm_ref(c["x"], c["gamma"], c["beta"], groups, R.EPS6, c["mask"], c["dy"])


def run_norm(SL, kind, C, groups, dtype, big=False):
    c, ref = norm_case(kind, C, groups, big)
    epc = 8 if dtype == torch.bfloat16 else 4
    nvox = int(c["mask"].sum())
    if big:
        assert -(-nvox // (256 // (C // epc))) > 1024                          # voxel_norm_bwd's 1024 workgroups loop over the tiles
    set_active(c["active"])
    if kind == "grn":
        mod = SL.SparseGRN(C).to(DEV)
        pg, pb = mod.gamma, mod.beta
    else:
        mod = (SL.SparseConvNeXtLayerNorm(C, eps=1e-6) if kind == "ln" else SL.SparseGroupNorm(groups, C, eps=1e-6)).to(DEV)
        pg, pb = mod.weight, mod.bias
    with torch.no_grad():
        pg.copy_(torch.from_numpy(c["gamma"]).view_as(pg)); pb.copy_(torch.from_numpy(c["beta"]).view_as(pb))
    xd, gd = dev(R.poison(c["x"], c["mask"]), dtype), dev(R.poison(c["dy"], c["mask"]), dtype)
    ncdhw = kind == "gn"

    def run():
        mod.zero_grad()
        x = xd.clone().requires_grad_(True)
        y = mod(nc(x) if ncdhw else x)
        assert y.dtype == dtype
        y.backward(nc(gd) if ncdhw else gd)
        return (cl(y.detach()) if ncdhw else y.detach()), x.grad, pg.grad.clone().view(-1), pb.grad.clone().view(-1)
    y, dx, dg, db = twice(run)
    Kf = R.K_chan_fold(nvox, C, epc, 1024)
    if kind == "grn":
        K = R.K_grn(C, epc)
        check("grn_fwd", y, ref["y"], ref["S_y"], K["y"], dtype)
        check("grn_dx", dx, ref["dx"], ref["S_dx"], K["dx"], dtype)
        check("grn_dgamma", dg, ref["dgamma"], ref["S_dgamma"], K["dgamma_term"] + Kf, dtype, acc=True)
        check("grn_dbeta", db, ref["dbeta"], ref["S_dbeta"], Kf, dtype, acc=True)
    else:
        check("gn_fwd", y, ref["y"], ref["S_y"], None, dtype, meas="gn_y")
        check("gn_dx", dx, ref["dx"], ref["S_dx"], None, dtype, meas="gn_dx")
        check("gn_dgamma", dg, ref["dgamma"], ref["S_dgamma"], None, dtype, meas="gn_dgamma", acc=True)
        check("gn_dbeta", db, ref["dbeta"], ref["S_dbeta"], Kf, dtype, acc=True)


WIDTHS = [(8, torch.float32), (8, torch.bfloat16), (24, torch.float32), (24, torch.bfloat16), (96, torch.float32), (96, torch.bfloat16),
          (768, torch.float32), (768, torch.bfloat16), (1024, torch.float32), (1024, torch.bfloat16), (2048, torch.bfloat16)]


@pytest.mark.parametrize("C,dtype", WIDTHS)
def test_layer_norm(SL, C, dtype):
    """chunks per voxel 1 .. 256: 24 channels in bf16 = 3 chunks (L = 3, NV = 85, one idle lane, and a tail tile: the voxel count is a multiple of 64), 96 = 12
    (NV = 21, four idle lanes), 768 in bf16 = 96 (NV = 2, 64 idle lanes), 2048 bf16 / 1024 fp32 = 256 (one voxel per workgroup)"""
    if C in (24, 96):
        assert int(R.vox_case("ln", C)["mask"].sum()) % (256 // (C // (8 if dtype == torch.bfloat16 else 4))) != 0     # the last tile is partial
    run_norm(SL, "ln", C, 1, dtype)


@pytest.mark.parametrize("C,dtype", WIDTHS)
def test_grn(SL, C, dtype):
    run_norm(SL, "grn", C, 1, dtype)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,groups", [(96, 4), (96, 48), (96, 96), (768, 32)])
def test_group_norm(SL, C, groups, dtype):
    """24 channels per group (3 chunks in bf16, 6 in fp32), 2 and 1 (inside a chunk), 24 at 768 channels"""
    run_norm(SL, "gn", C, groups, dtype)


@pytest.mark.parametrize("dtype", DT)
def test_group_norm_refuses_three_channels_per_group(SL, dtype):
    """96 channels in 32 groups: 3 channels neither fill nor divide a chunk.  Refused by the wrapper, before any allocation or launch."""
    set_active(np.ones((1, 1, 2, 2, 2), bool))
    with pytest.raises(NotImplementedError, match="3 channels per group"):
        SL.SparseGroupNorm(32, 96).to(DEV)(torch.zeros(1, 96, 4, 4, 4, device=DEV, dtype=dtype))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DT)
def test_layer_norm_grid_stride_loop(SL, dtype):
    run_norm(SL, "ln", 8, 1, dtype, big=True)


# ---------------------------------------------------------------------------------------------------------------- pointwise, mean
@pytest.mark.parametrize("dtype", DT)
def test_gelu(SL, dtype):
    """inputs over [-6, 6] with exact zeros among them; 96 channels"""
    c = R.gelu_inputs()
    x = c["x"]
    ref = R.gelu_ref(x, c["mask"], c["dy"])
    set_active(c["active"])
    mod = SL.SparseGELU()
    xd, gd = dev(R.poison(x, c["mask"]), dtype), dev(R.poison(c["dy"], c["mask"]), dtype)

    def run():
        xx = xd.clone().requires_grad_(True)
        y = mod(nc(xx))
        y.backward(nc(gd))
        return cl(y.detach()), xx.grad
    y, dx = twice(run)
    check("gelu_fwd", y, ref["y"], ref["S_y"], None, dtype, meas="gelu_y")
    check("gelu_dx", dx, ref["dx"], ref["S_dx"], None, dtype, meas="gelu_dx")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", [96, 768])
def test_scale_residual(SL, C, dtype):
    """y = res + gamma x on active voxels and res itself elsewhere; dx = gamma dy; dres = dy; dgamma folded over ragged voxel lanes"""
    c = R.vox_case("scale", C)
    epc = 8 if dtype == torch.bfloat16 else 4
    ref = R.scale_residual_ref(c["x"], c["res"], c["gamma"], c["mask"], c["dy"])
    set_active(c["active"])
    gamma = torch.from_numpy(c["gamma"]).to(DEV).requires_grad_(True)
    xd, rd, gd = dev(R.poison(c["x"], c["mask"]), dtype), dev(c["res"], dtype), dev(R.poison(c["dy"], c["mask"]), dtype)

    def run():
        gamma.grad = None
        xx, rr = xd.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        y = SL._ScaleResidualFn.apply(xx, rr, gamma)
        y.backward(gd)
        m = torch.from_numpy(c["mask"]).to(DEV)
        assert torch.equal(rr.grad[m], gd[m])
        return y.detach(), xx.grad, gamma.grad.clone()
    y, dx, dg = twice(run)
    check("scale_fwd", y, ref["y"], ref["S_y"], 2, dtype)
    check("scale_dx", dx, ref["dx"], ref["S_dx"], 1, dtype)
    check("scale_dgamma", dg, ref["dgamma"], ref["S_dgamma"], 1 + R.K_chan_fold(int(c["mask"].sum()), C, epc, 2048), dtype, acc=True)


@pytest.mark.parametrize("dtype", DT)
def test_masked_mean(SL, dtype):
    c = R.vox_case("mean", 96)
    B, C = c["x"].shape[0], 96
    dmean = R.q_bf16(np.random.RandomState(4).standard_normal((B, C)))
    ref = R.masked_mean_ref(c["x"], c["mask"], dmean)
    set_active(c["active"])
    mod = SL.SparseAdaptiveAvgPooling((1, 1, 1))
    xd, gd = dev(R.poison(c["x"], c["mask"]), dtype), dev(dmean, dtype)

    def run():
        xx = xd.clone().requires_grad_(True)
        y = mod(nc(xx))
        assert tuple(y.shape) == (B, C, 1, 1, 1) and y.dtype == dtype
        y.backward(gd[:, :, None, None, None])
        return y.detach().view(B, C), xx.grad
    y, dx = twice(run)
    check("mean_fwd", y, ref["y"], ref["S_y"], ref["K_y"], dtype)
    check("mean_dx", dx, ref["dx"], ref["S_dx"], ref["K_dx"], dtype)


# ---------------------------------------------------------------------------------------------------------------- pooling
POOLS = [("max", 3, 2, 1, True), ("avg", 3, 2, 1, True), ("avg", 3, 2, 1, False), ("max", 7, 1, 3, True)]


@functools.lru_cache(maxsize=None)
def pool_case(op, k, s, p, cip, masked):
    c = R.pool_inputs(k, masked)
    dy = c["dy_of"](R.pool_ref(c["x"], op, k, s, p, cip, c["m_in"], c["m_out_of"])["y"].shape)
    return c["x"], dy, c["active"], c["m_in"], R.pool_ref(c["x"], op, k, s, p, cip, c["m_in"], c["m_out_of"], dy)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("op,k,s,p,cip", POOLS)
def test_pooling(SL, op, k, s, p, cip, masked, dtype):
    """96 channels; dense with odd extents (7, 9, 11) and masked (8^3 on a 2^3 grid: the strided output sits at bshift 1).  The inputs
    are pairwise distinct inside every (sample, channel): the maximum has no ties, so y is an equality in both storage types"""
    x, dy, active, m_in, ref = pool_case(op, k, s, p, cip, masked)
    set_active(active)
    mod = SL.SparseMaxPooling(k, s, p) if op == "max" else SL.SparseAvgPooling(k, s, p, count_include_pad=cip)
    xd, gd = dev(R.poison(x, m_in), dtype), dev(R.poison(dy, ref["m_out"]), dtype)

    def run():
        xx = xd.clone().requires_grad_(True)
        y = mod(nc(xx))
        assert tuple(cl(y).shape) == ref["y"].shape
        y.backward(nc(gd))
        return cl(y.detach()), xx.grad
    y, dx = twice(run)
    K = R.K_pool(op, k, s)
    check(f"pool_{op}_fwd", y, ref["y"], ref["S_y"], K["y"], dtype)
    check(f"pool_{op}_dx", dx, ref["dx"], ref["S_dx"], K["dx"], dtype)


# ---------------------------------------------------------------------------------------------------------------- limits
def test_channel_limits(SL):
    """fp32 rows end at 1024 channels, bf16 rows at 2048; the entry point refuses (code -1) before it launches anything"""
    set_active(np.ones((1, 1, 2, 2, 2), bool))
    for C, dtype in ((1032, torch.float32), (2056, torch.bfloat16)):
        with pytest.raises(RuntimeError, match="am_voxel_norm_fwd failed with code -1"):
            SL.SparseConvNeXtLayerNorm(C).to(DEV)(torch.zeros(1, 2, 2, 2, C, device=DEV, dtype=dtype))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DT)
def test_depthwise_refuses_partial_chunks_and_unknown_sizes(SL, dtype):
    """SparseConv3d's stride-1 depthwise branch does not look at C % 8: am_dwconv3d itself refuses 12 channels (code -1, nothing is
    launched); k = 9 has no kernel"""
    set_active(None)
    x = torch.zeros(1, 12, 8, 8, 16, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError, match="am_dwconv3d failed with code -1"):
        SL.SparseConv3d(12, 12, kernel_size=3, padding=1, groups=12).to(DEV)(x)
    with pytest.raises(NotImplementedError):
        SL.SparseConv3d(16, 16, kernel_size=9, padding=4, groups=16).to(DEV)(torch.zeros(1, 16, 8, 8, 16, device=DEV, dtype=dtype))
    torch.cuda.synchronize()
