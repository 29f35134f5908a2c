"""GPU: the kernels of one bench.py step at the BENCHMARKED batch -- B = 16, 128^3, bf16 -- against references that share no code with them.

At that batch a level-0 decoder activation [16, 128, 128, 128, 64] is exactly 2^32 bytes: sample 8 starts at byte 2^31 and the element count
no longer fits an int.  The 64-bit parts of the kernels' addressing (the brick origin and the store / residual descriptor offsets of
conv_k3.hip, the per-sample descriptors of conv_wgk3.hip, the plane-anchored ones of conv_wgrad.hip, the voxel offsets of stream_ops.hip)
and the non-temporal stores conv_k3 switches to from 384 MiB of output on are only distinguishable from their 32-bit / plain versions here.

References (none goes through a bf16 or a library fp32 convolution of the whole problem):
  plane reference   fp64, per output sample b and plane d: the three source planes (two coarse planes for the transposed conv), upcast to
                    fp64 on the device, contracted tap by tap with fp64 matmuls (conv_plane_ref / convt_plane_ref; checked on the CPU
                    against torch's fp64 convolutions and autograd by tests/test_bench_batch_refs.py).
                    Planes: samples {0, 7, 8, 15} x planes {0, 7, 8, 63, 64, 127} (brick boundaries, the 2 GiB crossing, both ends).
                    Per plane (a) max error <= TOL[bf16] = 2e-2 of the plane's max, (b) relative L2 <= 1.5 x the SAME kernel's relative L2
                    on the verified small shape (B = 1, 64^3, same channels and input distribution), measured in the same test: rounding
                    statistics of a bf16 store do not depend on the batch; one misplaced 16-voxel row of a 128 x 128 plane adds ~4e-2.
  whole tensor      per sample F.conv3d / F.conv_transpose3d on the device in fp32 (TF32 off) on the upcast operands, 2e-2 of max: the
                    coarse net for a wrong brick anywhere.
  weight gradient   full random operands: per tap and sample X_shifted^T dY as fp32 device matmuls, fp64 accumulation over samples;
                    LOCALISED dY (one plane / one brick non-zero): the fp64 contraction over that region alone -- a skipped or
                    doubly counted region is then the whole signal, not 1 / 2048 of it.
  norms             closed-form normalisation and its backward in torch on the device, fp32 chunks with fp64 reductions.
Which kernel served a launch: am_conv3d_uses_k3 (the predicates conv_k3_launch / conv_k3t_launch decide by: 1 = conv_k3_kernel, 2 = its
transposed instantiation) for every convolution launch, with the options of that launch (fused epilogue, statistics); launches with
statistics also show it in part.rows == 8 x CUs; am_conv3d_wgrad_uses_k3 for the weight gradients; the row-walk norm kernels are the only
ones that accept this geometry (the linear ones return -4).

Skips: only when the device's TOTAL memory is below what a test allocates (never on an MI355X).

Measured on MI355X (every test prints its values; bound in brackets):
  conv_k3, per plane, all of fwd 64->64 / + bn + res + relu6 / + res + lrelu / dgrad 64->64 / fwd 64->32 / + bn + res 64->32 / dgrad 32->64 / convT:
      max err / max 2.6e-3 .. 3.5e-3 [2e-2]; relative L2 1.647e-3 .. 1.672e-3 against 1.650e-3 .. 1.670e-3 on the small shape [1.5 x: 2.48e-3 .. 2.51e-3];
      last sample's last plane 2.5e-3 .. 3.5e-3 / 1.64e-3 .. 1.67e-3; whole tensor, worst sample 2.2e-3 .. 3.7e-3 [2e-2]
  statistics rows: sum 3e-11 .. 2e-9 of the absolute sum, sum of squares 3.7e-6 (dgrad) / 7.2e-6 (64->32) / 8.4e-6 (64->64) [1e-5]; B = 2: 2.5e-7.
      The sum-of-squares error is systematic, not noise: at B = 16 a lane adds 2 048 squares of bf16 values into one fp32 accumulator (8 per
      unit, 256 units per workgroup), and the low bits of such squares are not uniform, so round-to-nearest is biased upwards.  It grows in
      proportion to the batch and stands at 0.84 of the bound at B = 16 (see STATS_TOL).
  weight gradients 64x64 / 64x32, default and deterministic mode: full random 4.7e-6 .. 1.1e-5, worst tap 1.3e-5; localised dY 2.3e-7 .. 3.6e-7,
      worst tap 4.5e-7 [1e-4]; deterministic launches bit-equal
  dense BatchNorm [16,128^3,64]: chan_stats sum 3.3e-10 / sum of squares 1.8e-6 [6.1e-5]; mean 4.2e-8, rstd 1.1e-6 [1.2e-4]; norm_apply 2.6e-3
      [2e-2]; dbeta / dgamma 4.6e-8 / 1.1e-6 of max [4e-2], 2e-11 / 1e-9 of the absolute sums [6.1e-5]; dx 3.2e-3 [4e-2]
  row-walk norm C = 32 / 64, mask 0.6: mean 4.2e-8, rstd 2.3e-7; norm_apply 3.4e-3; dbeta / dgamma 2.2e-7 / 3.8e-7 of max; dx 3.4e-3
  stem conv fp32 k3 / k1: forward 5.0e-7 / 1.2e-7 [2e-4]; weight gradient 9.5e-7 / 7.8e-7, bias gradient 1.1e-6 / 7.3e-7 [5e-4]
  module: 15 tests, 197 s wall time (70 s of it the fp32 device F.conv_transpose3d references), peak device memory 24.5 GiB
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import DEV, K3_CASES, TOL, close, q, rnd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B16 = 16
S128 = (128, 128, 128)
SAMPLES = (0, 7, 8, 15)
PLANES = (0, 7, 8, 63, 64, 127)
FINE_PLANES = (0, 1, 15, 16, 126, 127)
L2_FACTOR = 1.5


@pytest.fixture(scope="module")
def ops():
    from anatomask_amd import ops as _ops
    tf32 = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield _ops
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = tf32
    print(f"\ntest_bench_batch_gpu: wall time {time.time() - t0:.0f} s, peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def need_gib(gib):
    total = torch.cuda.get_device_properties(0).total_memory
    if total < gib * 2 ** 30:
        pytest.skip(f"device has {total / 2 ** 30:.0f} GiB in total, the case allocates {gib} GiB")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev_randn(B, S, C, seed, scale=1.0, shift=0.0):
    """[B, *S, C] bf16 on the device, generated per sample (no host tensor, 4 C S^3 bytes of fp32 scratch)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.empty(B, *S, C, device=DEV, dtype=BF)
    for b in range(B):
        t[b] = (torch.randn(*S, C, device=DEV, generator=g) * scale + shift).to(BF)
    return t


def conv_weight(cout, cin, seed):
    return q(rnd(cout, cin, 3, 3, 3, seed=seed, scale=1.0 / np.sqrt(27 * cin)), BF)


def dgrad_weight(w):
    """the data gradient of a k3 s1 p1 convolution is the convolution with mirrored taps and swapped channels"""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


# ------------------------------------------------------------------ references
def conv_plane_ref(x, w, bias, b, d):
    """fp64 [H, W, Cout]: plane d of sample b of conv3d(x, w, bias, k3 s1 p1); x channels-last [B, D, H, W, Cin], w (Cout, Cin, 3, 3, 3)."""
    _, D, H, W, Cin = x.shape
    w64 = w.to(device=x.device, dtype=torch.float64)
    slab = torch.zeros(3, H + 2, W + 2, Cin, device=x.device, dtype=torch.float64)
    for kd in range(3):
        if 0 <= d + kd - 1 < D:
            slab[kd, 1:-1, 1:-1] = x[b, d + kd - 1].double()
    out = torch.zeros(H * W, w.shape[0], device=x.device, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                out += slab[kd, kh:kh + H, kw:kw + W].reshape(H * W, Cin) @ w64[:, :, kd, kh, kw].t()
    if bias is not None:
        out += bias.to(device=x.device, dtype=torch.float64)
    return out.view(H, W, -1)


def convt_plane_ref(x, w, bias, b, od):
    """fp64 [2H, 2W, Cout]: fine plane od of sample b of conv_transpose3d(x, w, bias, k4 s2 p1) in SCATTER form (every coarse voxel adds
    w[.., k] to fine voxel 2 i - 1 + k); x [B, D, H, W, Cin], w (Cin, Cout, 4, 4, 4)."""
    _, D, H, W, Cin = x.shape
    w64 = w.to(device=x.device, dtype=torch.float64)
    Cout = w.shape[1]
    out = torch.zeros(2 * H + 2, 2 * W + 2, Cout, device=x.device, dtype=torch.float64)      # fine index + 1 (k = 0 of voxel 0 lands on -1)
    for i_d in range(D):
        kd = od + 1 - 2 * i_d
        if not 0 <= kd <= 3:
            continue
        xp = x[b, i_d].double().reshape(H * W, Cin)
        for kh in range(4):
            for kw in range(4):
                out[kh:kh + 2 * H:2, kw:kw + 2 * W:2] += (xp @ w64[:, :, kd, kh, kw]).view(H, W, Cout)
    out = out[1:2 * H + 1, 1:2 * W + 1]
    if bias is not None:
        out = out + bias.to(device=x.device, dtype=torch.float64)
    return out


def wgrad_region_ref(x, dy, b, reg):
    """fp64 (Cy, Cx, 3, 3, 3): sum over the voxels q of region reg = (d0, d1, h0, h1, w0, w1) of sample b of dy[q, cy] x[q + t - 1, cx]."""
    _, D, H, W, Cx = x.shape
    d0, d1, h0, h1, w0, w1 = reg
    nd, nh, nw = d1 - d0, h1 - h0, w1 - w0
    xs = torch.zeros(nd + 2, nh + 2, nw + 2, Cx, device=x.device, dtype=torch.float64)
    sd, sh, sw = max(d0 - 1, 0), max(h0 - 1, 0), max(w0 - 1, 0)
    ed, eh, ew = min(d1 + 1, D), min(h1 + 1, H), min(w1 + 1, W)
    xs[sd - d0 + 1:ed - d0 + 1, sh - h0 + 1:eh - h0 + 1, sw - w0 + 1:ew - w0 + 1] = x[b, sd:ed, sh:eh, sw:ew].double()
    g = dy[b, d0:d1, h0:h1, w0:w1].double().reshape(nd * nh * nw, -1)
    out = torch.zeros(g.shape[1], Cx, 3, 3, 3, device=x.device, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                out[:, :, kd, kh, kw] = g.t() @ xs[kd:kd + nd, kh:kh + nh, kw:kw + nw].reshape(nd * nh * nw, Cx)
    return out


def wgrad_full_ref(x, dy):
    """fp64 (Cy, Cx, 3, 3, 3): per tap and sample X_shifted^T dY as fp32 matmuls on the upcast operands, summed over samples in fp64."""
    B, D, H, W, Cx = x.shape
    out = torch.zeros(dy.shape[-1], Cx, 3, 3, 3, device=x.device, dtype=torch.float64)
    for b in range(B):
        xp = torch.zeros(D + 2, H + 2, W + 2, Cx, device=x.device, dtype=torch.float32)
        xp[1:-1, 1:-1, 1:-1] = x[b].float()
        g = dy[b].float().reshape(D * H * W, -1).t().contiguous()
        for kd in range(3):
            for kh in range(3):
                for kw in range(3):
                    out[:, :, kd, kh, kw] += (g @ xp[kd:kd + D, kh:kh + H, kw:kw + W].reshape(D * H * W, Cx)).double()
        del xp, g
    return out


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def baseline_l2(what, y_small, ref_fn, planes):
    """the kernel's relative L2 against the fp64 plane reference on the small verified shape: the largest of `planes` of sample 0"""
    vals = [rel_l2(y_small[0, d], ref_fn(0, d)) for d in planes]
    print(f"{what}: small-shape relative L2 per plane {['%.3e' % v for v in vals]} -> B = 16 bound {L2_FACTOR} x {max(vals):.3e}")
    return max(vals)


def check_planes(what, y, ref_fn, base, samples=SAMPLES, planes=PLANES, classes=False):
    """every (sample, plane): max error <= TOL of the plane's max and relative L2 <= L2_FACTOR x base; classes: the four (h, w) parity
    classes of a transposed convolution's fine plane separately as well.  Everything is printed first; the last sample's last plane is
    asserted on its own."""
    tol, rows, bad = TOL[BF], {}, []
    for b in samples:
        for d in planes:
            ref = ref_fn(b, d)
            got = y[b, d].double()
            err, scale, l2 = float((got - ref).abs().max()), float(ref.abs().max()), rel_l2(got, ref)
            rows[(b, d)] = (err / scale, l2)
            ok = err <= tol * scale and l2 <= L2_FACTOR * base
            if classes:
                for ph in range(2):
                    for pw in range(2):
                        g_, r_ = got[ph::2, pw::2], ref[ph::2, pw::2]
                        ok = ok and float((g_ - r_).abs().max()) <= tol * float(r_.abs().max())
            if not ok:
                bad.append((b, d, err / scale, l2))
    worst = max(rows.values(), key=lambda r: r[1])
    print(f"{what}: {len(rows)} planes, max err / max {max(r[0] for r in rows.values()):.3e} (bound {tol}), relative L2 max {worst[1]:.3e} "
          f"(bound {L2_FACTOR * base:.3e}); last sample, last plane {rows[(samples[-1], planes[-1])][0]:.3e} / {rows[(samples[-1], planes[-1])][1]:.3e}")
    last = (samples[-1], planes[-1])
    assert not [r for r in bad if (r[0], r[1]) == last], f"{what}: the LAST plane of the LAST sample is wrong (err / max, relative L2): {rows[last]}"
    assert not bad, f"{what}: planes (sample, plane, err / max, relative L2) out of bounds: {bad}"


def close32(got, want, tol, what):
    """`close` in fp32 (the operands are 512 MiB per sample; fp32 subtracts a bf16 from an fp32 value exactly enough for a 2e-2 bound)"""
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"
    return err / scale


def ncdhw(t_dhwc):
    return t_dhwc.float().permute(3, 0, 1, 2).unsqueeze(0).contiguous()


def check_whole(what, ys, ref_fn, B):
    """ys: {name: device tensor [B, D, H, W, C]}; ref_fn(b) -> {name: fp32 [1, C, D, H, W]} from a library convolution of sample b in fp32"""
    worst = {k: 0.0 for k in ys}
    for b in range(B):
        refs = ref_fn(b)
        for k, y in ys.items():
            worst[k] = max(worst[k], close32(ncdhw(y[b]), refs[k], TOL[BF], f"{what} {k}, sample {b}"))
        del refs
    print(f"{what}: whole tensor vs fp32 device convolution, max err / max over {B} samples: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def uses_k3(ops, mode, B, Si, cin, So, cout, ep=False, partials=False, k=3, s=1):
    """am_conv3d_uses_k3 for a dense bf16 launch without accumulation: 1 conv_k3_kernel, 2 its transposed instantiation, 0 another kernel"""
    from anatomask_amd import hip
    return hip.lib()._lib.am_conv3d_uses_k3(mode, hip.DT_BF16, k, s, B, *Si, cin, *So, cout, 0, 0, int(ep), int(partials))


def chan_sums(y):
    """per-channel fp64 (sum, sum of squares, sum of |.|) of a [B, D, H, W, C] tensor, one sample at a time"""
    C = y.shape[-1]
    s = torch.zeros(3, C, device=y.device, dtype=torch.float64)
    for b in range(y.shape[0]):
        yf = y[b].float().reshape(-1, C)
        s[0] += yf.sum(0, dtype=torch.float64); s[1] += (yf * yf).sum(0, dtype=torch.float64); s[2] += yf.abs().sum(0, dtype=torch.float64)
    return s


# Bound of the statistics rows.  conv_k3's ST epilogue keeps, per lane, one fp32 accumulator per (channel-tile pair, row) and adds to it the
# lane's own and its pair lane's stored value of every chunk: 8 sequential adds per unit, over all units of the workgroup -- 2 units at
# B = 1, 64^3 (16 adds), 32 at B = 2, 128^3 (256), 256 at B = 16, 128^3 (2 048) -- then three cross-lane adds; the rows are folded in fp64.
# Sequential fp32 summation of n terms is off by <= n 2^-24 of their absolute sum in the worst case (1.2e-4 at n = 2 048) and by
# ~sqrt(n) 2^-24 = 2.7e-6 for unbiased roundings.  The bound is the one tests/test_ops_gpu.py asserts for these rows, 1e-5, kept at this
# batch: forty times the unbiased estimate, a twelfth of the worst case.  The sum of squares does NOT round without bias (squares of bf16
# values have non-uniform low bits): its error grows in proportion to the adds per accumulator (2.5e-7 at 256, 8.4e-6 at 2 048) and would
# pass 1e-5 at about 2 400 adds, i.e. beyond 18 samples of 128^3 per launch.
STATS_TOL = 1e-5


def check_stats(what, part, y, ops):
    C = y.shape[-1]
    st = ops.NormStats(C, DEV)
    part.reduce(sums=st.sums)
    got, ref = st.sums[0].double(), chan_sums(y)
    e1, e2 = float((got[:, 0] - ref[0]).abs().max() / ref[2].max()), float((got[:, 1] - ref[1]).abs().max() / ref[1].max())
    print(f"{what}: statistics rows vs fp64 sums of the stored output: sum {e1:.3e} of the absolute sum, sum of squares {e2:.3e} (bound {STATS_TOL})")
    assert e1 <= STATS_TOL and e2 <= STATS_TOL, (what, e1, e2)


# ------------------------------------------------------------------ conv_k3: forward, statistics, fused epilogue, data gradient
def test_conv_k3_forward_bias_statistics_b16(ops):
    """conv_k3<4, ST> 64 -> 64 with bias and statistics rows at [16, 128^3, 64] (decoder conv.0 of the last block, train mode)."""
    need_gib(14)
    assert K3_CASES[0] == (64, 64, (64, 64, 64), 1)
    w, bias = conv_weight(64, 64, 702), rnd(64, seed=703)
    wp, bd = ops.pack_weight(w.to(DEV), BF, False, False), bias.to(DEV)
    xs = dev_randn(1, (64,) * 3, 64, 704)
    ys, ps = ops.conv3d(ops.CONV_FWD, xs, wp, bd, (64,) * 3, 3, 1, want_partials=True)
    assert ps.rows == 8 * cus() and uses_k3(ops, ops.CONV_FWD, 1, (64,) * 3, 64, (64,) * 3, 64, partials=True) == 1
    base = baseline_l2("conv_k3 fwd 64->64", ys, lambda b, d: conv_plane_ref(xs, w, bias, b, d), (0, 7, 8, 63))
    x = dev_randn(B16, S128, 64, 701)
    assert x.numel() == 2 ** 31 and x.numel() * x.element_size() == 2 ** 32
    y, part = ops.conv3d(ops.CONV_FWD, x, wp, bd, S128, 3, 1, want_partials=True)
    assert uses_k3(ops, ops.CONV_FWD, B16, S128, 64, S128, 64, partials=True) == 1
    assert part.rows == 8 * cus(), "the launch must have taken conv_k3_kernel (8 statistics rows per workgroup)"
    check_planes("conv_k3 fwd 64->64 B=16", y, lambda b, d: conv_plane_ref(x, w, bias, b, d), base)
    wd = w.to(DEV)
    check_whole("conv_k3 fwd 64->64 B=16", {"y": y}, lambda b: {"y": F.conv3d(ncdhw(x[b]), wd, bd, padding=1)}, B16)
    check_stats("conv_k3 fwd 64->64 B=16", part, y, ops)
    y2, part2 = ops.conv3d(ops.CONV_FWD, x, wp, bd, S128, 3, 1, want_partials=True)
    assert torch.equal(y, y2) and torch.equal(part.t[:part.rows], part2.t[:part2.rows]), "two launches: the same bits"


@pytest.mark.parametrize("act", ["relu6", "lrelu"])
def test_conv_k3_fused_epilogue_b16(ops, act):
    """conv_k3<4, EP>: act(conv * scale + shift + res) in the store, the 4 GiB skip tensor read through its own descriptor (pk_off)."""
    need_gib(18)
    w = conv_weight(64, 64, 712)
    sc, sh = rnd(64, seed=713).abs() + 0.5, rnd(64, seed=714)
    code = {"relu6": ops.ACT_RELU6, "lrelu": ops.ACT_LRELU}[act]
    fn = {"relu6": lambda t: torch.clamp(t, 0, 6), "lrelu": lambda t: F.leaky_relu(t, 0.01)}[act]
    wp, scd, shd, wd = ops.pack_weight(w.to(DEV), BF, False, False), sc.to(DEV), sh.to(DEV), w.to(DEV)
    kw = dict(ep_scale=scd, ep_shift=shd, ep_act=code)

    def plane(xx, rr):
        return lambda b, d: fn(conv_plane_ref(xx, w, None, b, d) * scd.double() + shd.double() + rr[b, d].double())
    xs, rs = dev_randn(1, (64,) * 3, 64, 715), dev_randn(1, (64,) * 3, 64, 716)
    assert uses_k3(ops, ops.CONV_FWD, 1, (64,) * 3, 64, (64,) * 3, 64, ep=True) == 1
    ys = ops.conv3d(ops.CONV_FWD, xs, wp, None, (64,) * 3, 3, 1, ep_res=rs, **kw)
    base = baseline_l2(f"conv_k3 + bn + res + {act}", ys, plane(xs, rs), (0, 7, 8, 63))
    x, res = dev_randn(B16, S128, 64, 711), dev_randn(B16, S128, 64, 717)
    assert uses_k3(ops, ops.CONV_FWD, B16, S128, 64, S128, 64, ep=True) == 1, "the launch must reach conv_k3_kernel<4, EP>"
    y = ops.conv3d(ops.CONV_FWD, x, wp, None, S128, 3, 1, ep_res=res, **kw)
    check_planes(f"conv_k3 + bn + res + {act} B=16", y, plane(x, res), base)
    bc = lambda t: t.view(1, -1, 1, 1, 1)
    check_whole(f"conv_k3 + bn + res + {act} B=16", {"y": y},
                lambda b: {"y": fn(F.conv3d(ncdhw(x[b]), wd, None, padding=1) * bc(scd) + bc(shd) + ncdhw(res[b]))}, B16)


def test_conv_k3_data_gradient_and_sum_only_statistics_b16(ops):
    """conv_k3<4> data gradient 64 -> 64 (mirrored taps, transposed packed weight), plain, with the full and with the SUM-ONLY statistics
    epilogue (what the decoder's backward launches: the transposed conv's bias gradient is the per-channel sum of this gradient)."""
    need_gib(18)
    w = conv_weight(64, 64, 722)
    wf = dgrad_weight(w)
    wpd, wd = ops.pack_weight(w.to(DEV), BF, False, True), w.to(DEV)
    dys = dev_randn(1, (64,) * 3, 64, 724)
    assert uses_k3(ops, ops.CONV_DGRAD, 1, (64,) * 3, 64, (64,) * 3, 64) == 1
    dxs = ops.conv3d(ops.CONV_DGRAD, dys, wpd, None, (64,) * 3, 3, 1)
    base = baseline_l2("conv_k3 dgrad 64->64", dxs, lambda b, d: conv_plane_ref(dys, wf, None, b, d), (0, 7, 8, 63))
    dy = dev_randn(B16, S128, 64, 721)
    assert uses_k3(ops, ops.CONV_DGRAD, B16, S128, 64, S128, 64) == 1 and uses_k3(ops, ops.CONV_DGRAD, B16, S128, 64, S128, 64, partials=True) == 1
    dx = ops.conv3d(ops.CONV_DGRAD, dy, wpd, None, S128, 3, 1)
    check_planes("conv_k3 dgrad 64->64 B=16", dx, lambda b, d: conv_plane_ref(dy, wf, None, b, d), base)
    check_whole("conv_k3 dgrad 64->64 B=16", {"dx": dx}, lambda b: {"dx": F.conv_transpose3d(ncdhw(dy[b]), wd, None, padding=1)}, B16)
    dx3, p3 = ops.conv3d(ops.CONV_DGRAD, dy, wpd, None, S128, 3, 1, want_partials=True)
    assert p3.rows == 8 * cus(), "the launch must have taken conv_k3_kernel"
    assert torch.equal(dx3, dx)
    check_stats("conv_k3 dgrad 64->64 B=16", p3, dx, ops)
    del dx3
    dx2, p2 = ops.conv3d(ops.CONV_DGRAD, dy, wpd, None, S128, 3, 1, want_partials=True, partials_sum_only=True)
    assert p2.rows == 8 * cus() and torch.equal(dx2, dx), "sum-only statistics: the same output bits"
    assert torch.equal(p2.t[:p2.rows, :, 0], p3.t[:p3.rows, :, 0]) and float(p2.t[:p2.rows, :, 1].abs().max()) == 0.0 and float(p3.t[:p3.rows, :, 1].abs().max()) > 0.0
    acc = torch.zeros(64, device=DEV)
    p2.finalize(None, sum_accum=acc)
    ref = chan_sums(dx)
    e = float((acc.double() - ref[0]).abs().max() / ref[2].max())
    print(f"conv_k3 dgrad 64->64 B=16, sum-only rows -> bias gradient: {e:.3e} of the absolute sum (bound {STATS_TOL})")
    assert e <= STATS_TOL
    # the sum-of-squares column of sum-only rows is not a statistic: the readers that would use it refuse such rows
    assert p2.sum_only and not p3.sum_only
    st = ops.NormStats(64, DEV)
    with pytest.raises(AssertionError):
        p2.reduce(sums=st.sums)
    with pytest.raises(AssertionError):
        p2.finalize(st, torch.ones(64, device=DEV), torch.zeros(64, device=DEV), 1e-5)


def test_conv_k3_32_channel_tiles_b16(ops):
    """conv_k3<2>: 64 -> 32 forward with statistics (decoder conv.3 of the last block), the same with the teacher's fused epilogue
    (scale, shift, skip tensor), and its 32 -> 64 data gradient (a ONE-slab contraction: Cin = 32)."""
    need_gib(16)
    w, bias = conv_weight(32, 64, 732), rnd(32, seed=733)
    wf = dgrad_weight(w)
    wp, wpd, wd, bd = ops.pack_weight(w.to(DEV), BF, False, False), ops.pack_weight(w.to(DEV), BF, False, True), w.to(DEV), bias.to(DEV)
    sc, sh = (rnd(32, seed=736).abs() + 0.5).to(DEV), rnd(32, seed=737).to(DEV)
    S64 = (64,) * 3
    xs, dys, rs = dev_randn(1, S64, 64, 734), dev_randn(1, S64, 32, 735), dev_randn(1, S64, 32, 738)
    ys, ps = ops.conv3d(ops.CONV_FWD, xs, wp, bd, S64, 3, 1, want_partials=True)
    assert ps.rows == 8 * cus() and uses_k3(ops, ops.CONV_DGRAD, 1, S64, 32, S64, 64) == 1 and uses_k3(ops, ops.CONV_FWD, 1, S64, 64, S64, 32, ep=True) == 1
    base_f = baseline_l2("conv_k3 fwd 64->32", ys, lambda b, d: conv_plane_ref(xs, w, bias, b, d), (0, 7, 8, 63))
    es = ops.conv3d(ops.CONV_FWD, xs, wp, None, S64, 3, 1, ep_scale=sc, ep_shift=sh, ep_res=rs)
    ep_plane = lambda xx, rr: (lambda b, d: conv_plane_ref(xx, w, None, b, d) * sc.double() + sh.double() + rr[b, d].double())
    base_e = baseline_l2("conv_k3 + bn + res 64->32", es, ep_plane(xs, rs), (0, 7, 8, 63))
    dxs = ops.conv3d(ops.CONV_DGRAD, dys, wpd, None, S64, 3, 1)
    base_d = baseline_l2("conv_k3 dgrad 32->64", dxs, lambda b, d: conv_plane_ref(dys, wf, None, b, d), (0, 7, 8, 63))
    x, res = dev_randn(B16, S128, 64, 731), dev_randn(B16, S128, 32, 739)
    y, part = ops.conv3d(ops.CONV_FWD, x, wp, bd, S128, 3, 1, want_partials=True)
    assert part.rows == 8 * cus(), "the launch must have taken conv_k3_kernel<2>"
    check_planes("conv_k3 fwd 64->32 B=16", y, lambda b, d: conv_plane_ref(x, w, bias, b, d), base_f)
    check_stats("conv_k3 fwd 64->32 B=16", part, y, ops)
    assert uses_k3(ops, ops.CONV_FWD, B16, S128, 64, S128, 32, partials=True) == 1 and uses_k3(ops, ops.CONV_FWD, B16, S128, 64, S128, 32, ep=True) == 1
    e = ops.conv3d(ops.CONV_FWD, x, wp, None, S128, 3, 1, ep_scale=sc, ep_shift=sh, ep_res=res)
    check_planes("conv_k3 + bn + res 64->32 B=16", e, ep_plane(x, res), base_e)
    bc = lambda t: t.view(1, -1, 1, 1, 1)

    def whole(b):
        c = F.conv3d(ncdhw(x[b]), wd, None, padding=1)
        return {"y": c + bc(bd), "y_ep": c * bc(sc) + bc(sh) + ncdhw(res[b])}
    check_whole("conv_k3 fwd 64->32 B=16", {"y": y, "y_ep": e}, whole, B16)
    del x, res, e
    dy = dev_randn(B16, S128, 32, 740)
    assert uses_k3(ops, ops.CONV_DGRAD, B16, S128, 32, S128, 64) == 1
    dx = ops.conv3d(ops.CONV_DGRAD, dy, wpd, None, S128, 3, 1)
    check_planes("conv_k3 dgrad 32->64 B=16", dx, lambda b, d: conv_plane_ref(dy, wf, None, b, d), base_d)
    check_whole("conv_k3 dgrad 32->64 B=16", {"dx": dx}, lambda b: {"dx": F.conv_transpose3d(ncdhw(dy[b]), wd, None, padding=1)}, B16)


def test_conv_transpose_b16(ops):
    """conv_k3<CT>: ConvTranspose3d k4 s2 p1 64 -> 64, [16, 64^3, 64] -> [16, 128^3, 64] (UNetBlock.up_sample of the LAST decoder block is
    cin -> cin with cin = width / 8 = 64 at width 512).  Fine planes {0, 1, 15, 16, 126, 127} (both d-parities, coarse brick boundary,
    both ends) of samples {0, 7, 8, 15}, each (h, w) parity class of a plane on its own; whole tensor."""
    need_gib(12)
    from anatomask_amd import modules as M
    dec = M.LightDecoder(16, width=512, sbn=False)
    up = dec.dec[-1].up_sample
    assert (up.in_channels, up.out_channels, up.kernel_size, up.stride, up.padding) == (64, 64, (4, 4, 4), (2, 2, 2), (1, 1, 1))
    cin = cout = 64
    assert uses_k3(ops, ops.CONVT_FWD, B16, (64,) * 3, cin, S128, cout, k=4, s=2) == 2, "the launch must reach the transposed instantiation of conv_k3_kernel"
    assert uses_k3(ops, ops.CONVT_FWD, 4, (32,) * 3, cin, (64,) * 3, cout, k=4, s=2) == 2
    w = q(rnd(cin, cout, 4, 4, 4, seed=742, scale=1.0 / np.sqrt(cin * 8)), BF)
    bias = rnd(cout, seed=743)
    wp, wd, bd = ops.pack_weight(w.to(DEV), BF, True, False), w.to(DEV), bias.to(DEV)
    xs = dev_randn(4, (32,) * 3, cin, 744)
    ys = ops.conv3d(ops.CONVT_FWD, xs, wp, bd, (64,) * 3, 4, 2)
    base = baseline_l2("convT 64->64", ys, lambda b, d: convt_plane_ref(xs, w, bias, b, d), (0, 1, 15, 16, 62, 63))
    x = dev_randn(B16, (64,) * 3, cin, 741)
    y = ops.conv3d(ops.CONVT_FWD, x, wp, bd, S128, 4, 2)
    assert y.numel() == 2 ** 31
    check_planes("convT 64->64 B=16", y, lambda b, d: convt_plane_ref(x, w, bias, b, d), base, planes=FINE_PLANES, classes=True)
    check_whole("convT 64->64 B=16", {"y": y}, lambda b: {"y": F.conv_transpose3d(ncdhw(x[b]), wd, bd, stride=2, padding=1)}, B16)
    # every one of the eight parity classes over the whole of the first and the last sample
    for b in (0, B16 - 1):
        ref, got = F.conv_transpose3d(ncdhw(x[b]), wd, bd, stride=2, padding=1)[0], ncdhw(y[b])[0]
        for pd in range(2):
            for ph in range(2):
                for pw in range(2):
                    close32(got[:, pd::2, ph::2, pw::2], ref[:, pd::2, ph::2, pw::2], TOL[BF], f"convT sample {b} class {pd}{ph}{pw}")
    y2 = ops.conv3d(ops.CONVT_FWD, x, wp, bd, S128, 4, 2)
    assert torch.equal(y, y2)


def test_conv_k3_nontemporal_store_threshold_full_cpu_reference(ops):
    """conv_k3 switches to non-temporal stores from 384 MiB of output on.  B = 2, 128^3, 64 -> 64 writes 512 MiB and is small enough for
    the FULL CPU F.conv3d reference of K3_CASES (2 x 0.46 TFLOP, a few seconds on 16 threads), forward and data gradient.  The ABI does not
    report which store a launch used: the 384 MiB below restates conv_k3_launch's threshold, it is not an observation."""
    B = 2
    assert B * 128 ** 3 * 64 * 2 >= 384 << 20 > 64 ** 3 * 64 * 2 * 8
    torch.set_num_threads(min(16, torch.get_num_threads()))
    w, bias = conv_weight(64, 64, 752), rnd(64, seed=753)
    x, dy = dev_randn(B, S128, 64, 751), dev_randn(B, S128, 64, 754)
    y, part = ops.conv3d(ops.CONV_FWD, x, ops.pack_weight(w.to(DEV), BF, False, False), bias.to(DEV), S128, 3, 1, want_partials=True)
    assert part.rows == 8 * cus() and uses_k3(ops, ops.CONV_FWD, B, S128, 64, S128, 64, partials=True) == 1 and uses_k3(ops, ops.CONV_DGRAD, B, S128, 64, S128, 64) == 1
    dx = ops.conv3d(ops.CONV_DGRAD, dy, ops.pack_weight(w.to(DEV), BF, False, True), None, S128, 3, 1)
    for b in range(B):
        yr = F.conv3d(ncdhw(x[b]).cpu(), w, bias, padding=1)
        close(ncdhw(y[b]).cpu(), yr, TOL[BF], f"conv_k3 fwd, non-temporal stores, sample {b}")
        dxr = F.conv_transpose3d(ncdhw(dy[b]).cpu(), w, None, padding=1)
        close(ncdhw(dx[b]).cpu(), dxr, TOL[BF], f"conv_k3 dgrad, non-temporal stores, sample {b}")
    check_stats("conv_k3 fwd B=2 (non-temporal stores)", part, y, ops)


# ------------------------------------------------------------------ weight gradients
LOCAL_REGIONS = {"sample 15, plane 127": (15, (127, 128, 0, 128, 0, 128)), "sample 8, plane 0": (8, (0, 1, 0, 128, 0, 128)),
                 "sample 0, plane 0": (0, (0, 1, 0, 128, 0, 128)), "far-corner brick of sample 15": (15, (120, 128, 124, 128, 112, 128))}


# Localised dY: the operands are exact in bf16, the products exact in fp32, and a region holds at most 16 384 voxels, so the kernels' fp32
# accumulation is off by ~sqrt(16 384) 2^-24 = 8e-6 of the result against the fp64 contraction (worst case 16 384 x 2^-24 = 1e-3 of the absolute
# sum, never met by random operands).  1e-4 is twelve times the estimate and 200 x tighter than the 2e-2 of the full random case: a partly
# wrong accumulation (one row of a plane counted twice is 1 / 128 of the result) fails it.
LOCAL_WGRAD_TOL = 1e-4


@pytest.mark.parametrize("ch", [(64, 64), (64, 32)])
def test_conv_wgrad_k3_b16(ops, ch):
    """Dense k3 s1 bf16 weight gradient at [16, 128^3]: wgrad_k3 (default mode, conv_wgk3.hip: per-sample descriptors b * samp) and the
    plane-brick kernels of conv_wgrad.hip (deterministic mode: plane-anchored descriptors).  The result sums 2^25 voxels, so one dropped
    plane is 1 / 2048 of it: beside the full random case, dY is zero except for ONE plane / ONE brick and the reference is the fp64
    contraction over that region alone.  Tolerance, whole tensor and every tap: 2e-2 of max for the full random case
    (test_conv_wgrad_k3_dense_8wave_dma_kernel), LOCAL_WGRAD_TOL = 1e-4 for the localised ones."""
    cin, cout = ch
    need_gib(14)
    from anatomask_amd import hip
    uses = lambda det: hip.lib()._lib.am_conv3d_wgrad_uses_k3(ops.CONV_FWD, hip.DT_BF16, 3, 1, B16, *S128, cin, cout, 0, det)
    assert uses(0) == 1, "default mode must reach wgrad_k3"
    assert uses(1) == 0, "deterministic mode must reach the plane-brick kernels of conv_wgrad.hip"
    x, dy = dev_randn(B16, S128, cin, 761), dev_randn(B16, S128, cout, 762)

    def run(det):
        ops.DETERMINISTIC_WGRAD = det
        try:
            dwp = ops.conv3d_wgrad(ops.CONV_FWD, x, dy, 3, 1)
        finally:
            ops.DETERMINISTIC_WGRAD = False
        dw = torch.zeros(cout, cin, 3, 3, 3, device=DEV)
        ops.unpack_grad(dwp, dw, transposed_conv=False, accumulate=False)
        return dwp, dw

    def compare(what, ref, tol=TOL[BF]):
        worst = {}
        for det in (False, True):
            dwp, dw = run(det)
            name = f"wgrad {cin}x{cout} {what}, {'deterministic' if det else 'default'} mode"
            e = float((dw.double() - ref).abs().max() / ref.abs().max())
            taps = max(float((dw.double()[:, :, t // 9, t // 3 % 3, t % 3] - ref[:, :, t // 9, t // 3 % 3, t % 3]).abs().max()
                             / (ref[:, :, t // 9, t // 3 % 3, t % 3].abs().max() + 1e-30)) for t in range(27))
            worst[det] = (e, taps)
            print(f"{name}: max err / max {e:.3e}, worst tap {taps:.3e} (bound {tol})")
            assert e <= tol and taps <= tol, name
            if det:
                assert torch.equal(dwp, run(True)[0]), f"{name}: two launches must give the same bits"
        return worst
    compare("full random", wgrad_full_ref(x, dy))
    for what, (b, reg) in LOCAL_REGIONS.items():
        d0, d1, h0, h1, w0, w1 = reg
        keep = dy[b, d0:d1, h0:h1, w0:w1].clone()
        dy.zero_()
        dy[b, d0:d1, h0:h1, w0:w1] = keep
        ref = wgrad_region_ref(x, dy, b, reg)
        assert float(ref.abs().max()) > 0
        compare(f"dY only in {what}", ref, LOCAL_WGRAD_TOL)
        if what != list(LOCAL_REGIONS)[-1]:
            dy = dev_randn(B16, S128, cout, 762)


# ------------------------------------------------------------------ dense norm passes (stream_ops.hip, linear walk, mask = NULL)
# sums of the linear-walk kernels: a thread adds <= 1024 values in fp32 before the fold goes to fp64 (vpw = 32 768 voxels over 32 voxel lanes);
# sequential fp32 summation of n terms is off by <= n 2^-24 of their absolute sum in the worst case
NORM_SUM_TOL = 1024 * 2.0 ** -24
GATE_EDGE = 1e-3      # elements whose pre-activation lies this close to a kink of the activation are left out of the dx comparison (the kernel
#                       recomputes the gate from x * scale + shift in fp32; the reference's fp64-derived coefficients differ in the last bit)


def bn_reference(x, mask=None, eps=1e-5):
    """fp64 per-channel (mean, rstd, count) over the (active) voxels of x, from fp32 chunks with fp64 reductions"""
    C = x.shape[-1]
    s = torch.zeros(2, C, device=x.device, dtype=torch.float64)
    n = 0.0
    for b in range(x.shape[0]):
        xf = x[b].float().reshape(-1, C)
        if mask is not None:
            xf = xf[mask[b].reshape(-1)]
        n += xf.shape[0]
        s[0] += xf.sum(0, dtype=torch.float64); s[1] += (xf * xf).sum(0, dtype=torch.float64)
    mean = s[0] / n
    var = s[1] / n - mean * mean
    return s, mean, torch.rsqrt(var + eps), n


def act_fns(ops, act):
    if act == ops.ACT_RELU6:
        return (lambda z: torch.clamp(z, 0, 6)), (lambda z: ((z > 0) & (z < 6)).float()), (lambda z: (z.abs() > GATE_EDGE) & ((z - 6).abs() > GATE_EDGE))
    if act == ops.ACT_LRELU:
        return (lambda z: F.leaky_relu(z, 0.01)), (lambda z: torch.where(z > 0, 1.0, 0.01)), (lambda z: z.abs() > GATE_EDGE)
    return (lambda z: z), (lambda z: torch.ones_like(z)), (lambda z: torch.ones_like(z, dtype=torch.bool))


def norm_fwd_bwd_check(ops, what, x, dout, res, gam, bet, st, act, mi, bs, mask, count):
    """norm_apply and norm_backward of y = act(norm(x) [+ res]) against the closed form; statistics in st (already finalised)"""
    B, C = x.shape[0], x.shape[-1]
    _, mean, rstd, n = bn_reference(x, mask)
    assert n == count
    e_m, e_r = float((st.mean.double() - mean).abs().max() / mean.abs().max()), float((st.rstd.double() / rstd - 1).abs().max())
    print(f"{what}: mean {e_m:.3e}, rstd {e_r:.3e} from the fp64 statistics (bound {2 * NORM_SUM_TOL:.1e})")
    assert e_m <= 2 * NORM_SUM_TOL and e_r <= 2 * NORM_SUM_TOL
    mean32, rstd32 = mean.float(), rstd.float()
    fwd, gate, safe = act_fns(ops, act)
    y = ops.norm_apply(x, st, act, mi, bs, res=res)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.norm_backward(dout, None, x, st, gam, act, mi, bs, dg, db)      # (out = None: the gate is recomputed, as the engine's decoder does)
    tol = TOL[BF]
    # pass 1: forward per sample + the two backward sums
    sums = torch.zeros(4, C, device=DEV, dtype=torch.float64)      # sum g, sum g xhat, and the absolute sums of both
    worst_y, last_y = 0.0, None
    for b in range(B):
        xh = (x[b].float() - mean32) * rstd32
        z = xh * gam + bet
        if res is not None:
            z = z + res[b].float()
        want = fwd(z)
        m = None if mask is None else mask[b]
        err = (y[b].float() - want).abs()
        if m is not None:
            err = torch.where(m, err, torch.zeros((), device=DEV))
        scale = float(want.abs().max())
        worst_y = max(worst_y, float(err.max()) / scale)
        if b == B - 1:
            last_y = float(err[-1].max()) / scale
        g = dout[b].float() * gate(z)
        if m is not None:
            g = torch.where(m, g, torch.zeros((), device=DEV))
        gx = (g * xh).reshape(-1, C)
        g = g.reshape(-1, C)
        sums[0] += g.sum(0, dtype=torch.float64); sums[1] += gx.sum(0, dtype=torch.float64)
        sums[2] += g.abs().sum(0, dtype=torch.float64); sums[3] += gx.abs().sum(0, dtype=torch.float64)
        del g, gx
    print(f"{what}: norm_apply max err / max {worst_y:.3e}, last sample's last plane {last_y:.3e} (bound {tol})")
    assert last_y <= tol, f"{what}: norm_apply, the LAST plane of the LAST sample"
    assert worst_y <= tol, f"{what}: norm_apply"
    d_b, d_g = float((db.double() - sums[0]).abs().max()), float((dg.double() - sums[1]).abs().max())
    e_b, e_g = d_b / float(sums[0].abs().max()), d_g / float(sums[1].abs().max())
    a_b, a_g = d_b / float(sums[2].max()), d_g / float(sums[3].max())
    print(f"{what}: dbeta {e_b:.3e}, dgamma {e_g:.3e} of max (bound {2 * tol}); {a_b:.3e}, {a_g:.3e} of the absolute sums (bound {NORM_SUM_TOL:.1e})")
    assert e_b <= 2 * tol and e_g <= 2 * tol and a_b <= NORM_SUM_TOL and a_g <= NORM_SUM_TOL
    # pass 2: dx = gamma rstd (g - mean(g) - xhat mean(g xhat))
    k1, k2 = (sums[0] / n).float(), (sums[1] / n).float()
    worst_dx, last_dx = 0.0, None
    for b in range(B):
        xh = (x[b].float() - mean32) * rstd32
        z = xh * gam + bet
        if res is not None:
            z = z + res[b].float()
        want = gam * rstd32 * (dout[b].float() * gate(z) - k1 - xh * k2)
        keep = safe(z) if mask is None else (safe(z) & mask[b])
        err = torch.where(keep, (dx[b].float() - want).abs(), torch.zeros((), device=DEV))
        scale = float(torch.where(keep, want.abs(), torch.zeros((), device=DEV)).max())
        worst_dx = max(worst_dx, float(err.max()) / scale)
        if b == B - 1:
            last_dx = float(err[-1].max()) / scale
    print(f"{what}: norm_backward dx max err / max {worst_dx:.3e}, last sample's last plane {last_dx:.3e} (bound {2 * tol})")
    assert last_dx <= 2 * tol, f"{what}: norm_backward, the LAST plane of the LAST sample"
    assert worst_dx <= 2 * tol, f"{what}: norm_backward"


@pytest.mark.parametrize("form", ["relu6", "none+res"])
def test_dense_batchnorm_passes_b16(ops, form):
    """ops.chan_stats, norm_finalize, norm_apply and norm_backward (am_norm_bwd_reduce with its fused finalize, am_norm_bwd_apply) on the
    dense [16, 128^3, 64] tensor in the two forms the decoder's BatchNorm takes in train mode: with the ReLU6 gate (conv.1, recomputed from
    the pre-activation in the backward) and without activation but with the skip tensor added (conv.4 + to_dec)."""
    need_gib(22)
    C = 64
    act, with_res = (ops.ACT_RELU6, False) if form == "relu6" else (ops.ACT_NONE, True)
    x = dev_randn(B16, S128, C, 771, scale=1.5, shift=0.7)
    dout = dev_randn(B16, S128, C, 772)
    res = dev_randn(B16, S128, C, 773) if with_res else None
    gam, bet = (torch.rand(C, generator=torch.Generator().manual_seed(774)) + 0.5).to(DEV), (2.0 * rnd(C, seed=775)).to(DEV)
    st = ops.NormStats(C, DEV)
    st.count_host = float(B16 * 128 ** 3)
    ops.chan_stats(x, None, 0, st)
    ref, _, _, _ = bn_reference(x)
    got = st.sums.sum(0).double()
    absx = chan_sums(x)[2]
    e1, e2 = float((got[:, 0] - ref[0]).abs().max() / absx.max()), float((got[:, 1] - ref[1]).abs().max() / ref[1].abs().max())
    print(f"dense chan_stats [16,128^3,64]: sum {e1:.3e} of the absolute sum, sum of squares {e2:.3e} (bound {NORM_SUM_TOL:.1e})")
    assert e1 <= NORM_SUM_TOL and e2 <= NORM_SUM_TOL
    ops.norm_finalize(st, gam, bet, 1e-5)
    norm_fwd_bwd_check(ops, f"dense BatchNorm ({form}) [16,128^3,64]", x, dout, res, gam, bet, st, act, None, 0, None, B16 * 128 ** 3)


# ------------------------------------------------------------------ block-sparse row-walk norm passes at the real widths
@pytest.mark.parametrize("C", [32, 64])
def test_row_walk_norm_passes_real_widths_b16(ops, C):
    """As test_row_walk_kernels_beyond_the_linear_decode_limit (tests/test_ops_gpu.py), at the widths the step uses (level 0: 32 channels;
    64) instead of a thin 8-channel tensor, mask 0.6 on 16^3 patches (205 of 512 visible per sample), forward AND backward.  The linear
    kernels refuse this geometry (-4), so a launch that returns was served by the row-walk kernels."""
    need_gib(20)
    B, S, f = B16, 128, 8
    assert B * S ** 3 * S >= 2 ** 32
    g = torch.Generator().manual_seed(C)
    mask = torch.zeros(B, f ** 3, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(f ** 3, generator=g)[:205]] = True
    mask = mask.view(B, 1, f, f, f)
    mi = ops.MaskInfo.from_bool(mask, DEV)
    mf = mask.to(DEV).repeat_interleave(16, 2).repeat_interleave(16, 3).repeat_interleave(16, 4)[:, 0, ..., None]     # (B,S,S,S,1)
    x = dev_randn(B, (S,) * 3, C, 781, scale=1.5, shift=0.7)
    dout = dev_randn(B, (S,) * 3, C, 782)
    gam, bet = (torch.rand(C, generator=torch.Generator().manual_seed(783)) + 0.5).to(DEV), rnd(C, seed=784).to(DEV)
    st = ops.NormStats(C, DEV)
    ops.chan_stats(x, mi, 4, st)
    st.count_host = float(B * 205 * 4096)
    ops.norm_finalize(st, gam, bet, 1e-5)
    norm_fwd_bwd_check(ops, f"row-walk norm C={C} [16,128^3] mask 0.6", x, dout, None, gam, bet, st, ops.ACT_LRELU, mi, 4, mf, B * 205 * 4096)
    with pytest.raises(RuntimeError, match="am_chan_sum failed with code -4"):      # a linear-walk kernel still refuses
        ops.chan_sum(x, mi, 4, torch.zeros(C, device=DEV))


# ------------------------------------------------------------------ fp32 storage: the stem's brick kernels at the batch
@pytest.mark.parametrize("k", [3, 1])
def test_stem_conv_fp32_storage_b16(ops, k):
    """The Cin = 1 stem convolution and its weight gradient in fp32 storage on [16, 128^3] with 16^3 patches, mask 0.6 -- the launches the
    fp32-storage step (the reference of test_config2_stunet_b_128_batch16_bf16_vs_fp32_storage) starts with.  am_stem_conv_fwd /
    am_stem_conv_wgrad used to refuse this geometry with -4, the limit of the LINEAR kernels' reciprocal-multiply voxel decode, although
    their brick kernels address by (b, d, h, w).  Forward: every sample against F.conv3d of the masked volume on the device (fp32, 2e-4 of
    max on the active voxels); weight / bias gradient: per tap and sample the masked dY contracted with the shifted masked volume in fp64
    (5e-4 of max, the bound of test_stem_conv)."""
    need_gib(12)
    B, S, f, C = B16, 128, 8, 32
    g = torch.Generator().manual_seed(790 + k)
    mask = torch.zeros(B, f ** 3, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(f ** 3, generator=g)[:205]] = True
    mask = mask.view(B, 1, f, f, f)
    mi = ops.MaskInfo.from_bool(mask, DEV)
    mf = mask.to(DEV).repeat_interleave(16, 2).repeat_interleave(16, 3).repeat_interleave(16, 4)[:, 0]        # (B,S,S,S)
    gd = torch.Generator(device=DEV).manual_seed(791)
    x = torch.randn(B, S, S, S, device=DEV, generator=gd)
    w, bias = rnd(C, 1, k, k, k, seed=792, scale=0.3).to(DEV), rnd(C, seed=793).to(DEV)
    y = ops.stem_conv_fwd(x, w, bias, mi, 4, torch.float32)
    dy = torch.empty(B, S, S, S, C, device=DEV)
    for b in range(B):
        dy[b] = torch.randn(S, S, S, C, device=DEV, generator=gd)
    dw, db = torch.zeros(C, k ** 3, device=DEV), torch.zeros(C, device=DEV)
    ops.stem_conv_wgrad(x, dy, k, mi, 4, dw, db)
    p = k // 2
    worst, dwr, dbr = 0.0, torch.zeros(C, k ** 3, device=DEV, dtype=torch.float64), torch.zeros(C, device=DEV, dtype=torch.float64)
    for b in range(B):
        xm = x[b] * mf[b]
        want = F.conv3d(xm[None, None], w, bias, padding=p)[0].permute(1, 2, 3, 0)          # (S,S,S,C)
        keep = mf[b][..., None]
        err = torch.where(keep, (y[b] - want).abs(), torch.zeros((), device=DEV))
        scale = float(torch.where(keep, want.abs(), torch.zeros((), device=DEV)).max())
        worst = max(worst, float(err.max()) / scale)
        assert float(err.max()) <= TOL[torch.float32] * scale, f"stem fwd fp32 k{k}, sample {b}: {float(err.max()) / scale:.3e}"
        del want, err
        dyb = torch.where(keep, dy[b], torch.zeros((), device=DEV)).reshape(-1, C).double()
        xp = F.pad(xm, (p, p, p, p, p, p)).double()
        cols = torch.stack([xp[t // (k * k):t // (k * k) + S, t // k % k:t // k % k + S, t % k:t % k + S].reshape(-1) for t in range(k ** 3)], 1)
        dwr += dyb.t() @ cols
        del cols
        dbr += dyb.sum(0)
        del dyb, xp
    e_w, e_b = float((dw.double() - dwr).abs().max() / dwr.abs().max()), float((db.double() - dbr).abs().max() / dbr.abs().max())
    print(f"stem conv k{k} fp32 [16,128^3] -> 32 channels, mask 0.6: forward max err / max {worst:.3e} (bound {TOL[torch.float32]}), "
          f"weight gradient {e_w:.3e}, bias gradient {e_b:.3e} (bound 5e-4)")
    assert e_w <= 5e-4 and e_b <= 5e-4
