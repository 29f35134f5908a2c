"""CPU: the reference helpers of tests/test_bench_batch_gpu.py (fp64 plane convolutions, region / full weight gradients) against torch's own
fp64 convolutions and autograd on small ragged shapes -- the B = 16 tests stand on these helpers, so they are pinned where a full
reference is cheap."""
import torch
import torch.nn.functional as F

from tests.test_bench_batch_gpu import conv_plane_ref, convt_plane_ref, dgrad_weight, wgrad_full_ref, wgrad_region_ref


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def test_conv_plane_reference_matches_torch_fp64():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 6, 7, 9, generator=g, dtype=torch.float64)           # (B, Cin, D, H, W)
    w = torch.randn(4, 5, 3, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(4, generator=g, dtype=torch.float64)
    ref = _cl(F.conv3d(x, w, bias, padding=1))
    refd = _cl(F.conv_transpose3d(ref.permute(0, 4, 1, 2, 3), w, None, padding=1))      # data gradient wrt x for dy = ref
    for b in range(2):
        for d in range(6):
            assert (conv_plane_ref(_cl(x), w, bias, b, d) - ref[b, d]).abs().max() < 1e-12
            assert (conv_plane_ref(ref, dgrad_weight(w), None, b, d) - refd[b, d]).abs().max() < 1e-11


def test_conv_transpose_plane_reference_matches_torch_fp64():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 3, 4, 5, generator=g, dtype=torch.float64)
    w = torch.randn(5, 6, 4, 4, 4, generator=g, dtype=torch.float64)
    bias = torch.randn(6, generator=g, dtype=torch.float64)
    ref = _cl(F.conv_transpose3d(x, w, bias, stride=2, padding=1))
    assert tuple(ref.shape) == (2, 6, 8, 10, 6)
    for b in range(2):
        for od in range(6):
            assert (convt_plane_ref(_cl(x), w, bias, b, od) - ref[b, od]).abs().max() < 1e-12


def test_weight_gradient_references_match_autograd_fp64():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 7, 9, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 4, 6, 7, 9, generator=g, dtype=torch.float64)
    w = torch.zeros(4, 5, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(x, w, None, padding=1).backward(dy)
    assert (wgrad_full_ref(_cl(x), _cl(dy)) - w.grad).abs().max() < 1e-4 * w.grad.abs().max()      # (fp32 matmuls inside)
    for b, reg in ((1, (5, 6, 0, 7, 0, 9)), (0, (0, 1, 0, 7, 0, 9)), (1, (2, 6, 3, 7, 4, 9)), (0, (1, 3, 2, 4, 0, 3))):
        d0, d1, h0, h1, w0, w1 = reg
        dz = torch.zeros_like(dy)
        dz[b, :, d0:d1, h0:h1, w0:w1] = dy[b, :, d0:d1, h0:h1, w0:w1]
        w2 = torch.zeros(4, 5, 3, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv3d(x, w2, None, padding=1).backward(dz)
        assert (wgrad_region_ref(_cl(x), _cl(dz), b, reg) - w2.grad).abs().max() < 1e-11
