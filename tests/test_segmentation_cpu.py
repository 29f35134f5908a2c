"""CPU: the STUNet segmentation network's test-side restatement (tests/seg_oracle.py) against the reference's own outputs
(tests/golden/seg_tiny.npz, made by tests/golden/make_seg_fixtures.py), and the host-side geometry of segmentation.SlidingWindowPredictor
(Gaussian, tile starts, padding) against the reference's functions."""
import numpy as np
import pytest
import torch

from anatomask_amd import segmentation as S
from tests import seg_oracle as SO


@pytest.fixture(scope="module")
def fx(golden_dir):
    import os
    return dict(np.load(os.path.join(golden_dir, "seg_tiny.npz")))


def _tiny(fx):
    keys = [(str(k), tuple(int(v) for v in str(s).split(","))) for k, s in zip(fx["keys"], fx["shapes"])]
    W = SO.seeded_weights(keys, int(fx["weight_seed"]))
    x = SO.smooth_input((1, *SO.TINY["size"]), int(fx["x_seed"]))[:, None]
    return W, x


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm())


def test_oracle_reproduces_reference_logits(fx):
    W, x = _tiny(fx)
    with torch.no_grad():
        plain = SO.forward(W, x, SO.TINY["depth"])
        ds = SO.forward(W, x, SO.TINY["depth"], deep_supervision=True)
    assert _rel(plain, fx["logits"]) <= 1e-5
    assert len(ds) == 5 and _rel(ds[0], fx["logits"]) <= 1e-5
    for i in range(1, 5):
        assert tuple(ds[i].shape) == fx[f"ds{i}"].shape
        assert _rel(ds[i], fx[f"ds{i}"]) <= 1e-5, i


def test_state_dict_keys_and_shapes_equal_reference(fx):
    t = SO.TINY
    net = S.STUNet(1, t["num_classes"], depth=t["depth"], dims=t["dims"], pool_op_kernel_sizes=SO.RECIPE_POOL,
                   conv_kernel_sizes=[[3, 3, 3]] * 6, enable_deep_supervision=False)
    got = [(k, ",".join(str(v) for v in p.shape)) for k, p in net.state_dict().items()]
    want = [(str(k), str(s)) for k, s in zip(fx["keys"], fx["shapes"])]
    assert got == want
    assert [(k, tuple(int(v) for v in s.split(","))) for k, s in want] == SO.state_keys(t["dims"], t["depth"], t["num_classes"])
    # the reference's TotalSegmentator build (initialize_from_trained_STUNet): STUNet-B, 105 classes
    b = S.STUNet(1, 105, depth=[1] * 6, dims=[32 * x for x in [1, 2, 4, 8, 16, 16]], pool_op_kernel_sizes=SO.RECIPE_POOL,
                 conv_kernel_sizes=[[3, 3, 3]] * 6, enable_deep_supervision=False)
    assert [(k, tuple(p.shape)) for k, p in b.state_dict().items()] == SO.state_keys(b.dims, b.depth, 105)


def test_unsupported_configurations_raise():
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):
        S.STUNet(1, 3, pool_op_kernel_sizes=[[2, 2, 2]] * 5, conv_kernel_sizes=[[3, 3, 3]] * 6)
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        S.STUNet(1, 3, pool_op_kernel_sizes=SO.RECIPE_POOL, conv_kernel_sizes=[[1, 3, 3]] + [[3, 3, 3]] * 5)
    with pytest.raises(NotImplementedError, match="input_channels"):
        S.STUNet(2, 3, pool_op_kernel_sizes=SO.RECIPE_POOL, conv_kernel_sizes=[[3, 3, 3]] * 6)


def test_host_gaussian_matches_reference(fx):
    for name, tile in (("g32", (32, 32, 32)), ("g_aniso", (32, 16, 48))):
        g = S.compute_gaussian(tile)
        assert g.dtype == torch.float32 and tuple(g.shape) == tile
        want = torch.from_numpy(fx[name])
        assert float((g - want).abs().max() / want.max()) <= 1e-6, name
        assert float(g.min()) > 0 and float(g.max()) == 1000.0


def test_steps_match_reference(fx):
    for i in range(int(fx["n_step_cases"])):
        c = fx[f"steps{i}.case"]
        img, tile, st = tuple(int(v) for v in c[:3]), tuple(int(v) for v in c[3:6]), float(c[6])
        want = [fx[f"steps{i}.{d}"].tolist() for d in range(3)]
        assert S.compute_steps_for_sliding_window(img, tile, st) == want, (img, tile, st)
        assert SO.steps_for(img, tile, st) == want


def test_padding_rule():
    below, new = S.padding_for((20, 64, 90), (32, 64, 64))
    assert below == (6, 0, 0) and new == (32, 64, 90)
    img = torch.arange(20 * 3 * 5, dtype=torch.float32).view(1, 20, 3, 5)
    pad, back = SO.pad_to(img, (32, 4, 5))
    assert tuple(pad.shape) == (1, 32, 4, 5) and torch.equal(pad[back], img)
    assert torch.equal(pad[:, 6:26, 0:3], img) and float(pad[:, :6].abs().sum()) == 0


def test_cpu_predictor_restatement_single_tile_is_the_forward(fx):
    """the restated predictor on an image of exactly one tile, step 1, no mirroring / Gaussian, is the network's forward; with mirroring
    of a mirror-symmetric network input it averages M predictions."""
    W, x = _tiny(fx)
    net = lambda t: SO.forward(W, t, SO.TINY["depth"])      # noqa: E731
    with torch.no_grad():
        out = SO.predict_sliding_window(net, x[0], (32, 32, 32), 1.0)
        assert torch.allclose(out, torch.from_numpy(fx["logits"][0]), rtol=1e-5, atol=1e-5)
        m = SO.mirror_predict(net, x, (0, 2))
        want = (net(x) + net(x.flip(2)).flip(2) + net(x.flip(4)).flip(4) + net(x.flip(2, 4)).flip(2, 4)) / 4
        assert torch.allclose(m, want, rtol=1e-6, atol=1e-6)


def test_pretraining_encoder_loads_into_segmentation_network():
    """a pretraining checkpoint's encoder_weights_for_finetuning (load_stunet_ssl_weights) loads with strict=False; what stays missing is
    stage 5, the upsampling convs, the decoder blocks and the heads -- nothing of stages 0-4, nothing unexpected."""
    from anatomask_amd import checkpoint, modules
    cfg = modules.STUNET_CONFIGS["B"]
    spark = modules.build_spark(cfg["dims"], cfg["depth"], cfg["width"], (64, 64, 64))
    enc = checkpoint.encoder_weights_for_finetuning({"module." + k: v for k, v in spark.state_dict().items()})
    seg = S.STUNet(1, 105, depth=cfg["depth"], dims=cfg["dims"], pool_op_kernel_sizes=SO.RECIPE_POOL, conv_kernel_sizes=[[3, 3, 3]] * 6,
                   enable_deep_supervision=False)
    res = seg.load_state_dict(enc, strict=False)
    assert not res.unexpected_keys
    assert res.missing_keys and all(k.startswith(("conv_blocks_context.5.", "upsample_layers.", "conv_blocks_localization.", "seg_outputs."))
                                    for k in res.missing_keys)
    for k, v in enc.items():
        assert torch.equal(seg.state_dict()[k], v), k
