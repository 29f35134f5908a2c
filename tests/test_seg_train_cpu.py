"""CPU: the ABI and the module API of the trainable segmentation network (anatomask_amd.seg_train, seg_bwd_ops.hip); no compute."""
import ctypes
import re

import pytest
import torch

from anatomask_amd import build, hip, ops, seg_train, segmentation as S
from tests import seg_oracle as SO


def test_header_declares_and_library_exports_the_backward_kernels():
    decl = hip.declared_functions()
    assert len(decl["am_seg_head_bwd"]) == 17 and len(decl["am_seg_upcat_bwd"]) == 11
    assert decl["am_seg_head_bwd"][-2] is ctypes.c_long                    # workspace_floats
    assert "seg_bwd_ops.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "am_seg_head_bwd") and hasattr(lib, "am_seg_upcat_bwd")


def test_workspace_formula_follows_the_header():
    txt = open(hip.HEADER).read()
    tile = int(re.search(r"#define AM_SEG_HEAD_BWD_TILE (\d+)", txt).group(1))
    slots = int(re.search(r"#define AM_SEG_HEAD_BWD_SLOTS (\d+)", txt).group(1))
    assert (ops.SEG_HEAD_BWD_TILE, ops.SEG_HEAD_BWD_SLOTS) == (tile, slots)
    assert ops.seg_head_bwd_workspace_floats(2, 210, 8, 3) == 2 * 4 * (3 * 8 + 3)              # 210 voxels: 4 tiles per sample
    assert ops.seg_head_bwd_workspace_floats(2, 128 ** 3, 32, 105) == slots * (105 * 32 + 105)  # bounded by the persistent grid


def _pair(ds=True):
    t = SO.TINY
    kw = dict(depth=t["depth"], dims=t["dims"], pool_op_kernel_sizes=SO.RECIPE_POOL, conv_kernel_sizes=[[3, 3, 3]] * 6, enable_deep_supervision=ds)
    return seg_train.STUNet(1, t["num_classes"], **kw), S.STUNet(1, t["num_classes"], **kw)


def test_state_dict_keys_and_round_trip_with_the_inference_network():
    t = SO.TINY
    train, infer = _pair()
    assert isinstance(train, S.STUNet)
    assert [(k, tuple(p.shape)) for k, p in train.state_dict().items()] == SO.state_keys(t["dims"], t["depth"], t["num_classes"])
    W = SO.seeded_weights(SO.state_keys(t["dims"], t["depth"], t["num_classes"]), 3)
    infer.load_state_dict(W)
    res = train.load_state_dict(infer.state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(train.state_dict()[k], v) for k, v in W.items())
    other = S.STUNet(1, t["num_classes"], depth=t["depth"], dims=t["dims"])
    other.load_state_dict(train.state_dict())
    assert all(torch.equal(other.state_dict()[k], v) for k, v in W.items())
    train.compute_dtype = torch.bfloat16                                    # the same switch as the parent's
    assert S.STUNet.compute_dtype == torch.float32 and infer.compute_dtype == torch.float32


def test_parent_errors_for_unsupported_configurations_and_cpu_tensors():
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):
        seg_train.STUNet(1, 3, pool_op_kernel_sizes=[[2, 2, 2]] * 5, conv_kernel_sizes=[[3, 3, 3]] * 6)
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        seg_train.STUNet(1, 3, pool_op_kernel_sizes=SO.RECIPE_POOL, conv_kernel_sizes=[[1, 3, 3]] + [[3, 3, 3]] * 5)
    with pytest.raises(NotImplementedError, match="input_channels"):
        seg_train.STUNet(2, 3)
    train, _ = _pair()
    x = torch.zeros(1, 1, 32, 32, 32)
    with pytest.raises(RuntimeError, match="cuda"):                          # grad enabled: the training path checks its input first
        train(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="cuda"):        # no_grad: the parent's path
        train(x)
