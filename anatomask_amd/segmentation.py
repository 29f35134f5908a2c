"""STUNet segmentation inference on the HIP engine: the network a pretrained encoder is finetuned into, and nnU-Net's sliding-window
predictor around it.

  STUNet                    P/STUNet.py:10-129 (same constructor, same state_dict keys and shapes; forward only)
  SlidingWindowPredictor    nnUNetPredictor.predict_sliding_window_return_logits, nnunetv2/inference/predict_from_raw_data.py:622-754,
                            with compute_gaussian / compute_steps_for_sliding_window of nnunetv2/inference/sliding_window_prediction.py

As in modules.py the torch modules are parameter containers: all arithmetic runs in the HIP library (engine.seg_forward, ops.seg_*).
Deliberate differences from the reference predictor: the accumulators are fp32 (the reference keeps fp16 ones), storage is bf16 / fp32
instead of fp16 autocast, the Gaussian is fp32 (not fp16), and the M mirrors of a tile run as one batch whose un-flipped features are
summed before the (linear) head is applied once.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import engine, ops
from .modules import BasicResBlock, _Decoder, _Standalone

_RECIPE_POOL = [[2, 2, 2]] * 4 + [[1, 1, 1]]


class Upsample_Layer_nearest(nn.Module):
    """P/STUNet.py:119-128 (parameters only): nearest upsampling then a 1x1 conv; the engine runs the conv at the coarse grid."""

    def __init__(self, input_channels, output_channels, pool_op_kernel_size, mode="nearest"):
        super().__init__()
        self.conv = nn.Conv3d(input_channels, output_channels, kernel_size=1)
        self.pool_op_kernel_size = pool_op_kernel_size
        self.mode = mode


class STUNet(nn.Module):
    """The full STUNet segmentation network, P/STUNet.py:10-93, inference only.

    Only the recipe the reference builds runs here: 3^3 kernels, pool [[2,2,2]]*4 + [[1,1,1]], one input channel; anything else raises
    NotImplementedError.  `compute_dtype` (torch.float32 or torch.bfloat16) selects the storage / matrix-core dtype, as on modules.STUNet."""

    compute_dtype = torch.float32

    def __init__(self, input_channels, num_classes, depth=[1, 1, 1, 1, 1, 1], dims=[32, 64, 128, 256, 512, 512],
                 pool_op_kernel_sizes=None, conv_kernel_sizes=None, enable_deep_supervision=True):
        super().__init__()
        pool_op_kernel_sizes = pool_op_kernel_sizes or _RECIPE_POOL       # (the reference requires both; None = the recipe, as modules.STUNet)
        conv_kernel_sizes = conv_kernel_sizes or [[3, 3, 3]] * 6
        if input_channels != 1:
            raise NotImplementedError(f"input_channels={input_channels}: only single-channel input is implemented")
        if [list(p) for p in pool_op_kernel_sizes] != _RECIPE_POOL:
            raise NotImplementedError(f"pool_op_kernel_sizes={pool_op_kernel_sizes}: only {_RECIPE_POOL} is implemented")
        if len(conv_kernel_sizes) != 6 or any(list(k) != [3, 3, 3] for k in conv_kernel_sizes):
            raise NotImplementedError(f"conv_kernel_sizes={conv_kernel_sizes}: only [[3, 3, 3]] * 6 is implemented")
        if len(dims) != 6 or len(depth) != 6 or any(d % 8 for d in dims) or min(depth) < 1:
            raise NotImplementedError(f"dims={dims}, depth={depth}: six stages, channel counts multiples of 8, depth >= 1")
        if dims[0] > ops.SEG_LDS_C:
            raise NotImplementedError(f"dims[0]={dims[0]}: the accumulating head takes at most {ops.SEG_LDS_C} channels")
        self.conv_op = nn.Conv3d
        self.input_channels, self.num_classes = input_channels, num_classes
        self.final_nonlin = lambda x: x
        self.decoder = _Decoder()
        self.decoder.deep_supervision = enable_deep_supervision
        self.upscale_logits = False
        self.dims, self.depth = list(dims), list(depth)
        self.pool_op_kernel_sizes, self.conv_kernel_sizes = pool_op_kernel_sizes, conv_kernel_sizes
        self.conv_pad_sizes = [[i // 2 for i in k] for k in conv_kernel_sizes]
        num_pool = len(pool_op_kernel_sizes)
        self.conv_blocks_context = nn.ModuleList()
        self.conv_blocks_context.append(nn.Sequential(
            BasicResBlock(input_channels, dims[0], 3, 1, use_1x1conv=True),
            *[BasicResBlock(dims[0], dims[0], 3, 1) for _ in range(depth[0] - 1)]))
        for d in range(1, num_pool + 1):
            self.conv_blocks_context.append(nn.Sequential(
                BasicResBlock(dims[d - 1], dims[d], 3, 1, stride=pool_op_kernel_sizes[d - 1], use_1x1conv=True),
                *[BasicResBlock(dims[d], dims[d], 3, 1) for _ in range(depth[d] - 1)]))
        self.upsample_layers = nn.ModuleList(
            [Upsample_Layer_nearest(dims[-1 - u], dims[-2 - u], pool_op_kernel_sizes[-1 - u]) for u in range(num_pool)])
        self.conv_blocks_localization = nn.ModuleList()
        for u in range(num_pool):
            self.conv_blocks_localization.append(nn.Sequential(
                BasicResBlock(dims[-2 - u] * 2, dims[-2 - u], 3, 1, use_1x1conv=True),
                *[BasicResBlock(dims[-2 - u], dims[-2 - u], 3, 1) for _ in range(depth[-2 - u] - 1)]))
        self.seg_outputs = nn.ModuleList([nn.Conv3d(dims[-2 - ds], num_classes, kernel_size=1) for ds in range(num_pool)])
        self.upscale_logits_ops = [lambda x: x for _ in range(num_pool - 1)]

    # ---------------------------------------------------------------- engine plumbing
    def _engine_ctx(self):
        """(W, PackCache): the fp32 masters under engine.NET and their packed compute-dtype copies (repacked when they may have changed)."""
        if self.compute_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"compute_dtype {self.compute_dtype}: bf16 or fp32")
        sa = self.__dict__.setdefault("_sa", _Standalone(self, engine.NET + ".", self.compute_dtype))
        if sa.dtype != self.compute_dtype:
            sa.dtype = self.compute_dtype
            sa.ptrs = None
        return sa.weights(), sa.pack

    def _head(self, u: int) -> Tuple[torch.Tensor, torch.Tensor]:
        h = self.seg_outputs[u]
        return h.weight.data.reshape(h.weight.shape[0], -1).float().contiguous(), h.bias.data.float().contiguous()

    def _check_inference(self):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("segmentation.STUNet is inference-only (no backward): call it under torch.no_grad() / torch.inference_mode() "
                               "or set requires_grad_(False)")

    def _check_input(self, x: torch.Tensor):
        if x.device.type != "cuda":
            raise RuntimeError("STUNet runs on the HIP engine: move the model and the input to a cuda (ROCm) device first")
        if x.dim() != 5 or x.shape[1] != 1:
            raise NotImplementedError(f"input {tuple(x.shape)}: (B, 1, D, H, W) only (single-channel input)")
        if any(v % 16 for v in x.shape[2:]):
            raise NotImplementedError(f"input {tuple(x.shape)}: spatial sizes must be multiples of 16")

    def features(self, x_bdhw: torch.Tensor, W=None, pk=None, all_levels: bool = False) -> List[torch.Tensor]:
        """decoder output features (channels-last, compute dtype) of x fp32 [B,D,H,W]: the last level, or levels 0..4 (coarse -> fine)."""
        if W is None:
            W, pk = self._engine_ctx()
        return engine.seg_forward(W, pk, x_bdhw, self.depth, all_levels=all_levels)

    def forward(self, x):
        """P/STUNet.py:70-93: x (B,1,D,H,W) fp32 -> logits (B,K,D,H,W) fp32, or with deep supervision the tuple of the five levels'
        logits, finest first (the reference's order)."""
        self._check_inference()
        self._check_input(x)
        W, pk = self._engine_ctx()
        inp = x[:, 0].float().contiguous()
        if not self.decoder.deep_supervision:
            f = self.features(inp, W, pk)[0]
            return ops.seg_head(f, *self._head(4))
        levels = self.features(inp, W, pk, all_levels=True)
        segs = [ops.seg_head(f, *self._head(u)) for u, f in enumerate(levels)]
        return tuple([segs[-1]] + segs[:-1][::-1])


# ====================================================================================== sliding window (host-side geometry)
def _gaussian_kernel1d(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage's order-0 Gaussian kernel (float64, normalised to sum 1)."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def compute_gaussian(tile_size: Sequence[int], sigma_scale: float = 1. / 8, value_scaling_factor: float = 1000.) -> torch.Tensor:
    """sliding_window_prediction.py:11-29 in fp32 on the host: gaussian_filter of a centred delta (mode 'constant', truncate 4) is the
    outer product of the three 1-D kernels, which scipy's axis-by-axis passes produce in float64 with the same roundings; then scaled to
    a maximum of value_scaling_factor and zeros replaced by the smallest non-zero value."""
    lines = []
    for n in tile_size:
        sigma = n * sigma_scale
        r = int(4.0 * float(sigma) + 0.5)
        k = _gaussian_kernel1d(sigma, r)
        line = np.zeros(n)
        c = n // 2
        for i in range(max(0, c - r), min(n, c + r + 1)):
            line[i] = k[i - c + r]
        lines.append(line)
    g = lines[0][:, None, None] * lines[1][None, :, None]
    g = g * lines[2][None, None, :]
    t = torch.from_numpy(g).float()
    t = t / torch.max(t) * value_scaling_factor
    t = t.float()
    t[t == 0] = torch.min(t[t != 0])
    return t


def compute_steps_for_sliding_window(image_size: Sequence[int], tile_size: Sequence[int], tile_step_size: float) -> List[List[int]]:
    """sliding_window_prediction.py:32-56 (whose image >= tile assert tests a non-empty list and never fires: an image smaller than the
    tile gets one step at 0, as there; the predictor pads to the tile first)."""
    assert 0 < tile_step_size <= 1, "step_size must be larger than 0 and smaller or equal to 1"
    target = [i * tile_step_size for i in tile_size]
    num_steps = [int(np.ceil((i - k) / j)) + 1 for i, j, k in zip(image_size, target, tile_size)]
    steps = []
    for d in range(len(tile_size)):
        max_step = image_size[d] - tile_size[d]
        actual = max_step / (num_steps[d] - 1) if num_steps[d] > 1 else 99999999999
        steps.append([int(np.round(actual * i)) for i in range(num_steps[d])])
    return steps


def padding_for(image_size: Sequence[int], patch_size: Sequence[int]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(pad_below, padded size) of acvl_utils' pad_nd_image(image, patch_size, 'constant', {'value': 0}, True): each spatial axis grows to
    at least the patch, diff // 2 below and the rest above.  (Restated from its documented behaviour; acvl_utils itself was not at hand.)"""
    new = tuple(max(int(i), int(p)) for i, p in zip(image_size, patch_size))
    below = tuple((n - i) // 2 for n, i in zip(new, image_size))
    return below, new


class SlidingWindowPredictor:
    """nnUNetPredictor.predict_sliding_window_return_logits (predict_from_raw_data.py:622-754) for a segmentation.STUNet:
    zero padding to the patch, tiles at compute_steps_for_sliding_window, all M mirrors of a tile in one network call, Gaussian-weighted
    fp32 accumulation on the device, crop back.  Works on one case [C=1, X, Y, Z]."""

    def __init__(self, network: STUNet, patch_size: Sequence[int], tile_step_size: float = 0.5, use_gaussian: bool = True,
                 use_mirroring: bool = True, allowed_mirroring_axes: Sequence[int] = (0, 1, 2)):
        if not isinstance(network, STUNet):
            raise TypeError("SlidingWindowPredictor drives a segmentation.STUNet")
        self.patch_size = tuple(int(p) for p in patch_size)
        if len(self.patch_size) != 3 or any(p <= 0 or p % 16 for p in self.patch_size):
            raise NotImplementedError(f"patch_size {patch_size}: three sizes, multiples of 16")
        if not 0 < tile_step_size <= 1:
            raise ValueError("tile_step_size must be in (0, 1]")
        self.network = network
        self.tile_step_size = float(tile_step_size)
        self.use_gaussian, self.use_mirroring = bool(use_gaussian), bool(use_mirroring)
        self.allowed_mirroring_axes = tuple(allowed_mirroring_axes) if allowed_mirroring_axes is not None else ()
        self._gauss: Dict[Tuple, torch.Tensor] = {}
        self.phase_seconds: Optional[Dict[str, float]] = None      # set by _run(timed=True): tools/seg_bench.py's split

    def _gaussian(self, device) -> torch.Tensor:
        key = (self.patch_size, str(device))
        if key not in self._gauss:                     # uploaded once per patch size
            self._gauss[key] = compute_gaussian(self.patch_size).to(device).contiguous()
        return self._gauss[key]

    def accumulate(self, image: torch.Tensor, list_of_parameters=None, timed: bool = False):
        """(acc, wsum, pad_below, size): every tile of the padded volume through the network and the accumulating head, once per state dict
        of `list_of_parameters` (None: the weights the network holds) into ONE accumulator pair.  seg_head_accumulate adds the Gaussian to
        wsum once per fold, so acc / wsum is the mean over the folds (predict_logits_from_preprocessed_data, predict_from_raw_data.py:562-620,
        without its division).  The network keeps the last fold's weights, as there."""
        net = self.network
        net._check_inference()
        if not isinstance(image, torch.Tensor) or image.dim() != 4:
            raise ValueError("image must be a 4-D torch.Tensor (c, x, y, z)")
        if image.shape[0] != 1:
            raise NotImplementedError(f"image with {image.shape[0]} channels: single-channel input only")
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("move the network to a cuda (ROCm) device first")
        folds = [None] if list_of_parameters is None else list(list_of_parameters)
        if not folds:
            raise ValueError("list_of_parameters is empty")
        vol = image[0].to(device=dev, dtype=torch.float32).contiguous()
        size = tuple(vol.shape)
        below, padded = padding_for(size, self.patch_size)
        steps = compute_steps_for_sliding_window(padded, self.patch_size, self.tile_step_size)
        axes = ops.mirror_axes_mask(self.allowed_mirroring_axes) if self.use_mirroring else 0
        K = net.num_classes
        acc = torch.zeros(K, *padded, device=dev, dtype=torch.float32)
        wsum = torch.zeros(*padded, device=dev, dtype=torch.float32)
        g = self._gaussian(dev) if self.use_gaussian else None
        tiles = torch.empty(1 << bin(axes).count("1"), *self.patch_size, device=dev, dtype=torch.float32)
        t = {"gather": 0.0, "network": 0.0, "head": 0.0} if timed else None
        ev = (lambda: torch.cuda.Event(enable_timing=True)) if timed else None
        for params in folds:
            if params is not None:
                net.load_state_dict(params)
            W, pk = net._engine_ctx()                  # re-fetched per fold: the packed copies and the head follow the new masters
            hw, hb = net._head(4)
            for sx in steps[0]:
                for sy in steps[1]:
                    for sz in steps[2]:
                        if timed:
                            e = [ev() for _ in range(4)]
                            e[0].record()
                        ops.seg_gather(vol, (sx - below[0], sy - below[1], sz - below[2]), self.patch_size, axes, out=tiles)
                        if timed:
                            e[1].record()
                        f = net.features(tiles, W, pk)[0]
                        if timed:
                            e[2].record()
                        ops.seg_head_accumulate(f, axes, hw, hb, g, acc, wsum, (sx, sy, sz))
                        if timed:
                            e[3].record()
                            torch.cuda.synchronize(dev)
                            t["gather"] += e[0].elapsed_time(e[1]) / 1e3
                            t["network"] += e[1].elapsed_time(e[2]) / 1e3
                            t["head"] += e[2].elapsed_time(e[3]) / 1e3
        self.phase_seconds = t
        return acc, wsum, below, size

    def _run(self, image: torch.Tensor, want_logits: bool, want_labels: bool, timed: bool = False, list_of_parameters=None):
        acc, wsum, below, size = self.accumulate(image, list_of_parameters, timed)
        return ops.seg_finalize(acc, wsum, below, size, want_logits, want_labels)

    def predict_sliding_window_return_logits(self, image: torch.Tensor) -> torch.Tensor:
        """image [1, X, Y, Z] -> logits fp32 [K, X, Y, Z] on the network's device."""
        return self._run(image, True, False)[0]

    def predict_labels(self, image: torch.Tensor) -> torch.Tensor:
        """image [1, X, Y, Z] -> argmax labels [X, Y, Z] (uint8 for K <= 255, else int16), from the finalize kernel."""
        return self._run(image, False, True)[1]

    def predict_logits_and_labels(self, image: torch.Tensor):
        return self._run(image, True, True)

    def predict_logits_from_preprocessed_data(self, image: torch.Tensor, list_of_parameters=None) -> torch.Tensor:
        """predict_from_raw_data.py:562-620: the mean over the folds (state dicts with the network's keys and shapes; None = the weights
        the network holds) of the sliding-window logits, fp32 [K, X, Y, Z].  Afterwards the network holds the last fold's weights."""
        return self._run(image, True, False, list_of_parameters=list_of_parameters)[0]

    def predict_probabilities_and_labels(self, image: torch.Tensor, list_of_parameters=None, regions_class_order=None,
                                         want_probabilities: bool = True):
        """(probabilities fp32 [K, X, Y, Z] or None, labels [X, Y, Z]) of the fold-mean logits, from the fused export kernel:
        LabelManager.apply_inference_nonlin + convert_probabilities_to_segmentation (label_handling.py:128-175).  Softmax + argmax of the
        logits, or, exactly when `regions_class_order` is given, sigmoid + the region rule."""
        acc, wsum, below, size = self.accumulate(image, list_of_parameters)
        return ops.seg_export(acc, wsum, below, size, "sigmoid" if regions_class_order is not None else "softmax", regions_class_order,
                              want_probabilities, True)
