"""Thin torch-tensor front end of the C ABI: every function takes device tensors (channels-last
[B,D,H,W,C]; fp32 or bf16), extracts raw pointers + the current HIP stream, and calls the HIP
library.  torch is used for memory and streams only; no arithmetic happens here."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import hip
from .hip import ACT_LRELU, ACT_NONE, ACT_RELU6, CONV_DGRAD, CONV_FWD, CONVT_DGRAD, CONVT_FWD  # noqa: F401


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return hip.DT_F32
    if t.dtype == torch.bfloat16:
        return hip.DT_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


# fp32-storage models compute their matrix products in one of two ways: exact fp32 products (v_mfma_f32_16x16x4_f32, the parity mode: 1/16
# of the bf16 matrix rate) or AM_DT_F32S: products from bf16 hi / lo splits of both operands with fp32 accumulation (16 significant bits
# per operand, 1/4 of the bf16 rate in the convolutions, three bf16 passes in the weight gradients).  The mode is a property of a MODEL
# (SparK.f32_split -> its PackCache): it travels with every packed weight copy (`_am_f32_split`, set by pack_weight) into conv3d and is an
# explicit argument of conv3d_wgrad -- no process-wide switch.  DEFAULT_F32_SPLIT is only what a newly CONSTRUCTED model starts with
# (anatomask_amd.set_f32_products).  The reference computes in fp32 (AMP = False, P/pretrain_AntoMask.py:239).
DEFAULT_F32_SPLIT = False


def _dtc(t: torch.Tensor, f32_split: bool) -> int:
    """dtype code of a CONVOLUTION operand (am_conv3d / am_pack_weight / am_packed_dims / am_conv3d_partials_rows)."""
    return hip.DT_F32S if (t.dtype == torch.float32 and f32_split) else _dt(t)


def _is_split(w_packed: torch.Tensor) -> bool:
    """the fp32 product mode a packed weight copy was made for (False for anything pack_weight did not mark)."""
    return getattr(w_packed, "_am_f32_split", False) is True


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class MaskInfo:
    """uint8 patch mask [B, fd, fh, fw] (1 = active)."""

    def __init__(self, mask_u8: torch.Tensor, n_active: Optional[int] = None):
        """n_active: number of active patches when the caller knows it (the trainer: B * len_keep); otherwise it is counted on
        first use (one host synchronisation, as the reference's `nonzero` calls incur in every layer)."""
        assert mask_u8.dtype == torch.uint8 and mask_u8.dim() == 4 and mask_u8.is_contiguous()
        self.t = mask_u8
        self.B, self.fd, self.fh, self.fw = mask_u8.shape
        self.n_active = n_active
        self._list: Optional[torch.Tensor] = None

    def active_list(self):
        """(device int32 list of the active patches, their number) -- built once per mask (am_mask_compact)."""
        if self._list is None:
            if max(self.B, self.fd, self.fh, self.fw) > 255:
                return None, 0
            if self.n_active is None:
                self.n_active = int(self.t.count_nonzero().item())
            buf = torch.empty(self.t.numel() + 1, device=self.t.device, dtype=torch.int32)
            hip.lib().mask_compact(self.t.data_ptr(), self.B, self.fd, self.fh, self.fw, buf.data_ptr(), buf[-1:].data_ptr(), _stream())
            self._list = buf
        return self._list, self.n_active

    @staticmethod
    def from_bool(active_b1fff: torch.Tensor, device) -> "MaskInfo":
        m = active_b1fff.reshape(active_b1fff.shape[0], *active_b1fff.shape[-3:]).to(device=device, dtype=torch.uint8).contiguous()
        return MaskInfo(m)


def _mk(mask: Optional[MaskInfo]):
    if mask is None:
        return None, 1, 1, 1
    return mask.t.data_ptr(), mask.fd, mask.fh, mask.fw


def _al(mask: Optional[MaskInfo]):
    """(active-patch list pointer, n_active) for the row-walk kernels, or (None, 0)."""
    if mask is None:
        return None, 0
    lst, n = mask.active_list()
    return (lst.data_ptr(), n) if lst is not None and n > 0 else (None, 0)


# ------------------------------------------------------------------ weights
def packed_dims(dtype: torch.dtype, rows: int, k: int):
    """Same rule as am_packed_dims: rows to the 32/64-channel output tile, K to the 64-byte channel slab."""
    tile = 32 if rows <= 32 else 64
    kc = 32 if dtype == torch.bfloat16 else 16
    return (rows + tile - 1) // tile * tile, (k + kc - 1) // kc * kc


class ConvPartials:
    """Per-workgroup per-channel (sum, sumsq) rows a conv launch leaves behind for the norm / bias-grad that follows.
    sum_only: the launch was asked for the SUM column alone (conv3d(partials_sum_only=True)); the sum-of-squares column may hold zeros,
    so everything that reads it (statistics, norm-backward sums) refuses such rows."""
    sum_only = False

    def __init__(self, mode, ksize, stride, B, out_spatial, cout, device, out_sparse=False, out_bshift=0, dtype=hip.DT_F32, cin=64, n_active=0):
        import ctypes
        n = ctypes.c_int(0)
        hip.lib().conv3d_partials_rows(mode, dtype, ksize, stride, B, *out_spatial, cin, cout, int(out_sparse), out_bshift, n_active, ctypes.addressof(n))
        self.rows, self.C = n.value, cout
        self.t = torch.empty(self.rows, cout, 2, device=device, dtype=torch.float32)

    def reduce(self, sums: Optional[torch.Tensor] = None, sum_accum: Optional[torch.Tensor] = None):
        assert sums is None or not self.sum_only, "sum-only rows carry no sum of squares"
        hip.lib().partials_reduce(self.t.data_ptr(), self.rows, self.C, _p(sums), _p(sum_accum), _stream())

    def finalize(self, st: Optional["NormStats"], gamma=None, beta=None, eps: float = 0.0, run_mean=None, run_var=None,
                 momentum: float = 0.1, num_batches_tracked=None, sum_accum: Optional[torch.Tensor] = None):
        """partials -> per-channel sums -> mean / rstd / scale / shift of `st` (+ BN running stats, num_batches_tracked) in ONE
        launch (am_partials_finalize); st None: only `sum_accum[c] += sum` (bias gradients)."""
        assert st is None or not self.sum_only, "sum-only rows carry no sum of squares"
        ws = _stats_workspace(self.t.device, self.C)
        norm = (None, 1.0, None, None, 0.0, None, None, None, None, None, None, 0.0, None) if st is None else (
            _p(st.count_ptr), float(st.count_host), gamma.data_ptr(), beta.data_ptr(), eps, st.mean.data_ptr(), st.rstd.data_ptr(),
            st.scale.data_ptr(), st.shift.data_ptr(), _p(run_mean), _p(run_var), momentum, _p(num_batches_tracked))
        hip.lib().partials_finalize(self.t.data_ptr(), self.rows, self.C, ws.data_ptr(), *norm, _p(sum_accum), _stream())
        if st is not None:
            st.nrep = 1


    def finalize_bwd(self, st: "NormStats", gamma: torch.Tensor, sc: "NormBwdScratch", dgamma=None, dbeta=None, dbeta2=None):
        """rows of a conv3d(norm_bwd=...) launch -> k0 / k1 / k2 of the apply pass + the affine gradients (am_norm_bwd_from_partials)."""
        assert not self.sum_only, "sum-only rows carry no second column"
        ws = _stats_workspace(self.t.device, self.C)
        hip.lib().norm_bwd_from_partials(self.t.data_ptr(), self.rows, self.C, ws.data_ptr(), _p(st.count_ptr), float(st.count_host),
                                         gamma.data_ptr(), st.mean.data_ptr(), st.rstd.data_ptr(), sc.k[0].data_ptr(), sc.k[1].data_ptr(),
                                         sc.k[2].data_ptr(), _p(dgamma), _p(dbeta), _p(dbeta2), _stream())


_WS = {}


FIN_REP = 16   # AM_FIN_REP


def _stats_workspace(device, C: int) -> torch.Tensor:
    """zero-initialised scratch of am_partials_finalize (left zero by every call), one per (device, stream)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < FIN_REP * 2 * C + 2:
        ws = _WS[key] = torch.zeros(FIN_REP * 2 * max(C, 2048) + 2, device=device, dtype=torch.float64)
    return ws


import ctypes as _ct

_ROWS_OUT = _ct.c_int(0)
_ROWS_ADDR = _ct.addressof(_ROWS_OUT)


def pack_weight(w: torch.Tensor, dtype: torch.dtype, transposed_conv: bool, for_dgrad: bool, f32_split: bool = False) -> torch.Tensor:
    """torch-layout fp32 weight -> packed [taps][rows][K] in `dtype`.
    Conv3d weight (Cout,Cin,k,k,k); ConvTranspose3d weight (Cin,Cout,k,k,k).
    forward: rows = output channels, K = input channels; dgrad: swapped."""
    d0, d1 = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    cout, cin = (d1, d0) if transposed_conv else (d0, d1)
    s_out, s_in = (taps, d1 * taps) if transposed_conv else (d1 * taps, taps)
    if not for_dgrad:
        R, K, sr, sk = cout, cin, s_out, s_in
    else:
        R, K, sr, sk = cin, cout, s_in, s_out
    Rp, Kp = packed_dims(dtype, R, K)
    out = torch.empty(taps, Rp, Kp, device=w.device, dtype=dtype)
    split = bool(out.dtype == torch.float32 and f32_split)
    hip.lib().pack_weight(_dtc(out, split), w.data_ptr(), out.data_ptr(), R, K, taps, sr, sk, Rp, Kp, _stream())
    out.logical = (R, K)
    out._am_f32_split = split      # (what the copy was made for: conv3d launches the matching kernels, PackCache re-makes it when the mode changes)
    out.pack_args = (R, K, taps, sr, sk, Rp, Kp)
    return out


class PackTable:
    """Device table of am_pack_desc for `am_pack_weights_batched`: every (master weight, packed copy) pair of a model."""

    def __init__(self, pairs, dtype: torch.dtype, device, f32_split: bool = False):
        import struct
        self.f32_split = bool(dtype == torch.float32 and f32_split)
        blob, first = b"", 0
        for w, out in pairs:
            R, K, taps, sr, sk, Rp, Kp = out.pack_args
            assert taps <= 64
            blob += struct.pack("<QQqqiiiiii", w.data_ptr(), out.data_ptr(), sr, sk, R, K, taps, Rp, Kp, first)
            first += Rp * ((Kp + 63) // 64)
        self.n, self.blocks, self.dtype = len(pairs), first, dtype
        self.ptrs = [(w.data_ptr(), out.data_ptr()) for w, out in pairs]
        self.dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)

    def matches(self, pairs) -> bool:
        return len(pairs) == self.n and all(p == (w.data_ptr(), o.data_ptr()) for p, (w, o) in zip(self.ptrs, pairs))

    def repack(self):
        code = hip.DT_BF16 if self.dtype == torch.bfloat16 else (hip.DT_F32S if self.f32_split else hip.DT_F32)
        hip.lib().pack_weights_batched(code, self.dev.data_ptr(), self.n, self.blocks, _stream())


def unpack_grad(dw_packed: torch.Tensor, grad_out: torch.Tensor, transposed_conv: bool, accumulate: bool):
    """packed fp32 [taps][Cy][Cx] (Cy = forward-output channels) -> torch-layout gradient."""
    taps, R, K = dw_packed.shape
    d1 = grad_out.shape[1]
    if transposed_conv:      # weight (Cin=Cx, Cout=Cy, taps)
        sr, sk = taps, d1 * taps
    else:                    # weight (Cout=Cy, Cin=Cx, taps)
        sr, sk = d1 * taps, taps
    hip.lib().unpack_grad(dw_packed.data_ptr(), grad_out.data_ptr(), R, K, taps, sr, sk, int(accumulate), _stream())


# ------------------------------------------------------------------ convolutions
def conv3d(mode: int, x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], out_spatial: Tuple[int, int, int],
           ksize: int, stride: int, in_mask: Optional[MaskInfo] = None, in_bshift: int = 0,
           out_mask: Optional[MaskInfo] = None, out_bshift: int = 0, out: Optional[torch.Tensor] = None,
           accumulate: bool = False, want_partials: bool = False, ep_scale: Optional[torch.Tensor] = None,
           ep_shift: Optional[torch.Tensor] = None, ep_res: Optional[torch.Tensor] = None, ep_act: int = 0,
           norm_bwd: Optional[tuple] = None, partials_sum_only: bool = False):
    """partials_sum_only (with want_partials): only the per-channel SUM of the rows will be read (AM_CONV_PARTIALS_SUM_ONLY).
    ep_*: fused store epilogue y = act(conv * scale + shift + res) (eval-mode BatchNorm / skip add / activation).
    norm_bwd = (x_pre, st, act): the output is the gradient wrt act(norm(x_pre)); the launch also leaves the norm-backward sums in
    its partial rows (am_conv3d_nbred) -> returns (out, rows) for norm_backward(..., reduced=rows).  bf16 only."""
    B, Di, Hi, Wi, Cin = x.shape
    Cout, Kl = w_packed.logical
    assert Kl == Cin and w_packed.dtype == x.dtype, (w_packed.logical, x.shape)
    Do, Ho, Wo = out_spatial
    mk = in_mask or out_mask
    mp, fd, fh, fw = _mk(mk)
    # the active-patch list: thin block-sparse layers (Cin <= 32) run on the resident-weight kernel, which walks the active bricks, and the
    # levels whose patches are smaller than a brick on the voxel-list gather kernel (conv_gather.hip)
    # (the list is that of OUT_mask: launches with a block-sparse output enumerate their live bricks from it)
    alp, aln = _al(out_mask) if (out_mask is not None and x.dtype == torch.bfloat16) else (None, 0)
    if norm_bwd is not None:
        xp, st, nact = norm_bwd
        assert x.dtype == torch.bfloat16 and xp.dtype == torch.bfloat16 and tuple(xp.shape) == (B, Do, Ho, Wo, Cout) and bias is None
        part = ConvPartials(mode, ksize, stride, B, out_spatial, Cout, x.device, out_mask is not None, out_bshift, _dt(x), 64, 0)   # (cin 64: the generic kernel's row count)
        if out is None:
            out = torch.empty(B, Do, Ho, Wo, Cout, device=x.device, dtype=x.dtype)
        hip.lib().conv3d_nbred(mode, _dt(x), ksize, stride, x.data_ptr(), w_packed.data_ptr(), out.data_ptr(),
                               B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout,
                               in_mask.t.data_ptr() if in_mask else None, in_bshift,
                               out_mask.t.data_ptr() if out_mask else None, out_bshift, fd, fh, fw, int(accumulate),
                               part.t.data_ptr(), xp.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), int(nact), _ROWS_ADDR, _stream())
        part.rows = _ROWS_OUT.value
        return out, part
    split = _is_split(w_packed)                                  # (the fp32 product mode rides on the packed weight copy)
    part = ConvPartials(mode, ksize, stride, B, out_spatial, Cout, x.device, out_mask is not None, out_bshift, _dtc(x, split), Cin, aln) if want_partials else None
    if out is None:
        out = torch.empty(B, Do, Ho, Wo, Cout, device=x.device, dtype=x.dtype)
    rows = _ROWS_OUT
    hip.lib().conv3d(mode, _dtc(x, split), ksize, stride, x.data_ptr(), w_packed.data_ptr(), _p(bias), out.data_ptr(),
                     B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout,
                     in_mask.t.data_ptr() if in_mask else None, in_bshift,
                     out_mask.t.data_ptr() if out_mask else None, out_bshift, fd, fh, fw,
                     int(accumulate) | (2 if (partials_sum_only and part is not None) else 0),
                     part.t.data_ptr() if part else None, _p(ep_scale), _p(ep_shift),
                     ep_res.data_ptr() if ep_res is not None else None, int(ep_act), alp, aln, _ROWS_ADDR if part else None, _stream())
    if part is not None:
        part.rows = rows.value                                   # what this launch actually wrote (<= the allocated bound)
        part.sum_only = bool(partials_sum_only)
    return (out, part) if want_partials else out


def conv3d_prenorm_supported(x: torch.Tensor, w_packed: torch.Tensor, out_spatial, ksize: int, stride: int, mask: Optional[MaskInfo], out_bshift: int) -> bool:
    """am_conv3d_prenorm serves this launch (bf16, Cin <= 32, k3, block-sparse with an active-patch list: conv_rw.hip)."""
    if mask is None or x.dtype != torch.bfloat16 or _is_split(w_packed):
        return False
    lst, n = mask.active_list()
    if lst is None or n <= 0:
        return False
    Cout, Cin = w_packed.logical
    return hip.lib()._lib.am_conv3d_prenorm_supported(CONV_FWD, _dt(x), ksize, stride, x.shape[0], *out_spatial, Cin, Cout, 1,
                                                      out_bshift + (1 if stride == 2 else 0), out_bshift, n) == 1


def conv3d_prenorm(x: torch.Tensor, st: "NormStats", act: int, w_packed: torch.Tensor, bias: Optional[torch.Tensor], out_spatial, ksize: int,
                   stride: int, mask: MaskInfo, out_bshift: int, want_partials: bool = False):
    """conv(act(x * st.scale + st.shift)) with the norm + activation applied while the source rows are staged: the normalised map
    never exists (passes that keep no tape).  x: the norm's INPUT, block-sparse under `mask`."""
    B, Di, Hi, Wi, Cin = x.shape
    Cout, Kl = w_packed.logical
    assert Kl == Cin and w_packed.dtype == x.dtype
    Do, Ho, Wo = out_spatial
    lst, n = mask.active_list()
    part = ConvPartials(CONV_FWD, ksize, stride, B, out_spatial, Cout, x.device, True, out_bshift, _dt(x), Cin, n) if want_partials else None
    out = torch.empty(B, Do, Ho, Wo, Cout, device=x.device, dtype=x.dtype)
    hip.lib().conv3d_prenorm(CONV_FWD, _dt(x), ksize, stride, x.data_ptr(), w_packed.data_ptr(), _p(bias), out.data_ptr(), B, Di, Hi, Wi, Cin,
                             Do, Ho, Wo, Cout, mask.t.data_ptr(), out_bshift + (1 if stride == 2 else 0), out_bshift, mask.fd, mask.fh, mask.fw,
                             part.t.data_ptr() if part else None, st.scale.data_ptr(), st.shift.data_ptr(), int(act), lst.data_ptr(), n,
                             _ROWS_ADDR if part else None, _stream())
    if part is not None:
        part.rows = _ROWS_OUT.value
    return (out, part) if want_partials else out


# Deterministic weight gradients (am_conv3d_wgrad's det_workspace): per-slot partial sums + an ordered fold instead of fp32 atomics.
# A property of a MODEL (SparK.deterministic_wgrad -> its PackCache -> the `deterministic` argument of the three gradient ops below);
# DETERMINISTIC_WGRAD is only what a direct caller of these ops gets when it passes deterministic=None (tests, tools).
DETERMINISTIC_WGRAD = False


def _det(flag) -> bool:
    return DETERMINISTIC_WGRAD if flag is None else bool(flag)
_DET_WS: dict = {}


def _det_workspace(device, floats_per_slot: int):
    """one cached workspace per device and stream (the side stream's weight gradients run concurrently with the main stream's):
    256 MB, or 8 slots of the largest gradient if that is more."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    need = max(64 << 20, 8 * floats_per_slot)
    t = _DET_WS.get(key)
    if t is None or t.numel() < need:
        t = _DET_WS[key] = torch.empty(need, device=device, dtype=torch.float32)
    return t


GATHER_WGRAD = True      # (tools: same-process A/B of the gather-form weight gradient)


def conv3d_wgrad(mode: int, x: torch.Tensor, dy: torch.Tensor, ksize: int, stride: int,
                 x_mask: Optional[MaskInfo] = None, x_bshift: int = 0, y_mask: Optional[MaskInfo] = None,
                 y_bshift: int = 0, f32_split: bool = False, deterministic: Optional[bool] = None) -> torch.Tensor:
    B, Dx, Hx, Wx, Cx = x.shape
    _, Dy, Hy, Wy, Cy = dy.shape
    taps = ksize ** 3
    dw = torch.zeros(taps, Cy, Cx, device=x.device, dtype=torch.float32)
    mk = x_mask or y_mask
    mp, fd, fh, fw = _mk(mk)
    ws = _det_workspace(x.device, taps * Cy * Cx) if _det(deterministic) else None

    al = _al(y_mask)
    # levels with 1- / 2-voxel patches: the gather form (K-major copies of the active voxels + plain GEMMs) needs scratch
    gb = 0
    if GATHER_WGRAD and al[1] > 0 and x.dtype == torch.bfloat16 and y_bshift <= 1:
        out_b = _ct.c_long(0)
        hip.lib().conv3d_wgrad_gather_bytes(mode, _dt(x), ksize, stride, B, Cx, Cy, y_bshift, int(y_mask is not None), al[1], fd, fh, fw, _ct.byref(out_b))
        gb = int(out_b.value)
    gws = torch.empty(gb, device=x.device, dtype=torch.uint8) if gb > 0 else None

    def launch(xx, yy):
        hip.lib().conv3d_wgrad(mode, _dt(xx), ksize, stride, xx.data_ptr(), yy.data_ptr(), dw.data_ptr(),
                               B, Dx, Hx, Wx, Cx, Dy, Hy, Wy, Cy,
                               x_mask.t.data_ptr() if x_mask else None, x_bshift,
                               y_mask.t.data_ptr() if y_mask else None, y_bshift, fd, fh, fw,
                               ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, *al,
                               gws.data_ptr() if gws is not None else None, gb, _stream())
    if x.dtype == torch.float32 and f32_split:
        # AM_DT_F32S: dW = X^T dY with X = Xh + Xl, dY = Yh + Yl (bf16 planes, am_split_bf16): three bf16 matrix-core contractions
        # accumulate into the ONE fp32 gradient (atomics, or the deterministic fold: both add into dw); the lo lo term (2^-16 of the
        # result) is dropped.  The planes are transient (2 x 2 bytes per element = the size of the fp32 tensor).
        xh, xl = split_bf16(x)
        yh, yl = split_bf16(dy)
        launch(xh, yh); launch(xl, yh); launch(xh, yl)
        return dw
    launch(x, dy)
    return dw


def split_bf16(x: torch.Tensor):
    """fp32 tensor -> (hi, lo) bf16 tensors of the same shape: hi = bf16(x), lo = bf16(x - hi) (am_split_bf16)."""
    x = x.contiguous()
    hi, lo = torch.empty_like(x, dtype=torch.bfloat16), torch.empty_like(x, dtype=torch.bfloat16)
    hip.lib().split_bf16(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), x.numel(), _stream())
    return hi, lo


def stem_conv_fwd(x_b1: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], mask: Optional[MaskInfo], bshift: int,
                  dtype: torch.dtype, want_partials: bool = False, out: Optional[torch.Tensor] = None):
    """x_b1: fp32 [B,D,H,W]; w: (C,1,k,k,k) fp32.  want_partials: also return the (sum, sumsq) rows for the norm that follows."""
    B, D, H, W = x_b1.shape
    Cc, k = w.shape[0], w.shape[2]
    y = torch.empty(B, D, H, W, Cc, device=x_b1.device, dtype=dtype) if out is None else out
    mp, fd, fh, fw = _mk(mask)
    part = None
    if want_partials:
        part = ConvPartials.__new__(ConvPartials)
        part.rows, part.C = B * (D // 4) * (H // 8) * (W // 16), Cc
        part.t = torch.empty(part.rows, Cc, 2, device=x_b1.device, dtype=torch.float32)
    hip.lib().stem_conv_fwd(_dt(y), x_b1.data_ptr(), B, D, H, W, Cc, k, mp, bshift, fd, fh, fw, w.data_ptr(), _p(bias),
                            y.data_ptr(), part.t.data_ptr() if part else None, *_al(mask), _ROWS_ADDR if part else None, _stream())
    if part is not None:
        part.rows = _ROWS_OUT.value
    return (y, part) if want_partials else y


def stem_conv_wgrad(x_b1: torch.Tensor, dy: torch.Tensor, ksize: int, mask: Optional[MaskInfo], bshift: int,
                    dw_accum: torch.Tensor, db_accum: Optional[torch.Tensor], deterministic: Optional[bool] = None):
    B, D, H, W, Cc = dy.shape
    mp, fd, fh, fw = _mk(mask)
    ws = _det_workspace(dy.device, 1024 * Cc * (ksize ** 3 + 1) // 8) if (_det(deterministic) and dy.dtype == torch.bfloat16) else None
    hip.lib().stem_conv_wgrad(_dt(dy), x_b1.data_ptr(), dy.data_ptr(), B, D, H, W, Cc, ksize, mp, bshift, fd, fh, fw,
                              dw_accum.data_ptr(), _p(db_accum), *_al(mask), _p(ws), ws.numel() if ws is not None else 0, _stream())


# ------------------------------------------------------------------ norms
NREP = 8   # AM_NREP
DXREP = 64  # AM_DXREP


class NormStats:
    """Per-channel statistics + folded coefficients of one norm instance (all fp32, length C)."""

    def __init__(self, C: int, device):
        self.sums = torch.empty(NREP, C, 2, device=device, dtype=torch.float64)
        self.nrep = NREP
        self.buf = torch.empty(4, C, device=device, dtype=torch.float32)
        self.mean, self.rstd, self.scale, self.shift = self.buf[0], self.buf[1], self.buf[2], self.buf[3]
        self.count_ptr: Optional[torch.Tensor] = None
        self.count_host: float = 0.0
        self.sync_world: int = 1          # > 1: SyncBatchNorm statistics (the backward all-reduces its two sums as well)


def chan_stats(x: torch.Tensor, mask: Optional[MaskInfo], bshift: int, st: NormStats):
    B, D, H, W, Cc = x.shape
    mp, fd, fh, fw = _mk(mask)
    hip.lib().chan_stats(_dt(x), x.data_ptr(), B, D, H, W, Cc, mp, bshift, fd, fh, fw, st.sums.data_ptr(), *_al(mask), _stream())
    st.nrep = NREP


def mask_count(mask: MaskInfo, voxels_per_patch: int, out: torch.Tensor):
    hip.lib().mask_count(mask.t.data_ptr(), mask.t.numel(), voxels_per_patch, out.data_ptr(), _stream())


def norm_finalize(st: NormStats, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                  run_mean: Optional[torch.Tensor] = None, run_var: Optional[torch.Tensor] = None, momentum: float = 0.1):
    Cc = gamma.numel()
    hip.lib().norm_finalize(st.sums.data_ptr(), st.nrep, _p(st.count_ptr), float(st.count_host), Cc, gamma.data_ptr(), beta.data_ptr(),
                            eps, st.mean.data_ptr(), st.rstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(),
                            _p(run_mean), _p(run_var), momentum, _stream())


def norm_fold_running(st: NormStats, gamma, beta, run_mean, run_var, eps: float):
    hip.lib().norm_fold_running(gamma.numel(), gamma.data_ptr(), beta.data_ptr(), run_mean.data_ptr(), run_var.data_ptr(), eps,
                                st.scale.data_ptr(), st.shift.data_ptr(), _stream())


def norm_apply(x: torch.Tensor, st: NormStats, act: int, mask: Optional[MaskInfo] = None, bshift: int = 0,
               res: Optional[torch.Tensor] = None, stem: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
               fill: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, D, H, W, Cc = x.shape
    if out is None:
        out = torch.empty_like(x)
    mp, fd, fh, fw = _mk(mask)
    sx, sw, sb = stem if stem is not None else (None, None, None)
    hip.lib().norm_apply(_dt(x), x.data_ptr(), B, D, H, W, Cc, mp, bshift, fd, fh, fw, st.scale.data_ptr(), st.shift.data_ptr(),
                         act, _p(res), _p(sx), _p(sw), _p(sb), _p(fill), out.data_ptr(), *_al(mask), _stream())
    return out


class NormBwdScratch:
    def __init__(self, C: int, device):
        self.k = torch.empty(3, C, device=device, dtype=torch.float32)


def norm_backward(dout: torch.Tensor, out: Optional[torch.Tensor], x: torch.Tensor, st: NormStats, gamma: torch.Tensor, act: int,
                  mask: Optional[MaskInfo], bshift: int, dgamma: Optional[torch.Tensor], dbeta: Optional[torch.Tensor],
                  dtoken: Optional[torch.Tensor] = None, fill: bool = False, dx: Optional[torch.Tensor] = None,
                  dres: Optional[torch.Tensor] = None, scratch: Optional[NormBwdScratch] = None,
                  dbeta2: Optional[torch.Tensor] = None, dxsum: Optional[torch.Tensor] = None,
                  reduced: Optional[ConvPartials] = None) -> torch.Tensor:
    """Backward of y = act(norm(x) [+res]) (or the densify fill).  Returns dx; accumulates dgamma/dbeta/dtoken.
    out=None with an activation (layers WITHOUT a residual): the derivative comes from the recomputed x*st.scale + st.shift.
    reduced: the partial rows of the conv3d(norm_bwd=(x, st, act)) launch that produced dout -- the reduce pass is skipped."""
    B, D, H, W, Cc = x.shape
    sc = scratch or NormBwdScratch(Cc, x.device)
    L = hip.lib()
    s = _stream()
    ws_b, ws_x = _bwd_workspaces(x.device, Cc)
    mp, fd, fh, fw = _mk(mask)
    geo = (B, D, H, W, Cc, mp, bshift, fd, fh, fw)
    k = [sc.k[i].data_ptr() for i in range(3)]
    grads = (_p(dgamma), _p(dbeta), _p(dtoken), _p(dbeta2))
    sync = st.sync_world > 1
    # the reduce's last workgroup folds the sums into k0/k1/k2 and the parameter gradients, unless the sums have to be all-reduced
    # first (SyncBatchNorm) or the three-launch form is asked for (tools/step_ab.py: same-process A/B timing)
    fused_tail = FUSED_BWD_TAILS and not sync
    need_finalize = reduced is None and not fused_tail       # a separate norm_bwd_finalize launch
    if reduced is not None:
        assert not sync and out is None and dtoken is None and not fill
        reduced.finalize_bwd(st, gamma, sc, dgamma, dbeta, dbeta2)
    else:
        fin = (_p(st.count_ptr), float(st.count_host), gamma.data_ptr(), *k, *grads) if fused_tail else (None, 0.0) + (None,) * 8
        L.norm_bwd_reduce(_dt(x), dout.data_ptr(), _p(out), x.data_ptr(), *geo, st.mean.data_ptr(), st.rstd.data_ptr(), act, int(fill),
                          ws_b.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), *_al(mask), *fin, s)
    if need_finalize:
        bsum = ws_b[:NREP * Cc * 3]
        # SyncBatchNorm backward (torch.nn.SyncBatchNorm): dx needs the sums over the GLOBAL batch (count_host), the affine gradients stay
        # LOCAL sums (DDP then averages them like every other gradient): reduce -> finalize (param grads) -> all-reduce -> finalize (k's)
        L.norm_bwd_finalize(ws_b.data_ptr(), None if sync else _p(st.count_ptr), float(st.count_host), Cc, gamma.data_ptr(),
                            st.rstd.data_ptr(), *k, *grads, s)
        if sync:
            import torch.distributed as dist
            dist.all_reduce(bsum)
            L.norm_bwd_finalize(ws_b.data_ptr(), None, float(st.count_host), Cc, gamma.data_ptr(), st.rstd.data_ptr(), *k,
                                None, None, None, None, s)
        bsum.zero_()                                                   # the shared workspaces' contract: zero on entry, LEFT zero
    if dx is None:
        dx = torch.empty_like(x)
    zero_ws = sync or not need_finalize                      # ws_x is the zero workspace: the apply's last workgroup folds the dxsum replicas itself
    L.norm_bwd_apply(_dt(x), dout.data_ptr(), _p(out), x.data_ptr(), *geo, st.mean.data_ptr(), st.rstd.data_ptr(), *k, act,
                     dx.data_ptr(), _p(dres), _p(dxsum), ws_x.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), *_al(mask), int(zero_ws), s)
    if dxsum is not None and not zero_ws:
        ws_x[:DXREP * Cc].zero_()
    return dx


_BWS = {}
FUSED_BWD_TAILS = True
# bf16: the norm-backward reduce of a data gradient rides in the dgrad's epilogue (am_conv3d_nbred).  Measured neutral on the STUNet-B
# step (143.0 vs 142.7-143.3 ms, tools/step_ab.py ops.FUSED_NORM_BWD_REDUCE=1,0; profiles/r02_experiments.md), so it stays off.
FUSED_NORM_BWD_REDUCE = False


def _bwd_workspaces(device, C: int):
    """zero-initialised accumulators of the fused backward tails (left zero by every call), one pair per (device, stream)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _BWS.get(key)
    if ws is None or ws[2] < C:
        cap = max(C, 2048)
        ws = _BWS[key] = (torch.zeros(NREP * cap * 3 + 2, device=device, dtype=torch.float64),
                          torch.zeros(DXREP * cap + 2, device=device, dtype=torch.float64), cap)
    return ws[0], ws[1]


def chan_sum(x: torch.Tensor, mask: Optional[MaskInfo], bshift: int, out_accum: torch.Tensor):
    B, D, H, W, Cc = x.shape
    mp, fd, fh, fw = _mk(mask)
    hip.lib().chan_sum(_dt(x), x.data_ptr(), B, D, H, W, Cc, mp, bshift, fd, fh, fw, out_accum.data_ptr(), _stream())


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(a)
    hip.lib().add(_dt(a), a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream())
    return out


# ------------------------------------------------------------------ proj / loss / sampler / optimizer
def proj_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, pre: Optional["NormStats"] = None) -> torch.Tensor:
    """pre: x is the INPUT of the (train-mode) BatchNorm `pre`; rec = proj(x * pre.scale + pre.shift), the BatchNorm output is never written."""
    B, D, H, W, Cc = x.shape
    rec = torch.empty(B, D, H, W, device=x.device, dtype=torch.float32)
    hip.lib().proj_fwd(_dt(x), x.data_ptr(), B * D * H * W, Cc, w.data_ptr(), b.data_ptr(), _p(pre.scale) if pre else None,
                       _p(pre.shift) if pre else None, rec.data_ptr(), _stream())
    return rec


def proj_norm_bwd(x: torch.Tensor, st: "NormStats", drec: torch.Tensor, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                  dgamma: torch.Tensor, dbeta: torch.Tensor, dw_accum: torch.Tensor, db_accum: torch.Tensor) -> torch.Tensor:
    """backward of proj_fwd(x, w, b, pre=st) through the projection AND the BatchNorm (am_proj_norm_bwd): returns d loss / d x,
    accumulates the four parameter gradients."""
    B, D, H, W, Cc = x.shape
    assert st.sync_world <= 1
    dx = torch.empty_like(x)
    ws_b, _ = _bwd_workspaces(x.device, Cc)
    coef = torch.empty(3, Cc, device=x.device, dtype=torch.float32)
    hip.lib().proj_norm_bwd(_dt(x), x.data_ptr(), drec.data_ptr(), B * D * H * W, Cc, w.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                            st.mean.data_ptr(), st.rstd.data_ptr(), st.scale.data_ptr(), ws_b.data_ptr(), coef.data_ptr(), dx.data_ptr(),
                            dgamma.data_ptr(), dbeta.data_ptr(), dw_accum.data_ptr(), db_accum.data_ptr(), _stream())
    return dx


def proj_bwd(x: torch.Tensor, drec: torch.Tensor, w: torch.Tensor, dw_accum: torch.Tensor, db_accum: torch.Tensor,
             deterministic: Optional[bool] = None) -> torch.Tensor:
    B, D, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    ws = _det_workspace(x.device, 4096 * (Cc + 1) // 8) if _det(deterministic) else None
    hip.lib().proj_bwd(_dt(x), x.data_ptr(), drec.data_ptr(), B * D * H * W, Cc, w.data_ptr(), dx.data_ptr(), dw_accum.data_ptr(),
                       db_accum.data_ptr(), _p(ws), ws.numel() if ws is not None else 0, _stream())
    return dx


def head_stencil_supported(x: torch.Tensor) -> bool:
    """am_head_stencil serves this channels-last tensor (16^3 patches of a [B,D,H,W,C] map, C in {32, 64, 128, 192})."""
    B, D, H, W, C = x.shape
    ok = hip.lib()._lib.am_head_stencil_supported(_dt(x), C) == 1
    return bool(ok and D % 16 == 0 and H % 16 == 0 and W % 16 == 0 and max(B, D // 16, H // 16, W // 16) <= 255)


def head_fold(w2: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, wproj: torch.Tensor, bproj: torch.Tensor):
    """conv3x3x3 (Cmid, Cin, 3, 3, 3; no bias) -> eval BatchNorm (scale, shift) -> 1x1 projection, folded into (W_eff [27, Cin], b_eff [1])."""
    cmid, cin = w2.shape[0], w2.shape[1]
    assert tuple(w2.shape[2:]) == (3, 3, 3) and w2.is_contiguous() and wproj.numel() == cmid
    weff = torch.empty(27, cin, device=w2.device, dtype=torch.float32)
    beff = torch.empty(1, device=w2.device, dtype=torch.float32)
    hip.lib().head_fold(w2.data_ptr(), cmid, cin, scale.data_ptr(), shift.data_ptr(), wproj.data_ptr(), bproj.data_ptr(), weff.data_ptr(),
                        beff.data_ptr(), _stream())
    return weff, beff


def head_stencil(r: torch.Tensor, weff: torch.Tensor, beff: torch.Tensor, patches: MaskInfo, rec: Optional[torch.Tensor] = None,
                 inp: Optional[torch.Tensor] = None, l2: Optional[torch.Tensor] = None):
    """rec[q] = b_eff + sum_t W_eff[t] . r[q + t] on the ACTIVE 16^3 patches of `patches` (fp32 [B,D,H,W], other patches untouched) and / or
    their raw per-patch l2 against inp (fp32 [B, L] entries of those patches)."""
    B, D, H, W, C = r.shape
    lst, n = patches.active_list()
    assert lst is not None and (patches.fd, patches.fh, patches.fw) == (D // 16, H // 16, W // 16) and r.is_contiguous()
    assert rec is None or (rec.dtype == torch.float32 and tuple(rec.shape) == (B, D, H, W) and rec.is_contiguous())
    assert l2 is None or (inp is not None and l2.dtype == torch.float32 and l2.numel() == B * patches.fd * patches.fh * patches.fw)
    hip.lib().head_stencil(_dt(r), r.data_ptr(), B, D, H, W, C, weff.data_ptr(), beff.data_ptr(), lst.data_ptr(), n, _p(rec), _p(inp), _p(l2), _stream())


def patch_loss_fwd(inp: torch.Tensor, rec: torch.Tensor, mask: MaskInfo, normalized: bool, want_loss: bool = True):
    """inp/rec fp32 [B,D,H,W] -> (l2m [B,L], pmean, prstd, lossinfo[2] or None)."""
    B, D, H, W = inp.shape
    L = mask.fd * mask.fh * mask.fw
    l2m = torch.empty(B, L, device=inp.device, dtype=torch.float32)
    # want_loss=False (teacher pass): pmean/prstd stay NULL, which is also the kernel's cue to skip the visible patches entirely
    # (their l2 is 0 by definition and their rec voxels may never have been written, engine.forward(needed_patches=...))
    pm = torch.empty(B, L, device=inp.device, dtype=torch.float32) if want_loss else None
    pr = torch.empty(B, L, device=inp.device, dtype=torch.float32) if want_loss else None
    info = torch.empty(2, device=inp.device, dtype=torch.float32) if want_loss else None
    hip.lib().patch_loss_fwd(inp.data_ptr(), rec.data_ptr(), mask.t.data_ptr(), B, D, H, W, int(normalized), l2m.data_ptr(),
                             _p(pm), _p(pr), _p(info), _stream())
    return l2m, pm, pr, info


def patch_loss_bwd(inp, rec, mask: MaskInfo, pm, pr, info, gout: Optional[torch.Tensor]) -> torch.Tensor:
    B, D, H, W = inp.shape
    drec = torch.empty_like(rec)
    hip.lib().patch_loss_bwd(inp.data_ptr(), rec.data_ptr(), mask.t.data_ptr(), B, D, H, W, pm.data_ptr(), pr.data_ptr(),
                             info.data_ptr(), _p(gout), drec.data_ptr(), _stream())
    return drec


def mask_sampler(loss: torch.Tensor, keys: torch.Tensor, len_keep: int, len_loss: int) -> torch.Tensor:
    B, L = loss.shape
    out = torch.empty(B, L, device=loss.device, dtype=torch.uint8)
    hip.lib().mask_sampler(loss.data_ptr(), keys.data_ptr(), B, L, len_keep, len_loss, out.data_ptr(), _stream())
    return out


def sumsq(g: torch.Tensor, out: torch.Tensor):
    hip.lib().sumsq(g.data_ptr(), g.numel(), out.data_ptr(), _stream())


def adamw_ema(p, g, m, v, ema, n, lr, betas, eps, wd, step, sumsq_t, max_norm, ema_decay, gnorm_out, grad_scale: float = 1.0, dyn=None,
              guard: Optional[torch.Tensor] = None):
    """guard: device int32[4] {latched, first bad call, calls, 0} -- the per-step non-finite stop (am_adamw_ema)."""
    assert guard is None or (guard.dtype == torch.int32 and guard.numel() >= 4)
    hip.lib().adamw_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(ema), n, lr, betas[0], betas[1], eps, wd, step,
                        _p(sumsq_t), max_norm, ema_decay, grad_scale, _p(gnorm_out), _p(dyn), _p(guard), _stream())


def adam_dyn_scalars(lr: float, betas, step: int, ema_decay: float):
    """the float[4] am_adamw_ema reads from device memory in graph replays (same roundings as its by-value path)."""
    import math
    return [float(lr), 1.0 - betas[0] ** step, math.sqrt(1.0 - betas[1] ** step), float(ema_decay)]


def ema(ema_t: torch.Tensor, p: torch.Tensor, decay: float, guard: Optional[torch.Tensor] = None):
    hip.lib().ema(ema_t.data_ptr(), p.data_ptr(), p.numel(), decay, _p(guard), _stream())


def ema_i64(ema_t: torch.Tensor, p: torch.Tensor, decay: float, guard: Optional[torch.Tensor] = None):
    """timm's ModelEma.update on int64 entries (num_batches_tracked), all of them in one launch."""
    assert ema_t.dtype == p.dtype == torch.int64 and ema_t.numel() == p.numel() and ema_t.is_contiguous() and p.is_contiguous()
    hip.lib().ema_i64(ema_t.data_ptr(), p.data_ptr(), p.numel(), decay, _p(guard), _stream())


def guard_restore(dst: torch.Tensor, snapshot: torch.Tensor, guard: torch.Tensor):
    """dst = snapshot where the non-finite guard is latched (device-side decision, no host round trip)."""
    assert dst.dtype == snapshot.dtype and dst.numel() == snapshot.numel() and dst.is_contiguous() and snapshot.is_contiguous()
    hip.lib().guard_restore(dst.data_ptr(), snapshot.data_ptr(), dst.numel() * dst.element_size(), guard.data_ptr(), _stream())


# ------------------------------------------------------------------ data-feed augmentation (device side)
def spline_prefilter(vol: torch.Tensor):
    """in place: cubic B-spline coefficients of an fp32 [D,H,W] volume (== scipy.ndimage.spline_filter(order=3, mode='mirror'))."""
    assert vol.dtype == torch.float32 and vol.dim() == 3 and vol.is_contiguous()
    hip.lib().spline_prefilter(vol.data_ptr(), *vol.shape, _stream())
    return vol


def resample_affine(src: torch.Tensor, dst: torch.Tensor, affine_3x4, order: int, cval: float = 0.0):
    """dst[o] = interp(src, A (o, 1)); src fp32 [Ds,Hs,Ws] (prefiltered when order == 3), dst fp32 [D,H,W]."""
    assert src.dtype == dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
    arr = (_ct.c_float * 12)(*[float(v) for v in affine_3x4])
    hip.lib().resample_affine(src.data_ptr(), *src.shape, dst.data_ptr(), *dst.shape, _ct.addressof(arr), int(order), float(cval), _stream())
    return dst


def resample_labels(src: torch.Tensor, dst: Optional[torch.Tensor], affine_3x4, order: int, cval: int = -1, remove=(-1, 0),
                    region_bits: Optional[torch.Tensor] = None, n_regions: int = 0, regions_out: Optional[torch.Tensor] = None):
    """The label half of resample_affine at the same coordinates: src int16 [Ds,Hs,Ws] -> dst int16 [D,H,W] (None: regions only) by
    batchgenerators' label interpolation (order 1: the largest label whose trilinear mask value is >= 0.5, else 0; order 0: nearest,
    outside -> cval), then remove[0] -> remove[1] (None: nothing removed).  region_bits int32 [n_lut] (data.region_lut) + regions_out
    uint8 [n_regions,D,H,W]: one plane per region of the removed labels.  Returns (dst, regions_out)."""
    assert src.dtype == torch.int16 and src.dim() == 3 and src.is_contiguous()
    assert dst is not None or regions_out is not None
    out_shape = tuple(dst.shape) if dst is not None else tuple(regions_out.shape[1:])
    if dst is not None:
        assert dst.dtype == torch.int16 and dst.dim() == 3 and dst.is_contiguous()
    if regions_out is not None:
        assert region_bits is not None and region_bits.dtype == torch.int32 and region_bits.dim() == 1 and region_bits.is_contiguous()
        assert regions_out.dtype == torch.uint8 and regions_out.is_contiguous() and tuple(regions_out.shape) == (int(n_regions), *out_shape)
    rm_from, rm_to = (int(v) for v in remove) if remove is not None else (0, 0)
    arr = (_ct.c_float * 12)(*[float(v) for v in affine_3x4])
    hip.lib().resample_labels(src.data_ptr(), *src.shape, _p(dst), *out_shape, _ct.addressof(arr), int(order), int(cval), rm_from, rm_to,
                              _p(region_bits), 0 if region_bits is None else region_bits.numel(), int(n_regions), _p(regions_out), _stream())
    return dst, regions_out


# ------------------------------------------------------------------ segmentation inference (seg_ops.hip)
SEG_LDS_C = 240   # AM_SEG_LDS_C


def mirror_axes_mask(axes) -> int:
    """allowed mirroring axes (spatial, 0..2) -> the kernels' bitmask; its M = 2^len mirrors: bit j of m flips the j-th axis (ascending)."""
    m = 0
    for a in axes:
        if not 0 <= int(a) <= 2:
            raise ValueError(f"mirroring axis {a} is not a spatial axis of a 3-D volume")
        m |= 1 << int(a)
    return m


def seg_gather(vol: torch.Tensor, origin, tile, axes_mask: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vol fp32 [X,Y,Z]; origin = tile start - pad_below (may be negative: zeros outside the volume) -> [M,T0,T1,T2] fp32."""
    assert vol.dtype == torch.float32 and vol.dim() == 3 and vol.is_contiguous()
    M = 1 << bin(axes_mask).count("1")
    if out is None:
        out = torch.empty(M, *tile, device=vol.device, dtype=torch.float32)
    assert tuple(out.shape) == (M, *tile) and out.dtype == torch.float32 and out.is_contiguous()
    hip.lib().seg_gather(vol.data_ptr(), *vol.shape, *(int(o) for o in origin), *(int(t) for t in tile), int(axes_mask), out.data_ptr(), _stream())
    return out


def seg_upcat(u: torch.Tensor, skip: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cat(nearest_up(u), skip) along channels: u [B,d,h,w,C], skip [B,D,H,W,C] (D = d or 2d) -> [B,D,H,W,2C]."""
    B, D, H, W, Cc = skip.shape
    f = D // u.shape[1]
    assert u.dtype == skip.dtype and u.shape[0] == B and u.shape[-1] == Cc and tuple(v * f for v in u.shape[1:4]) == (D, H, W)
    if out is None:
        out = torch.empty(B, D, H, W, 2 * Cc, device=skip.device, dtype=skip.dtype)
    hip.lib().seg_upcat(_dt(skip), u.data_ptr(), skip.data_ptr(), out.data_ptr(), B, D, H, W, Cc, f, _stream())
    return out


def seg_head(f: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """plain 1x1 head: f [B,D,H,W,C] -> logits fp32 [B,K,D,H,W]; w fp32 (K,C[,1,1,1]), b fp32 [K]."""
    B, D, H, W, Cc = f.shape
    K = w.shape[0]
    assert w.dtype == torch.float32 and w.numel() == K * Cc and w.is_contiguous() and b.numel() == K
    out = torch.empty(B, K, D, H, W, device=f.device, dtype=torch.float32)
    hip.lib().seg_head(_dt(f), f.data_ptr(), B, D, H, W, Cc, w.data_ptr(), b.data_ptr(), K, out.data_ptr(), _stream())
    return out


def seg_head_accumulate(f: torch.Tensor, axes_mask: int, w: torch.Tensor, b: torch.Tensor, gauss: Optional[torch.Tensor], acc: torch.Tensor,
                        wsum: torch.Tensor, start):
    """f = the M mirrored predictions of one tile [M,T0,T1,T2,C]; acc fp32 [K,X,Y,Z] and wsum fp32 [X,Y,Z] (padded volume) += the
    un-flipped mirror mean of the head, Gaussian-weighted, at the tile start."""
    M, T0, T1, T2, Cc = f.shape
    K = w.shape[0]
    assert M == 1 << bin(axes_mask).count("1") and w.dtype == torch.float32 and w.numel() == K * Cc and w.is_contiguous() and b.numel() == K
    assert acc.dtype == torch.float32 and wsum.dtype == torch.float32 and acc.shape[0] == K and tuple(acc.shape[1:]) == tuple(wsum.shape)
    assert gauss is None or (gauss.dtype == torch.float32 and gauss.numel() == T0 * T1 * T2)
    hip.lib().seg_head_accumulate(_dt(f), f.data_ptr(), int(axes_mask), T0, T1, T2, Cc, w.data_ptr(), b.data_ptr(), K, _p(gauss), acc.data_ptr(),
                                  wsum.data_ptr(), *wsum.shape, *(int(s) for s in start), _stream())


def seg_finalize(acc: torch.Tensor, wsum: torch.Tensor, crop_start, crop_size, want_logits: bool = True, want_labels: bool = False):
    """(logits fp32 [K,X,Y,Z] or None, labels [X,Y,Z] or None): acc / wsum over the crop; labels = argmax (uint8 for K <= 255, else int16)."""
    K = acc.shape[0]
    logits = torch.empty(K, *crop_size, device=acc.device, dtype=torch.float32) if want_logits else None
    labels = torch.empty(*crop_size, device=acc.device, dtype=torch.uint8 if K <= 255 else torch.int16) if want_labels else None
    hip.lib().seg_finalize(acc.data_ptr(), wsum.data_ptr(), K, *acc.shape[1:], *(int(c) for c in crop_start), *(int(s) for s in crop_size),
                           _p(logits), _p(labels), labels.element_size() if labels is not None else 1, _stream())
    return logits, labels


SEG_SOFTMAX, SEG_SIGMOID = 0, 1   # AM_SEG_SOFTMAX / AM_SEG_SIGMOID


def seg_export(acc: torch.Tensor, wsum: torch.Tensor, crop_start, crop_size, nonlin: str = "softmax", regions_class_order=None,
               want_probabilities: bool = True, want_labels: bool = True):
    """(probabilities fp32 [K,X,Y,Z] or None, labels [X,Y,Z] or None) of acc / wsum over the crop in one pass.  nonlin "softmax": labels =
    argmax of the logits (seg_finalize's labels); "sigmoid": labels = 0, then regions_class_order[i] wherever p_i > 0.5, in order.  Labels
    are uint8 when the largest possible label (K - 1, or max(regions_class_order)) is <= 255, else int16."""
    K = acc.shape[0]
    if nonlin not in ("softmax", "sigmoid"):
        raise ValueError(f"nonlin {nonlin!r}: 'softmax' or 'sigmoid'")
    order = None
    if nonlin == "softmax":
        if regions_class_order is not None:
            raise ValueError("regions_class_order belongs to nonlin='sigmoid' (region-based labels), not to softmax")
        top = K - 1
    else:
        if regions_class_order is None:
            raise ValueError("nonlin='sigmoid' needs regions_class_order")
        order = [int(c) for c in regions_class_order]
        if len(order) != K:
            raise ValueError(f"regions_class_order has {len(order)} entries for {K} regions")
        if any(c < 0 or c > 32767 for c in order):
            raise ValueError(f"regions_class_order {order}: labels must lie in [0, 32767]")
        top = max(order)
    if top > 32767:
        raise ValueError(f"label {top} does not fit int16")
    if not (want_probabilities or want_labels):
        raise ValueError("seg_export: nothing asked for (want_probabilities and want_labels are both False)")
    assert acc.dtype == torch.float32 and wsum.dtype == torch.float32 and acc.is_contiguous() and wsum.is_contiguous()
    assert tuple(acc.shape[1:]) == tuple(wsum.shape)
    order_t = torch.tensor(order, dtype=torch.int32, device=acc.device) if order is not None else None
    probs = torch.empty(K, *crop_size, device=acc.device, dtype=torch.float32) if want_probabilities else None
    labels = torch.empty(*crop_size, device=acc.device, dtype=torch.uint8 if top <= 255 else torch.int16) if want_labels else None
    hip.lib().seg_export(acc.data_ptr(), wsum.data_ptr(), K, *acc.shape[1:], *(int(c) for c in crop_start), *(int(s) for s in crop_size),
                         SEG_SIGMOID if order is not None else SEG_SOFTMAX, _p(order_t), _p(probs), _p(labels),
                         labels.element_size() if labels is not None else 1, _stream())
    return probs, labels


# ------------------------------------------------------------------ segmentation fine-tuning (seg_bwd_ops.hip)
SEG_HEAD_BWD_TILE, SEG_HEAD_BWD_SLOTS = 64, 1024   # AM_SEG_HEAD_BWD_TILE / AM_SEG_HEAD_BWD_SLOTS


def seg_head_bwd_workspace_floats(B: int, n_voxels: int, C: int, K: int) -> int:
    """floats of am_seg_head_bwd's workspace: one slot (partial dw, db) per workgroup of its persistent grid."""
    slots = min(B * ((n_voxels + SEG_HEAD_BWD_TILE - 1) // SEG_HEAD_BWD_TILE), SEG_HEAD_BWD_SLOTS)
    return slots * (K * C + K)


def seg_head_bwd(dlogits: torch.Tensor, f: torch.Tensor, w: torch.Tensor, dw_accum: torch.Tensor, db_accum: torch.Tensor,
                 df: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """backward of seg_head in one pass over dlogits fp32 [B,K,D,H,W]: returns df [B,D,H,W,C] (f's dtype; accumulate: added to the given
    df, one rounding) and adds the weight / bias gradients to dw_accum fp32 (K,C[,1,1,1]) / db_accum fp32 [K].  No atomics: two calls on
    the same input give the same bits."""
    B, D, H, W, Cc = f.shape
    K = w.shape[0]
    assert dlogits.dtype == torch.float32 and tuple(dlogits.shape) == (B, K, D, H, W) and dlogits.is_contiguous() and f.is_contiguous()
    assert w.dtype == torch.float32 and w.numel() == K * Cc and w.is_contiguous()
    assert dw_accum.dtype == torch.float32 and dw_accum.numel() == K * Cc and dw_accum.is_contiguous()
    assert db_accum.dtype == torch.float32 and db_accum.numel() == K and db_accum.is_contiguous()
    if df is None:
        assert not accumulate, "accumulate needs the df to add to"
        df = torch.empty_like(f)
    assert df.dtype == f.dtype and tuple(df.shape) == tuple(f.shape) and df.is_contiguous()
    ws = torch.empty(seg_head_bwd_workspace_floats(B, D * H * W, Cc, K), device=f.device, dtype=torch.float32)
    hip.lib().seg_head_bwd(_dt(f), dlogits.data_ptr(), f.data_ptr(), w.data_ptr(), B, D, H, W, Cc, K, df.data_ptr(), int(bool(accumulate)),
                           dw_accum.data_ptr(), db_accum.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return df


def seg_upcat_bwd(dy: torch.Tensor, factor: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """backward of seg_upcat: dy [B,D,H,W,2C] -> (du [B,D/f,H/f,W/f,C] = fp32 sum of the f^3 fine voxels of the first half, rounded once;
    dskip [B,D,H,W,C] = the second half).  Unsupported arguments (C % 8, factor not 1 / 2, sizes no multiple of it) raise from the ABI."""
    B, D, H, W, C2 = dy.shape
    factor = int(factor)
    assert dy.is_contiguous() and C2 % 2 == 0
    Cc = C2 // 2
    f = max(factor, 1)
    du = torch.empty(B, D // f, H // f, W // f, Cc, device=dy.device, dtype=dy.dtype)
    dskip = torch.empty(B, D, H, W, Cc, device=dy.device, dtype=dy.dtype)
    hip.lib().seg_upcat_bwd(_dt(dy), dy.data_ptr(), du.data_ptr(), dskip.data_ptr(), B, D, H, W, Cc, factor, _stream())
    return du, dskip


# ------------------------------------------------------------------ segmentation loss (loss_ops.hip)
SEG_LOSS_TILE = 256   # AM_SEG_LOSS_TILE


def _seg_loss_geometry(mode: int, logits: torch.Tensor, target: torch.Tensor, has_ignore: bool):
    """validate (logits fp32 [B,K,D,H,W] contiguous on the GPU; target int16 [B,1,D,H,W] (softmax) or uint8 / bool [B,K(+1),D,H,W]
    (sigmoid), any strides, same device) -> (B, K, D, H, W, the target's element strides)."""
    if mode not in (SEG_SOFTMAX, SEG_SIGMOID):
        raise ValueError(f"mode {mode}: SEG_SOFTMAX or SEG_SIGMOID")
    if not logits.is_cuda:
        raise RuntimeError("the segmentation loss runs on the GPU only (no CPU path exists)")
    if logits.dtype != torch.float32 or logits.dim() != 5 or not logits.is_contiguous():
        raise ValueError(f"logits must be contiguous fp32 [B,K,D,H,W], got {logits.dtype} {tuple(logits.shape)} contiguous={logits.is_contiguous()}")
    if target.device != logits.device:
        raise RuntimeError(f"target on {target.device}, logits on {logits.device}")
    B, K, D, H, W = logits.shape
    want_c = 1 if mode == SEG_SOFTMAX else K + (1 if has_ignore else 0)
    if target.dim() != 5 or tuple(target.shape) != (B, want_c, D, H, W):
        raise ValueError(f"target {tuple(target.shape)} does not match logits {tuple(logits.shape)}: expected {(B, want_c, D, H, W)}")
    if mode == SEG_SOFTMAX:
        if target.dtype != torch.int16:
            raise TypeError(f"softmax mode reads int16 labels, got {target.dtype}")
        if K < 2 or K > 32767:
            raise ValueError(f"K = {K}: 2 .. 32767 classes")
    elif target.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"sigmoid mode reads uint8 / bool region channels, got {target.dtype}")
    return B, K, D, H, W, tuple(int(s) for s in target.stride())


def seg_loss_sums(mode: int, logits: torch.Tensor, target: torch.Tensor, ignore_label: Optional[int] = None, keep_lse: bool = True):
    """Pass 1 of the fused Dice + CE / BCE loss: (sums fp64 [B,K+1,4], lse fp32 [B,D*H*W,2] or None: per voxel the maximum and the log of the
    rescaled sum, whose sum is the log-sum-exp -- kept apart so that x - max stays exact under large shifted logits).  sums[b,k] = (sum p y m, sum p m,
    sum y m, CE / BCE numerator of class k), sums[b,K] = (unmasked voxels, CE part of voxels of no class, 0, 0).  softmax: ignore_label
    (None: none) masks voxels; sigmoid: ignore_label is not None says that the target's last channel is the ignore mask.  The target is
    read through its strides (a deep-supervision view is consumed as it is)."""
    has_ignore = ignore_label is not None
    B, K, D, H, W, ts = _seg_loss_geometry(mode, logits, target, has_ignore)
    N = D * H * W
    rows = (N + SEG_LOSS_TILE - 1) // SEG_LOSS_TILE
    partials = torch.empty(B * rows * (K + 1) * 4, device=logits.device, dtype=torch.float32)
    sums = torch.empty(B, K + 1, 4, device=logits.device, dtype=torch.float64)
    lse = torch.empty(B, N, 2, device=logits.device, dtype=torch.float32) if (keep_lse and mode == SEG_SOFTMAX) else None
    hip.lib().seg_loss_sums(mode, logits.data_ptr(), B, K, D, H, W, target.data_ptr(), *ts, int(has_ignore),
                            int(ignore_label) if (has_ignore and mode == SEG_SOFTMAX) else 0, partials.data_ptr(), sums.data_ptr(), _p(lse), _stream())
    return sums, lse


def seg_loss_coeffs(mode: int, sums: torch.Tensor, n_voxels: int, batch_dice: bool, do_bg: bool, has_ignore: bool, smooth: float,
                    weight_dice: float, weight_ce: float, level_weight: float = 1.0, loss_total: Optional[torch.Tensor] = None):
    """The sums table -> (coef fp32 [2*B*K + 1], loss fp32 [1]) on the device, no read-back: coef = w_dice (a_c, b_c) per (sample, class)
    and, last, w_ce / n.  loss_total fp32 [1] (optional) += level_weight * loss."""
    assert sums.dtype == torch.float64 and sums.dim() == 3 and sums.shape[2] == 4 and sums.is_contiguous()
    B, K = sums.shape[0], sums.shape[1] - 1
    if not do_bg and K < 2:
        raise ValueError("do_bg=False leaves no class to average")
    coef = torch.empty(2 * B * K + 1, device=sums.device, dtype=torch.float32)
    loss = torch.empty(1, device=sums.device, dtype=torch.float32)
    if loss_total is not None:
        assert loss_total.dtype == torch.float32 and loss_total.numel() == 1 and loss_total.device == sums.device
    hip.lib().seg_loss_coeffs(mode, sums.data_ptr(), B, K, int(n_voxels), int(bool(batch_dice)), int(bool(do_bg)), int(bool(has_ignore)),
                              float(smooth), float(weight_dice), float(weight_ce), float(level_weight), coef.data_ptr(), loss.data_ptr(),
                              _p(loss_total), _stream())
    return coef, loss


def seg_loss_grad(mode: int, logits: torch.Tensor, target: torch.Tensor, ignore_label: Optional[int], lse: Optional[torch.Tensor],
                  coef: torch.Tensor, gscale: torch.Tensor, weight: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pass 2: dlogits fp32 [B,K,D,H,W] = gscale * weight * d loss / d logits; gscale is a one-element fp32 DEVICE tensor (the upstream
    gradient is never read back)."""
    has_ignore = ignore_label is not None
    B, K, D, H, W, ts = _seg_loss_geometry(mode, logits, target, has_ignore)
    assert coef.dtype == torch.float32 and coef.numel() == 2 * B * K + 1 and coef.is_contiguous() and coef.device == logits.device
    assert gscale.dtype == torch.float32 and gscale.numel() == 1 and gscale.device == logits.device
    if mode == SEG_SOFTMAX:
        assert lse is not None and lse.dtype == torch.float32 and lse.numel() == 2 * B * D * H * W and lse.is_contiguous()
    if out is None:
        out = torch.empty_like(logits)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(logits.shape) and out.is_contiguous() and out.device == logits.device
    hip.lib().seg_loss_grad(mode, logits.data_ptr(), B, K, D, H, W, target.data_ptr(), *ts, int(has_ignore),
                            int(ignore_label) if (has_ignore and mode == SEG_SOFTMAX) else 0, _p(lse), coef.data_ptr(), gscale.data_ptr(),
                            float(weight), out.data_ptr(), _stream())
    return out


# ------------------------------------------------------------------ segmentation validation counts (seg_eval_ops.hip)
SEG_COUNTS_TILE = 256   # AM_SEG_COUNTS_TILE


def seg_hard_counts_workspace_bytes(B: int, n_voxels: int, K: int) -> int:
    """bytes of am_seg_hard_counts's workspace: one int32 x 4 partial per (sample, tile of SEG_COUNTS_TILE voxels, class)."""
    return int(B) * ((int(n_voxels) + SEG_COUNTS_TILE - 1) // SEG_COUNTS_TILE) * int(K) * 16


def seg_hard_counts(mode: int, logits: torch.Tensor, target: torch.Tensor, ignore_label: Optional[int] = None,
                    out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """tp / fp / fn of the hard prediction per class, summed over the batch and all voxels: int64 [K, 3], exact, in one pass over the logits
    (fp32 [B,K,D,H,W] contiguous).  softmax: the prediction is the first index of the maximum (torch.argmax), target int16 labels
    [B,1,D,H,W], ignore_label (None: none) masks voxels, a label outside [0, K) belongs to no class.  sigmoid: the prediction of region k is
    x_k > 0, target uint8 / bool [B,K(+1),D,H,W], ignore_label is not None says that its last channel is the ignore mask.  The target is read
    through its strides.  out (int64 [K,3] on the device): written, or added to with accumulate=True; nothing is read back."""
    if mode not in (SEG_SOFTMAX, SEG_SIGMOID):
        raise ValueError(f"mode {mode}: SEG_SOFTMAX or SEG_SIGMOID")
    if not logits.is_cuda:
        raise RuntimeError("the segmentation counts run on the GPU only (no CPU path exists)")
    if logits.dtype != torch.float32 or logits.dim() != 5 or not logits.is_contiguous():
        raise ValueError(f"logits must be contiguous fp32 [B,K,D,H,W], got {logits.dtype} {tuple(logits.shape)} contiguous={logits.is_contiguous()}")
    if target.device != logits.device:
        raise RuntimeError(f"target on {target.device}, logits on {logits.device}")
    has_ignore = ignore_label is not None
    B, K, D, H, W = logits.shape
    if K < 1:
        raise ValueError("K = 0: at least one class")
    want_c = 1 if mode == SEG_SOFTMAX else K + (1 if has_ignore else 0)
    if target.dim() != 5 or tuple(target.shape) != (B, want_c, D, H, W):
        raise ValueError(f"target {tuple(target.shape)} does not match logits {tuple(logits.shape)}: expected {(B, want_c, D, H, W)}")
    if mode == SEG_SOFTMAX and target.dtype != torch.int16:
        raise TypeError(f"softmax mode reads int16 labels, got {target.dtype}")
    if mode == SEG_SIGMOID and target.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"sigmoid mode reads uint8 / bool region channels, got {target.dtype}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the table to add to")
        out = torch.empty(K, 3, device=logits.device, dtype=torch.int64)
    if out.dtype != torch.int64 or tuple(out.shape) != (K, 3) or not out.is_contiguous() or out.device != logits.device:
        raise ValueError(f"out must be a contiguous int64 [{K}, 3] tensor on {logits.device}")
    ws = torch.empty(max(seg_hard_counts_workspace_bytes(B, D * H * W, K), 16), device=logits.device, dtype=torch.uint8)
    hip.lib().seg_hard_counts(mode, logits.data_ptr(), B, K, D, H, W, target.data_ptr(), *(int(s) for s in target.stride()), int(has_ignore),
                              int(ignore_label) if (has_ignore and mode == SEG_SOFTMAX) else 0, ws.data_ptr(), ws.numel(), out.data_ptr(),
                              int(bool(accumulate)), _stream())
    return out
